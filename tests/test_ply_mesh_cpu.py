"""pcio::read_ply_mesh as a stand-alone program (tests/native/test_ply_mesh.cpp) compiled with -fsanitize=address,undefined and run on
well-formed and malformed PLY files: the malformed ones are refused with a message and no sanitizer report.  No GPU needed."""
import os
import subprocess

import numpy as np

import _ply_mesh_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reader_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_ply_mesh")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "test_ply_mesh.cpp")])
    v = np.random.default_rng(1).normal(size=(7, 3))
    faces = [(0, 1, 2, 3, 4), (4, 5, 6), (1, 1, 2)]
    files, expect = [], []
    for binary in (True, False):
        tag = "b" if binary else "a"
        files.append(F.write_ply_mesh(tmp_path / f"good_{tag}.ply", v, faces, binary, face_extra=True, edges=2))
        expect.append("ok 7 5")
        files.append(F.write_ply_mesh(tmp_path / f"range_{tag}.ply", v, [(0, 1, 7)], binary))
        expect.append("fail")
        files.append(F.write_ply_mesh(tmp_path / f"two_{tag}.ply", v, [(0, 1, 2), (3, 4)], binary))
        expect.append("fail")
        files.append(F.write_ply_mesh(tmp_path / f"neg_{tag}.ply", v, [(0, -3, 2)], binary))
        expect.append("fail")
    data = open(files[0], "rb").read()
    body = data.index(b"end_header\n") + 11
    for k, cut in enumerate((len(data) - 1, len(data) - 9, body + 50, body + 1, body, body - 4, 20, 3)):  # truncated everywhere
        p = tmp_path / f"cut{k}.ply"
        p.write_bytes(data[:cut])
        files.append(p)
        expect.append("fail")
    huge = tmp_path / "huge.ply"  # a list count far beyond the file
    huge.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                     b"element face 1\nproperty list int int vertex_indices\nend_header\n" + b"\0" * 12 + (2 ** 31 - 1).to_bytes(4, "little"))
    files.append(huge)
    expect.append("fail")
    text = open(files[4], "rb").read()  # the ascii good file, cut inside a face row
    acut = tmp_path / "acut.ply"
    acut.write_bytes(text[:len(text) - 12])
    files.append(acut)
    expect.append("fail")
    word = tmp_path / "word.ply"  # a token that is not a number
    word.write_bytes(text.replace(b" 4 5 6", b" 4 x5 6"))
    assert b"x5" in word.read_bytes()
    files.append(word)
    expect.append("fail")
    out = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(files)
    for f, ln, e in zip(files, lines, expect):
        assert ln.startswith(e), (str(f), ln)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
