"""pcio::write_ply_mesh -> pcio::read_ply_mesh as a stand-alone program (tests/native/test_ply_mesh_write.cpp) compiled with
-fsanitize=address,undefined: the round trip is bit for bit, a zero-triangle mesh included, and what the writer leaves is the PLY the
Python side reads as well.  No GPU needed."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_writer_round_trip_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_ply_mesh_write")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "test_ply_mesh_write.cpp")])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    data = (tmp_path / "mesh.ply").read_bytes()
    head, body = data.split(b"end_header\n", 1)
    assert b"format binary_little_endian 1.0" in head and b"element vertex 5" in head and b"property double x" in head
    assert b"element face 4" in head and b"property list uchar int vertex_indices" in head
    assert len(body) == 5 * 24 + 4 * 13
    v = np.frombuffer(body[:120], "<f8").reshape(5, 3)
    assert v[1].tolist() == [4.0e5 + 0.1, -3.0e5 - 0.3, 50.25] and np.signbit(v[0, 1])
    rows = np.frombuffer(body[120:], np.uint8).reshape(4, 13)
    assert (rows[:, 0] == 3).all() and np.frombuffer(rows[:, 1:].tobytes(), "<i4").tolist() == [0, 1, 2, 2, 3, 4, 4, 4, 0, 3, 1, 0]
    assert b"element face 0" in (tmp_path / "no_faces.ply").read_bytes()
