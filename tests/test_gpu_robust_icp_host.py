"""The C++ host with icp_robust_kernel, icp_multi_scale_* and icp_information_matrix, from PCD files: the aligned transformation against
the Python path (icp.icp_multi_scale) to the printed digits, registration_information.txt against Engine.icp_information, the refusal
of a kernel without its scale, and no new output without the keys."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _robust_reg_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
VOXELS, DISTS, ITERS, SCALE, GATE = [0.4, 0.2, 0.0], [1.0, 0.5, 0.25], [10, 10, 15], 1.0, 1.0


def _write_pcd(path, pts):
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    gt, m, pose = RR.outlier_scene(30_000)  # the ghosted map: 20 % of it a rigid copy 0.21 m off the surface
    d = tmp_path_factory.mktemp("pair")
    _write_pcd(d / "gt.pcd", gt)
    return d, gt, m, pose


def _run(pair, name, extra=""):
    base, gt, m, _ = pair
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", m)
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 2
icp_max_distance: {GATE}
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
estimate_map_path: {d}
gt_map_path: {base / 'gt.pcd'}
scene_name: ghost
save_immediate_result: true
evaluate_mme: false
evaluate_gt_mme: false
nn_radius: 0.1
evaluate_using_initial: false
vmd_voxel_size: 0.5
downsample_size: 0.0
enable_debug: false
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=300)
    return r, d / "map_results"


def _aligned(folder):
    txt = open(folder / "map_results.txt").read()
    body = txt[txt.index("Aligned cloud:") + len("Aligned cloud:"):txt.index("Aligned results:")]
    return np.array([float(v) for v in body.split()]).reshape(4, 4)


def test_host_robust_multi_scale_and_information(pair):
    from cloud_map_evaluation_amd import icp
    from cloud_map_evaluation_amd.engine import Engine

    _, gt, m, pose = pair
    r, f = _run(pair, "robust", f"""icp_robust_kernel: tukey
icp_robust_scale: {SCALE}
icp_multi_scale_voxels: {VOXELS}
icp_multi_scale_distances: {DISTS}
icp_multi_scale_iterations: {ITERS}
icp_information_matrix: true
""")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    T_host = _aligned(f)
    with Engine(0) as e:
        e.upload(0, m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        out = icp.icp_multi_scale(e, VOXELS, DISTS, ITERS, 2, kernel="tukey", kernel_scale=SCALE)
        e.nn1(0, 1, fetch=False)
        info, n = e.icp_information(0, GATE)
    print(f"\nhost - python, largest entry: {np.abs(T_host - out['transformation']).max():.2e}; pose error {RR.pose_error(T_host, pose):.2e}")
    # the file prints five decimals: half a unit of the last one, and 1e-7 for the two solvers (Gaussian elimination, LAPACK)
    assert np.abs(T_host - out["transformation"]).max() <= 0.5e-5 + 1e-7
    assert RR.pose_error(T_host, pose) < RR.pose_error(np.eye(4), pose) / 10  # (an alignment: a tenth of the misalignment it started from)
    lines = open(f / "registration_information.txt").read().splitlines()
    H = np.array([[float(v) for v in lines[i].split()] for i in range(6)])
    kv = {l.split()[0]: [float(v) for v in l.split()[1:]] for l in lines[6:]}
    assert set(kv) == {"n_corr", "eigenvalues", "ratio"} and H.shape == (6, 6) and np.array_equal(H, H.T)
    assert int(kv["n_corr"][0]) == n == len(m)
    assert np.abs(H - info).max() <= 1e-9 * np.abs(info).max()
    ev = np.linalg.eigvalsh(info)
    assert np.allclose(kv["eigenvalues"], ev, rtol=1e-9, atol=1e-9 * ev[-1]) and kv["eigenvalues"] == sorted(kv["eigenvalues"])
    assert kv["ratio"][0] == pytest.approx(ev[0] / ev[-1], rel=1e-6)
    line = [l for l in r.stdout.splitlines() if l.startswith("INFO: Information matrix eigenvalue ratio")]
    assert len(line) == 1 and float(re.search(r": ([-+0-9.eE]+) over", line[0]).group(1)) == pytest.approx(kv["ratio"][0], rel=1e-4)
    assert "Information" not in open(f / "map_results.txt").read()  # no new line in the parsed file


def test_host_without_the_keys_writes_nothing_new_and_loses_to_the_robust_run(pair):
    _, _, _, pose = pair
    r, f = _run(pair, "plain")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not (f / "registration_information.txt").exists() and "Information matrix" not in r.stdout
    assert RR.pose_error(_aligned(f), pose) > 10 * RR.pose_error(_aligned(f.parent.parent / "robust" / "map_results"), pose)


def test_host_kernel_without_scale_fails_with_a_message(pair):
    r, f = _run(pair, "noscale", "icp_robust_kernel: tukey\n")
    assert r.returncode != 0
    assert "icp_robust_scale" in (r.stdout + r.stderr)
