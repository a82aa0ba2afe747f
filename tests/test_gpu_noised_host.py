"""The C++ host in simulation mode (evaluate_noised_gt: true): no estimate file, the map is the perturbed ground truth.  Its
map_results.txt and noise_gt_map.pcd against the Engine path (upload, down-sample, perturb, the suite on the resident clouds), the
noise_sweep.txt rows against single runs, and one run on the registration path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
EST, GT = 0, 1
DOWNSAMPLE = 0.005
STAGES = dict(noise_seed=11, noise_sparse_ratio=0.7, noise_dense_ratio=1.0, noise_region_size=0.5, noise_outlier_ratio=0.01,
              noise_outlier_range=0.2, noise_deform_radius=0.4, noise_deform_strength=0.02)
CENTER = (0.1, -0.2, 0.05)


def _T():
    T = np.eye(4)
    th = 0.002
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:3, 3] = [0.004, -0.002, 0.001]
    return T


def _write_pcd(path, pts):
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _read_pcd(path):
    raw = open(path, "rb").read()
    k = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    hdr = raw[:k].decode()
    assert "FIELDS x y z\n" in hdr and "SIZE 8 8 8\n" in hdr
    n = int(re.search(r"POINTS (\d+)", hdr).group(1))
    return np.frombuffer(raw[k:], dtype="<f8").reshape(n, 3)


def _cfg(est_dir, gt_path, sigma, initial=True, sweep=None):
    T = _T()
    rows = "\n".join("  - [" + ", ".join(repr(float(v)) for v in T[i]) + "]" for i in range(4))
    extra = "".join(f"{k}: {v}\n" for k, v in STAGES.items())
    extra += f"noise_deform_center: [{CENTER[0]}, {CENTER[1]}, {CENTER[2]}]\n"
    if sweep:
        extra += "noise_sweep: [" + ", ".join(repr(s) for s in sweep) + "]\n"
    return f"""registration_methods: 0
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
{rows}
estimate_map_path: {est_dir}
gt_map_path: {gt_path}
scene_name: noised
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.1
evaluate_using_initial: {'true' if initial else 'false'}
evaluate_noised_gt: true
noise_std_dev: {sigma!r}
vmd_voxel_size: 0.5
downsample_size: {DOWNSAMPLE}
enable_debug: false
{extra}"""


def _run(tmp_path, name, gt_path, sigma, **kw):
    d = tmp_path / name
    d.mkdir()
    cfg = d / "config.yaml"
    cfg.write_text(_cfg(d, gt_path, sigma, **kw))
    assert not (d / "map.pcd").exists()
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return d / "map_results"


def _results(folder):
    txt = open(folder / "map_results.txt").read()
    out = {}
    for key in ("RMSE/AC", "Comp", "FULL CD", "VMD", "SCS", "MME"):
        out[key] = re.search(rf"^{re.escape(key)}: (.*)$", txt, flags=re.M).group(1).split()
    out["counts"] = tuple(int(v) for v in re.search(r"point count: (\d+) / (\d+)", txt).groups())
    return out


def _printed(vals, decimals):
    return [f"{v:.{decimals}f}" for v in vals]


def _check_row_against_results(row, res):
    """a noise_sweep.txt row (noise_std_dev n_est ac[5] com[5] full_cd mme_est mme_gt awd scs) against a map_results.txt, at the latter's
    printed precision"""
    assert int(row[1]) == res["counts"][0]
    assert _printed(row[2:7], 15) == res["RMSE/AC"]
    assert _printed(row[7:12], 15) == res["Comp"]
    assert _printed(row[12:13], 5) == res["FULL CD"]
    assert _printed(row[13:15], 5) == res["MME"][:2]
    assert _printed(row[15:16], 5) == res["VMD"]
    assert _printed(row[16:17], 5) == res["SCS"]


@pytest.fixture(scope="module")
def gt_file(tmp_path_factory):
    from cloud_map_evaluation_amd import synth

    _, gt = synth.cube_pair(100_000, seed=42)
    d = tmp_path_factory.mktemp("gt")
    _write_pcd(d / "gt.pcd", gt.numpy())
    return d / "gt.pcd", gt.numpy()


def test_noised_run_equals_the_engine_path_and_the_sweep(tmp_path, gt_file):
    from cloud_map_evaluation_amd.engine import Engine, Param

    assert os.path.exists(EXE), "build the host first (__graft_entry__.build())"
    gt_path, gt = gt_file
    sigma, levels = 0.01, [0.005, 0.01, 0.02]
    folder = _run(tmp_path, "main", gt_path, sigma, sweep=levels)
    res = _results(folder)

    # the Engine path: upload the ground truth, down-sample it, perturb, the suite on the resident clouds
    p = Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=0.5, initial_matrix_=_T())
    with Engine(0) as eng:
        eng.upload(GT, gt, cell_size=0.1)
        ng = eng.voxel_downsample(GT, DOWNSAMPLE)
        kw = dict(noise_std=sigma, sparse_ratio=STAGES["noise_sparse_ratio"], dense_ratio=STAGES["noise_dense_ratio"],
                  region_size=STAGES["noise_region_size"], outlier_ratio=STAGES["noise_outlier_ratio"],
                  outlier_range=STAGES["noise_outlier_range"], deform_radius=STAGES["noise_deform_radius"],
                  deform_strength=STAGES["noise_deform_strength"], deform_center=CENTER, seed=STAGES["noise_seed"])
        ne = eng.perturb(EST, GT, **kw)
        o = eng.run_suite_from(None, None, p, overlap=True)
        est_t = eng.download(EST)
    assert res["counts"] == (ne, ng)
    assert _printed(list(o.est_gt.rmse), 15) == res["RMSE/AC"]
    assert _printed(list(o.est_gt.fitness), 15) == res["Comp"]
    assert _printed([o.est_gt.mean_nn_dist + o.gt_est.mean_nn_dist], 5) == res["FULL CD"]
    assert _printed([o.mme_est, o.mme_gt], 5) == res["MME"][:2]
    assert _printed([o.awd], 5) == res["VMD"] and _printed([o.scs], 5) == res["SCS"]
    # noise_gt_map.pcd = the map as evaluated (after the transform), bit for bit
    pcd = _read_pcd(folder / "noise_gt_map.pcd")
    assert pcd.shape == est_t.shape and np.array_equal(pcd.view(np.uint64), est_t.view(np.uint64))

    # noise_sweep.txt: one row per level; the row of noise_std_dev is map_results.txt; AC grows with the noise
    lines = open(folder / "noise_sweep.txt").read().splitlines()
    assert lines[0].startswith("#") and "noise_std_dev n_est" in lines[0]
    rows = [[float(v) for v in ln.split()] for ln in lines[1:]]
    assert [r[0] for r in rows] == levels and all(len(r) == 17 for r in rows)
    _check_row_against_results(rows[1], res)
    assert rows[0][2] < rows[1][2] < rows[2][2]
    # ... and every row equals a separate single run at that level
    for k in (0, 2):
        single = _results(_run(tmp_path, f"single{k}", gt_path, levels[k]))
        _check_row_against_results(rows[k], single)


def test_noised_registration_path(tmp_path, gt_file):
    gt_path, _ = gt_file
    folder = _run(tmp_path, "icp", gt_path, 0.01, initial=False)
    res = _results(folder)
    pcd = _read_pcd(folder / "noise_gt_map.pcd")
    assert len(pcd) == res["counts"][0] > 0
    assert float(res["RMSE/AC"][0]) > 0
