"""The C++ host's mesh_signed key on the MI355X: the MeshSigned line of map_results.txt and the topology and sign blocks of
mesh_distance.txt carry Engine.mesh_signed_distance's numbers, with gt_mesh_path and with the reconstructed ground-truth mesh; without
the key every output byte is what it was."""
import numpy as np
import pytest

import _mesh_sign_ref as S
from test_gpu_mesh_host import KEYS, MAXD, T, _lines, _run, _SKIP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    """a torus (closed: both signs occur) with noisy samples of it as the map, stored where the initial matrix brings it back"""
    import _mesh_ref as R

    v, tri = S.torus(24, 12, 2.0, 0.7)
    rng = np.random.default_rng(5)
    on_mesh = R.sample(v, tri, 6000, 1)[0] + rng.normal(0, 0.02, (6000, 3))
    est = (on_mesh - T[:3, 3]) @ T[:3, :3]
    gt = R.sample(v, tri, 5000, 2)[0]
    return v, tri, np.ascontiguousarray(est), np.ascontiguousarray(gt)


def _blocks(folder):
    by = {}
    for r in (ln.split() for ln in open(folder / "mesh_distance.txt").read().splitlines()):
        by.setdefault(r[0], []).append(r[1:])
    return by


def _check(out, sg, topo):
    line = [ln for ln in _lines(out) if ln.startswith("MeshSigned")]
    assert line == [f"MeshSigned mean-meanabs-inside-unreliable: {sg['mean_signed']:.5f} {sg['mean_abs']:.5f} {sg['inside_share']:.5f} "
                    f"{sg['unreliable_share']:.5f}"]
    order = [ln.split(":")[0] for ln in _lines(out)]
    assert order.index("MeshAC @t") + 1 == order.index("MeshSigned mean-meanabs-inside-unreliable") < order.index("VMD")
    by = _blocks(out)
    assert {r[0]: int(r[1]) for r in by["topology"]} == {k: int(x) for k, x in topo.items()}
    sign = {r[0]: r[1:] for r in by["sign"]}
    assert [int(x) for x in sign["counts"]] == [sg[k] for k in ("n_matched", "n_signed", "n_inside", "n_outside", "n_on", "n_unsigned",
                                                                "n_unreliable")]
    assert [int(x) for x in sign["regions"]] == sg["n_by_region"].tolist()
    n = sg["n_signed"]  # (a sum is formed in the order of the slot's index: n terms agree within n 2^-52 of the sum of the magnitudes)
    sums = [float(x) for x in sign["sums"]]
    assert abs(sums[0] - sg["sum_signed"]) <= n * 2.0 ** -52 * sg["sum_abs_signed"]
    assert abs(sums[1] - sg["sum_abs_signed"]) <= n * 2.0 ** -52 * sg["sum_abs_signed"]
    assert abs(sums[2] - sg["sum_signed2"]) <= n * 2.0 ** -52 * sg["sum_signed2"]
    assert [float(sign["extremes"][0]), int(sign["extremes"][1]), float(sign["extremes"][2]), int(sign["extremes"][3])] == [
        sg["min_signed"], sg["argmin"], sg["max_signed"], sg["argmax"]]


def test_line_and_blocks_equal_engine(scene, tmp_path):
    from cloud_map_evaluation_amd.engine import Engine

    v, tri, est, gt = scene
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.5)
        e.upload(1, gt, cell_size=0.5)
        e.transform_cloud(0, T)  # (the host's calls, in the host's order)
        e.mesh_upload(v, tri)
        e.mesh_distance(0, MAXD)
        topo = e.mesh_topology()
        sg = e.mesh_signed_distance(0, MAXD)
    assert topo["closed"] and topo["oriented_manifold"] and 0 < sg["n_matched"] < 6000 and sg["n_inside"] > 0 and sg["n_outside"] > 0
    out = _run(tmp_path, "on", scene, "evaluate_mesh_distance: true\nmesh_signed: true\n" + KEYS)
    _check(out, sg, topo)


def test_reconstructed_ground_truth_mesh(scene, tmp_path):
    """no gt_mesh_path: the map against the mesh the host reconstructs from the ground-truth cloud; the blocks are there and agree
    with the file's own totals (the numbers against Engine are the test above's)"""
    extra = ("evaluate_mesh_distance: true\nmesh_signed: true\nevaluate_mesh: true\nmesh_voxel_size: 0.25\nmesh_min_points: 4\n"
             f"mesh_max_distance: {MAXD}\n")
    out = _run(tmp_path, "recon", scene, extra)
    by = _blocks(out)
    nv, nt = int(by["vertices"][0][0]), int(by["triangles"][0][0])
    assert nt > 100 and (out / "gt_mesh.ply").exists()
    topo = {r[0]: int(r[1]) for r in by["topology"]}
    assert topo["n_edges"] > 0 and set(topo) == {"n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "n_zero_edges",
                                                 "n_zero_vertices", "n_tainted_vertices", "n_unreferenced_vertices", "closed", "oriented_manifold"}
    counts = [int(x) for x in {r[0]: r[1:] for r in by["sign"]}["counts"]]
    assert counts[0] == int(by["totals"][0][1]) and counts[1] + counts[5] == counts[0] and counts[1] == counts[2] + counts[3] + counts[4]
    assert len([ln for ln in _lines(out) if ln.startswith("MeshSigned")]) == 1 and nv > 0


def test_without_the_key_nothing_changes(scene, tmp_path):
    on = _run(tmp_path, "on", scene, "evaluate_mesh_distance: true\n" + KEYS)
    false = _run(tmp_path, "false", scene, "evaluate_mesh_distance: true\nmesh_signed: false\n" + KEYS)
    signed = _run(tmp_path, "signed", scene, "evaluate_mesh_distance: true\nmesh_signed: true\n" + KEYS)
    names = sorted(p.name for p in on.iterdir())
    assert sorted(p.name for p in false.iterdir()) == names == sorted(p.name for p in signed.iterdir())
    keep = lambda folder: [ln for ln in _lines(folder) if not any(s in ln for s in _SKIP)]
    assert keep(false) == keep(on) and not any(ln.startswith("MeshSigned") for ln in keep(on))
    assert [ln for ln in keep(signed) if not ln.startswith("MeshSigned")] == keep(on) and len(keep(signed)) == len(keep(on)) + 1
    for name in names:
        if name == "map_results.txt":
            continue
        assert (false / name).read_bytes() == (on / name).read_bytes(), name
        if name != "mesh_distance.txt":
            assert (signed / name).read_bytes() == (on / name).read_bytes(), name
    plain, more = (on / "mesh_distance.txt").read_bytes(), (signed / "mesh_distance.txt").read_bytes()
    assert more.startswith(plain) and more[len(plain):].startswith(b"topology n_edges ")
