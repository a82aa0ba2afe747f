"""The C++ host's mesh_orient: propagate on the MI355X: a torus pair — which the default bounding-box viewpoint cannot orient — is
reconstructed onto the surface, reconstruction.txt carries the integers of me_orient_out that the model gives on the same normals,
and a configuration without the key writes exactly the bytes of one that names the default."""
import numpy as np
import pytest

import _orient_ref as R
from test_gpu_recon_host import _SKIP, _run

pytestmark = pytest.mark.gpu

N, MAJOR, MINOR = 8000, 4.0, 1.6  # the torus of test_orient_cpu.py, four times the size: ~25 points within nn_radius = 0.5
H, NR, K = 0.2, 0.5, 12
KEYS = f"evaluate_mesh: true\nmesh_voxel_size: {H}\nmesh_normal_radius: {NR}\n"


@pytest.fixture(scope="module")
def scene():
    return R.torus(N, 21, MAJOR, MINOR)[0], R.torus(N, 22, MAJOR, MINOR)[0]


def test_propagate_orients_both_clouds_and_reports_the_model_integers(scene, tmp_path):
    from cloud_map_evaluation_amd.engine import Engine

    out = _run(tmp_path, "propagate", scene, KEYS + f"mesh_orient: propagate\nmesh_orient_k: {K}\n")
    lines = open(out / "reconstruction.txt").read().splitlines()
    assert ["orient propagate", f"orient_k {K}", "orient_inward 0"] == [ln for ln in lines if ln.startswith("orient")]
    assert not any("viewpoint" in ln for ln in lines)
    got = {ln.split()[1].rstrip(":"): [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("Orientation ")}
    assert sorted(got) == ["est", "gt"]
    with Engine(0) as e:
        for slot, tag in ((0, "est"), (1, "gt")):
            e.upload(slot, scene[slot], cell_size=NR)
            e.radius_normals(slot, NR, 5, viewpoint=None)
            m = R.orient(scene[slot], e.get_normals(slot), K)
            assert got[tag] == [m[f] for f in R.FIELDS], tag
            assert m["n_components"] == 1 and m["n_inconsistent_edges"] == 0
    nv = int([ln for ln in lines if ln.startswith("gt n_vertices ")][0].split()[2])
    body = (out / "gt_mesh.ply").read_bytes().split(b"end_header\n", 1)[1]
    v = np.frombuffer(body[:nv * 24], dtype="<f8").reshape(nv, 3)
    d = R.torus_distance(v, MAJOR, MINOR)
    print(f"gt_mesh.ply: {nv} vertices, max distance to the torus {d.max():.4f} (voxel {H})")
    assert nv > 5000 and d.max() <= H


def test_without_the_key_the_bytes_are_those_of_the_named_default(scene, tmp_path):
    plain = _run(tmp_path, "plain", scene, KEYS)
    named = _run(tmp_path, "named", scene, KEYS + "mesh_orient: viewpoint\nmesh_orient_k: 7\nmesh_orient_inward: true\n")  # (unused by the default)
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in named.iterdir()) == names and "reconstruction.txt" in names
    keep = lambda folder: [ln for ln in open(folder / "map_results.txt").read().splitlines() if not any(s in ln for s in _SKIP)]
    assert keep(plain) == keep(named)
    for name in names:
        if name != "map_results.txt":
            assert (plain / name).read_bytes() == (named / name).read_bytes(), name
    txt = open(plain / "reconstruction.txt").read()
    assert "Orientation" not in txt and "orient" not in txt and "est viewpoint " in txt and "gt viewpoint " in txt
