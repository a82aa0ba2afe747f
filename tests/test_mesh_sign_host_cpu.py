"""The C++ host's mesh_signed key through --parse-config: default, value read, and the refusal that names the key.  No GPU needed."""
import json

from test_mesh_host_cpu import _parse


def test_default_is_off(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["mesh_signed"] is False


def test_key_is_read(tmp_path):
    ok = "evaluate_mesh_distance: true\ngt_mesh_path: /data/gt.ply\n"
    for text, want in (("true", True), ("false", False)):
        r = _parse(tmp_path, ok + f"mesh_signed: {text}\n")
        assert r.returncode == 0, r.stderr
        p = json.loads(r.stdout)
        assert p["mesh_signed"] is want and p["evaluate_mesh_distance"] is True
    # the reconstructed ground-truth mesh in place of a file
    r = _parse(tmp_path, "evaluate_mesh_distance: true\nevaluate_mesh: true\nmesh_voxel_size: 0.05\nmesh_signed: true\n")
    assert r.returncode == 0 and json.loads(r.stdout)["mesh_signed"] is True, r.stderr


def test_refused_by_name_without_the_mesh_distance(tmp_path):
    for extra in ("mesh_signed: true\n", "mesh_signed: true\nevaluate_mesh_distance: false\ngt_mesh_path: /data/gt.ply\n",
                  "mesh_signed: true\nevaluate_mesh: true\nmesh_voxel_size: 0.05\n"):
        r = _parse(tmp_path, extra)
        assert r.returncode != 0 and "mesh_signed" in r.stderr and "evaluate_mesh_distance" in r.stderr, (extra, r.stderr)
    assert _parse(tmp_path, "mesh_signed: false\n").returncode == 0  # off: nothing of it is judged
    r = _parse(tmp_path, "evaluate_mesh_distance: true\ngt_mesh_path: /data/gt.ply\nmesh_signed: true\nnum_gpus: 2\n")
    assert r.returncode != 0 and "single GPU only" in r.stderr
