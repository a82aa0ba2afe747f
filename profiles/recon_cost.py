"""Cost of me_reconstruct (me_recon.hip) on a 5 M-point synth.campus_scene with radius normals, next to me_local_geometry at the same
radius on the same cloud (the nearest kernel of the same shape: a radius stream per query).  Prints one JSON line.

    python profiles/recon_cost.py [--points 5000000] [--voxel 0.05] [--band 1]

"recon_field_ms" / "recon_extract_ms" / "sort_ms": the device timers of the ONE reconstruct call; "wall_ms": that call on the host
(allocations of the first call included); "local_geom_ms": device timer "local_geom" of a call at radius 3 * voxel after a settling one;
"field_ns_per_pair" / "local_geom_ns_per_pair": device time per accepted (query, neighbour) pair (sum_k of each)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--band", type=int, default=1)
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    pts = synth.campus_scene(a.points, device="cuda")
    R = 3.0 * a.voxel
    lo, hi = pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()
    view = [float(0.5 * (lo[0] + hi[0])), float(0.5 * (lo[1] + hi[1])), float(hi[2] + 50.0)]
    out = {"scene": "campus_scene", "points": int(pts.shape[0]), "voxel": a.voxel, "radius": R, "band": a.band}
    with Engine(0) as eng:
        eng.upload(0, pts, cell_size=R)
        del pts
        torch.cuda.synchronize()
        eng.timers_enable(True)
        lg = []
        for _ in range(2):
            eng.timers_reset()
            info = eng.local_geometry(0, R, 5)
            lg.append(eng.timer("local_geom")[0])
        eng.timers_reset()
        nrm = eng.radius_normals(0, R, 5, viewpoint=view)
        out["radius_normals_ms"] = round(eng.timer("radius_normals")[0], 3)
        eng.timers_reset()
        t0 = time.perf_counter()
        d = eng.reconstruct(0, a.voxel, band=a.band, fetch=False)
        out["wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        field, extract, sort = eng.timer("recon_field")[0], eng.timer("recon_extract")[0], eng.timer("sort")[0]
        out.update(recon_field_ms=round(field, 3), recon_extract_ms=round(extract, 3), sort_ms=round(sort, 3), local_geom_ms=round(lg[1], 3))
        out["nodes_per_s"] = round(d["n_nodes"] / (field * 1e-3)) if field > 0 else 0
        out["field_ns_per_pair"] = round(field * 1e6 / max(d["sum_k"], 1), 4)
        out["local_geom_ns_per_pair"] = round(lg[1] * 1e6 / max(info["sum_k"], 1), 4)
        out["normals"] = nrm
        out["local_geom"] = {"n": info["n"], "n_valid": info["n_valid"], "sum_k": info["sum_k"]}
        out["recon"] = d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
