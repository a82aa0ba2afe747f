"""Cost of me_orient_normals (me_orient.hip) on a synth.campus_scene with unoriented radius normals, next to me_knn_search of the cloud
in itself at k + 1 (the same octree walk with the lists written out).  Prints one JSON line.

    python profiles/orient_cost.py [--points 1000000] [--k 12] [--radius 0.15] [--repeats 3]

One warm-up call, then `repeats` calls, each on freshly estimated (unoriented) normals so that every call does the same work.  Per call
the device timers "orient_normals" (the whole call), "orient_walk" (validity + the k-NN lists) and "orient_forest" (edges, Boruvka rounds,
roots, flips), the host's wall time and the Boruvka rounds; "knn_search_ms": device timer "knn_search" at k + 1 after a settling call.
"bytes_per_point": the buffers of the call, 20 (k + 1) + 38, from the allocation sizes in me_orient.hip."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--radius", type=float, default=0.15)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    pts = synth.campus_scene(a.points, device="cuda")
    out = {"scene": "campus_scene", "points": int(pts.shape[0]), "k": a.k, "normal_radius": a.radius, "bytes_per_point": 20 * (a.k + 1) + 38}
    with Engine(0) as eng:
        eng.upload(0, pts, cell_size=a.radius)
        del pts
        torch.cuda.synchronize()
        eng.timers_enable(True)
        calls = []
        for rep in range(a.repeats + 1):
            out["normals"] = eng.radius_normals(0, a.radius, 5, viewpoint=None)
            eng.timers_reset()
            t0 = time.perf_counter()
            d = eng.orient_normals(0, a.k)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:  # (the first call settles allocations and code loading)
                calls.append({"orient_normals_ms": round(eng.timer("orient_normals")[0], 3), "orient_walk_ms": round(eng.timer("orient_walk")[0], 3),
                              "orient_forest_ms": round(eng.timer("orient_forest")[0], 3), "wall_ms": round(wall, 3),
                              "rounds": eng.timer("orient_rounds")[1]})
        out["calls"] = calls
        out["orient"] = d
        knn = []
        for _ in range(2):
            eng.timers_reset()
            eng.knn_search(0, 0, a.k + 1)
            knn.append(round(eng.timer("knn_search")[0], 3))
        out["knn_search_ms"] = knn[1]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
