"""Cost of me_local_geometry (me_localgeom.hip) on the 50 M-point bench map, next to me_mme on the same resident cloud and grid.
Prints one JSON line.

    python profiles/localgeom_cost.py [--points 50000000] [--radius 0.1] [--min-k 5] [--reps 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/localgeom_cost.py --reps 1     (per-kernel device time, a run of its own)

"local_geom_ms": device timer "local_geom" (k_local_geom and the two reduction launches) per call after one settling call;
"mme_ms": device timer "mme" (k_mme3, min_k 10 as the map's MME) per call on the same cloud; "info": the result."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--min-k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    est, _ = synth.multisession_pair(a.points, device="cuda")  # bench.py's default workload (c4_multisession): the map
    out = {"scene": "c4_multisession", "points": int(est.shape[0]), "radius": a.radius, "min_k": a.min_k, "reps": a.reps}
    with Engine(0) as eng:
        eng.upload(0, est, cell_size=a.radius)
        del est
        torch.cuda.synchronize()
        eng.timers_enable(True)
        mme_ms, lg_ms = [], []
        for _ in range(a.reps + 1):
            eng.timers_reset()
            mme = eng.mme(0, a.radius, 10, per_point=False)
            mme_ms.append(eng.timer("mme")[0])
            eng.timers_reset()
            info = eng.local_geometry(0, a.radius, a.min_k)
            lg_ms.append(eng.timer("local_geom")[0])
        out["mme_ms"] = [round(t, 3) for t in mme_ms[1:]]
        out["local_geom_ms"] = [round(t, 3) for t in lg_ms[1:]]
        out["mme"] = {"mean": mme[0], "n_valid": mme[3]}
        out["info"] = info
    print(json.dumps(out))


if __name__ == "__main__":
    main()
