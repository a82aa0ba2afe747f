"""Cost of DBSCAN clustering (me_cluster.hip) on the 50 M-point bench map against the radius filter's pass at the same radius, measured
in ONE process: me_radius_outlier(r = eps) and me_cluster_dbscan(eps, min_points) for every eps, device timers, the median of --reps
calls after one warm-up call each.  Prints one JSON line.

    python profiles/cluster_cost.py [--points 50000000] [--eps 0.05 0.1] [--min-points 10] [--reps 5] [--out profiles/cluster_cost.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/cluster_cost.py --reps 1      (per-kernel device time, a run of its own)

"radius_ms": timer "outlier" of the radius pass (k_radius_count).  "cluster_ms": timer "cluster" (the kernels of me_cluster.hip) and
"cluster_sort_ms": timer "sort" of the same call (the roots' radix sort); "ratio" = (cluster + sort) / radius.  The index is built at eps
before the timed calls (both rebuild it when the cell differs), so no call pays for it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--eps", type=float, nargs="+", default=[0.05, 0.1])
    ap.add_argument("--min-points", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    est, _ = synth.multisession_pair(a.points, device="cuda")  # bench.py's default workload (c4_multisession)
    out = {"scene": "c4_multisession", "points": a.points, "min_points": a.min_points, "reps": a.reps, "runs": []}
    with Engine(0) as eng:
        eng.upload(0, est, cell_size=0.2)
        del est
        torch.cuda.synchronize()
        eng.timers_enable(True)
        for eps in a.eps:
            rad, clu, srt = [], [], []
            for r in range(a.reps + 1):  # (call 0: warm-up, and the index rebuild at eps)
                eng.timers_reset()
                ri = eng.radius_outlier(0, 5, eps)
                rad.append(eng.timer("outlier")[0])
            for r in range(a.reps + 1):
                eng.timers_reset()
                ci = eng.cluster_dbscan(0, eps, a.min_points)
                clu.append(eng.timer("cluster")[0])
                srt.append(eng.timer("sort")[0])
            rm, cm, sm = statistics.median(rad[1:]), statistics.median(clu[1:]), statistics.median(srt[1:])
            out["runs"].append({"eps": eps, "radius_ms": round(rm, 3), "cluster_ms": round(cm, 3), "cluster_sort_ms": round(sm, 3),
                                "ratio": round((cm + sm) / rm, 3), "radius_ms_all": [round(t, 3) for t in rad[1:]],
                                "cluster_ms_all": [round(t, 3) for t in clu[1:]], "cluster_info": ci, "radius_kept": ri["n_kept"]})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
