"""Cost of me_mom and of its grouped radix select (k_gs_hist and friends, me_mom.hip) on the bench workload's map.  Prints one JSON line.

    python profiles/mom_cost.py [--points 50000000] [--workload c4_multisession] [--reps 5]

The map of bench.py's workload is uploaded, me_local_geometry runs at r = 0.1 and me_segment_planes extracts up to eight planes; then
me_mom is called reps + 1 times (the first call settles the allocations) with the device timers on.  "select_ms": timer "group_select"
per call (k_gs_init, k_gs_stat, the two reduction levels, eight histogram passes with their narrowing kernels, k_gs_out);
"gather_ms": timer "mom" (k_mom_gather); "call_ms": wall clock of the whole me_mom call, the result read back included.
Byte model of the select: k_gs_stat and each of the eight passes read the 8-byte key and the group byte of every point, 9 B per point
and pass, 81 B per point in all; "select_gbps" = 81 N / select time, next to the ~4 TB/s a streaming read reaches on this part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--workload", default="c4_multisession")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import bench
    from cloud_map_evaluation_amd.engine import Engine

    w = bench.WORKLOADS[a.workload]
    args = argparse.Namespace(workload=a.workload, points=a.points, density=w["density"])
    est, gt = bench.make_pair(args, torch.device("cuda:0"))
    del gt
    out = {"workload": a.workload, "points": int(est.shape[0]), "reps": a.reps}
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.1)
        lg = e.local_geometry(0, 0.1, 5)
        info, planes = e.segment_planes(0, 0.05, 1000, 8, 1000, seed=1)
        out["local_geometry"] = {"n_valid": lg["n_valid"], "mpv": lg["mpv"]}
        out["planes"] = {"n_planes": info["n_planes"], "n_labelled": info["n_labelled"]}
        e.timers_enable(True)
        select_ms, gather_ms, call_ms = [], [], []
        for _ in range(a.reps + 1):
            e.timers_reset()
            t0 = time.perf_counter()
            res = e.mom(0, min_axis_points=1000)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            select_ms.append(e.timer("group_select")[0])
            gather_ms.append(e.timer("mom")[0])
    n = out["points"]
    out["select_ms"] = [round(t, 4) for t in select_ms[1:]]
    out["gather_ms"] = [round(t, 4) for t in gather_ms[1:]]
    out["call_ms"] = [round(t, 4) for t in call_ms[1:]]
    out["select_bytes_per_point"] = 81
    out["select_gbps"] = [round(81 * n / (t * 1e-3) / 1e9, 1) for t in select_ms[1:]] if res["n_axes"] else []
    out["mom"] = {"n_axes": res["n_axes"], "n_directions": res["n_directions"], "mom_median": res["mom_median"], "mom_mean": res["mom_mean"],
                  "n_valid": [d["n_valid"] for d in res["axes"]], "n_points": [d["n_points"] for d in res["axes"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
