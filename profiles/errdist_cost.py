"""Cost of me_nn_error_distribution and of its multi-rank radix select (k_rs_hist and friends, me_errdist.hip) on the bench workload's
map after the suite's map -> ground-truth search.  Prints one JSON line.

    python profiles/errdist_cost.py [--points 50000000] [--workload c4_multisession] [--reps 5]

Both clouds of bench.py's workload are uploaded and the map's 1-NN search runs; then, with the device timers on and reps + 1 calls
each (the first settles the allocations): "rank_select_1_ms" / "rank_select_16_ms": timer "rank_select" of a call with one quantile
(the median) and with sixteen; "errdist_ms": timer "errdist" (k_ed_stat, the one-block total, k_ed_hist with 1000 bins) of the same calls;
"group_select_ms": timer "group_select" of me_group_order_stats on the same squared distances as one group — the eight-full-pass
select, on the same box in the same run (its k_gs_prep included, as the upload is not).  "rank_select_direct_ms": timer "rank_select" of me_rank_select on the same array (its stat pass and the
select: the like-for-like figure beside "group_select").  "compactions" / "last_list": what the
select's compaction did.  Byte model: a pass over the uncompacted list reads 9 B per entry (key and use byte), a scatter reads the
same and writes 8 B per survivor, a pass over a compacted list 8 B per entry of that list; the eight-pass select reads 9 B per entry
in k_gs_stat and in each of its eight passes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q16 = [0.01, 0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95, 0.99, 0.999]


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
    out = {"workload": a.workload, "points": int(est.shape[0]), "reps": a.reps}
    taus = [0.2, 0.1, 0.08, 0.05, 0.01]
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        d2 = e.nn1(0, 1)[1]
        e.timers_enable(True)
        for name, q in (("rank_select_1_ms", [0.5]), ("rank_select_16_ms", Q16)):
            sel, ed = [], []
            for _ in range(a.reps + 1):
                e.timers_reset()
                r = e.nn_error_distribution(0, q, taus, 1000, 2.5 / 1000)
                sel.append(e.timer("rank_select")[0])
                ed.append(e.timer("errdist")[0])
            out[name] = [round(t, 4) for t in sel[1:]]
            out[name.replace("rank_select", "errdist")] = [round(t, 4) for t in ed[1:]]
            out[name.replace("_ms", "_compactions")] = [e.timer("rank_select_compactions")[1], e.timer("rank_select_list")[1]]
        out["result"] = {"n_used": r["n_used"], "max_d": r["max_d"], "median_d": float(r["quantile_d"][7]), "n_within": r["n_within"].tolist()}
        import numpy as np

        grp, gs = np.zeros(len(d2), np.int32), []
        for _ in range(a.reps + 1):
            e.timers_reset()
            g = e.group_order_stats(d2, grp, 1)
            gs.append(e.timer("group_select")[0])
        out["group_select_ms"] = [round(t, 4) for t in gs[1:]]
        direct = []
        for _ in range(a.reps + 1):  # me_rank_select on the same host array: its timer covers the stat pass AND the select, as "group_select" does
            e.timers_reset()
            rs = e.rank_select(d2, [(len(d2) - 1) // 2])
            direct.append(e.timer("rank_select")[0])
        out["rank_select_direct_ms"] = [round(t, 4) for t in direct[1:]]
        out["direct_agrees"] = bool(rs["value"][0] == g["lower"][0])
        out["medians_agree"] = bool(g["lower"][0] == r["quantile_d2"][7] or g["upper"][0] == r["quantile_d2"][7])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
