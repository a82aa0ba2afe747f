"""Cost of the outlier filters (me_outlier.hip) on the 50 M-point bench map, and of coarse alignment with the statistical filter in front
of it on the 50 M + 50 M bench pair (the map moved by a known large transform).  Prints one JSON line.

    python profiles/outlier_cost.py [--points 50000000] [--k 20] [--radius 0.1] [--nb-points 5] [--voxel 1.0] [--reps 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/outlier_cost.py --reps 1     (per-kernel device time, a run of its own)

"sor" / "ror": device timer "outlier" per pass (last rep), the statistical pass's fallback share (queries the octree walk settled) and
what was kept.  "coarse": what Engine.coarse_align(voxel, outlier_nb_neighbors=k) does, written out so that the timers of both contexts
can be read — SOR on both resident clouds ("outlier", first context), the kept points into the second context ("outlier_select"),
the in-place down-sample ("downsample", "sort"), normals, FPFH, matching, RANSAC and its re-scoring — and the error of T."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("outlier_select", "downsample", "normals", "fpfh", "fpfh_match", "ransac", "ransac_validate", "nn1", "sort")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--std-ratio", type=float, default=2.0)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--nb-points", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--iterations", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = synth.multisession_pair(a.points, device="cuda")  # bench.py's default workload (c4_multisession)
    yaw, roll, pitch = 2.5, 0.05, -0.04
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Tm = np.eye(4)
    Tm[:3, :3] = R
    Tm[:3, 3] = (40.0, -25.0, 3.0)
    Ttrue = np.linalg.inv(Tm)
    v = a.voxel
    out = {"scene": "c4_multisession", "points": a.points, "k": a.k, "std_ratio": a.std_ratio, "radius": a.radius,
           "nb_points": a.nb_points, "voxel": v, "iterations": a.iterations, "reps": a.reps}
    with Engine(0) as eng, Engine(0) as co:
        eng.upload(0, est, T=Tm, cell_size=0.2)
        eng.upload(1, gt, cell_size=0.2)
        del est, gt
        torch.cuda.synchronize()
        eng.timers_enable(True)
        co.timers_enable(True)
        sor_ms, ror_ms = [], []
        for r in range(a.reps + 1):
            eng.timers_reset()
            info = eng.statistical_outlier(0, a.k, a.std_ratio)
            sor_ms.append(eng.timer("outlier")[0])
        out["sor"] = {"outlier_ms": [round(t, 3) for t in sor_ms[1:]], "info": info,
                      "fallback_share": info["n_fallback"] / info["n_in"]}
        with Engine(0) as rr:  # (ROR rebuilds the slot's index at the radius: on a copy of the map, not on the pair used below)
            rr.upload(0, eng.download(0), cell_size=0.2)
            rr.timers_enable(True)
            for r in range(a.reps + 1):
                rr.timers_reset()
                info = rr.radius_outlier(0, a.nb_points, a.radius)
                ror_ms.append(rr.timer("outlier")[0])
            out["ror"] = {"outlier_ms": [round(t, 3) for t in ror_ms[1:]], "info": info}
        walls = []
        for r in range(a.reps + 1):
            eng.timers_reset()
            co.timers_reset()
            t0 = time.perf_counter()
            outl = []
            for s in (0, 1):
                outl.append(eng.statistical_outlier(s, a.k, a.std_ratio))
                eng.select_kept_into(s, co, s)
                co.voxel_downsample(s, v)
            T, info = co.global_register(0, 1, radius=5 * v, max_corr_dist=1.5 * v, max_iterations=a.iterations)
            walls.append((time.perf_counter() - t0) * 1e3)
        tm = {"outlier": round(eng.timer("outlier")[0], 3)}
        tm.update({s: round(co.timer(s)[0], 3) for s in STAGES})
        out["coarse"] = {"n_coarse": [co.size(0), co.size(1)], "filter": outl, "timers_ms_last_rep": tm,
                         "device_ms_last_rep": round(sum(tm.values()), 3), "call_ms": [round(w, 2) for w in walls[1:]], "info": info}
    dR = T[:3, :3] @ Ttrue[:3, :3].T
    out["coarse"]["rot_err_deg"] = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))
    out["coarse"]["trans_err_m"] = float(np.linalg.norm(T[:3, 3] - Ttrue[:3, 3]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
