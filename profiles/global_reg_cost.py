"""Cost of the coarse global registration (me_globreg.hip) on the 50 M + 50 M bench pair: the map moved by a known large transform,
from resident clouds to T.  Prints one JSON line with the per-stage device timers and the error of T.

    python profiles/global_reg_cost.py [--points 50000000] [--voxel 1.0] [--iterations 1000000] [--reps 3] [--outlier-ratio 0]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/global_reg_cost.py --reps 1     (per-kernel device time, a run of its own)

What Engine.coarse_align does, written out so that the timers of the second context can be read: the two down-samples into a second
context (timer "downsample"), the normals ("normals"), FPFH ("fpfh"), matching ("fpfh_match"), RANSAC ("ransac") and the re-scoring of
the top hypotheses ("ransac_validate", whose 1-NN search counts to "nn1").  `call_ms` is the wall time of the whole pipeline.
On the bench pair the map carries 0.1 % sparse outliers (sigma 5 m): at 1 m voxels they are ~2 / 3 of the coarse map's points, isolated,
with empty or one-pair FPFH, and almost no feature match is true; --outlier-ratio 0 is the same scene without them."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("downsample", "normals", "fpfh", "fpfh_match", "ransac", "ransac_validate", "nn1", "sort")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--iterations", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outlier-ratio", type=float, default=None,
                    help="instead of the bench pair: scan_pair of the same scene with this share of sparse outliers in the map (0: none)")
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    if a.outlier_ratio is None:
        est, gt = synth.multisession_pair(a.points, device="cuda")  # bench.py's default workload (c4_multisession)
    else:
        est, gt = synth.scan_pair(a.points, device="cuda", outlier_ratio=a.outlier_ratio)
    yaw, roll, pitch = 2.5, 0.05, -0.04
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Tm = np.eye(4)
    Tm[:3, :3] = R
    Tm[:3, 3] = (40.0, -25.0, 3.0)
    Ttrue = np.linalg.inv(Tm)
    v = a.voxel
    out = {"scene": "c4_multisession" if a.outlier_ratio is None else f"scan_pair(outlier_ratio={a.outlier_ratio})", "points": a.points, "voxel": v, "iterations": a.iterations, "reps": a.reps}
    with Engine(0) as eng, Engine(0) as co:
        eng.upload(0, est, T=Tm, cell_size=0.2)
        eng.upload(1, gt, cell_size=0.2)
        del est, gt
        torch.cuda.synchronize()
        co.timers_enable(True)
        walls = []
        for r in range(a.reps + 1):
            co.timers_reset()
            t0 = time.perf_counter()
            ns = eng.downsample_into(0, co, 0, v)
            nr = eng.downsample_into(1, co, 1, v)
            T, info = co.global_register(0, 1, radius=5 * v, max_corr_dist=1.5 * v, max_iterations=a.iterations)
            walls.append((time.perf_counter() - t0) * 1e3)
        out["n_coarse"] = [ns, nr]
        out["timers_ms_last_rep"] = {s: round(co.timer(s)[0], 3) for s in STAGES}
        out["device_ms_last_rep"] = round(sum(out["timers_ms_last_rep"][s] for s in STAGES), 3)
        out["call_ms"] = [round(w, 2) for w in walls[1:]]  # (the first, with allocations, is not counted)
        out["info"] = info
    dR = T[:3, :3] @ Ttrue[:3, :3].T
    out["rot_err_deg"] = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))
    out["trans_err_m"] = float(np.linalg.norm(T[:3, 3] - Ttrue[:3, 3]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
