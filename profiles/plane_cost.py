"""Cost of me_segment_planes' scoring kernel (k_plane_score, me_plane.hip): point-plane tests per second next to the fp64 vector issue
bound.  Prints one JSON line.

    python profiles/plane_cost.py [--points 5000000] [--hyp 1000] [--reps 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/plane_cost.py --reps 1     (per-kernel device time, a run of its own)

Scene: three noisy orthogonal planes, 60 m a side, shuffled.  One plane is extracted (max_planes 1): k_plane_score runs once per call
over all N points and H hypotheses.  "score_ms": device timer "plane_score" per call after one settling call; "other_ms": timer "plane"
(compaction, hypotheses, winner, labels, moments, refit, residuals) without the stream compaction's own launches;
"tests_per_s" = N H / score time; "bound" = 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz / 7 fp64 vector instructions per test."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--hyp", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from cloud_map_evaluation_amd.engine import Engine

    n, H = a.points, a.hyp
    rng = np.random.default_rng(0)
    per = n // 3 + 1
    parts = []
    for axis in range(3):
        p = rng.uniform(0.0, 60.0, (per, 3))
        p[:, axis] = rng.normal(scale=0.02, size=per)
        parts.append(p)
    xyz = np.ascontiguousarray(np.concatenate(parts)[rng.permutation(3 * per)][:n])
    out = {"points": n, "hyp": H, "reps": a.reps}
    with Engine(0) as e:
        e.upload(0, xyz)
        e.timers_enable(True)
        score_ms, other_ms = [], []
        for _ in range(a.reps + 1):
            e.timers_reset()
            info, planes = e.segment_planes(0, 0.05, H, 1, 1000, seed=1)
            ms, launches = e.timer("plane_score")
            assert launches == 1
            score_ms.append(ms)
            other_ms.append(e.timer("plane")[0])
    out["score_ms"] = [round(t, 4) for t in score_ms[1:]]
    out["other_ms"] = [round(t, 4) for t in other_ms[1:]]
    out["tests_per_s"] = [n * H / (t * 1e-3) for t in score_ms[1:]]
    out["bound"] = 256 * 4 * 16 * 2.4e9 / 7
    out["best_fraction_of_bound"] = max(out["tests_per_s"]) / out["bound"]
    out["plane"] = {"count": planes[0]["count"], "rms": planes[0]["rms"], "h": planes[0]["h"], "n_valid_hypotheses": info["n_valid_hypotheses"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
