"""Cost of the ray kernels (me_ray.hip) on the mesh of DESIGN.md section 4.18's measurement: heightfield_mesh(708, 708, step 0.0502,
amplitude 0.3), 999 698 triangles, the ground under a synth.campus_scene.  Prints one JSON line.

    python profiles/raycast_cost.py [--rays 5000000] [--poses 200] [--beams 64] [--azimuth 1800] [--points 5000000] [--repeats 3]

Three workloads, each after one warm-up call, `repeats` calls, device timers and the host's wall time per call:
  cast        `rays` rays from 1 - 3 m above the mesh, tilted up to 45 degrees off the vertical: closest hit (timer "ray_cast") and any hit
              ("ray_occl"); the wall time includes the copies of the rays in and of the five result arrays out
  scan        `poses` poses on a closed loop 1.5 m above the mesh x lidar_directions(beams, azimuth, -25, 15): timer "scan" (trace + emit),
              wall time of the whole call including the slot's index build
  visibility  `points` mesh_sample points seen from the loop's `poses` origins, first_only, tolerance 0.02: timer "ray_occl", n_tests
Mrays/s are rays (or segments cast) per device-timer second."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=5_000_000)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=1800)
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    nx, step = 708, 0.0502
    v, tri = synth.heightfield_mesh(nx, nx, step, 0.3)
    ext = (nx - 1) * step
    out = {"mesh": f"heightfield_mesh({nx}, {nx}, {step}, 0.3)", "triangles": int(len(tri)), "repeats": a.repeats}
    rng = np.random.default_rng(1)
    o = np.stack([rng.uniform(0.1 * ext, 0.9 * ext, a.rays), rng.uniform(0.1 * ext, 0.9 * ext, a.rays), rng.uniform(1.0, 3.0, a.rays)], -1)
    d = np.stack([rng.uniform(-1.0, 1.0, a.rays), rng.uniform(-1.0, 1.0, a.rays), np.full(a.rays, -1.0)], -1)
    ang = 2.0 * math.pi * np.arange(a.poses) / a.poses
    P = np.tile(np.eye(4), (a.poses, 1, 1))
    P[:, 0, 3] = 0.5 * ext + 0.35 * ext * np.cos(ang)
    P[:, 1, 3] = 0.5 * ext + 0.35 * ext * np.sin(ang)
    P[:, 2, 3] = 1.5
    P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1] = -np.sin(ang), -np.cos(ang), np.cos(ang), -np.sin(ang)  # heading along the loop
    dirs = synth.lidar_directions(a.beams, a.azimuth, -25.0, 15.0)
    with Engine(0) as eng:
        eng.mesh_upload(v, tri)
        out["depth"] = eng.mesh_info()["depth"]
        eng.timers_enable(True)
        for name, timer, anyh in (("cast_closest", "ray_cast", False), ("cast_any", "ray_occl", True)):
            calls = []
            for rep in range(a.repeats + 1):
                eng.timers_reset()
                t0 = time.perf_counter()
                r = eng.mesh_raycast(o, d, any_hit=anyh)
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    ms = eng.timer(timer)[0]
                    calls.append({"ms": round(ms, 3), "wall_ms": round(wall, 3), "mrays_s": round(a.rays / ms / 1e3, 1)})
            out[name] = {"rays": a.rays, "n_hit": int(r["n_hit"]), "calls": calls}
        calls = []
        for rep in range(a.repeats + 1):
            eng.timers_reset()
            t0 = time.perf_counter()
            s = eng.mesh_scan(0, P, dirs, max_range=60.0)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                ms = eng.timer("scan")[0]
                calls.append({"ms": round(ms, 3), "wall_ms": round(wall, 3), "mrays_s": round(s["n_rays"] / ms / 1e3, 1)})
        out["scan"] = {"poses": a.poses, "dirs": int(len(dirs)), "n_rays": s["n_rays"], "n_hit": s["n_hit"], "calls": calls}
        eng.mesh_sample(1, a.points, seed=3)
        calls = []
        for rep in range(a.repeats + 1):
            eng.timers_reset()
            t0 = time.perf_counter()
            vis = eng.cloud_visibility(1, P[:, :3, 3], tolerance=0.02, first_only=True)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                ms = eng.timer("ray_occl")[0]
                calls.append({"ms": round(ms, 3), "wall_ms": round(wall, 3), "msegments_s": round(vis["n_tests"] / ms / 1e3, 1)})
        out["visibility"] = {"points": a.points, "origins": a.poses, "n_tests": vis["n_tests"], "n_visible": vis["n_visible"], "calls": calls}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
