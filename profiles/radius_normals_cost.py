"""Cost of me_radius_normals next to me_local_geometry, and of me_nn_surface_error next to me_nn_error_distribution, on the 50 M-point
bench map.  Prints one JSON line.

    python profiles/radius_normals_cost.py [--points 50000000] [--radius 0.1] [--min-k 5] [--reps 3] [--parent-lib PATH]

"local_geom_ms" / "radius_normals_ms": device timers "local_geom" / "radius_normals" (the kernel and the two reduction launches) per
call after one settling call, alternating on the same resident cloud and grid.  --parent-lib: a libmapeval_hip.so built from the
parent commit; its me_local_geometry is measured in the same run, in a child process of its own (MAPEVAL_HIP_LIB), as
"parent_local_geom_ms".  "surface_ms" / "errdist_ms": device timers "surface" and "errdist" (no quantiles, five thresholds) on the
map's 1-NN result against the ground truth, which carries radius normals."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def local_geom_only(a):
    """The child of --parent-lib: me_local_geometry on the library MAPEVAL_HIP_LIB names, through a binding of its own that asks
    for the five entry points it calls and nothing else — a parent build lacks the newer symbols cloud_map_evaluation_amd._lib binds."""
    import ctypes as C

    import torch

    from cloud_map_evaluation_amd import synth

    L = C.CDLL(os.environ["MAPEVAL_HIP_LIB"])
    vp = C.c_void_p
    L.me_create.restype = vp
    L.me_create.argtypes = [C.c_int, C.c_int]
    L.me_destroy.argtypes = [vp]
    L.me_destroy.restype = None
    L.me_last_error.restype = C.c_char_p
    L.me_last_error.argtypes = [vp]
    L.me_upload_cloud_device.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_double]
    L.me_timers_enable.argtypes = [vp, C.c_int]
    L.me_timers_reset.argtypes = [vp]
    L.me_timer_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.me_local_geometry.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp]

    est = synth.multisession_pair(a.points, device="cuda")[0].to(torch.float64).contiguous()  # (the map alone)
    torch.cuda.synchronize()
    ctx = L.me_create(0, 0)
    if not ctx:
        raise RuntimeError("me_create failed")

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"[{rc}] " + L.me_last_error(ctx).decode())

    ck(L.me_upload_cloud_device(ctx, 0, est.data_ptr(), int(est.shape[0]), None, a.radius))
    torch.cuda.synchronize()
    ck(L.me_timers_enable(ctx, 1))
    ms = []
    for _ in range(a.reps + 1):
        ck(L.me_timers_reset(ctx))
        ck(L.me_local_geometry(ctx, 0, a.radius, a.min_k, None))
        t, c = C.c_double(), C.c_int64()
        ck(L.me_timer_get(ctx, b"local_geom", C.byref(t), C.byref(c)))
        ms.append(t.value)
    L.me_destroy(ctx)
    print(json.dumps({"local_geom_ms": [round(t, 3) for t in ms[1:]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--min-k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-local-geom", action="store_true", help="(the child of --parent-lib)")
    a = ap.parse_args()
    if a.only_local_geom:
        return local_geom_only(a)
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = synth.multisession_pair(a.points, device="cuda")  # bench.py's default workload (c4_multisession)
    out = {"scene": "c4_multisession", "points": int(est.shape[0]), "radius": a.radius, "min_k": a.min_k, "reps": a.reps}
    with Engine(0) as eng:
        eng.upload(0, est, cell_size=a.radius)
        del est
        torch.cuda.synchronize()
        eng.timers_enable(True)
        lg_ms, rn_ms = [], []
        for _ in range(a.reps + 1):
            eng.timers_reset()
            info = eng.local_geometry(0, a.radius, a.min_k)
            lg_ms.append(eng.timer("local_geom")[0])
            eng.timers_reset()
            rn = eng.radius_normals(0, a.radius, a.min_k)
            rn_ms.append(eng.timer("radius_normals")[0])
        out["local_geom_ms"] = [round(t, 3) for t in lg_ms[1:]]
        out["n_valid"] = info["n_valid"]
        out["radius_normals_ms"] = [round(t, 3) for t in rn_ms[1:]]
        out["radius_normals"] = rn
        eng.upload(1, gt, cell_size=a.radius)
        del gt
        eng.radius_normals(1, a.radius, a.min_k)
        eng.nn1(0, 1, fetch=False)
        sf_ms, ed_ms = [], []
        taus = (0.01, 0.02, 0.05, 0.1, 0.2)
        for _ in range(a.reps + 1):
            eng.timers_reset()
            sf = eng.nn_surface_error(0, taus, (5.0, 10.0, 20.0))
            sf_ms.append(eng.timer("surface")[0])
            eng.timers_reset()
            eng.nn_error_distribution(0, quantiles=(), thresholds=taus)
            ed_ms.append(eng.timer("errdist")[0])
        out["surface_ms"] = [round(t, 3) for t in sf_ms[1:]]
        out["errdist_ms"] = [round(t, 3) for t in ed_ms[1:]]
        out["surface"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in sf.items()}
    if a.parent_lib:
        env = dict(os.environ, MAPEVAL_HIP_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--only-local-geom", "--points", str(a.points), "--radius", str(a.radius),
               "--min-k", str(a.min_k), "--reps", str(a.reps)]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not line:
            sys.stderr.write(res.stderr[-4000:])
            raise SystemExit(f"the --parent-lib child failed (exit {res.returncode}): no parent figure, no result line")
        out["parent_local_geom_ms"] = json.loads(line[-1])["local_geom_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
