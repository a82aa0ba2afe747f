"""Cost of me_perturb_cloud (the simulation mode's generators) on a 50 M-point cloud resident on the device, against the same four
stages composed from torch ops on the same device.  Prints one JSON line.

    python profiles/perturb_cost.py [--points 50000000] [--reps 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/perturb_cost.py --reps 3     (per-kernel device time, a run of its own)

`perturb_ms` is the library's "perturb" timer (HIP events around the three passes and the scan, without the index build of the result);
`call_ms` the whole call, index build included; `torch_ms` the torch composition (deform, rand + boolean-mask compaction, randn,
randint gather + randn), with torch's own generator: the same work, not the same numbers."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_stages(src, kw, gen):
    import torch

    p = src
    c = torch.tensor(kw["deform_center"], dtype=torch.float64, device=src.device)
    dv = p - c
    d = torch.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    m = (d < kw["deform_radius"]) & (d > 0)
    w = 0.5 * (1.0 + torch.cos(math.pi * d / kw["deform_radius"]))
    step = torch.where(m, kw["deform_strength"] * w / torch.where(m, d, torch.ones_like(d)), torch.zeros_like(d))
    p = p + dv * step[:, None]
    xn = torch.sin(p[:, 0] / kw["region_size"] * math.pi)
    yn = torch.sin(p[:, 1] / kw["region_size"] * math.pi)
    keep = torch.where(xn * yn > 0, kw["sparse_ratio"], kw["dense_ratio"])
    u = torch.rand(len(p), dtype=torch.float64, device=src.device, generator=gen)
    p = p[u < keep]
    p = p + kw["noise_std"] * torch.randn(p.shape, dtype=torch.float64, device=src.device, generator=gen)
    n_kept = len(p)
    mo = int(n_kept * kw["outlier_ratio"])
    b = torch.randint(0, n_kept, (mo,), device=src.device, generator=gen)
    outl = p[b] + kw["outlier_range"] * torch.randn((mo, 3), dtype=torch.float64, device=src.device, generator=gen)
    return torch.cat([p, outl])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    src = synth.campus_scene(a.points, seed=5, device="cuda")
    kw = dict(noise_std=0.05, sparse_ratio=0.5, dense_ratio=0.9, region_size=2.0, outlier_ratio=0.05, outlier_range=1.0,
              deform_radius=20.0, deform_strength=0.3, deform_center=tuple(src.mean(dim=0).tolist()))
    out = {"points": a.points, "reps": a.reps}
    with Engine(0) as eng:
        eng.upload(1, src, cell_size=0.2)
        for name, args in (("all", kw), ("noise_only", {"noise_std": 0.05})):
            eng.perturb(0, 1, seed=99, **args)  # warm-up
            eng.timers_enable(True)
            eng.timers_reset()
            t0 = time.perf_counter()
            for r in range(a.reps):
                n = eng.perturb(0, 1, seed=r, **args)
            call = (time.perf_counter() - t0) * 1e3 / a.reps
            ms, cnt = eng.timer("perturb")
            eng.timers_enable(False)
            out[name] = {"perturb_ms": ms / cnt, "call_ms": call, "n_out": n}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    torch_stages(src, kw, gen)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        res = torch_stages(src, kw, gen)
    e1.record()
    torch.cuda.synchronize()
    out["torch_ms"] = e0.elapsed_time(e1) / a.reps
    out["torch_n_out"] = len(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
