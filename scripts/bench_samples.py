#!/usr/bin/env python3
"""Times nerfacc_amd.samples.sample_positions (csrc/samples.hip forward, SamplePosBwdOp of csrc/segscan.hip backward)
with HIP events against the torch composition it replaces, on the same inputs in the same run, and prints one JSON line
per case.
    python scripts/bench_samples.py [--reps 20] [--sizes 32200000,1000000]
Inputs: ray-sorted samples as sampling() returns them -- 30 % empty rays, the others 1..87 samples (31 per ray on
average, the headline workload's 32.2 M samples over 2^20 rays), t increasing along each ray.
Cases: aabb=None; aabb + selector; sphere contraction + "unit" dirs + selector.  Forward, and forward + backward towards
rays_o and rays_d (camera-pose optimisation) with a fixed upstream gradient.
Algorithmic bytes per sample: forward 8 (ray index) + 8 (t_starts, t_ends) + 12 (positions) [+ 12 dirs] [+ 1 selector];
backward 8 (t_starts, t_ends) + 12 (g_positions) [+ 12 g_dirs]; the ray rows (24 B per ray, read from cache), packed_info
and the per-ray gradients are not counted.  The fraction is of the 8 TB/s HBM peak (6.3 TB/s is what streaming reaches)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd._segments import seginfo_from_ray_indices  # noqa: E402
from nerfacc_amd.samples import sample_positions  # noqa: E402

HBM_PEAK = 8.0e12
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]


def timed(fn, reps):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps   # ms


def make_inputs(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    n_rays = max(1, round(n / 30.8))
    counts = torch.randint(1, 88, (n_rays,), generator=g, device=dev)
    counts = torch.where(torch.rand(n_rays, generator=g, device=dev) < 0.3, torch.zeros_like(counts), counts)
    ri = torch.repeat_interleave(torch.arange(n_rays, device=dev), counts)
    if ri.numel() < n:   # top up the last ray
        ri = torch.cat([ri, torch.full((n - ri.numel(),), n_rays - 1, device=dev)])
    ri = ri[:n].contiguous()
    starts = torch.cumsum(counts, 0) - counts
    k = torch.arange(n, device=dev) - starts[ri]
    ts = (0.05 + k * (3.4 / 88)).float()
    te = ts + 3.4 / 88
    o = (torch.rand(n_rays, 3, generator=g, device=dev) - 0.5) * 0.5
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g, device=dev), dim=-1)
    return o, d, ts, te, ri, n_rays


def torch_composition(o, d, ts, te, ri, aabb, contraction, dirs, selector):
    """What the reference's trainers and fields run (examples/utils.py:83-85, ngp.py:42-66,158-164,185)."""
    t_origins = o[ri]
    t_dirs = d[ri]
    x = t_origins + t_dirs * (ts + te)[:, None] / 2.0
    sel = None
    if aabb is not None:
        aabb_min, aabb_max = torch.split(aabb, 3, dim=-1)
        x = (x - aabb_min) / (aabb_max - aabb_min)
        if contraction:
            x = x * 2 - 1
            mag = torch.linalg.norm(x, ord=2, dim=-1, keepdim=True)
            # (the reference assigns through a boolean mask, in place: that cannot be differentiated w.r.t. x and
            #  synchronises; torch.where is the form that serves both directions)
            x = torch.where(mag > 1, (2 - 1 / mag) * (x / mag), x)
            x = x / 4 + 0.5
        if selector:
            sel = ((x > 0.0) & (x < 1.0)).all(dim=-1)
    return x, ((t_dirs + 1.0) / 2.0 if dirs else None), sel


CASES = {
    "none": dict(aabb=False, contraction=None, dirs=None, selector=False),
    "aabb_selector": dict(aabb=True, contraction=None, dirs=None, selector=True),
    "sphere_unit_selector": dict(aabb=True, contraction="sphere", dirs="unit", selector=True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="32200000,1000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_samples.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B.load()
    for n in [int(s) for s in args.sizes.split(",")]:
        o, d, ts, te, ri, n_rays = make_inputs(n, dev)
        seginfo_from_ray_indices(ri, n_rays)   # what sampling() attaches to the indices it returns
        box = torch.tensor(AABB, device=dev)
        og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        for cname, cfg in CASES.items():
            kw = dict(aabb=AABB if cfg["aabb"] else None, contraction=cfg["contraction"], dirs=cfg["dirs"], selector=cfg["selector"])
            tkw = dict(aabb=box if cfg["aabb"] else None, contraction=cfg["contraction"], dirs=cfg["dirs"], selector=cfg["selector"])
            gx = torch.randn(n, 3, device=dev)
            gd = torch.randn(n, 3, device=dev) if cfg["dirs"] else None
            fwd_b = 16 + 12 + (12 if cfg["dirs"] else 0) + (1 if cfg["selector"] else 0)
            bwd_b = 8 + 12 + (12 if cfg["dirs"] else 0)
            row = dict(case=cname, n=n, n_rays=n_rays, fwd_bytes_per_sample=fwd_b, bwd_bytes_per_sample=bwd_b)

            def fused_fwd():
                with torch.no_grad():
                    return sample_positions(o, d, ts, te, ri, **kw)

            def torch_fwd():
                with torch.no_grad():
                    return torch_composition(o, d, ts, te, ri, **tkw)

            def both(fn, **k):
                out = fn(og, dg, ts, te, ri, **k)
                outs, gs = [out[0]], [gx]
                if gd is not None:
                    outs.append(out[1])
                    gs.append(gd)
                return torch.autograd.grad(outs, [og, dg], gs)

            a, b = fused_fwd(), torch_fwd()
            row["fwd_max_abs_diff"] = float((a.positions - b[0]).abs().max())
            row["selector_mismatches"] = int((a.selector != b[2]).sum()) if cfg["selector"] else 0
            ga, gb = both(sample_positions, **kw), both(torch_composition, **tkw)
            row["grad_o_max_rel_diff"] = float((ga[0] - gb[0]).abs().max() / gb[0].abs().max())
            row["grad_d_max_rel_diff"] = float((ga[1] - gb[1]).abs().max() / gb[1].abs().max())
            del a, b, ga, gb
            # alternate the two implementations
            row["fused_fwd_ms"] = timed(fused_fwd, args.reps)
            row["torch_fwd_ms"] = timed(torch_fwd, max(3, args.reps // 4))
            row["fused_fwd_bwd_ms"] = timed(lambda: both(sample_positions, **kw), args.reps)
            row["torch_fwd_bwd_ms"] = timed(lambda: both(torch_composition, **tkw), max(3, args.reps // 4))
            row["fused_fwd_ms_again"] = timed(fused_fwd, args.reps)
            row["fused_bwd_ms"] = row["fused_fwd_bwd_ms"] - row["fused_fwd_ms"]
            row["fused_fwd_GBps"] = fwd_b * n / row["fused_fwd_ms"] / 1e6
            row["fused_fwd_frac_hbm_peak"] = row["fused_fwd_GBps"] * 1e9 / HBM_PEAK
            row["fused_bwd_GBps"] = bwd_b * n / row["fused_bwd_ms"] / 1e6
            row["fused_bwd_frac_hbm_peak"] = row["fused_bwd_GBps"] * 1e9 / HBM_PEAK
            row["torch_fwd_GBps_same_bytes"] = fwd_b * n / row["torch_fwd_ms"] / 1e6
            row["speedup_fwd"] = row["torch_fwd_ms"] / row["fused_fwd_ms"]
            row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["fused_fwd_bwd_ms"]
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del gx, gd


if __name__ == "__main__":
    main()
