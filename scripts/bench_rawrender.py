#!/usr/bin/env python3
"""Times nerfacc_amd.rawrender.rendering_from_raw (RenderRawFwdOp / RenderRawBwdOp of csrc/segscan.hip) with HIP events
against the torch composition it replaces -- trunc_exp(x - 1) * selector, sigmoid, then rendering() -- on the same inputs
in the same run, the two alternating, and prints one JSON line per size.
    python scripts/bench_rawrender.py [--reps 20] [--sizes 32200000,1000000]
Inputs: ray-sorted samples as sampling() returns them -- 30 % empty rays, the others 1..87 samples (31 per ray on
average, the headline workload's 32.2 M samples over 2^20 rays), about 20 % of the samples masked.  Forward alone (no
grad) and forward + backward towards the raw outputs with fixed upstream gradients at colors / opacities / depths.
`rendering()` on already activated values (the existing render_fused passes) is timed in the same run as the yardstick
of the two native passes.
Algorithmic bytes per sample: raw forward 12 (t_starts, t_ends, raw_sigma) + 12 (raw_rgb) + 1 (selector) + 12 (weights,
trans, alphas) = 37; raw backward 16 (t_starts, t_ends, raw_sigma, trans) + 12 (raw_rgb) + 1 + 16 (gradients) = 45;
render_fused forward 36, backward 44.  Per-ray arrays and packed_info are not counted.
    python scripts/bench_rawrender.py --dtype bfloat16 [--sizes 1048576,4194304] [--reps 20] [--windows 7]
times fp16 / bf16 raw inputs instead (nfa_render_raw_{fwd,bwd}_t: 29 B per sample each way) against what the same user
code runs without them -- `.float()` on both raw tensors, the float32 passes, and the cast's backward -- the two
alternating window by window in one process; each figure is the median over the windows."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd import rendering  # noqa: E402
from nerfacc_amd._segments import seginfo_from_ray_indices  # noqa: E402
from nerfacc_amd.rawrender import _TruncExp, rendering_from_raw  # noqa: E402

RAW_FWD_B, RAW_BWD_B, FUSED_FWD_B, FUSED_BWD_B = 37, 45, 36, 44


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


def half_rows(args, dev, dtype):
    import statistics
    for n in [int(s) for s in args.sizes.split(",")]:
        ts, te, raw_sig, raw_rgb, sel, ri, R = make_inputs(n, dev)
        seginfo_from_ray_indices(ri, R)
        rs, rc = raw_sig.to(dtype).requires_grad_(True), raw_rgb.to(dtype).requires_grad_(True)
        gout = [torch.randn(R, 3, device=dev), torch.randn(R, 1, device=dev), torch.randn(R, 1, device=dev)]

        def half(a, b):
            return rendering_from_raw(ts, te, b, a, ri, R, density_activation="trunc_exp", density_bias=-1.0,
                                      rgb_activation="sigmoid", selector=sel)[:3]

        def widened(a, b):
            return half(a.float(), b.float())

        def fwd(fn):
            with torch.no_grad():
                return fn(rs, rc)

        def both(fn):
            return torch.autograd.grad(fn(rs, rc), [rs, rc], gout)

        assert all(torch.equal(u, v) for u, v in zip(fwd(half), fwd(widened)))
        assert all(torch.equal(u, v) for u, v in zip(both(half), both(widened)))
        fns = {"half_fwd_ms": lambda: fwd(half), "f32_cast_fwd_ms": lambda: fwd(widened),
               "half_fwd_bwd_ms": lambda: both(half), "f32_cast_fwd_bwd_ms": lambda: both(widened)}
        times = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                times[k].append(timed(fn, args.reps))
        row = dict(n=n, n_rays=R, dtype=str(dtype), **{k: statistics.median(v) for k, v in times.items()})
        row["speedup_fwd"] = row["f32_cast_fwd_ms"] / row["half_fwd_ms"]
        row["speedup_fwd_bwd"] = row["f32_cast_fwd_bwd_ms"] / row["half_fwd_bwd_ms"]
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


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
    raw_sig = torch.randn(n, generator=g, device=dev) * 1.5
    raw_rgb = torch.randn(n, 3, generator=g, device=dev) * 2.0
    sel = torch.rand(n, generator=g, device=dev) > 0.2
    return ts, te, raw_sig, raw_rgb, sel, ri, n_rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="32200000,1000000")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16", "bfloat16"])
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rawrender.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B.load()
    if args.dtype != "float32":
        return half_rows(args, dev, getattr(torch, args.dtype))
    for n in [int(s) for s in args.sizes.split(",")]:
        ts, te, raw_sig, raw_rgb, sel, ri, R = make_inputs(n, dev)
        seginfo_from_ray_indices(ri, R)   # what sampling() attaches to the indices it returns
        rs, rc = raw_sig.clone().requires_grad_(True), raw_rgb.clone().requires_grad_(True)
        gout = [torch.randn(R, 3, device=dev), torch.randn(R, 1, device=dev), torch.randn(R, 1, device=dev)]

        def fused(a, b):
            return rendering_from_raw(ts, te, b, a, ri, R, density_activation="trunc_exp", density_bias=-1.0,
                                      rgb_activation="sigmoid", selector=sel)[:3]

        def composition(a, b):   # examples/radiance_fields/ngp.py:164,174-175,196 followed by rendering()
            sig = _TruncExp.apply(a - 1.0) * sel
            rgb = torch.sigmoid(b)
            return rendering(ts, te, ri, n_rays=R, rgb_sigma_fn=lambda *_: (rgb, sig))[:3]

        with torch.no_grad():   # activated once: the existing fused passes alone
            act_sig = (torch.exp(raw_sig - 1.0) * sel).requires_grad_(True)
            act_rgb = torch.sigmoid(raw_rgb).requires_grad_(True)

        def existing(a, b):
            return rendering(ts, te, ri, n_rays=R, rgb_sigma_fn=lambda *_: (b, a))[:3]

        def fwd(fn, a, b):
            with torch.no_grad():
                return fn(a, b)

        def both(fn, a, b):
            return torch.autograd.grad(fn(a, b), [a, b], gout)

        row = dict(n=n, n_rays=R)
        oa, ob = fwd(fused, rs, rc), fwd(composition, rs, rc)
        row["colors_max_abs_diff"] = float((oa[0] - ob[0]).abs().max())
        ga, gb = both(fused, rs, rc), both(composition, rs, rc)
        row["grad_sigma_max_rel_diff"] = float((ga[0] - gb[0]).abs().max() / gb[0].abs().max())
        row["grad_rgb_max_rel_diff"] = float((ga[1] - gb[1]).abs().max() / gb[1].abs().max())
        del oa, ob, ga, gb
        # the two implementations alternate; the fused one is timed a second time at the end
        r = args.reps
        row["fused_fwd_ms"] = timed(lambda: fwd(fused, rs, rc), r)
        row["torch_fwd_ms"] = timed(lambda: fwd(composition, rs, rc), r)
        row["fused_fwd_bwd_ms"] = timed(lambda: both(fused, rs, rc), r)
        row["torch_fwd_bwd_ms"] = timed(lambda: both(composition, rs, rc), r)
        row["existing_fwd_ms"] = timed(lambda: fwd(existing, act_sig, act_rgb), r)
        row["existing_fwd_bwd_ms"] = timed(lambda: both(existing, act_sig, act_rgb), r)
        row["fused_fwd_ms_again"] = timed(lambda: fwd(fused, rs, rc), r)
        row["fused_fwd_bwd_ms_again"] = timed(lambda: both(fused, rs, rc), r)
        row["torch_fwd_bwd_ms_again"] = timed(lambda: both(composition, rs, rc), r)
        row["fused_bwd_ms"] = row["fused_fwd_bwd_ms"] - row["fused_fwd_ms"]
        row["existing_bwd_ms"] = row["existing_fwd_bwd_ms"] - row["existing_fwd_ms"]
        row["fused_fwd_GBps"] = RAW_FWD_B * n / row["fused_fwd_ms"] / 1e6
        row["fused_bwd_GBps"] = RAW_BWD_B * n / row["fused_bwd_ms"] / 1e6
        row["existing_fwd_GBps"] = FUSED_FWD_B * n / row["existing_fwd_ms"] / 1e6
        row["existing_bwd_GBps"] = FUSED_BWD_B * n / row["existing_bwd_ms"] / 1e6
        row["speedup_fwd"] = row["torch_fwd_ms"] / row["fused_fwd_ms"]
        row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["fused_fwd_bwd_ms"]
        row["fused_below_composition"] = bool(max(row["fused_fwd_bwd_ms"], row["fused_fwd_bwd_ms_again"])
                                              < min(row["torch_fwd_bwd_ms"], row["torch_fwd_bwd_ms_again"]))
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
