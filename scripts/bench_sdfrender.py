#!/usr/bin/env python3
"""Times nerfacc_amd.sdfrender.rendering_from_sdf (RenderSdfFwdOp / RenderSdfBwdOp of csrc/segscan.hip) with HIP events,
forward + backward, for both models, against
  * the torch composition it replaces -- neus_alpha or laplace_density in torch, sigmoid, then rendering() -- and
  * rendering_from_raw(density_activation="none") on the precomputed density: the same two passes without the
    conversion and without its extra streams, the floor that shows what the conversion costs inside the pass,
on the same inputs in one process, the three alternating window by window; prints one JSON line per model and size with
the median of every figure over the windows and its spread (min, max).
    python scripts/bench_sdfrender.py [--reps 10] [--windows 7] [--sizes 32200000]
Inputs: ray-sorted samples as sampling() returns them -- the packing of scripts/bench_rawrender.py: 30 % empty rays, the
others 1..87 samples (31 per ray on average, the headline workload's 32.2 M samples over 2^20 rays), about 20 % of the
samples masked; |sdf| <= 0.2, cos in [-1.2, 1.2], inv_s = 64 and beta = 0.05 as device tensors that require a gradient.
Gradients towards sdfs, cos (NeuS), raw_rgbs and the parameter, from fixed upstream gradients at colors / opacities /
depths.
Algorithmic bytes per sample, forward + backward (per-ray arrays and packed_info are not counted): the floor
37 + 45 = 82 (scripts/bench_rawrender.py); NeuS adds cos in each way and g_cos, g_param out: 98, and the 4 the sum of the
g_param stream reads: 102; VolSDF adds g_param out and that sum: 90.  `expected_ms` is the floor's time plus the extra
bytes at the floor's own rate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_rawrender import make_inputs, timed  # noqa: E402
from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd import rendering  # noqa: E402
from nerfacc_amd._segments import seginfo_from_ray_indices  # noqa: E402
from nerfacc_amd.rawrender import rendering_from_raw  # noqa: E402
from nerfacc_amd.sdfrender import laplace_density, neus_alpha, rendering_from_sdf  # noqa: E402

FLOOR_B = 37 + 45
STEP_B = {"neus": FLOOR_B + 16 + 4, "volsdf": FLOOR_B + 4 + 4}
INV_S, BETA, RATIO = 64.0, 0.05, 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="32200000")
    ap.add_argument("--models", default="neus,volsdf")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdfrender.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B.load()
    for n in [int(s) for s in args.sizes.split(",")]:
        ts, te, _, raw_rgb, sel, ri, R = make_inputs(n, dev)
        seginfo_from_ray_indices(ri, R)   # what sampling() attaches to the indices it returns
        g = torch.Generator(device=dev).manual_seed(1)
        sdf = (torch.rand(n, generator=g, device=dev) * 0.4 - 0.2).requires_grad_(True)
        cos = (torch.rand(n, generator=g, device=dev) * 2.4 - 1.2).requires_grad_(True)
        rc = raw_rgb.clone().requires_grad_(True)
        gout = [torch.randn(R, 3, device=dev), torch.randn(R, 1, device=dev), torch.randn(R, 1, device=dev)]
        for model in args.models.split(","):
            neus = model == "neus"
            p = torch.full((1,), INV_S if neus else BETA, device=dev, requires_grad=True)
            ins = [sdf, rc, p] + ([cos] if neus else [])

            def native():
                kw = dict(model="neus", inv_s=p, cos=cos, cos_anneal_ratio=RATIO) if neus else dict(model="volsdf", beta=p)
                return torch.autograd.grad(rendering_from_sdf(ts, te, rc, sdf, ri, R, selector=sel, **kw)[:3], ins, gout)

            def composition():
                rgb = torch.sigmoid(rc)
                if neus:
                    al = neus_alpha(sdf, cos, te - ts, p, RATIO) * sel
                    out = rendering(ts, te, ri, n_rays=R, rgb_alpha_fn=lambda *_: (rgb, al))[:3]
                else:
                    sig = laplace_density(sdf, p) * sel
                    out = rendering(ts, te, ri, n_rays=R, rgb_sigma_fn=lambda *_: (rgb, sig))[:3]
                return torch.autograd.grad(out, ins, gout)

            with torch.no_grad():   # the density that gives the same x, converted once
                if neus:
                    sig0 = -torch.log1p(-neus_alpha(sdf, cos, te - ts, p, RATIO)) / (te - ts)
                else:
                    sig0 = laplace_density(sdf, p)
            sig0.requires_grad_(True)

            def floor():
                out = rendering_from_raw(ts, te, rc, sig0, ri, R, density_activation="none", rgb_activation="sigmoid", selector=sel)[:3]
                return torch.autograd.grad(out, [sig0, rc], gout)

            row = dict(model=model, n=n, n_rays=R)
            ga, gb = native(), composition()
            for name, u, v in zip(["sdf", "rgb", "param"] + (["cos"] if neus else []), ga, gb):
                row[f"grad_{name}_max_rel_diff"] = float((u - v).abs().max() / v.abs().max())
            del ga, gb
            fns = {"native_ms": native, "torch_ms": composition, "floor_ms": floor}
            times = {k: [] for k in fns}
            for _ in range(args.windows):
                for k, fn in fns.items():
                    times[k].append(timed(fn, args.reps))
            for k, v in times.items():
                row[k] = statistics.median(v)
                row[k + "_min"], row[k + "_max"] = min(v), max(v)
            row["native_TBps"] = STEP_B[model] * n / row["native_ms"] / 1e9
            row["floor_TBps"] = FLOOR_B * n / row["floor_ms"] / 1e9
            row["expected_ms"] = row["floor_ms"] * STEP_B[model] / FLOOR_B
            row["speedup_over_torch"] = row["torch_ms"] / row["native_ms"]
            row["native_below_torch"] = bool(row["native_ms_max"] < row["torch_ms_min"])
            spread = max(row["native_ms_max"] - row["native_ms_min"], row["floor_ms_max"] - row["floor_ms_min"])
            row["native_within_spread_of_expected"] = bool(row["native_ms"] <= row["expected_ms"] + spread)
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
