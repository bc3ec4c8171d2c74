#!/usr/bin/env python3
"""Times the fused training pass of the Instant-NGP fields (fused_training=True: csrc/ngp_field.hip, one launch forward, one
launch backward plus the networks' weight-gradient passes) against the composed chain of the SAME module with grad enabled, and
prints one JSON line per (field, N).
    python scripts/bench_ngp_train.py [--log2n 18 20 22] [--window-ms 200] [--windows 5]
Method and points (64 consecutive samples on each ray through the box) are scripts/bench_ngp_field.py's: the paths take turns
window by window, `*_us` is the median of the windows' means, `*_spread` their (min, max).  `fwd`: the query with grad enabled
(what it saves included); `fb`: the query and torch.autograd.backward with fixed output gradients into all parameters;
`fused_fb_noscatter`: the same with the table frozen, so the backward launch gets no grad_table and skips dEnc and the atomics
(the difference to `fused_fb` is the scatter's share, the zero fill of the table gradient included).  Ratios are the composed
chain's time over the fused one (above 1: the fused pass is faster).  Fields: `radiance/full` = NGPRadianceField.forward (16
levels, 2^19 entries, finest resolution 4096), `proposal/density` = NGPDensityField.forward (5 levels, 2^17 entries, 128); fp16."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bench_ngp_field import AABB, measure, ray_points, stream_gbps  # noqa: E402
from nerfacc_amd.fields import NGPDensityField, NGPRadianceField  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20, 22])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    gbps = stream_gbps(dev)
    rad = NGPRadianceField(AABB, fused_training=True).to(dev)
    prop = NGPDensityField(AABB, fused_training=True).to(dev)
    with torch.no_grad():
        for f in (rad, prop):
            f.encoding.params.uniform_(-0.5, 0.5)
    for log2n in args.log2n:
        n = 1 << log2n
        x, d = ray_points(n, dev, gen)
        g_rgb, g_den = torch.randn(n, 3, generator=gen, device=dev), torch.randn(n, 1, generator=gen, device=dev)
        for name, field, query, gs in (("radiance/full", rad, lambda: rad(x, d), (g_rgb, g_den)),
                                       ("proposal/density", prop, lambda: (prop(x),), (g_den,))):
            def run(fused, backward, table=True):
                def fn():
                    field.fused_training = fused
                    field.encoding.params.requires_grad_(table)
                    outs = query()
                    if backward:
                        for p in field.parameters():
                            p.grad = None
                        torch.autograd.backward(outs, gs)
                    field.encoding.params.requires_grad_(True)
                return fn
            row = {"query": name, "n": n, "stream_gbps": round(gbps, 1)}
            row.update(measure({"fused_fwd": run(True, False), "composed_fwd": run(False, False), "fused_fb": run(True, True),
                                "composed_fb": run(False, True), "fused_fb_noscatter": run(True, True, False)},
                               args.window_ms, args.windows))
            row["fwd_ratio"] = round(row["composed_fwd_us"] / row["fused_fwd_us"], 2)
            row["fb_ratio"] = round(row["composed_fb_us"] / row["fused_fb_us"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
