#!/usr/bin/env python3
"""Times the fused T-NeRF field's training pass (csrc/nerf_field.hip's WARP training forward, csrc/nerf_train.hip's WARP backward,
`TNeRFRadianceField(fused_training=True)`) against the composed chain of the same module (`fused_training=False`) and against the
same field in torch under `torch.autocast` (scripts/bench_tnerf_field.py: TorchTNerf), in one process:
    python scripts/bench_tnerf_train.py [--log2n 18 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5] [--table]
One JSON line per (pass, input form, dtype, N): `fwd` is forward(x, t, d) with grad enabled (everything the backward needs is
saved), `fwd_bwd` is that plus `backward()` of a sum of the outputs, the three networks' parameter gradients included; `points`
gives positions, times and directions per sample, `rays` packed ray samples with per-ray timestamps (the torch field then forms
the midpoints and gathers directions and times itself).  Measured as scripts/bench_nerf_train.py measures: the variants take
turns window by window; `*_us` is the median of the windows' means, `*_spread` their (min, max); `vs_composed` and `vs_torch`
are the other variant's time over the fused pass's; `fused_wins` says whether the fused pass's slowest window is faster than the
composed chain's fastest.  `--table` prints the rows again as the markdown table of DESIGN.md ("Fused T-NeRF field: training"), a
row that does not win in **bold**."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from bench_mlp_stream import measure  # noqa: E402
from bench_tnerf_field import TorchTNerf  # noqa: E402
from nerfacc_amd.fields import TNeRFRadianceField  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tnerf_train.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    rows = []
    for dtype in (getattr(torch, d) for d in a.dtypes):
        fused = TNeRFRadianceField(dtype=dtype, fused_training=True).to(dev)
        composed = TNeRFRadianceField(dtype=dtype).to(dev)
        composed.load_state_dict(fused.state_dict())
        ref = TorchTNerf(fused).to(dev)
        for log2n in a.log2n:
            N = 1 << log2n
            n_rays = max(N // 128, 1)
            o, rd = torch.rand(n_rays, 3, device=dev) - 0.5, nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
            stamps = torch.rand(n_rays, 1, device=dev)
            ri = torch.arange(N, device=dev) // 128
            ts = (torch.arange(N, device=dev) % 128).float() * 0.01
            te = ts + 0.01
            x, d, t = o[ri] + rd[ri] * ((ts + te) / 2)[:, None], rd[ri], stamps[ri]
            for form in ("points", "rays"):
                def query(f):
                    return (lambda: f(x, t, d)) if form == "points" else (lambda: f.query_on_rays(o, rd, ts, te, ri, stamps, raw=False))

                def torch_query():
                    with torch.autocast("cuda", dtype=dtype):
                        if form == "points":
                            return ref(x, t, d)
                        return ref(o[ri] + rd[ri] * ((ts + te) / 2)[:, None], stamps[ri], rd[ri])

                forward = {"fused": query(fused), "composed": query(composed), "torch": torch_query}
                for mode in ("fwd", "fwd_bwd"):
                    def with_backward(fn, mod):
                        def step():
                            rgb, sigma = fn()
                            (rgb.float().sum() + sigma.float().sum()).backward()
                            for p in mod.parameters():
                                p.grad = None
                        return step

                    passes = forward if mode == "fwd" else {k: with_backward(fn, m) for (k, fn), m in zip(forward.items(), (fused, composed, ref))}
                    row = {"pass": mode, "form": form, "dtype": str(dtype).split(".")[-1], "n_points": N}
                    row.update(measure(passes, a.window_ms, a.windows))
                    row["vs_composed"] = round(row["composed_us"] / row["fused_us"], 2)
                    row["vs_torch"] = round(row["torch_us"] / row["fused_us"], 2)
                    row["fused_wins"] = row["fused_spread"][1] < row["composed_spread"][0]
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.table:
        print("| pass | input | type | points | fused training | composed chain | torch autocast | vs composed | vs torch |\n|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            us = lambda k: f"{r[k + '_us']:.0f} ({r[k + '_spread'][0]:.0f}, {r[k + '_spread'][1]:.0f})"
            cells = [r["pass"], r["form"], "fp16" if r["dtype"] == "float16" else "bf16", f"2^{r['n_points'].bit_length() - 1}", us("fused"),
                     us("composed"), us("torch"), f"{r['vs_composed']:.2f}x", f"{r['vs_torch']:.2f}x"]
            print("| " + " | ".join(c if r["fused_wins"] else f"**{c}**" for c in cells) + " |")


if __name__ == "__main__":
    main()
