#!/usr/bin/env python3
"""Times the fused T-NeRF field query (csrc/nerf_field.hip, the WARP instantiations; nerfacc_amd.fields.TNeRFRadianceField)
against (a) the composed chain of the same module (`fused=False`: two SinusoidalEncoding, cat, FusedMLP, add, then the vanilla
field's composed chain), (b) the same field written as torch modules under `torch.autocast`, and (c) the fused VANILLA query
at the same N, whose distance to the fused T-NeRF query is the warp stage's cost, in one process:
    python scripts/bench_tnerf_field.py [--log2n 18 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5] [--table]
One JSON line per (query kind, input form, dtype, N), measured as scripts/bench_nerf_field.py measures: the four variants take
turns window by window; `*_us` is the median of the windows' means, `*_spread` their (min, max).  `vs_composed`, `vs_torch`:
the other variant's time over the fused launch's; `warp_cost`: the fused T-NeRF launch's time over the fused vanilla launch's;
`fused_wins`: the fused launch's slowest window is faster than the composed chain's fastest.  `--table` prints the rows again
as the markdown table of DESIGN.md ("Fused T-NeRF field"), a row that does not win in **bold**."""
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
from bench_nerf_field import TorchField  # noqa: E402
from nerfacc_amd.fields import TNeRFRadianceField  # noqa: E402


class TorchTNerf(nn.Module):
    """The reference's T-NeRF field in torch: the warp MLP (input appended after hidden layer 2) in front of TorchField."""

    def __init__(self, f: TNeRFRadianceField):
        super().__init__()
        self.nerf = TorchField(f.nerf)
        ws, bs = f.warp.linear_weights(), f.warp.linear_biases()
        self.layers = nn.ModuleList(nn.Linear(w.shape[1], w.shape[0]) for w in ws)
        with torch.no_grad():
            for lin, w, b in zip(self.layers, ws, bs):
                lin.weight.copy_(w), lin.bias.copy_(b)
        self.mask = f.warp.skip_mask
        self.register_buffer("s4", 2.0 ** torch.arange(4))

    def forward(self, x, t, d=None):
        row = torch.cat([TorchField.encode(x, self.s4), TorchField.encode(t, self.s4)], -1)
        h = row
        for l, lin in enumerate(self.layers):
            h = lin(torch.cat([h, row], -1) if (self.mask >> l) & 1 else h)
            if l < len(self.layers) - 1:
                h = torch.relu(h)
        return self.nerf(x + h.float(), d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    rows = []
    if not torch.cuda.is_available():
        raise SystemExit("bench_tnerf_field.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    for dtype in (getattr(torch, d) for d in a.dtypes):
        fused = TNeRFRadianceField(dtype=dtype).to(dev)
        composed = TNeRFRadianceField(dtype=dtype, fused=False).to(dev)
        composed.load_state_dict(fused.state_dict())
        ref = TorchTNerf(fused).to(dev)
        vanilla = fused.nerf
        for log2n in a.log2n:
            N = 1 << log2n
            n_rays = max(N // 128, 1)
            o, rd = torch.rand(n_rays, 3, device=dev) - 0.5, nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
            stamps = torch.rand(n_rays, 1, device=dev)
            ri = torch.arange(N, device=dev) // 128
            ts = (torch.arange(N, device=dev) % 128).float() * 0.01
            te = ts + 0.01
            x, d, t = o[ri] + rd[ri] * ((ts + te) / 2)[:, None], rd[ri], stamps[ri]
            for kind in ("full", "density"):
                for form in ("points", "rays"):
                    def query(f):
                        if form == "points":
                            return (lambda: f(x, t, d)) if kind == "full" else (lambda: f.query_density(x, t))
                        if kind == "full":
                            return lambda: f.query_on_rays(o, rd, ts, te, ri, stamps, raw=False)
                        return lambda: f.density_on_rays(o, rd, ts, te, ri, stamps)

                    def vanilla_query():
                        if form == "points":
                            return vanilla(x, d) if kind == "full" else vanilla.query_density(x)
                        if kind == "full":
                            return vanilla.query_on_rays(o, rd, ts, te, ri, raw=False)
                        return vanilla.density_on_rays(o, rd, ts, te, ri)

                    def torch_query():
                        with torch.autocast("cuda", dtype=dtype):
                            if form == "points":
                                return ref(x, t, d if kind == "full" else None)
                            xs = o[ri] + rd[ri] * ((ts + te) / 2)[:, None]
                            return ref(xs, stamps[ri], rd[ri] if kind == "full" else None)

                    passes = {"fused": query(fused), "composed": query(composed), "torch": torch_query, "vanilla": vanilla_query}
                    with torch.no_grad():
                        first = lambda y: (y[0] if isinstance(y, tuple) else y).float().reshape(N, -1)
                        diff = float((first(passes["fused"]()) - first(passes["torch"]())).abs().max())
                        row = {"kind": kind, "form": form, "dtype": str(dtype).split(".")[-1], "n_points": N, "max_abs_diff_vs_torch": diff}
                        row.update(measure(passes, a.window_ms, a.windows))
                    row["vs_composed"] = round(row["composed_us"] / row["fused_us"], 2)
                    row["vs_torch"] = round(row["torch_us"] / row["fused_us"], 2)
                    row["warp_cost"] = round(row["fused_us"] / row["vanilla_us"], 3)
                    row["fused_wins"] = row["fused_spread"][1] < row["composed_spread"][0]
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.table:
        print("| query | input | type | points | fused | composed chain | torch autocast | fused vanilla | vs composed | vs torch | warp cost |\n"
              "|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            us = lambda k: f"{r[k + '_us']:.0f} ({r[k + '_spread'][0]:.0f}, {r[k + '_spread'][1]:.0f})"
            cells = [r["kind"], r["form"], "fp16" if r["dtype"] == "float16" else "bf16", f"2^{r['n_points'].bit_length() - 1}", us("fused"),
                     us("composed"), us("torch"), us("vanilla"), f"{r['vs_composed']:.2f}x", f"{r['vs_torch']:.2f}x", f"{r['warp_cost']:.3f}"]
            print("| " + " | ".join(c if r["fused_wins"] else f"**{c}**" for c in cells) + " |")


if __name__ == "__main__":
    main()
