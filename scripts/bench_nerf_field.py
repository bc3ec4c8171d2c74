#!/usr/bin/env python3
"""Times the fused NeRF field query (csrc/nerf_field.hip, nerfacc_amd.fields.VanillaNeRFRadianceField) against the composed
chain of the same module (`fused=False`: SinusoidalEncoding, StreamedMLP, split, cat, StreamedMLP, activations) and against the
same field written here as a torch sinusoidal encoder and `nn.Linear` / `ReLU` / `cat` under `torch.autocast`, in one process:
    python scripts/bench_nerf_field.py [--log2n 18 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5]
One JSON line per (query kind, input form, dtype, N): `full` is forward(x, d) -> (rgb, sigma), `density` is query_density(x);
`points` gives positions (and directions) per sample, `rays` packed ray samples with per-ray origins and directions (the torch
field then forms the midpoints and gathers the directions itself).  Measured as scripts/bench_mlp_stream.py measures: the
variants take turns window by window; a window is as many calls as fill `--window-ms` of device time between two HIP events;
`*_us` is the median of the windows' means, `*_spread` their (min, max).  `vs_composed` and `vs_torch` are the other variant's
time over the fused launch's (above 1 the fused launch is faster); `fused_wins` says whether the fused launch's slowest window
is faster than the composed chain's fastest, i.e. whether it is faster by more than the windows' spread.  `--table` prints the
rows again at the end as the markdown table of DESIGN.md ("Fused NeRF field"), a row that does not win in **bold**: `fused`
should default to off for that query kind."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from bench_mlp_stream import TorchNerf, measure  # noqa: E402
from nerfacc_amd.fields import VanillaNeRFRadianceField  # noqa: E402


class TorchField(nn.Module):
    """The reference's field in torch: sin(2^k x) and sin(2^k x + pi / 2) blocks behind x, then the two networks."""

    def __init__(self, f: VanillaNeRFRadianceField):
        super().__init__()
        self.net = TorchNerf(f.mlp)
        self.register_buffer("s10", 2.0 ** torch.arange(10))
        self.register_buffer("s4", 2.0 ** torch.arange(4))

    @staticmethod
    def encode(x, scales):
        xb = (x[:, None, :] * scales[:, None]).reshape(x.shape[0], -1)
        return torch.cat([x, torch.sin(torch.cat([xb, xb + 0.5 * torch.pi], -1))], -1)

    def forward(self, x, d=None):
        ex = self.encode(x, self.s10)
        if d is None:
            return torch.relu(self.net.trunk(ex)[:, self.net.W:])
        rgb, sigma = self.net(ex, self.encode(d, self.s4))
        return torch.sigmoid(rgb), torch.relu(sigma)


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
        raise SystemExit("bench_nerf_field.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    for dtype in (getattr(torch, d) for d in a.dtypes):
        fused = VanillaNeRFRadianceField(dtype=dtype).to(dev)
        composed = VanillaNeRFRadianceField(dtype=dtype, fused=False).to(dev)
        composed.load_state_dict(fused.state_dict())
        ref = TorchField(fused).to(dev)
        for log2n in a.log2n:
            N = 1 << log2n
            n_rays = max(N // 128, 1)
            o, rd = torch.rand(n_rays, 3, device=dev) - 0.5, nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
            ri = torch.arange(N, device=dev) // 128
            ts = (torch.arange(N, device=dev) % 128).float() * 0.01
            te = ts + 0.01
            x, d = o[ri] + rd[ri] * ((ts + te) / 2)[:, None], rd[ri]
            for kind in ("full", "density"):
                for form in ("points", "rays"):
                    def query(f):
                        if form == "points":
                            return (lambda: f(x, d)) if kind == "full" else (lambda: f.query_density(x))
                        if kind == "full":
                            return lambda: f.query_on_rays(o, rd, ts, te, ri, raw=False)
                        return lambda: f.density_on_rays(o, rd, ts, te, ri)

                    def torch_query():
                        with torch.autocast("cuda", dtype=dtype):
                            if form == "points":
                                return ref(x, d if kind == "full" else None)
                            xs = o[ri] + rd[ri] * ((ts + te) / 2)[:, None]
                            return ref(xs, rd[ri] if kind == "full" else None)

                    passes = {"fused": query(fused), "composed": query(composed), "torch": torch_query}
                    with torch.no_grad():
                        first = lambda y: (y[0] if isinstance(y, tuple) else y).float().reshape(N, -1)
                        diff = float((first(passes["fused"]()) - first(passes["torch"]())).abs().max())
                        row = {"kind": kind, "form": form, "dtype": str(dtype).split(".")[-1], "n_points": N, "max_abs_diff_vs_torch": diff}
                        row.update(measure(passes, a.window_ms, a.windows))
                    row["vs_composed"] = round(row["composed_us"] / row["fused_us"], 2)
                    row["vs_torch"] = round(row["torch_us"] / row["fused_us"], 2)
                    row["fused_wins"] = row["fused_spread"][1] < row["composed_spread"][0]
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.table:
        print("| query | input | type | points | fused | composed chain | torch autocast | vs composed | vs torch |\n|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            us = lambda k: f"{r[k + '_us']:.0f} ({r[k + '_spread'][0]:.0f}, {r[k + '_spread'][1]:.0f})"
            cells = [r["kind"], r["form"], "fp16" if r["dtype"] == "float16" else "bf16", f"2^{r['n_points'].bit_length() - 1}", us("fused"),
                     us("composed"), us("torch"), f"{r['vs_composed']:.2f}x", f"{r['vs_torch']:.2f}x"]
            print("| " + " | ".join(c if r["fused_wins"] else f"**{c}**" for c in cells) + " |")


if __name__ == "__main__":
    main()
