#!/usr/bin/env python3
"""Times the fused NDR T-NeRF field query (csrc/ndr_warp.h, nerf_field.hip WARP == 2; nerfacc_amd.fields.NDRTNeRFRadianceField)
against (a) the composed chain of the same module (`fused=False`) and (b) the fused VANILLA query at the same N, whose distance to
the fused NDR query is the warp stage's cost, in one process:
    python scripts/bench_ndr_field.py [--log2n 18 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5] [--table]
One JSON line per (query kind, dtype, N) on points, measured as scripts/bench_tnerf_field.py measures: the variants take turns
window by window; `*_us` is the median of the windows' means, `*_spread` their (min, max).  `vs_composed`: the composed chain's time
over the fused launch's; `warp_cost`: the fused NDR launch's time over the fused vanilla launch's (none for the warp alone);
`fused_wins`: the fused launch's slowest window is faster than the composed chain's fastest.  `--table` prints the rows again as the
markdown table of DESIGN.md ("Fused NDR field"), a row that does not win in **bold**."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_mlp_stream import measure  # noqa: E402
from nerfacc_amd.fields import NDRTNeRFRadianceField  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ndr_field.py measures on a GPU; none is available")
    dev, rows = torch.device("cuda"), []
    for dtype in (getattr(torch, d) for d in a.dtypes):
        fused = NDRTNeRFRadianceField(dtype=dtype, fused=True).to(dev)
        composed = NDRTNeRFRadianceField(dtype=dtype, fused=False).to(dev)
        composed.load_state_dict(fused.state_dict())
        vanilla = fused.nerf
        for log2n in a.log2n:
            N = 1 << log2n
            x, t = torch.rand(N, 3, device=dev) * 2 - 1, torch.rand(N, 1, device=dev)
            d = torch.nn.functional.normalize(torch.randn(N, 3, device=dev), dim=-1)
            for kind in ("full", "density", "warp"):
                query = lambda f: {"full": lambda: f(x, t, d), "density": lambda: f.query_density(x, t), "warp": lambda: f.warp(x, t)}[kind]
                passes = {"fused": query(fused), "composed": query(composed)}
                if kind != "warp":
                    passes["vanilla"] = (lambda: vanilla(x, d)) if kind == "full" else (lambda: vanilla.query_density(x))
                with torch.no_grad():
                    row = {"kind": kind, "dtype": str(dtype).split(".")[-1], "n_points": N}
                    row.update(measure(passes, a.window_ms, a.windows))
                row["vs_composed"] = round(row["composed_us"] / row["fused_us"], 2)
                row["warp_cost"] = round(row["fused_us"] / row["vanilla_us"], 3) if kind != "warp" else None
                row["fused_wins"] = row["fused_spread"][1] < row["composed_spread"][0]
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.table:
        print("| query | type | points | fused | composed chain | fused vanilla | vs composed | warp cost |\n|---|---|---|---|---|---|---|---|")
        for r in rows:
            us = lambda k: f"{r[k + '_us']:.0f} ({r[k + '_spread'][0]:.0f}, {r[k + '_spread'][1]:.0f})" if k + "_us" in r else "-"
            cells = [r["kind"], "fp16" if r["dtype"] == "float16" else "bf16", f"2^{r['n_points'].bit_length() - 1}", us("fused"), us("composed"),
                     us("vanilla"), f"{r['vs_composed']:.2f}x", "-" if r["warp_cost"] is None else f"{r['warp_cost']:.3f}"]
            print("| " + " | ".join(c if r["fused_wins"] else f"**{c}**" for c in cells) + " |")


if __name__ == "__main__":
    main()
