#!/usr/bin/env python3
"""Times the plane grid's native passes against the torch composition K-Planes runs (one `grid_sample` per plane, the
products, autograd) on the K-Planes D-NeRF hybrid shape -- D = 4, resolution (64, 64, 64, 150), multiscale_res (1, 2, 4, 8),
F = 32, product -- and its static D = 3 part, at N uniform points, and prints one JSON line per (shape, N).
    python scripts/bench_planegrid.py [--log2n 18 20] [--window-ms 200] [--windows 5] [--features 32] [--reduce product]
Per line: the native forward (`fwd`), the native forward + backward towards the table and x, zeroing of the table gradient
included (`fwd_bwd`), and the same two through the composition (`torch_fwd`, `torch_fwd_bwd`), whose planes are copies of the
same parameters in K-Planes' own [1, F, H, W] layout.  The four take turns window by window in one process.  A window is as
many calls as fill `--window-ms` of device time (at least 3; counted once per pass from a timed probe after 3 warm-up
calls) between two HIP events; `*_us` is the median of the windows' means, `*_spread` their (min, max), `*_reps` the calls
per window.  `*_peak_mib`: the allocator's peak during one forward + backward of that form, above what was allocated
before it.  `bound`: per native pass, the bytes it cannot avoid and the time they need at the rates of the
hardware.  Forward: x, the output rows and each plane float once (or the gathered rows, if those are fewer) at the
measured HBM copy rate (6.29 TB/s); `fwd_gather_tbps` is the rate at which the corner rows (4 F bytes each, 4 per plane,
counted every time: most are served by a cache) were gathered, to be held against the gather rates of a table of this size.
Backward (`bwd_us` = `fwd_bwd_us` - `fwd_us`): x, dL/dx, dL/dy, the table read once and its gradient zeroed once at the
HBM rate, plus the table gradient's float atomics (one add per gathered float) at the chip-wide atomic rate (1.3 TB/s of
added bytes).  `*_bound_frac` = bound time / measured time."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

from nerfacc_amd.encodings import PlaneGridEncoding  # noqa: E402

HBM_BPS = 6.29e12      # measured float4 copy rate
ATOMIC_BPS = 1.3e12    # chip-wide rate of float atomic adds, in added bytes


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def composition(enc):
    """K-Planes' form of the same field: leaf [1, F, H, W] planes and a function of x in [0, 1]^D."""
    imgs = [[enc.plane(s, k).detach().permute(2, 0, 1)[None].contiguous().requires_grad_(True) for k in range(len(enc.planes))]
            for s in range(enc.n_scales)]

    def f(x):
        u = 2.0 * x - 1.0
        outs = []
        for row in imgs:
            acc = None
            for img, (a, b) in zip(row, enc.planes):
                v = TF.grid_sample(img, u[:, [a, b]][None, None], mode="bilinear", padding_mode="border",
                                   align_corners=True)[0, :, 0].t()
                acc = v if acc is None else (acc * v if enc.reduce == "product" else acc + v)
            outs.append(acc)
        return torch.cat(outs, -1)
    return f, [i for row in imgs for i in row]


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--reduce", default="product")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = {4: (64, 64, 64, 150), 3: (64, 64, 64)}
    ms = (1, 2, 4, 8)
    for D, res in shapes.items():
        torch.manual_seed(D)
        enc = PlaneGridEncoding(D, res, ms, n_features=a.features, reduce=a.reduce).to(dev)
        comp, leaves = composition(enc)
        for log2n in a.log2n:
            n = 1 << log2n
            x = torch.rand(n, D, device=dev).requires_grad_(True)
            gy = torch.randn(n, enc.n_output_dims, device=dev)

            def fwd():
                with torch.no_grad():
                    return enc(x)

            def fwd_bwd():
                return torch.autograd.grad(enc(x), (x, enc.params), gy)

            def torch_fwd():
                with torch.no_grad():
                    return comp(x)

            def torch_fwd_bwd():
                return torch.autograd.grad(comp(x), (x, *leaves), gy)
            passes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
            if not a.no_torch:
                passes.update(torch_fwd=torch_fwd, torch_fwd_bwd=torch_fwd_bwd)
                with torch.no_grad():   # the two forms compute the same thing at the size that is timed
                    err = float((enc(x) - comp(x)).abs().max())
            times, reps = {k: [] for k in passes}, {}
            for k, fn in passes.items():
                for _ in range(3):
                    fn()
                reps[k] = max(3, int(math.ceil(a.window_ms * 1e3 / timed(fn, 3))))
            for _ in range(a.windows):
                for k, fn in passes.items():
                    times[k].append(timed(fn, reps[k]))
            S, F, K = len(ms), a.features, len(enc.planes)
            rows = n * S * K * 4 * F * 4                      # gathered corner rows = floats added atomically, bytes
            out, table = n * S * F * 4, enc.params.numel() * 4
            fwd_bytes = {"x": n * D * 4, "y": out, "table_once": min(table, rows)}
            bwd_bytes = {"x": n * D * 4, "grad_x": n * D * 4, "grad_y": out, "table_once": min(table, rows), "zero_grad": table,
                         "atomic": rows}
            fwd_bound = sum(fwd_bytes.values()) / HBM_BPS * 1e6
            bwd_bound = ((sum(bwd_bytes.values()) - rows) / HBM_BPS + rows / ATOMIC_BPS) * 1e6
            row = {"n_dims": D, "n_points": n, "resolution": list(res), "multiscale_res": list(ms), "n_features": F,
                   "reduce": a.reduce, "n_params": enc.params.numel(), "window_ms": a.window_ms, "windows": a.windows}
            for k, v in times.items():
                row[k + "_us"] = round(float(np.median(v)), 1)
                row[k + "_spread"] = [round(min(v), 1), round(max(v), 1)]
                row[k + "_reps"] = reps[k]
            row["bwd_us"] = round(row["fwd_bwd_us"] - row["fwd_us"], 1)
            row["fwd_bwd_peak_mib"] = peak_mib(fwd_bwd)
            if not a.no_torch:
                row["torch_fwd_bwd_peak_mib"] = peak_mib(torch_fwd_bwd)
                row["fwd_ratio"] = round(row["torch_fwd_us"] / row["fwd_us"], 2)
                row["fwd_bwd_ratio"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
                row["max_abs_diff_vs_torch"] = err
            row["bound"] = {"fwd_bytes": fwd_bytes, "fwd_us": round(fwd_bound, 1), "bwd_bytes": bwd_bytes,
                            "bwd_us": round(bwd_bound, 1), "gathered_bytes": rows}
            row["fwd_gather_tbps"] = round(rows / row["fwd_us"] / 1e6, 2)
            row["bwd_atomic_tbps"] = round(rows / row["bwd_us"] / 1e6, 3)
            row["fwd_bound_frac"] = round(fwd_bound / row["fwd_us"], 3)
            row["bwd_bound_frac"] = round(bwd_bound / row["bwd_us"], 3)
            print(json.dumps(row), flush=True)
            del x, gy
        del enc, comp, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
