#!/usr/bin/env python3
"""Times `vm_regularization` (total variation, L1 and the orthogonality penalty of the VM tables: csrc/vmreg.hip) against the
same formulas in torch (`losses._vm_terms_torch`: slice differences, squares, means and a matmul per mode, autograd) on the
same GPU, on TensoRF's shapes -- resolution 300^3 and 128^3, C = 16 (density) and C = 48 (appearance) -- and prints one JSON
line per shape.
    python scripts/bench_vmreg.py [--window-ms 200] [--windows 5] [--no-torch]
Per line: the native forward (`fwd`, under no_grad), the native forward + backward into `params.grad`-sized storage
(`fwd_bwd`), and the same two through torch (`torch_fwd`, `torch_fwd_bwd`) on the same parameters, all four weights non-zero.
The four take turns window by window in one process.  A window is as many calls as fill `--window-ms` of device time (at
least 3; counted once per pass from a timed probe after 3 warm-up calls) between two HIP events; `*_us` is the median of the
windows' means, `*_spread` their (min, max), `*_reps` the calls per window.  `bwd_us` = `fwd_bwd_us` - `fwd_us`.
`*_peak_mib`: the allocator's peak during one forward + backward of that form, above what was allocated before it.
`bound`: the bytes a pass cannot avoid -- the table read once forward, read once and its gradient written once backward --
and the time they take at the measured HBM copy rate (6.29 TB/s); `fwd_tbps` / `bwd_tbps` are those bytes over the measured
times (achieved rates of the minimum traffic, not of the traffic the kernels cause: halo rows and neighbour nodes are read
again, mostly from a cache; the times include the second launch with the Gram matrices and the weighting in torch),
`*_bound_frac` = bound time / measured time.  `max_rel_diff_vs_torch`: the two forms' losses at the size that is timed."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd import losses  # noqa: E402
from nerfacc_amd.encodings import VMGridEncoding  # noqa: E402

HBM_BPS = 6.29e12      # measured float4 copy rate
WEIGHTS = dict(tv=2e-3, l1=8e-5, tv_line=1e-3, ortho=1e-2)
SHAPES = [((300, 300, 300), 48), ((300, 300, 300), 16), ((128, 128, 128), 48), ((128, 128, 128), 16)]


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


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
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vmreg.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    for res, C in SHAPES:
        torch.manual_seed(C)
        enc = VMGridEncoding(res, n_components=C).to(dev)   # TensoRF's initial table: 0.1 randn
        w = losses._vm_weights(enc, WEIGHTS["tv"], WEIGHTS["l1"], WEIGHTS["tv_line"], WEIGHTS["ortho"])

        def native():
            return losses.vm_regularization(enc, **WEIGHTS)

        def composed():
            return (losses._vm_terms_torch(enc.params, enc.table) * w).sum()

        def no_grad(f):
            def g():
                with torch.no_grad():
                    return f()
            return g

        def with_grad(f):
            return lambda: torch.autograd.grad(f(), enc.params)
        passes = {"fwd": no_grad(native), "fwd_bwd": with_grad(native)}
        if not a.no_torch:
            passes.update(torch_fwd=no_grad(composed), torch_fwd_bwd=with_grad(composed))
            with torch.no_grad():
                x, y = float(native()), float(composed())
            err = abs(x - y) / abs(y)
        times, reps = {k: [] for k in passes}, {}
        for k, fn in passes.items():
            for _ in range(3):
                fn()
            reps[k] = max(3, int(math.ceil(a.window_ms * 1e3 / timed(fn, 3))))
        for _ in range(a.windows):
            for k, fn in passes.items():
                times[k].append(timed(fn, reps[k]))
        table = enc.params.numel() * 4
        row = {"resolution": list(res), "n_components": C, "n_params": enc.params.numel(), "weights": WEIGHTS,
               "window_ms": a.window_ms, "windows": a.windows}
        for k, v in times.items():
            row[k + "_us"] = round(float(np.median(v)), 1)
            row[k + "_spread"] = [round(min(v), 1), round(max(v), 1)]
            row[k + "_reps"] = reps[k]
        row["bwd_us"] = round(row["fwd_bwd_us"] - row["fwd_us"], 1)
        row["fwd_bwd_peak_mib"] = peak_mib(passes["fwd_bwd"])
        if not a.no_torch:
            row["torch_bwd_us"] = round(row["torch_fwd_bwd_us"] - row["torch_fwd_us"], 1)
            row["torch_fwd_bwd_peak_mib"] = peak_mib(passes["torch_fwd_bwd"])
            row["fwd_ratio"] = round(row["torch_fwd_us"] / row["fwd_us"], 2)
            row["fwd_bwd_ratio"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
            row["max_rel_diff_vs_torch"] = err
        fwd_bound, bwd_bound = table / HBM_BPS * 1e6, 2 * table / HBM_BPS * 1e6
        row["bound"] = {"fwd_bytes": table, "fwd_us": round(fwd_bound, 1), "bwd_bytes": 2 * table, "bwd_us": round(bwd_bound, 1)}
        row["fwd_tbps"] = round(table / row["fwd_us"] / 1e6, 2)
        row["bwd_tbps"] = round(2 * table / row["bwd_us"] / 1e6, 2)
        row["fwd_bound_frac"] = round(fwd_bound / row["fwd_us"], 3)
        row["bwd_bound_frac"] = round(bwd_bound / row["bwd_us"], 3)
        print(json.dumps(row), flush=True)
        del enc, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
