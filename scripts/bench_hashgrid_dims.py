#!/usr/bin/env python3
"""Times the hash grid's native passes for 2, 3 and 4 input dimensions on one table shape (default L 16, F 2, 2^19 entries,
base 16, scale 1.447: ngp.py's radiance-field grid) at N uniform points, and prints one JSON line per dimension.
    python scripts/bench_hashgrid_dims.py [--log2n 20] [--window-ms 100] [--windows 7] [--features 2] [--no-torch]
Per dimension: the forward, the backward towards the table and x with float atomics (zeroing of the table gradient
included) and with deterministic=True, and the same two calls through the torch path on the same device: the forward of
`_hashgrid_torch` without an autograd graph, and its forward + backward (towards the table and x) through autograd,
which cannot be split.  The dimensions take turns window by window in one process.  A window is as many calls as fill
`--window-ms` of device time (at least 3; counted once per pass from a timed probe after 3 warm-up calls) between two HIP
events; `*_us` is the median of the windows' means, `*_spread` their (min, max), `*_reps` the calls per window."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd.encodings import HashGridEncoding, _hashgrid_torch  # noqa: E402


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--features", type=int, default=2)
    ap.add_argument("--interpolation", default="Linear")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 1 << a.log2n
    scale = float(np.exp((np.log(4096) - np.log(16)) / 15))
    passes = {}
    for D in (2, 3, 4):
        torch.manual_seed(D)
        grids = {det: HashGridEncoding(D, 16, a.features, 19, 16, scale, deterministic=det, interpolation=a.interpolation).to(dev)
                 for det in (False, True)}
        for g in grids.values():
            with torch.no_grad():
                g.params.uniform_(-1, 1)
        x = torch.rand(n, D, device=dev).requires_grad_(True)
        gy = torch.randn(n, grids[False].n_output_dims, device=dev)
        ys = {det: g(x) for det, g in grids.items()}
        enc = grids[False]
        passes[D] = {
            "fwd": lambda enc=enc, x=x: enc(x.detach()),
            "bwd_atomic": lambda y=ys[False], x=x, p=grids[False].params, gy=gy: torch.autograd.grad(y, (x, p), gy, retain_graph=True),
            "bwd_sorted": lambda y=ys[True], x=x, p=grids[True].params, gy=gy: torch.autograd.grad(y, (x, p), gy, retain_graph=True),
        }
        if not a.no_torch:
            def torch_fwd(enc=enc, x=x):
                with torch.no_grad():
                    return _hashgrid_torch(x.detach(), enc.params, enc.table, enc.n_features_per_level, enc.interp)
            passes[D]["torch_fwd"] = torch_fwd

            def torch_fwd_bwd(enc=enc, x=x, gy=gy):
                y = _hashgrid_torch(x, enc.params, enc.table, enc.n_features_per_level, enc.interp)
                return torch.autograd.grad(y, (x, enc.params), gy)
            passes[D]["torch_fwd_bwd"] = torch_fwd_bwd
    times = {D: {k: [] for k in p} for D, p in passes.items()}
    reps = {}
    for D, p in passes.items():   # warm up, then size each pass's window
        for k, fn in p.items():
            for _ in range(3):
                fn()
            reps[D, k] = max(3, int(math.ceil(a.window_ms * 1e3 / timed(fn, 3))))
    for _ in range(a.windows):
        for D, p in passes.items():
            for k, fn in p.items():
                times[D][k].append(timed(fn, reps[D, k]))
    for D in passes:
        row = {"n_dims": D, "n_points": n, "n_levels": 16, "n_features": a.features, "log2_hashmap_size": 19,
               "interpolation": a.interpolation, "window_ms": a.window_ms, "windows": a.windows}
        for k, v in times[D].items():
            row[k + "_us"] = round(float(np.median(v)), 1)
            row[k + "_spread"] = [round(min(v), 1), round(max(v), 1)]
            row[k + "_reps"] = reps[D, k]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
