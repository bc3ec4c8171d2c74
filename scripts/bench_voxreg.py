#!/usr/bin/env python3
"""Times the voxel grid's native regularisers (csrc/voxreg.hip) against the same formulas in torch -- slicing along the three
axes of the [R_z, R_y, R_x, C] table with autograd for `voxel_regularization`, the float32 restatement of the gradient plus a
masked add for `voxel_tv_add_grad_` -- on a 160^3 table with C = 1 (DVGO's density grid) and C = 12 (its `k0` grid) and a
161^3 table with C = 4 (TiNeuVox), and prints one JSON line per shape.
    python scripts/bench_voxreg.py [--window-ms 200] [--windows 5] [--no-torch]
Per line, for kind in (l2, huber): `<kind>_fwd` is `voxel_regularization` under `no_grad`, `<kind>_fwd_bwd` the same plus
the gradient towards the table; `add_dense` / `add_sparse` are `voxel_tv_add_grad_` (huber, "sum") into an existing gradient,
`add_sparse` with about 10 % of the gradient non-zero; `torch_*` the torch forms of the same.  An add changes the gradient, so
every timed add has a refill of the gradient in front of it; the refill is also timed as a pass of its own (`refill`) and its
time taken off the four adds.  The passes take turns window by
window in one process.  A window is as many calls as fill `--window-ms` of device time (at least 3; counted once per pass
from a timed probe after 3 warm-up calls) between two HIP events; `*_us` is the median of the windows' means, `*_spread`
their (min, max), `*_reps` the calls per window.  `*_min_bytes` is the least traffic the pass needs (4 bytes per table float
forward: the table read once; 8 forward + backward: read once more and the gradient written; 12 for the in-place add: the
table and the gradient read, the gradient written), `*_tbps` that over the time, `*_of_copy` its fraction of the 6.29 TB/s a
plain copy reaches on this GPU.  `*_ratio` is torch's time over the native one.  The agreement of the two forms at the timed
size is printed as `*_max_rel_diff` (terms) and `*_bits_equal` (the in-place add)."""
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
from nerfacc_amd.encodings import VoxelGridEncoding  # noqa: E402

SHAPES = [(160, 1), (160, 12), (161, 4)]
COPY_TBPS = 6.29
W = (0.01, 0.01, 0.01)


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def measure(passes, window_ms, windows):
    times, reps = {k: [] for k in passes}, {}
    for k, fn in passes.items():
        for _ in range(3):
            fn()
        reps[k] = max(3, int(math.ceil(window_ms * 1e3 / timed(fn, 3))))
    for _ in range(windows):
        for k, fn in passes.items():
            times[k].append(timed(fn, reps[k]))
    row = {}
    for k, v in times.items():
        row[k + "_us"] = round(float(np.median(v)), 1)
        row[k + "_spread"] = [round(min(v), 1), round(max(v), 1)]
        row[k + "_reps"] = reps[k]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxreg.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    for R, C in SHAPES:
        torch.manual_seed(C)
        res = (R, R, R)
        enc = VoxelGridEncoding(res, C, init_scale=1.0).to(dev)
        n = enc.params.numel()
        gen = torch.Generator().manual_seed(R + C)
        dense_grad = torch.randn(n, generator=gen).to(dev)
        sparse_grad = dense_grad * (torch.rand(n, generator=gen) < 0.1).to(dev)
        enc.params.grad = torch.empty_like(dense_grad)
        w4 = torch.tensor((*W, 0.0), device=dev)
        passes, row = {}, {"resolution": list(res), "n_features": C, "n_params": n, "window_ms": a.window_ms, "windows": a.windows,
                           "sparse_nonzero": round(float((sparse_grad != 0).float().mean()), 4)}

        def native(kind, grad):
            def f():
                loss = losses.voxel_regularization(enc, tv=1.0, l1=0.1, kind=kind)
                return torch.autograd.grad(loss, enc.params) if grad else loss
            return f

        def composed(kind, grad):
            wt = losses._voxel_weights(enc, 1.0, 1.0, 1.0, 0.1)

            def f():
                loss = (losses._voxel_terms_torch(enc.params, res, C, kind, "mean") * wt).sum()
                return torch.autograd.grad(loss, enc.params) if grad else loss
            return f

        def no_grad(f):
            def g():
                with torch.no_grad():
                    return f()
            return g

        def add(dense, start, native_path):
            def f():   # (the refill of the gradient is part of neither form's work: both are timed with it)
                enc.params.grad.copy_(start)
                if native_path:
                    losses.voxel_tv_add_grad_(enc, *W, dense=dense)
                else:
                    G = losses._voxel_terms_grad_torch(enc.params, w4, res, C, "huber", "sum")
                    g = enc.params.grad
                    total = g + G
                    g.copy_(total if dense else torch.where(g != 0, total, g))
                return enc.params.grad
            return f

        for kind in ("l2", "huber"):
            passes[kind + "_fwd"] = no_grad(native(kind, False))
            passes[kind + "_fwd_bwd"] = native(kind, True)
            if not a.no_torch:
                passes["torch_" + kind + "_fwd"] = no_grad(composed(kind, False))
                passes["torch_" + kind + "_fwd_bwd"] = composed(kind, True)
                with torch.no_grad():   # the two forms compute the same thing at the size that is timed
                    t_native = losses.voxel_terms(enc, kind).double()
                    t_torch = losses._voxel_terms_torch(enc.params.double(), res, C, kind, "mean")
                row[kind + "_max_rel_diff"] = float(((t_native - t_torch).abs() / t_torch.abs()).max())
        passes["refill"] = lambda: enc.params.grad.copy_(dense_grad)
        passes["add_dense"] = add(True, dense_grad, True)
        passes["add_sparse"] = add(False, sparse_grad, True)
        if not a.no_torch:
            passes["torch_add_dense"] = add(True, dense_grad, False)
            passes["torch_add_sparse"] = add(False, sparse_grad, False)
            for name in ("add_dense", "add_sparse"):
                got = passes[name]().clone()
                row[name + "_bits_equal"] = bool(torch.equal(got.view(torch.int32), passes["torch_" + name]().view(torch.int32)))
        row.update(measure(passes, a.window_ms, a.windows))
        for k in [k for k in passes if k.startswith("add_") or k.startswith("torch_add_")]:   # the add alone: the refill taken off
            row[k + "_us"] = round(row[k + "_us"] - row["refill_us"], 1)
        per_float = {"fwd": 4, "fwd_bwd": 8, "add": 12}
        for k in [k for k in passes if not k.startswith("torch_") and k != "refill"]:
            b = n * per_float["add" if k.startswith("add") else k.split("_", 1)[1]]
            row[k + "_min_bytes"] = b
            if row[k + "_us"] <= 0.0:   # (an add faster than the noise of the refill it is timed behind)
                continue
            row[k + "_tbps"] = round(b / row[k + "_us"] / 1e6, 3)
            row[k + "_of_copy"] = round(row[k + "_tbps"] / COPY_TBPS, 3)
            if not a.no_torch:
                row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
        print(json.dumps(row), flush=True)
        del enc, dense_grad, sparse_grad, passes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
