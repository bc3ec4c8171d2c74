#!/usr/bin/env python3
"""Times the VM grid's native passes against the torch composition TensoRF runs (`grid_sample` on three planes and three
lines, the products, `cat` or `sum`, autograd; `F.interpolate` for the resampling) on TensoRF's shapes -- resolution 300^3
and 128^3, each with C = 16 "sum" (the density grid) and C = 48 "concat" (the appearance grid) -- at N uniform points, and
prints one JSON line per shape, then one per resampling 128^3 -> 300^3.
    python scripts/bench_vmgrid.py [--log2n 20] [--window-ms 200] [--windows 5] [--no-torch]
Per shape line: the native forward (`fwd`), the native forward + backward towards the table, zeroing of the table gradient
included (`fwd_bwd`: what a TensoRF step runs, its points carry no gradient), the same towards the table and x
(`fwd_bwd_x`), and the three through the composition (`torch_*`), whose planes and lines are copies of the same parameters
in TensoRF's own [1, C, H, W] / [1, C, R, 1] layout.  The passes take turns window by window in one process.  A window is
as many calls as fill `--window-ms` of device time (at least 3; counted once per pass from a timed probe after 3 warm-up
calls) between two HIP events; `*_us` is the median of the windows' means, `*_spread` their (min, max), `*_reps` the calls
per window.  `atomic_bytes`: the floats the backward adds to the planes (4 corners per mode, per point and component) and,
per workgroup flush, to the lines; `bwd_atomic_tbps` holds the plane adds against `bwd_us` = `fwd_bwd_us` - `fwd_us`, to be
compared with the chip-wide float-atomic rate (1.3 TB/s of added bytes).
Per resampling line: `resample` is `enc.resampled((300, 300, 300))` as a user calls it (the new module is built on the
host every time, which is what it costs at these sizes), `resample_call` the `nfa_vmgrid_resample` launch alone into an
existing table, `torch_resample` the six `F.interpolate` calls of `up_sampling_VM` under `no_grad`."""
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

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd.encodings import VM_MODES, VMGridEncoding  # noqa: E402

SAMPLE = dict(mode="bilinear", padding_mode="border", align_corners=True)


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def tensorf_tensors(enc):
    """TensoRF's form of the same table: leaf [1, C, R_b, R_a] planes and [1, C, R_c, 1] lines."""
    planes = [enc.plane(m).detach().permute(2, 0, 1)[None].contiguous().requires_grad_(True) for m in range(3)]
    lines = [enc.line(m).detach().t()[None, :, :, None].contiguous().requires_grad_(True) for m in range(3)]
    return planes, lines


def composition(enc):
    planes, lines = tensorf_tensors(enc)

    def f(x):
        u = 2.0 * x - 1.0
        terms = []
        for plane, line, (a, b, c) in zip(planes, lines, VM_MODES):
            coordinate_plane = u[:, [a, b]][None, None]
            coordinate_line = torch.stack([torch.zeros_like(u[:, c]), u[:, c]], -1)[None, None]
            terms.append(TF.grid_sample(plane, coordinate_plane, **SAMPLE)[0, :, 0] * TF.grid_sample(line, coordinate_line, **SAMPLE)[0, :, 0])
        if enc.reduce == "concat":
            return torch.cat(terms, 0).t()
        return torch.cat(terms, 0).sum(0)[:, None]
    return f, planes + lines


def up_sampling_vm(planes, lines, res):
    out = []
    for plane, line, (a, b, c) in zip(planes, lines, VM_MODES):
        out.append(TF.interpolate(plane, size=(res[b], res[a]), mode="bilinear", align_corners=True))
        out.append(TF.interpolate(line, size=(res[c], 1), mode="bilinear", align_corners=True))
    return out


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
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vmgrid.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    n = 1 << a.log2n
    settings = [(16, "sum"), (48, "concat")]
    for R in (300, 128):
        for C, reduce in settings:
            torch.manual_seed(C)
            enc = VMGridEncoding((R, R, R), C, reduce).to(dev)
            x = torch.rand(n, 3, device=dev).requires_grad_(True)
            gy = torch.randn(n, enc.n_output_dims, device=dev)

            def fwd():
                with torch.no_grad():
                    return enc(x)

            def fwd_bwd():
                return torch.autograd.grad(enc(x), enc.params, gy)

            def fwd_bwd_x():
                return torch.autograd.grad(enc(x), (x, enc.params), gy)
            passes = {"fwd": fwd, "fwd_bwd": fwd_bwd, "fwd_bwd_x": fwd_bwd_x}
            row = {"n_points": n, "resolution": [R, R, R], "n_components": C, "reduce": reduce, "n_params": enc.params.numel(),
                   "window_ms": a.window_ms, "windows": a.windows}
            if not a.no_torch:
                comp, leaves = composition(enc)

                def torch_fwd():
                    with torch.no_grad():
                        return comp(x)

                def torch_fwd_bwd():
                    return torch.autograd.grad(comp(x), leaves, gy)

                def torch_fwd_bwd_x():
                    return torch.autograd.grad(comp(x), (x, *leaves), gy)
                passes.update(torch_fwd=torch_fwd, torch_fwd_bwd=torch_fwd_bwd, torch_fwd_bwd_x=torch_fwd_bwd_x)
                with torch.no_grad():   # the two forms compute the same thing at the size that is timed
                    row["max_abs_diff_vs_torch"] = float((enc(x) - comp(x)).abs().max())
            row.update(measure(passes, a.window_ms, a.windows))
            row["bwd_us"] = round(row["fwd_bwd_us"] - row["fwd_us"], 1)
            plane_adds = n * 3 * 4 * C * 4
            row["atomic_bytes"] = {"planes": plane_adds, "lines_direct": n * 3 * 2 * C * 4}
            row["bwd_atomic_tbps"] = round(plane_adds / row["bwd_us"] / 1e6, 3)
            if not a.no_torch:
                for k in ("fwd", "fwd_bwd", "fwd_bwd_x"):
                    row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
            print(json.dumps(row), flush=True)
            del x, gy, enc, passes
            torch.cuda.empty_cache()
    for C, reduce in settings:
        torch.manual_seed(C)
        enc = VMGridEncoding((128, 128, 128), C, reduce).to(dev)
        big = enc.resampled((300, 300, 300))
        dst = torch.empty_like(big.params)

        def resample_call():   # the launch alone, into a table that exists: `resampled` also builds the new module
            B.call("nfa_vmgrid_resample", B.ptr(enc.params), enc.table.c_res, B.ptr(dst), big.table.c_res, C, B.stream())
        passes = {"resample": lambda: enc.resampled((300, 300, 300)), "resample_call": resample_call}
        row = {"resample": [128, 300], "n_components": C}
        if not a.no_torch:
            planes, lines = tensorf_tensors(enc)

            def torch_resample():
                with torch.no_grad():
                    return up_sampling_vm(planes, lines, (300, 300, 300))
            passes["torch_resample"] = torch_resample
        row.update(measure(passes, a.window_ms, a.windows))
        row["dst_bytes"] = dst.numel() * 4
        row["resample_call_tbps"] = round(row["dst_bytes"] / row["resample_call_us"] / 1e6, 2)
        if not a.no_torch:
            row["resample_ratio"] = round(row["torch_resample_us"] / row["resample_us"], 2)
            row["resample_call_ratio"] = round(row["torch_resample_us"] / row["resample_call_us"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
