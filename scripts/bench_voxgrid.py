#!/usr/bin/env python3
"""Times the dense voxel grid's native passes against the torch composition DVGO and TiNeuVox run (`F.grid_sample` on the
[1, C, N_x, N_y, N_z] tensor with flipped coordinates, once per stride on the view [::s, ::s, ::s], then a `cat`, autograd;
`F.interpolate` for the resampling) -- a 160^3 grid with C = 1 (DVGO's density grid) and with C = 12 (its `k0` grid), a 161^3
grid with C = 4 and strides (1, 2, 4) (TiNeuVox's `mult_dist_interp`) -- at N points drawn along rays, and prints one JSON line
per shape, then one per resampling 80^3 -> 160^3.
    python scripts/bench_voxgrid.py [--log2n 20] [--samples-per-ray 128] [--window-ms 200] [--windows 5] [--no-torch]
The points: N / samples-per-ray chords through the unit box, from a random point on one face to a random point on the opposite
one, sampled at equal steps in ray order, so that consecutive points are neighbours in the grid as a renderer's are.
Per shape line: the native forward (`fwd`), the native forward + backward towards the table, zeroing of the table gradient
included (`fwd_bwd`: what a DVGO step runs, its points carry no gradient), the same towards the table and x (`fwd_bwd_x`),
and the three through the composition (`torch_*`), whose grid is a copy of the same parameters in DVGO's own layout.  The
passes take turns window by window in one process.  A window is as many calls as fill `--window-ms` of device time (at
least 3; counted once per pass from a timed probe after 3 warm-up calls) between two HIP events; `*_us` is the median of the
windows' means, `*_spread` their (min, max), `*_reps` the calls per window.  `atomic_bytes`: the floats the backward adds to
the table (8 corners per stride, point and feature); `bwd_atomic_tbps` holds them against `bwd_us` = `fwd_bwd_us` - `fwd_us`,
to be compared with the chip-wide float-atomic rate (1.3 TB/s of added bytes).
Per resampling line: `resample` is `enc.resampled((160, 160, 160))` as a user calls it, `resample_call` the
`nfa_voxgrid_resample` launch alone into an existing table, `torch_resample` the `F.interpolate` call of `scale_volume_grid`
under `no_grad`."""
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
from nerfacc_amd.encodings import VoxelGridEncoding  # noqa: E402

SAMPLE = dict(mode="bilinear", padding_mode="border", align_corners=True)
SHAPES = [(160, 1, (1,)), (160, 12, (1,)), (161, 4, (1, 2, 4))]


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def ray_points(n, per_ray, seed):
    """[n, 3] float32 points on n / per_ray chords of the unit box, in ray order."""
    g = torch.Generator().manual_seed(seed)
    rays = n // per_ray
    a, b = torch.rand(rays, 3, generator=g), torch.rand(rays, 3, generator=g)
    axis = torch.randint(0, 3, (rays,), generator=g)
    a[torch.arange(rays), axis], b[torch.arange(rays), axis] = 0.0, 1.0
    t = (torch.arange(per_ray, dtype=torch.float32) + 0.5) / per_ray
    return (a[:, None] + t[None, :, None] * (b - a)[:, None]).reshape(-1, 3).contiguous()


def composition(enc):
    grid = enc.grid().detach().permute(3, 2, 1, 0)[None].contiguous().requires_grad_(True)   # DVGO's [1, C, N_x, N_y, N_z]
    C = enc.n_features

    def f(x):
        ind_norm = (2.0 * x - 1.0).flip(-1)[None, None, None]
        return torch.cat([TF.grid_sample(grid[:, :, ::s, ::s, ::s], ind_norm, **SAMPLE).reshape(C, -1).t() for s in enc.strides], -1)
    return f, grid


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
    ap.add_argument("--samples-per-ray", type=int, default=128)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxgrid.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    n = 1 << a.log2n
    for R, C, strides in SHAPES:
        torch.manual_seed(C)
        enc = VoxelGridEncoding((R, R, R), C, strides).to(dev)
        x = ray_points(n, a.samples_per_ray, seed=R + C).to(dev)   # a DVGO step's points carry no gradient: the backward gets no grad_x
        xg = x.clone().requires_grad_(True)
        gy = torch.randn(n, enc.n_output_dims, device=dev)

        def fwd():
            with torch.no_grad():
                return enc(x)

        def fwd_bwd():
            return torch.autograd.grad(enc(x), enc.params, gy)

        def fwd_bwd_x():
            return torch.autograd.grad(enc(xg), (xg, enc.params), gy)
        passes = {"fwd": fwd, "fwd_bwd": fwd_bwd, "fwd_bwd_x": fwd_bwd_x}
        row = {"n_points": n, "samples_per_ray": a.samples_per_ray, "resolution": [R, R, R], "n_features": C, "strides": list(strides),
               "n_params": enc.params.numel(), "window_ms": a.window_ms, "windows": a.windows}
        if not a.no_torch:
            comp, grid = composition(enc)

            def torch_fwd():
                with torch.no_grad():
                    return comp(x)

            def torch_fwd_bwd():
                return torch.autograd.grad(comp(x), grid, gy)

            def torch_fwd_bwd_x():
                return torch.autograd.grad(comp(xg), (xg, grid), gy)
            passes.update(torch_fwd=torch_fwd, torch_fwd_bwd=torch_fwd_bwd, torch_fwd_bwd_x=torch_fwd_bwd_x)
            with torch.no_grad():   # the two forms compute the same thing at the size that is timed
                row["max_abs_diff_vs_torch"] = float((enc(x) - comp(x)).abs().max())
        row.update(measure(passes, a.window_ms, a.windows))
        row["bwd_us"] = round(row["fwd_bwd_us"] - row["fwd_us"], 1)
        row["atomic_bytes"] = n * len(strides) * 8 * C * 4
        row["bwd_atomic_tbps"] = round(row["atomic_bytes"] / row["bwd_us"] / 1e6, 3)
        if not a.no_torch:
            for k in ("fwd", "fwd_bwd", "fwd_bwd_x"):
                row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
        print(json.dumps(row), flush=True)
        del x, xg, gy, enc, passes
        torch.cuda.empty_cache()
    for C in (1, 12):
        torch.manual_seed(C)
        enc = VoxelGridEncoding((80, 80, 80), C).to(dev)
        big = enc.resampled((160, 160, 160))
        dst = torch.empty_like(big.params)

        def resample_call():   # the launch alone, into a table that exists: `resampled` also builds the new module
            B.call("nfa_voxgrid_resample", B.ptr(enc.params), enc.table.c_res, B.ptr(dst), big.table.c_res, C, B.stream())
        passes = {"resample": lambda: enc.resampled((160, 160, 160)), "resample_call": resample_call}
        row = {"resample": [80, 160], "n_features": C}
        if not a.no_torch:
            grid = enc.grid().detach().permute(3, 2, 1, 0)[None].contiguous()

            def torch_resample():
                with torch.no_grad():
                    return TF.interpolate(grid, size=(160, 160, 160), mode="trilinear", align_corners=True)
            passes["torch_resample"] = torch_resample
            row["max_abs_diff_vs_torch"] = float((big.grid().detach().permute(3, 2, 1, 0)[None] - torch_resample()).abs().max())
        row.update(measure(passes, a.window_ms, a.windows))
        row["dst_bytes"] = dst.numel() * 4
        row["resample_call_tbps"] = round(row["dst_bytes"] / row["resample_call_us"] / 1e6, 2)
        if not a.no_torch:
            row["resample_ratio"] = round(row["torch_resample_us"] / row["resample_us"], 2)
            row["resample_call_ratio"] = round(row["torch_resample_us"] / row["resample_call_us"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
