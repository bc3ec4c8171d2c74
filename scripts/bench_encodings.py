#!/usr/bin/env python3
"""Times the hash-grid and spherical-harmonics encodings (csrc/encoding.hip) with HIP events against the torch path of
nerfacc_amd.encodings on the same GPU, and prints one JSON line per case.
    python scripts/bench_encodings.py [--reps 20] [--sizes 18,20] [--no-torch]
Cases: ngp.py's NGPRadianceField grid (L 16, F 2, 2^19) and NGPDensityField grid (L 5, F 2, 2^17) at N = 2^18 and 2^20, on
two point sets: uniform in [0, 1]^3, and the midpoints of OccGridEstimator.sampling on bench.py's cfg 2 scene (1024^2 image
rays, 128^3 shell grid), in the order a training step presents them (ray by ray, along each ray).
Algorithmic bytes: forward reads x (12 B) and 8 corners x F x 4 B per (point, level), writes L F 4 B per point; backward
reads x and dL/dy (12 + L F 4 B per point) and adds 8 x F x 4 B per (point, level) to the table gradient (the atomic
bytes); dL/dx adds the 8 corner reads again and writes 12 B per point.  Zeroing the gradient is timed on its own.
    python scripts/bench_encodings.py --dtype bfloat16 [--sizes 20,22] [--reps 20] [--windows 7]
times the half-precision output instead (out_dtype, the `_t` entries): forward and forward + backward of the grid with a
half output and a half incoming gradient, against what the same user code runs without out_dtype -- the float32 op
followed by `.to(dtype)`, whose backward widens the gradient again.  The two alternate, window by window, in one process;
each figure is the median over the windows.
    python scripts/bench_encodings.py --eikonal [--sizes 18] [--reps 10] [--windows 7]
times an Eikonal-shaped step on uniform points: forward, `autograd.grad(y, x, g, create_graph=True)`, then the backward of a
function of that dL/dx (sum of squares) towards the table -- natively (nfa_hashgrid_fwd, _bwd, _bwd_bwd) and through
`_hashgrid_torch` on the same GPU, the only way to run such a step without the second-order pass.  The two alternate window by
window; medians.  The native step is also split: the first-order part (forward + backward with create_graph) and the
second-order pass alone (the step minus the first-order part).
    python scripts/bench_encodings.py --deterministic [--dtype bfloat16] [--sizes 18,20] [--reps 10] [--windows 7]
    python scripts/bench_encodings.py --deterministic --eikonal [--sizes 18]
times the reproducible table gradient (HashGridEncoding(deterministic=True): nfa_hashgrid_bwd_sorted, _bwd_bwd_sorted) next
to the atomic one of the same build: the backward towards the table (zeroing included) on uniform and occgrid points, or the
Eikonal-shaped step.  The two alternate window by window; each figure is the median over the windows, `*_spread` the
(min, max) over them.  `scratch_bytes` is what one sorted call allocates.
    python scripts/bench_encodings.py --interpolation Smoothstep [--sizes 20] [--reps 10] [--windows 7]
times the three native passes of a HashGridEncoding(interpolation=...) next to the Linear grid on the same table, uniform
points: the forward, the backward (table gradient and dL/dx; atomic and deterministic=True) and the second-order pass alone (the
backward of a dL/dx built with create_graph; atomic and sorted).  All take turns window by window in one process; `*_us` is
the median over the windows, `*_spread` the (min, max), `*_ratio` the named grid's median over Linear's.  With
`--interpolation Linear` the second grid is Linear again: the ratios are then the spread of a pass against itself."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd.encodings import HashGridEncoding, SphericalHarmonicsEncoding, _hashgrid_torch  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def alternating_medians(fns, reps, windows):
    """{name: median us} of `windows` timed windows per function, the functions taking turns."""
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(timed(fn, reps))
    return {k: float(np.median(v)) for k, v in times.items()}


def alternating_stats(fns, reps, windows):
    """{name_us: median, name_spread: (min, max)} of `windows` timed windows per function, the functions taking turns."""
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(timed(fn, reps))
    out = {}
    for k, v in times.items():
        out[k + "_us"] = float(np.median(v))
        out[k + "_spread"] = (float(min(v)), float(max(v)))
    return out


def sorted_pair(cfg, dev, out_dtype=None):
    """(atomic grid, sorted grid) on one parameter tensor, uniform in +-1."""
    torch.manual_seed(0)
    enc = HashGridEncoding(3, out_dtype=out_dtype, **cfg).to(dev)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    det = HashGridEncoding(3, out_dtype=out_dtype, deterministic=True, **cfg)
    det.params = enc.params
    return enc, det


def deterministic_rows(args, dev, dtype):
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    scratch = B.load().nfa_hashgrid_sorted_scratch_bytes
    torch.manual_seed(0)
    uni = torch.rand(max(sizes), 3, device=dev)
    if args.eikonal:
        for cname, cfg in CONFIGS.items():
            enc, det = sorted_pair(cfg, dev)
            L, F = enc.n_levels, enc.n_features_per_level
            for N in sizes:
                x = uni[:N].clone().requires_grad_(True)
                g = torch.randn(N, L * F, device=dev)

                def step(fn):
                    enc.params.grad = None
                    x.grad = None
                    (g_x,) = torch.autograd.grad(fn(x), x, g, create_graph=True)
                    (g_x ** 2).sum().backward()

                step(det)
                gp = enc.params.grad.clone()
                step(det)
                row = dict(config=cname, mode="eikonal", N=N, L=L, F=F, sorted_repeats_bitwise=bool(torch.equal(gp, enc.params.grad)),
                           scratch_bytes=int(scratch(N, L, cfg["log2_hashmap_size"])))
                step(enc)
                row["sorted_vs_atomic_max_abs"] = float((enc.params.grad - gp).abs().max())
                row["grad_max_abs"] = float(gp.abs().max())
                row.update(alternating_stats({"atomic_step": lambda: step(enc), "sorted_step": lambda: step(det)}, args.reps, args.windows))
                row["sorted_over_atomic"] = row["sorted_step_us"] / row["atomic_step_us"]
                print(json.dumps(row), flush=True)
        return
    real, _ = occgrid_midpoints(dev, max(sizes))
    out_dtype = None if dtype == torch.float32 else dtype
    for cname, cfg in CONFIGS.items():
        enc, det = sorted_pair(cfg, dev, out_dtype)
        L, F = enc.n_levels, enc.n_features_per_level
        for N in sizes:
            for pname, pts in (("uniform", uni[:N]), ("occgrid", real[:N])):
                x = pts.clone()
                g = torch.randn(N, L * F, device=dev).to(dtype)
                ys = {"atomic": enc(x), "sorted": det(x)}

                def bwd(k):
                    enc.params.grad = None
                    torch.autograd.backward(ys[k], g, retain_graph=True)

                bwd("sorted")
                gp = enc.params.grad.clone()
                bwd("sorted")
                row = dict(config=cname, points=pname, dtype=str(dtype), N=N, L=L, F=F,
                           sorted_repeats_bitwise=bool(torch.equal(gp, enc.params.grad)),
                           scratch_bytes=int(scratch(N, L, cfg["log2_hashmap_size"])))
                bwd("atomic")
                row["sorted_vs_atomic_max_abs"] = float((enc.params.grad - gp).abs().max())
                row["grad_max_abs"] = float(gp.abs().max())
                row.update(alternating_stats({"atomic_bwd_params": lambda: bwd("atomic"), "sorted_bwd_params": lambda: bwd("sorted")},
                                             args.reps, args.windows))
                row["sorted_over_atomic"] = row["sorted_bwd_params_us"] / row["atomic_bwd_params_us"]
                print(json.dumps(row), flush=True)
                del ys


def interpolation_rows(args, dev):
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    torch.manual_seed(0)
    uni = torch.rand(max(sizes), 3, device=dev)
    other = "linear_again" if args.interpolation.lower() == "linear" else args.interpolation.lower()
    for cname, cfg in CONFIGS.items():
        torch.manual_seed(0)
        base = HashGridEncoding(3, **cfg).to(dev)
        with torch.no_grad():
            base.params.uniform_(-1, 1)
        L, F = base.n_levels, base.n_features_per_level

        def grid(interpolation, deterministic):
            enc = HashGridEncoding(3, deterministic=deterministic, interpolation=interpolation, **cfg)
            enc.params = base.params
            return enc

        for N in sizes:
            x = uni[:N].clone().requires_grad_(True)
            g = torch.randn(N, L * F, device=dev, requires_grad=True)
            v = torch.randn(N, 3, device=dev)

            def fwd(enc):
                with torch.no_grad():
                    enc(x)

            def bwd(out, grad):   # out = y: the backward; out = dL/dx built with create_graph: the second-order pass alone
                base.params.grad = x.grad = g.grad = None
                torch.autograd.backward(out, grad, retain_graph=True)

            fns = {}
            for tag, name in (("linear", "Linear"), (other, args.interpolation)):
                for mode, enc in (("atomic", grid(name, False)), ("sorted", grid(name, True))):
                    if mode == "atomic":
                        fns[f"{tag}_fwd"] = lambda enc=enc: fwd(enc)
                    y = enc(x)
                    (g_x,) = torch.autograd.grad(enc(x), x, g, create_graph=True)
                    fns[f"{tag}_bwd_{mode}"] = lambda y=y: bwd(y, g.detach())
                    fns[f"{tag}_bwd2_{mode}"] = lambda g_x=g_x: bwd(g_x, v)
            row = dict(config=cname, interpolation=args.interpolation, N=N, L=L, F=F)
            row.update(alternating_stats(fns, args.reps, args.windows))
            for k in ("fwd", "bwd_atomic", "bwd_sorted", "bwd2_atomic", "bwd2_sorted"):
                row[k + "_ratio"] = row[f"{other}_{k}_us"] / row[f"linear_{k}_us"]
            print(json.dumps(row), flush=True)
            del fns


def half_rows(args, dev, dtype):
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    torch.manual_seed(0)
    uni = torch.rand(max(sizes), 3, device=dev)
    for cname, cfg in CONFIGS.items():
        torch.manual_seed(0)
        enc = HashGridEncoding(3, **cfg).to(dev)
        half = HashGridEncoding(3, out_dtype=dtype, **cfg)
        half.params = enc.params
        L, F = enc.n_levels, enc.n_features_per_level
        for N in sizes:
            x = uni[:N].clone()
            g = torch.randn(N, L * F, device=dev).to(dtype)
            assert torch.equal(half(x), enc(x).to(dtype))

            def step(fn):
                enc.params.grad = None
                fn(x).backward(g)

            def fwd(fn):
                with torch.no_grad():
                    fn(x)

            native, cast = half, (lambda t: enc(t).to(dtype))
            m = alternating_medians({"half_fwd_us": lambda: fwd(native), "f32_cast_fwd_us": lambda: fwd(cast),
                                     "half_fwd_bwd_us": lambda: step(native), "f32_cast_fwd_bwd_us": lambda: step(cast)},
                                    args.reps, args.windows)
            row = dict(config=cname, dtype=str(dtype), N=N, L=L, F=F, **m)
            row["speedup_fwd"] = m["f32_cast_fwd_us"] / m["half_fwd_us"]
            row["speedup_fwd_bwd"] = m["f32_cast_fwd_bwd_us"] / m["half_fwd_bwd_us"]
            print(json.dumps(row), flush=True)


def eikonal_rows(args, dev):
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    torch.manual_seed(0)
    uni = torch.rand(max(sizes), 3, device=dev)
    for cname, cfg in CONFIGS.items():
        torch.manual_seed(0)
        enc = HashGridEncoding(3, **cfg).to(dev)
        with torch.no_grad():
            enc.params.uniform_(-1, 1)
        L, F = enc.n_levels, enc.n_features_per_level
        for N in sizes:
            x = uni[:N].clone().requires_grad_(True)
            g = torch.randn(N, L * F, device=dev)

            def first(fn):
                (g_x,) = torch.autograd.grad(fn(x), x, g, create_graph=True)
                return g_x

            def step(fn):
                enc.params.grad = None
                x.grad = None
                (first(fn) ** 2).sum().backward()

            native, torch_path = enc, (lambda t: _hashgrid_torch(t, enc.params, enc.table, F))
            step(native)
            gp, gx = enc.params.grad.clone(), x.grad.clone()
            step(torch_path)
            row = dict(config=cname, mode="eikonal", N=N, L=L, F=F,
                       grad_params_max_abs_diff=float((enc.params.grad - gp).abs().max()), grad_params_max_abs=float(gp.abs().max()),
                       grad_x_max_abs_diff=float((x.grad - gx).abs().max()), grad_x_max_abs=float(gx.abs().max()))
            m = alternating_medians({"native_step_us": lambda: step(native), "torch_step_us": lambda: step(torch_path),
                                     "native_first_order_us": lambda: first(native)}, args.reps, args.windows)
            row.update(m)
            row["native_second_order_us"] = m["native_step_us"] - m["native_first_order_us"]
            row["speedup"] = m["torch_step_us"] / m["native_step_us"]
            print(json.dumps(row), flush=True)


def occgrid_midpoints(dev, n):
    import bench
    w = bench.make_workload(dev)
    ri, ts, te = w["estimator"].sampling(w["rays_o"], w["rays_d"], sigma_fn=w["sigma_fn"], render_step_size=w["step"],
                                         early_stop_eps=1e-4, alpha_thre=0.0)
    ri, m = ri[:n], ((ts + te) / 2)[:n]
    x = w["rays_o"][ri] + w["rays_d"][ri] * m[:, None]
    return ((x + 1.0) / 2.0).contiguous(), int(ts.numel())


CONFIGS = {
    "radiance": dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16,
                     per_level_scale=np.exp((np.log(4096) - np.log(16)) / 15).tolist()),
    "density": dict(n_levels=5, n_features_per_level=2, log2_hashmap_size=17, base_resolution=16,
                    per_level_scale=np.exp((np.log(128) - np.log(16)) / 4).tolist()),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="18,20")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16", "bfloat16"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--eikonal", action="store_true")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--interpolation", default=None, help="time this interpolation's passes against Linear's")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B.load()
    if args.interpolation is not None:
        return interpolation_rows(args, dev)
    if args.deterministic:
        return deterministic_rows(args, dev, getattr(torch, args.dtype))
    if args.eikonal:
        return eikonal_rows(args, dev)
    if args.dtype != "float32":
        return half_rows(args, dev, getattr(torch, args.dtype))
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    real, n_samples = occgrid_midpoints(dev, max(sizes))
    assert real.shape[0] >= max(sizes), (real.shape, n_samples)
    torch.manual_seed(0)
    uni = torch.rand(max(sizes), 3, device=dev)
    for cname, cfg in CONFIGS.items():
        torch.manual_seed(0)
        enc = HashGridEncoding(3, **cfg).to(dev)
        L, F = enc.n_levels, enc.n_features_per_level
        P = enc.params
        for N in sizes:
            for pname, pts in (("uniform", uni[:N]), ("occgrid", real[:N])):
                x = pts.clone()
                xg = pts.clone().requires_grad_(True)
                g = torch.randn(N, L * F, device=dev)
                row = dict(config=cname, points=pname, N=N, L=L, F=F, params=P.numel())
                with torch.no_grad():
                    row["fwd_us"] = timed(lambda: enc(x), args.reps)
                y = enc(x)
                row["zero_grad_us"] = timed(lambda: torch.zeros_like(P), args.reps)

                def bwd_params():
                    enc.params.grad = None
                    torch.autograd.backward(y, g, retain_graph=True)

                row["bwd_params_us_incl_zero"] = timed(bwd_params, args.reps)
                yx = enc(xg)

                def bwd_both():
                    enc.params.grad = None
                    xg.grad = None
                    torch.autograd.backward(yx, g, retain_graph=True)

                row["bwd_params_x_us_incl_zero"] = timed(bwd_both, args.reps)
                row["bwd_params_us"] = row["bwd_params_us_incl_zero"] - row["zero_grad_us"]
                row["bwd_params_x_us"] = row["bwd_params_x_us_incl_zero"] - row["zero_grad_us"]
                corner_b = 8 * F * 4 * N * L
                row["fwd_bytes"] = 12 * N + corner_b + L * F * 4 * N
                row["fwd_TBps"] = row["fwd_bytes"] / row["fwd_us"] / 1e6
                row["atomic_bytes"] = corner_b
                row["bwd_atomic_TBps"] = corner_b / row["bwd_params_us"] / 1e6
                row["Mpts_per_s_fwd"] = N / row["fwd_us"]
                if not args.no_torch:
                    with torch.no_grad():
                        row["torch_fwd_us"] = timed(lambda: _hashgrid_torch(x, P, enc.table, F), max(2, args.reps // 4))
                        yt = _hashgrid_torch(x, P, enc.table, F)
                    row["torch_fwd_bit_identical"] = bool(torch.equal(yt, enc(x)))
                    pt = P.detach().clone().requires_grad_(True)
                    yt = _hashgrid_torch(x, pt, enc.table, F)

                    def torch_bwd():
                        pt.grad = None
                        torch.autograd.backward(yt, g, retain_graph=True)

                    row["torch_bwd_params_us"] = timed(torch_bwd, max(2, args.reps // 4))
                    enc.params.grad = None
                    torch.autograd.backward(y, g, retain_graph=True)
                    d = (pt.grad - enc.params.grad).abs()
                    row["torch_vs_native_grad_max_abs"] = float(d.max())
                    row["grad_max_abs"] = float(pt.grad.abs().max())
                    row["speedup_fwd"] = row["torch_fwd_us"] / row["fwd_us"]
                    row["speedup_bwd_params"] = row["torch_bwd_params_us"] / row["bwd_params_us_incl_zero"]
                print(json.dumps(row), flush=True)
                del y, yx
    for N in sizes:
        sh = SphericalHarmonicsEncoding(3, 4)
        d = (torch.rand(N, 3, device=dev)).requires_grad_(True)
        out = sh(d)
        go = torch.randn_like(out)
        row = dict(config="sh4", N=N)
        with torch.no_grad():
            row["fwd_us"] = timed(lambda: sh(d), args.reps)

        def shb():
            d.grad = None
            torch.autograd.backward(out, go, retain_graph=True)

        row["bwd_us"] = timed(shb, args.reps)
        row["fwd_TBps"] = (12 + 64) * N / row["fwd_us"] / 1e6
        row["bwd_TBps"] = (12 + 64 + 12) * N / row["bwd_us"] / 1e6
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(occgrid_samples_cfg2=n_samples)), flush=True)


if __name__ == "__main__":
    main()
