#!/usr/bin/env python3
"""Times the sinusoidal encoding's native passes (csrc/sinenc.hip) against the torch composition the reference runs
(`_sinusoidal_torch`: multiply, reshape, cat, add, sin, cat, and autograd through them) on the same GPU, at N = 2^22 points,
for the reference's position encoder (3, 0, 10) and direction encoder (3, 0, 4), float32 and bf16 outputs, and prints one
JSON line per shape.
    python scripts/bench_sinusoidal.py [--log2n 22] [--window-ms 200] [--windows 5] [--no-torch]
Per line: the forward (`fwd`), forward + backward towards x (`fwd_bwd`), and forward + backward with create_graph + the
backward of sum(dL/dx * v) towards x and grad_out (`fwd_bwd2`: what an Eikonal term adds), each native and through the
composition (`torch_*`; for bf16 the composition's float32 result is cast).  The passes take turns window by window in one
process.  A window is as many calls as fill `--window-ms` of device time (at least 3; counted once per pass from a timed
probe after 3 warm-up calls) between two HIP events; `*_us` is the median of the windows' means, `*_spread` their
(min, max), `*_reps` the calls per window.  `*_bytes` are the bytes the native kernels of a pass must move (x in, the
[N, K] stream out; the backward: x and grad_out in, grad_x out; the second order: x, grad_out, v in, grad_grad_out and
grad_x out), `*_gbps` those bytes over the time -- for `fwd` to be held against the 4.4 TB/s a pure write stream reaches
(DESIGN.md, section 4).  `fwd_bwd2` also contains the torch ops of the scalar (a multiply and a sum over [N, 3]).
`*_ratio`: the composition's time over the native one."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd.encodings import SinusoidalEncoding, _sinusoidal_torch  # noqa: E402


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


def passes_of(f, x, g, v, prefix=""):
    def fwd():
        with torch.no_grad():
            return f(x)

    def fwd_bwd():
        return torch.autograd.grad(f(x), x, g)

    def fwd_bwd2():
        (gx,) = torch.autograd.grad(f(x), x, g, create_graph=True)
        return torch.autograd.grad((gx * v).sum(), (x, g))
    return {prefix + "fwd": fwd, prefix + "fwd_bwd": fwd_bwd, prefix + "fwd_bwd2": fwd_bwd2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinusoidal.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    n = 1 << a.log2n
    for cfg in ((3, 0, 10), (3, 0, 4)):
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(cfg[2])
            enc = SinusoidalEncoding(*cfg, out_dtype=dtype)
            K, D, e = enc.latent_dim, cfg[0], torch.empty(0, dtype=dtype).element_size()
            x = (torch.rand(n, D, device=dev) * 3.0 - 1.5).requires_grad_(True)
            g = torch.randn(n, K, device=dev).to(dtype).requires_grad_(True)
            v = torch.randn(n, D, device=dev)
            passes = passes_of(enc, x, g, v)
            row = {"n_points": n, "config": list(cfg), "dtype": str(dtype).replace("torch.", ""), "latent_dim": K,
                   "window_ms": a.window_ms, "windows": a.windows}
            if not a.no_torch:
                def comp(t):
                    y = _sinusoidal_torch(t, cfg[1], cfg[2], True)
                    return y if dtype == torch.float32 else y.to(dtype)
                passes.update(passes_of(comp, x, g, v, "torch_"))
                with torch.no_grad():   # the two forms compute the same thing at the size that is timed
                    row["max_abs_diff_vs_torch"] = float((enc(x).float() - comp(x).float()).abs().max())
            row.update(measure(passes, a.window_ms, a.windows))
            stream, pts = n * K * e, n * D * 4
            row["fwd_bytes"] = pts + stream
            row["fwd_bwd_bytes"] = row["fwd_bytes"] + pts + stream + pts
            row["fwd_bwd2_bytes"] = row["fwd_bwd_bytes"] + 3 * pts + 2 * stream + pts
            for k in ("fwd", "fwd_bwd", "fwd_bwd2"):
                row[k + "_gbps"] = round(row[k + "_bytes"] / row[k + "_us"] / 1e3, 1)
                if not a.no_torch:
                    row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
            print(json.dumps(row), flush=True)
            del x, g, v, passes
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
