#!/usr/bin/env python3
"""Times the fused MLP (csrc/mlp.hip, nerfacc_amd.mlp.FusedMLP) against the same network as `nn.Sequential` of
`nn.Linear(bias=False)` / `nn.ReLU` under `torch.autocast` on the same GPU, at the three NGP shapes (base 32 -> 64 -> 16,
head 32 -> 64 -> 64 -> 3, proposal 10 -> 64 -> 1) for N = 2^20 and 2^22 points, and prints one JSON line per (shape, N, dtype).
    python scripts/bench_mlp.py [--log2n 20 22] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5]
Inputs and output gradients are of the half type (what the encodings hand over and the renderer hands back).  Per line: the
forward without autograd (`fwd`) and forward + backward towards x and the parameters (`fwd_bwd`), native and baseline
(`torch_*`), taking turns window by window in one process.  A window is as many calls as fill `--window-ms` of device time (at
least 3; counted once per pass from a timed probe after 3 warm-up calls) between two HIP events; `*_us` is the median of the
windows' means, `*_spread` their (min, max).  `*_ratio` is the baseline's time over the native one: above 1 the native pass
is faster.  The two roofs are computed from the shape:
  `*_hbm_us`  the bytes the native passes must move (fwd: x in, y out; fwd_bwd adds the hidden activations out and in, g in,
              every dZ_l out and in again for the weight gradient, x in again, dx out) over the stream rate measured in this
              run (`stream_gbps`: a device-to-device copy of 1 GiB, bytes read + written over its time);
  `*_mfma_us` the FLOPs of the padded MFMA tiles the kernels issue (fwd: 2 N sum_l pad32(out_l) pad16(in_l); the backward about
              twice that) over the dense fp16 / bf16 MFMA rate of MI355X_MICROARCH.md (2.5 PFLOP/s, the spec at peak clock)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from nerfacc_amd.mlp import FusedMLP, layer_dims  # noqa: E402

SHAPES = {"base": (32, 16, 64, 1), "head": (32, 3, 64, 2), "proposal": (10, 1, 64, 1)}
MFMA_FLOPS = 2.5e15


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
    return row


def stream_rate():
    """Bytes per second of a device-to-device copy of 1 GiB (read + write)."""
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    us = min(timed(lambda: dst.copy_(src), 10) for _ in range(3))
    return 2 * src.numel() / (us * 1e-6)


def roofs(shape, N, stream):
    n_in, n_out, W, n_hidden = shape
    dims = layer_dims(*shape)
    pad = lambda v, m: -(-v // m) * m
    fwd_flops = 2 * N * sum(pad(o, 32) * pad(i, 16) for o, i in dims)
    # data gradient: the transposed products; weight gradient: [out, in] tiles of 32 x 32 over N
    bwd_flops = 2 * N * sum(pad(i, 32) * pad(o, 16) for o, i in dims) + 2 * N * sum(pad(o, 32) * pad(i, 32) for o, i in dims)
    fwd_bytes = 2 * N * (n_in + n_out)
    hid = 2 * N * W * n_hidden
    # forward with the activations saved; data gradient: g and hidden in, dz and dx out; weight gradient: x, hidden, dz, g in
    fb_bytes = fwd_bytes + hid + (2 * N * n_out + hid + hid + 2 * N * n_in) + (2 * N * n_in + hid + hid + 2 * N * n_out)
    return {"fwd_hbm_us": round(fwd_bytes / stream * 1e6, 1), "fwd_mfma_us": round(fwd_flops / MFMA_FLOPS * 1e6, 1),
            "fwd_bwd_hbm_us": round(fb_bytes / stream * 1e6, 1), "fwd_bwd_mfma_us": round((fwd_flops + bwd_flops) / MFMA_FLOPS * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    stream = stream_rate()
    for name, shape in SHAPES.items():
        n_in, n_out, W, n_hidden = shape
        for dtype in (getattr(torch, d) for d in a.dtypes):
            mlp = FusedMLP(*shape, dtype=dtype).to(dev)
            layers = []
            for o, i in layer_dims(*shape):
                layers += [nn.Linear(i, o, bias=False), nn.ReLU()]
            seq = nn.Sequential(*layers[:-1]).to(dev)
            with torch.no_grad():
                for lin, w in zip([m for m in seq if isinstance(m, nn.Linear)], mlp.linear_weights()):
                    lin.weight.copy_(w)
            for log2n in a.log2n:
                N = 1 << log2n
                x = torch.randn(N, n_in, device=dev).to(dtype).requires_grad_(True)
                g = torch.randn(N, n_out, device=dev).to(dtype)
                seq_params = list(seq.parameters())

                def fwd():
                    with torch.no_grad():
                        return mlp(x)

                def fwd_bwd():
                    return torch.autograd.grad(mlp(x), (x, mlp.params), g)

                def torch_fwd():
                    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                        return seq(x)

                def torch_fwd_bwd():
                    with torch.autocast("cuda", dtype=dtype):
                        y = seq(x)
                    return torch.autograd.grad(y, [x] + seq_params, g)

                # the two must compute the same network before their times are compared
                diff = float((fwd().float() - torch_fwd().float()).abs().max())
                row = {"shape": name, "dims": list(shape), "dtype": str(dtype).split(".")[-1], "n_points": N, "max_abs_diff_vs_torch": diff,
                       "stream_gbps": round(stream / 1e9, 1)}
                row.update(measure({"fwd": fwd, "torch_fwd": torch_fwd, "fwd_bwd": fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd},
                                   a.window_ms, a.windows))
                row["fwd_ratio"] = round(row["torch_fwd_us"] / row["fwd_us"], 2)
                row["fwd_bwd_ratio"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
                row.update(roofs(shape, N, stream))
                print(json.dumps(row), flush=True)
                del x, g


if __name__ == "__main__":
    main()
