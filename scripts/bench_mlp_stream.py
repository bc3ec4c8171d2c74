#!/usr/bin/env python3
"""Times the streamed-weight fused MLP (csrc/mlp_stream.hip, nerfacc_amd.mlp.StreamedMLP / NerfMLP) against the same networks
written here as `nn.Linear` / `ReLU` / `cat` under `torch.autocast`, in the same process on the same GPU:
  trunk        63 -> 8 x 256 -> 257, the input appended after hidden layer 4, biases (NeRF's trunk with its merged output layer);
  colour_head  283 -> 128 -> 3, biases;
  nerf_mlp     the whole NerfMLP(63, 27): trunk, split, cat with the condition, colour head.
    python scripts/bench_mlp_stream.py [--log2n 18 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5] [--nets ...]
One JSON line per (network, N, dtype), measured as scripts/bench_mlp.py measures: `fwd` without autograd and `fwd_bwd` towards
x and the parameters, native and baseline (`torch_*`) taking turns window by window; a window is as many calls as fill
`--window-ms` of device time between two HIP events; `*_us` is the median of the windows' means, `*_spread` their (min, max);
`*_ratio` is the baseline's time over the native one (above 1 the native pass is faster).  Beside them
  `*_mfma_us`      the FLOPs of the padded MFMA tiles over the dense fp16 / bf16 MFMA rate of 2.5 PFLOP/s (forward: 2 N
                   sum_l pad32(out_l) pad16(in_l); the backward about twice that);
  `fwd_lds_gb`, `bwd_lds_gb`  the bytes of packed image a pass pulls through the LDS: ceil(N / 128) image passes of the forward
                   image, of the backward image for the data gradient (NFA_MLP_STREAM_POINTS = 128 points per pass)."""
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

from nerfacc_amd.mlp import STREAM_POINTS, NerfMLP, StreamedMLP, image_elems, layer_dims  # noqa: E402

MFMA_FLOPS = 2.5e15
TRUNK = dict(n_input_dims=63, n_output_dims=257, n_neurons=256, n_hidden_layers=8, skip_layer=4)
HEAD = dict(n_input_dims=283, n_output_dims=3, n_neurons=128, n_hidden_layers=1, skip_layer=None)


class TorchMLP(nn.Module):
    """The same network in torch: Linear + ReLU, the input appended where the module's skip_mask says."""

    def __init__(self, m: StreamedMLP):
        super().__init__()
        self.skip_mask = m.skip_mask
        self.layers = nn.ModuleList(nn.Linear(i, o) for o, i in m._dims)
        with torch.no_grad():
            for lin, w, b in zip(self.layers, m.linear_weights(), m.linear_biases()):
                lin.weight.copy_(w)
                lin.bias.copy_(b)

    def forward(self, x):
        h = x
        for l, lin in enumerate(self.layers):
            if (self.skip_mask >> l) & 1:
                h = torch.cat([h, x], -1)
            h = lin(h)
            if l < len(self.layers) - 1:
                h = torch.relu(h)
        return h


class TorchNerf(nn.Module):
    def __init__(self, m: NerfMLP):
        super().__init__()
        self.trunk, self.head, self.W = TorchMLP(m.trunk), TorchMLP(m.head), m.net_width

    def forward(self, x, c):
        y = self.trunk(x)
        return self.head(torch.cat([y[:, :self.W], c.to(y.dtype)], -1)), y[:, self.W:]


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


def roofs(mods, N):
    pad = lambda v, m: -(-v // m) * m
    fwd_flops = bwd_flops = fwd_img = bwd_img = 0
    for m in mods:
        dims = m._dims
        fwd_flops += 2 * N * sum(pad(o, 32) * pad(i, 16) for o, i in dims)
        bwd_flops += 2 * N * sum(pad(i, 32) * pad(o, 16) for o, i in dims) + 2 * N * sum(pad(o, 32) * pad(i, 32) for o, i in dims)
        fe, be = image_elems(m.n_input_dims, m.n_output_dims, m.n_neurons, m.n_hidden_layers, m.skip_mask)
        fwd_img, bwd_img = fwd_img + 2 * fe, bwd_img + 2 * be
    passes = -(-N // STREAM_POINTS)
    return {"fwd_mfma_us": round(fwd_flops / MFMA_FLOPS * 1e6, 1), "fwd_bwd_mfma_us": round((fwd_flops + bwd_flops) / MFMA_FLOPS * 1e6, 1),
            "fwd_image_kib": fwd_img // 1024, "bwd_image_kib": bwd_img // 1024,
            "fwd_lds_gb": round(passes * fwd_img / 1e9, 2), "bwd_lds_gb": round(passes * bwd_img / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--nets", nargs="+", default=["trunk", "colour_head", "nerf_mlp"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_stream.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    for net in a.nets:
        for dtype in (getattr(torch, d) for d in a.dtypes):
            if net == "nerf_mlp":
                mod = NerfMLP(63, 27, dtype=dtype).to(dev)
                ref, mods, n_in, n_out = TorchNerf(mod).to(dev), [mod.trunk, mod.head], 63, 3
            else:
                mod = StreamedMLP(dtype=dtype, **(TRUNK if net == "trunk" else HEAD)).to(dev)
                ref, mods, n_in, n_out = TorchMLP(mod).to(dev), [mod], mod.n_input_dims, mod.n_output_dims
            params, ref_params = list(mod.parameters()), list(ref.parameters())
            for log2n in a.log2n:
                N = 1 << log2n
                x = torch.randn(N, n_in, device=dev).to(dtype).requires_grad_(True)
                extra = (torch.randn(N, 27, device=dev).to(dtype),) if net == "nerf_mlp" else ()
                g = torch.randn(N, n_out, device=dev).to(dtype)
                gs = (g, torch.randn(N, 1, device=dev).to(dtype)) if net == "nerf_mlp" else (g,)
                outs = (lambda y: list(y)) if net == "nerf_mlp" else (lambda y: [y])

                def fwd():
                    with torch.no_grad():
                        return mod(x, *extra)

                def fwd_bwd():
                    return torch.autograd.grad(outs(mod(x, *extra)), [x] + params, gs)

                def torch_fwd():
                    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                        return ref(x, *extra)

                def torch_fwd_bwd():
                    with torch.autocast("cuda", dtype=dtype):
                        y = ref(x, *extra)
                    return torch.autograd.grad(outs(y), [x] + ref_params, gs)

                # the two must compute the same network before their times are compared
                diff = float((outs(fwd())[0].float() - outs(torch_fwd())[0].float()).abs().max())
                row = {"net": net, "dtype": str(dtype).split(".")[-1], "n_points": N, "max_abs_diff_vs_torch": diff}
                row.update(measure({"fwd": fwd, "torch_fwd": torch_fwd, "fwd_bwd": fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd},
                                   a.window_ms, a.windows))
                row["fwd_ratio"] = round(row["torch_fwd_us"] / row["fwd_us"], 2)
                row["fwd_bwd_ratio"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
                row.update(roofs(mods, N))
                print(json.dumps(row), flush=True)
                del x, g, gs, extra


if __name__ == "__main__":
    main()
