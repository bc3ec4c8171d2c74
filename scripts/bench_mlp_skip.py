#!/usr/bin/env python3
"""Times FusedMLP with biases and skip connections (csrc/mlp.hip behind nfa_mlp_desc) against the same network as a torch
module (`nn.Linear(bias=True)`, `torch.cat`, ReLU: the reference's `MLP` forward written out) under `torch.autocast` on the
same GPU, and prints one JSON line per (shape, dtype).
    python scripts/bench_mlp_skip.py [--log2n 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5]
Shapes: T-NeRF's warp network 36 -> 4 x 64 -> 3 with skip_layer=2 and biases, and the SDF head 32 -> 64 -> 64 -> 1 with biases.
Passes: the forward without autograd (`fwd`), forward + backward towards x and the parameters (`fwd_bwd`) and, for the SDF
head, the Eikonal step `y -> dL/dx (create_graph) -> mean((|dL/dx| - 1)^2).backward()` (`eikonal`); native and baseline
(`torch_*`) take turns window by window, measured as scripts/bench_mlp.py measures (its `measure`): windows of `--window-ms`
of device time between two HIP events, the median of the windows' means, half inputs and output gradients.  `*_hbm_us` is
the time the bytes the native passes must move take at the stream rate measured in this run (a device-to-device copy of
1 GiB), computed as bench_mlp.py computes it; a cat layer reads x once more in the forward and in the weight gradient and the
biases are a few hundred bytes, so the roofs are those of the plain chain plus 2 N n_in bytes per cat layer and pass."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from bench_mlp import measure, stream_rate  # noqa: E402
from nerfacc_amd.mlp import FusedMLP  # noqa: E402

SHAPES = {"warp": (36, 3, 64, 4, 2), "sdf_head": (32, 1, 64, 2, None)}   # n_in, n_out, width, n_hidden, skip_layer


class TorchMLP(nn.Module):
    """The reference's MLP forward: Linear, ReLU, and cat([h, x]) after hidden layer i when i > 0 and i % skip_layer == 0."""

    def __init__(self, mlp: FusedMLP):
        super().__init__()
        self.skip_layer = mlp.skip_layer
        self.layers = nn.ModuleList(nn.Linear(w.shape[1], w.shape[0], bias=True) for w in mlp.linear_weights())
        with torch.no_grad():
            for lin, w, b in zip(self.layers, mlp.linear_weights(), mlp.linear_biases()):
                lin.weight.copy_(w)
                lin.bias.copy_(b)

    def forward(self, x):
        h = x
        for i, lin in enumerate(self.layers[:-1]):
            h = torch.relu(lin(h))
            if self.skip_layer is not None and i % self.skip_layer == 0 and i > 0:
                h = torch.cat([h, x], dim=-1)
        return self.layers[-1](h)


def roofs(mlp, N, stream):
    n_in, n_out, W, n_hidden = mlp._shape
    cats = bin(mlp.skip_mask).count("1")
    fwd_bytes = 2 * N * (n_in + n_out) + 2 * N * n_in * cats
    hid = 2 * N * W * n_hidden
    # forward with the activations saved; data gradient: g and hidden in, dz and dx out (a cat layer's dz in again); weight
    # gradient: x, hidden, dz, g in (x once more per cat layer)
    fb_bytes = fwd_bytes + hid + (2 * N * n_out + hid + hid + 2 * N * n_in + 2 * N * W * cats) + (2 * N * n_in * (1 + cats) + hid + hid + 2 * N * n_out)
    return {"fwd_hbm_us": round(fwd_bytes / stream * 1e6, 1), "fwd_bwd_hbm_us": round(fb_bytes / stream * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_skip.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    stream = stream_rate()
    N = 1 << a.log2n
    for name, (n_in, n_out, W, n_hidden, skip_layer) in SHAPES.items():
        for dtype in (getattr(torch, d) for d in a.dtypes):
            mlp = FusedMLP(n_in, n_out, W, n_hidden, dtype=dtype, bias=True, skip_layer=skip_layer, second_order=True).to(dev)
            with torch.no_grad():
                mlp.params[mlp._offsets[-1]:].uniform_(-0.5, 0.5)
            ref = TorchMLP(mlp).to(dev)
            ref_params = list(ref.parameters())
            x = torch.randn(N, n_in, device=dev).to(dtype).requires_grad_(True)
            g = torch.randn(N, n_out, device=dev).to(dtype)

            def fwd():
                with torch.no_grad():
                    return mlp(x)

            def fwd_bwd():
                return torch.autograd.grad(mlp(x), (x, mlp.params), g)

            def torch_fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                    return ref(x)

            def torch_fwd_bwd():
                with torch.autocast("cuda", dtype=dtype):
                    y = ref(x)
                return torch.autograd.grad(y, [x] + ref_params, g)

            def eikonal_of(net, params, autocast):
                def step():
                    with torch.autocast("cuda", dtype=dtype, enabled=autocast):
                        y = net(x)
                    (n,) = torch.autograd.grad(y.float().sum(), x, create_graph=True)
                    return torch.autograd.grad(((n.float().norm(dim=-1) - 1.0) ** 2).mean(), params)
                return step

            passes = {"fwd": fwd, "torch_fwd": torch_fwd, "fwd_bwd": fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
            if name == "sdf_head":
                n_w = mlp._offsets[-1]
                passes["eikonal"] = eikonal_of(mlp, [mlp.params], False)
                passes["torch_eikonal"] = eikonal_of(ref, [p for p in ref_params if p.dim() == 2], True)   # d/db is zero
                assert not bool(passes["eikonal"]()[0][n_w:].any())
            # the two must compute the same network before their times are compared
            diff = float((fwd().float() - torch_fwd().float()).abs().max())
            row = {"shape": name, "dims": [n_in, n_out, W, n_hidden], "skip_layer": skip_layer, "bias": True, "dtype": str(dtype).split(".")[-1],
                   "n_points": N, "max_abs_diff_vs_torch": diff, "stream_gbps": round(stream / 1e9, 1)}
            row.update(measure(passes, a.window_ms, a.windows))
            for k in ("fwd", "fwd_bwd") + (("eikonal",) if name == "sdf_head" else ()):
                row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
            row.update(roofs(mlp, N, stream))
            print(json.dumps(row), flush=True)
            del x, g


if __name__ == "__main__":
    main()
