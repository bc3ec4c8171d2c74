#!/usr/bin/env python3
"""Times the fused MLP with activations (csrc/mlp.hip: the nfa_mlp_act_* entries, nerfacc_amd.mlp.FusedMLP(activation=...))
at N = 2^20 points, fp16 and bf16, and prints one JSON line per (network, dtype):
  sdf   32 -> 64 -> 64 -> 1, biases, Softplus (beta 100) hidden layers: forward, forward + backward, and forward + backward +
        second order (an Eikonal-style step: ds/dparams, ds/dx and ds/dg of s = <v, dL/dx>);
  head  32 -> 64 -> 64 -> 3, ReLU hidden layers and a Sigmoid output: forward, forward + backward.
Each against the same network as `nn.Sequential` under `torch.autocast` (`torch_*`; its second order is torch's double
backward) and against the same FusedMLP with ReLU / no output activation (`relu_*`: the price of the transcendentals).
    python scripts/bench_mlp_act.py [--log2n 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5]
Windows, medians and spreads are those of scripts/bench_mlp.py: the passes take turns window by window in one process, a window
is as many calls as fill --window-ms of device time between two HIP events, `*_us` is the median of the windows' means and
`*_spread` their (min, max).  `*_ratio` is torch's time over the native one: above 1 the native pass is faster."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from bench_mlp import measure  # noqa: E402
from nerfacc_amd.mlp import FusedMLP, layer_dims  # noqa: E402

NETS = {"sdf": dict(shape=(32, 1, 64, 2), bias=True, activation="Softplus", output_activation="None", beta=100.0, second=True),
        "head": dict(shape=(32, 3, 64, 2), bias=False, activation="ReLU", output_activation="Sigmoid", beta=10.0, second=False)}
TORCH_ACT = {"ReLU": lambda b: nn.ReLU(), "Softplus": lambda b: nn.Softplus(beta=b), "Sigmoid": lambda b: nn.Sigmoid(), "None": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_act.py measures on a GPU; none is available")
    dev, N = torch.device("cuda"), 1 << a.log2n
    for name, net in NETS.items():
        shape, bias = net["shape"], net["bias"]
        for dtype in (getattr(torch, d) for d in a.dtypes):
            mlp = FusedMLP(*shape, dtype=dtype, bias=bias, second_order=net["second"], activation=net["activation"],
                           output_activation=net["output_activation"], activation_beta=net["beta"]).to(dev)
            relu = FusedMLP(*shape, dtype=dtype, bias=bias, second_order=net["second"]).to(dev)
            layers = []
            for l, (o, i) in enumerate(layer_dims(*shape)):
                layers.append(nn.Linear(i, o, bias=bias))
                act = TORCH_ACT[net["activation"] if l < shape[3] else net["output_activation"]]
                if act is not None:
                    layers.append(act(net["beta"]))
            seq = nn.Sequential(*layers).to(dev)
            with torch.no_grad():
                relu.params.copy_(mlp.params)
                for lin, w in zip([m for m in seq if isinstance(m, nn.Linear)], mlp.linear_weights()):
                    lin.weight.copy_(w)
                    if bias:
                        lin.bias.zero_()
            seq_params = list(seq.parameters())
            x = torch.randn(N, shape[0], device=dev).to(dtype).requires_grad_(True)
            g = torch.randn(N, shape[1], device=dev).to(dtype).requires_grad_(True)
            v = torch.randn(N, shape[0], device=dev).to(dtype)

            def native(m):
                def fwd():
                    with torch.no_grad():
                        return m(x)

                def fwd_bwd():
                    return torch.autograd.grad(m(x), (x, m.params), g)

                def fwd_bwd_2nd():
                    (g_x,) = torch.autograd.grad(m(x), x, g, create_graph=True)
                    return torch.autograd.grad(g_x, (m.params, g) + ((x,) if m._curved else ()), v)
                return fwd, fwd_bwd, fwd_bwd_2nd

            def torch_fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
                    return seq(x)

            def torch_fwd_bwd():
                with torch.autocast("cuda", dtype=dtype):
                    y = seq(x)
                return torch.autograd.grad(y, [x] + seq_params, g)

            def torch_fwd_bwd_2nd():
                with torch.autocast("cuda", dtype=dtype):
                    y = seq(x)
                (g_x,) = torch.autograd.grad(y, x, g, create_graph=True)
                return torch.autograd.grad(g_x, seq_params + [g, x], v, allow_unused=True)

            fwd, fwd_bwd, fwd_bwd_2nd = native(mlp)
            r_fwd, r_fwd_bwd, r_fwd_bwd_2nd = native(relu)
            diff = float((fwd().float() - torch_fwd().float()).abs().max())   # the two compute the same network
            passes = {"fwd": fwd, "torch_fwd": torch_fwd, "relu_fwd": r_fwd, "fwd_bwd": fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd,
                      "relu_fwd_bwd": r_fwd_bwd}
            if net["second"]:
                passes.update({"fwd_bwd_2nd": fwd_bwd_2nd, "torch_fwd_bwd_2nd": torch_fwd_bwd_2nd, "relu_fwd_bwd_2nd": r_fwd_bwd_2nd})
            row = {"net": name, "dims": list(shape), "activation": net["activation"], "output_activation": net["output_activation"],
                   "beta": net["beta"], "dtype": str(dtype).split(".")[-1], "n_points": N, "max_abs_diff_vs_torch": diff}
            row.update(measure(passes, a.window_ms, a.windows))
            for k in ("fwd", "fwd_bwd") + (("fwd_bwd_2nd",) if net["second"] else ()):
                row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
                row[k + "_over_relu"] = round(row[k + "_us"] / row["relu_" + k + "_us"], 2)
            print(json.dumps(row), flush=True)
            del x, g, v


if __name__ == "__main__":
    main()
