#!/usr/bin/env python3
"""Times the fused MLP's second order (csrc/mlp.hip: nfa_mlp_tangent plus nfa_mlp_bwd_weights on the tangent activations,
`FusedMLP(second_order=True)`) against the same network as `nn.Sequential` of `nn.Linear(bias=False)` / `nn.ReLU` under
`torch.autocast` on the same GPU, at the base network 32 -> 64 -> 16 and an SDF head 32 -> 64 -> 64 -> 1 for N = 2^20 points,
and prints one JSON line per (shape, N, dtype).
    python scripts/bench_mlp_grad2.py [--log2n 20] [--dtypes float16 bfloat16] [--window-ms 200] [--windows 5]
Inputs, output gradients and the cotangent v of dL/dx are of the half type.  Per line, native and baseline (`torch_*`) taking
turns window by window in one process, as scripts/bench_mlp.py measures (a window is as many calls as fill `--window-ms` of
device time between two HIP events; `*_us` is the median of the windows' means, `*_spread` their (min, max)):
  `pass2`    the second pass alone: the gradients of <v, dL/dx> towards the parameters and dL/dy, on a graph built once
             (`retain_graph=True`): natively the tangent launch and the weight gradient's two;
  `eikonal`  the whole step y -> dL/dx (create_graph=True) -> loss(dL/dx).backward(), loss = mean((|dL/dx| - 1)^2), gradients
             towards the parameters;
  `fwd_bwd`  forward + first-order backward towards x and the parameters, the yardstick the second pass is compared with.
`*_ratio` is the baseline's time over the native one: above 1 the native pass is faster."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from bench_mlp import measure  # noqa: E402
from nerfacc_amd.mlp import FusedMLP, layer_dims  # noqa: E402

SHAPES = {"base": (32, 16, 64, 1), "sdf_head": (32, 1, 64, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[20])
    ap.add_argument("--dtypes", nargs="+", default=["float16", "bfloat16"])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_grad2.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    for name, shape in SHAPES.items():
        n_in, n_out, W, n_hidden = shape
        for dtype in (getattr(torch, d) for d in a.dtypes):
            mlp = FusedMLP(*shape, dtype=dtype, second_order=True).to(dev)
            layers = []
            for o, i in layer_dims(*shape):
                layers += [nn.Linear(i, o, bias=False), nn.ReLU()]
            seq = nn.Sequential(*layers[:-1]).to(dev)
            with torch.no_grad():
                for lin, w in zip([m for m in seq if isinstance(m, nn.Linear)], mlp.linear_weights()):
                    lin.weight.copy_(w)
            seq_params = list(seq.parameters())
            for log2n in a.log2n:
                N = 1 << log2n
                x = torch.randn(N, n_in, device=dev).to(dtype).requires_grad_(True)
                g = torch.randn(N, n_out, device=dev).to(dtype).requires_grad_(True)
                v = torch.randn(N, n_in, device=dev).to(dtype)

                def native(xx):
                    return mlp(xx)

                def baseline(xx):
                    with torch.autocast("cuda", dtype=dtype):
                        return seq(xx)

                def eikonal(net, params):
                    (n,) = torch.autograd.grad(net(x), x, g.detach(), create_graph=True)
                    return torch.autograd.grad(((n.float().norm(dim=-1) - 1.0) ** 2).mean(), params)

                # the second pass alone: one graph each, differentiated again and again
                (gx_native,) = torch.autograd.grad(native(x), x, g, create_graph=True)
                (gx_torch,) = torch.autograd.grad(baseline(x), x, g, create_graph=True)
                passes = {
                    "pass2": lambda: torch.autograd.grad(gx_native, [mlp.params, g], v, retain_graph=True),
                    "torch_pass2": lambda: torch.autograd.grad(gx_torch, seq_params + [g], v, retain_graph=True),
                    "eikonal": lambda: eikonal(native, [mlp.params]),
                    "torch_eikonal": lambda: eikonal(baseline, seq_params),
                    "fwd_bwd": lambda: torch.autograd.grad(native(x), (x, mlp.params), g.detach()),
                    "torch_fwd_bwd": lambda: torch.autograd.grad(baseline(x), [x] + seq_params, g.detach()),
                }
                # the two must compute the same thing before their times are compared
                u_n, u_t = passes["pass2"]()[-1], passes["torch_pass2"]()[-1]
                row = {"shape": name, "dims": list(shape), "dtype": str(dtype).split(".")[-1], "n_points": N,
                       "max_abs_diff_u_vs_torch": float((u_n.float() - u_t.float()).abs().max())}
                row.update(measure(passes, a.window_ms, a.windows))
                for k in ("pass2", "eikonal", "fwd_bwd"):
                    row[k + "_ratio"] = round(row["torch_" + k + "_us"] / row[k + "_us"], 2)
                row["pass2_over_fwd_bwd"] = round(row["pass2_us"] / row["fwd_bwd_us"], 2)
                print(json.dumps(row), flush=True)
                del x, g, v, gx_native, gx_torch, passes


if __name__ == "__main__":
    main()
