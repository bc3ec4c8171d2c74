#!/usr/bin/env python3
"""Writes tests/golden/ref_nerf_mlp.npz from the reference's own ``NerfMLP`` class (examples/radiance_fields/mlp.py), on the CPU:
    python scripts/gen_nerf_mlp_golden.py /path/to/the/reference/checkout
The network of the reference's vanilla NeRF and T-NeRF fields, 63 -> 8 x 256 (input appended after hidden layer 4) with its
sigma, bottleneck and colour layers, run in float64 on N = 33 points, with a 27-wide condition and without one, each with
  exact   integer weights, biases and inputs: every number of the float64 run is a small integer, stored as int8 / int16 /
          int32; nerfacc_amd.mlp.NerfMLP must reproduce them bit for bit;
  xavier  Xavier-uniform weights rounded to multiples of 2^-8, x, condition and the output gradients multiples of 2^-5 inside
          +-4 (stored as int8 numerators beside `x_scale` = 32), biases uniform in +-0.5: both half types hold the inputs
          exactly, and the only difference to the half-precision passes is the rounding the tests' bound derives.  Results
          are stored as float32.
The 0.6 M weights are NOT stored: tests/mlp_stream_reference.py (nerf_state_dict) makes them by a deterministic rule and the
fixture holds their checksum.  Stored per case `<cond|nocond>_<exact|xavier>/`: `checksum`, `x`, `condition`, `g_rgb`, `g_sigma`
(the fixed output gradients), the reference's `raw_rgb`, `raw_sigma`, `dx`, `dcondition`, and of every parameter gradient the
row sums `rsum/<key>` and column sums `csum/<key>` (a bias gradient whole, as `rsum/<key>`).  Data only; no test imports this
script."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlp_stream_reference as Q  # noqa: E402

N, INPUT_DIM, CONDITION_DIM = 33, 63, 27


def small_int(a):
    a = np.asarray(a)
    r = np.rint(a)
    assert np.array_equal(r, a), "not integer-valued"
    for t in (np.int8, np.int16, np.int32):
        if np.abs(r).max(initial=0) <= np.iinfo(t).max:
            return r.astype(t)
    raise ValueError("too large")


def inputs(kind, condition_dim):
    n = torch.arange(N).view(-1, 1)
    if kind == "exact":
        cols = lambda k: torch.arange(k).view(1, -1)
        x = (3 * n + 5 * cols(INPUT_DIM) + 3) % 7 - 1
        c = (n + 2 * cols(max(condition_dim, 1))) % 5 - 2
        g_rgb, g_sigma = (2 * n + 3 * cols(3)) % 5 - 2, (n % 3) - 1
        return [t.float() for t in (x, c[:, :condition_dim], g_rgb, g_sigma)]
    gen = torch.Generator().manual_seed(7)
    q = lambda *s: (torch.round(torch.randn(*s, generator=gen) * 32) / 32).clamp(-127 / 32, 127 / 32)
    return [q(N, INPUT_DIM), q(N, max(condition_dim, 1))[:, :condition_dim], q(N, 3), q(N, 1)]


def main():
    spec = importlib.util.spec_from_file_location("ref_mlp", os.path.join(sys.argv[1], "examples", "radiance_fields", "mlp.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, cd in (("cond", CONDITION_DIM), ("nocond", 0)):
        for kind in ("exact", "xavier"):
            net = ref.NerfMLP(input_dim=INPUT_DIM, condition_dim=cd)
            sd = Q.nerf_state_dict(kind, INPUT_DIM, cd)
            assert set(sd) == set(net.state_dict()), sorted(set(sd) ^ set(net.state_dict()))
            net.load_state_dict(sd)
            net = net.double()
            x, c, g_rgb, g_sigma = inputs(kind, cd)
            xd = x.double().requires_grad_(True)
            cdt = c.double().requires_grad_(True)
            rgb, sigma = net(xd, cdt) if cd else net(xd)
            params = dict(net.named_parameters())
            grads = torch.autograd.grad([rgb, sigma], [xd] + ([cdt] if cd else []) + list(params.values()), [g_rgb.double(), g_sigma.double()])
            conv = small_int if kind == "exact" else (lambda a: np.asarray(a, dtype=np.float32))
            scale = 1 if kind == "exact" else 32
            pre = f"{name}_{kind}/"
            out[pre + "checksum"], out[pre + "x_scale"] = np.float64(Q.checksum(sd)), np.int32(scale)
            for k, v in (("x", x), ("condition", c), ("g_rgb", g_rgb), ("g_sigma", g_sigma)):
                out[pre + k] = small_int(v.numpy() * scale)
            out[pre + "raw_rgb"], out[pre + "raw_sigma"] = conv(rgb.detach().numpy()), conv(sigma.detach().numpy())
            out[pre + "dx"] = conv(grads[0].numpy())
            out[pre + "dcondition"] = conv(grads[1].numpy()) if cd else np.zeros((N, 0), np.float32)
            for k, gr in zip(params, grads[2 if cd else 1:]):
                if gr.dim() == 2:
                    out[pre + "rsum/" + k], out[pre + "csum/" + k] = conv(gr.sum(1).numpy()), conv(gr.sum(0).numpy())
                else:
                    out[pre + "rsum/" + k] = conv(gr.numpy())
    path = os.path.join(ROOT, "tests", "golden", "ref_nerf_mlp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
