#!/usr/bin/env python3
"""Measures how far the device's float32 evaluation of each smooth activation of the fused MLP (csrc/mlp_tiles.h: act_value,
built on expf, log1pf, tanhf) is from float64, in ulps of float32 of the result: the constants C_F of tests/mlp_act_reference.py
are twice the worst value printed here.
    python scripts/measure_mlp_act_ulps.py
The probe is the forward entry itself: a 1 -> 64 -> 1 network with hidden activation None whose first matrix copies x into one
neuron and whose output matrix scales it by w, so z = w * x is an exact float32 product of two fp16 numbers, and a float32
output: y = f_out(z) as the kernel computes it, unrounded.  x runs over every fp16 number with |x| <= 8 and w over a few
factors whose products fill the float32 mantissa; the pre-activations of the tests stay within |z| < 8."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nerfacc_amd.mlp import FusedMLP  # noqa: E402

FACTORS = (1.0, 0.99951171875, 0.7939453125, 0.333251953125, 0.0626220703125)


def f64(name, z, beta):
    if name == "Sigmoid":
        return torch.sigmoid(z)
    if name == "Tanh":
        return torch.tanh(z)
    if name == "Softplus":
        return z.clamp_min(0) + torch.log1p(torch.exp(-beta * z.abs())) / beta
    return torch.exp(z)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("measure_mlp_act_ulps.py measures on a GPU; none is available")
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16)
    x = x[torch.isfinite(x) & (x.abs() <= 8)].view(-1, 1).contiguous()
    for name, beta in [("Sigmoid", 10.0), ("Tanh", 10.0), ("Softplus", 10.0), ("Softplus", 100.0), ("Exponential", 10.0)]:
        worst, worst_z, n = 0.0, 0.0, 0
        for w in FACTORS:
            m = FusedMLP(1, 1, 64, 1, out_dtype=torch.float32, activation="None", output_activation=name, activation_beta=beta)
            w0, w1 = torch.zeros(64, 1), torch.zeros(1, 64)
            w0[0, 0], w1[0, 0] = 1.0, w
            m.load_linear_weights([w0, w1])
            with torch.no_grad():
                y = m.cuda()(x.cuda()).cpu().double().view(-1)
            z = x.double().view(-1) * w
            want = f64(name, z, beta)
            e = torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))).clamp_min(-126)
            err = (y - want).abs() / torch.exp2(e - 23)
            err = torch.where(torch.isfinite(err), err, torch.zeros_like(err))
            k = int(err.argmax())
            if float(err[k]) > worst:
                worst, worst_z = float(err[k]), float(z[k])
            n += z.numel()
        print(json.dumps({"activation": name, "beta": beta, "samples": n, "worst_ulp32": round(worst, 3), "at_z": worst_z}), flush=True)


if __name__ == "__main__":
    main()
