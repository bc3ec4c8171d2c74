#!/usr/bin/env python3
"""Writes tests/golden/ref_mlp.npz from the reference's own ``MLP`` class (examples/radiance_fields/mlp.py), on the CPU:
    python scripts/gen_mlp_golden.py /path/to/the/reference/checkout
Two networks, each with an exact integer family and with Xavier weights, run in float64 on N = 33 points:
  warp  T-NeRF's warp network, 36 -> 4 x 64 -> 3, skip_layer=2, biases;
  wide  40 -> 128 -> 3, biases, no skip.
Stored per case `<net>_<exact|xavier>/`: the constructor arguments, the state dict (`sd/<key>`), `x`, `g`, and the reference's
`y`, `dx` (dL/dx) and `grad/<key>` (dL/dparams) for that fixed `g`.  Data only; no test imports this script.
  exact   the 'dense' family and the integer biases of tests/mlp_bias_skip_reference.py, integer inputs: every number of the
          float64 run is a small integer, stored as int8 / int16; the module must reproduce them bit for bit.
  xavier  the reference's own initialisation (Xavier uniform), then weights rounded to multiples of 2^-8 and x, g to multiples of
          2^-5 inside +-4, so that fp16 and bf16 both hold the inputs exactly and the only difference between the reference's
          float64 run and the half-precision passes is the rounding the tests' bound derives; biases uniform in +-0.5, float32
          (a bias is never rounded).  Weights, x and g are stored as their int8 numerators beside `w_scale` = 256 and `x_scale` =
          32 (1 in the exact cases), biases and the reference's float64 results as float32."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlp_bias_skip_reference as S  # noqa: E402
import mlp_reference as R  # noqa: E402

N = 33
NETS = {"warp": dict(input_dim=36, output_dim=3, net_depth=4, net_width=64, skip_layer=2),
        "wide": dict(input_dim=40, output_dim=3, net_depth=1, net_width=128, skip_layer=None)}


def small_int(a):
    a = np.asarray(a)
    r = np.rint(a)
    assert np.array_equal(r, a), "not integer-valued"
    for t in (np.int8, np.int16, np.int32):
        if np.abs(r).max(initial=0) <= np.iinfo(t).max:
            return r.astype(t)
    raise ValueError("too large")


def main():
    spec = importlib.util.spec_from_file_location("ref_mlp", os.path.join(sys.argv[1], "examples", "radiance_fields", "mlp.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for net, kw in NETS.items():
        for kind in ("exact", "xavier"):
            torch.manual_seed(20 + len(out))
            mlp = ref.MLP(**kw)
            names = [f"hidden_layers.{i}" for i in range(kw["net_depth"])] + ["output_layer"]
            sd = mlp.state_dict()
            if kind == "exact":
                shape = (kw["input_dim"], kw["output_dim"], kw["net_width"], kw["net_depth"])
                ws = S.exact_weights("dense", *shape, S.skip_mask_of(kw["skip_layer"], kw["net_depth"]))
                bs = S.exact_biases(kw["output_dim"], kw["net_width"], kw["net_depth"])
                for n, w, b in zip(names, ws, bs):
                    assert sd[n + ".weight"].shape == w.shape, (n, sd[n + ".weight"].shape, w.shape)
                    sd[n + ".weight"], sd[n + ".bias"] = w, b
                x, g = R.exact_inputs(N, kw["input_dim"], kw["output_dim"], torch.float32, torch.float32)
            else:
                gen = torch.Generator().manual_seed(7)
                for n in names:
                    sd[n + ".weight"] = torch.round(sd[n + ".weight"] * 256) / 256
                    sd[n + ".bias"] = torch.rand(sd[n + ".bias"].shape, generator=gen) - 0.5
                q = lambda t: (torch.round(t * 32) / 32).clamp(-127 / 32, 127 / 32)
                x, g = q(torch.randn(N, kw["input_dim"], generator=gen)), q(torch.randn(N, kw["output_dim"], generator=gen))
            mlp.load_state_dict(sd)
            mlp = mlp.double()
            xd = x.double().requires_grad_(True)
            y = mlp(xd)
            params = dict(mlp.named_parameters())
            grads = torch.autograd.grad(y, [xd] + list(params.values()), g.double())
            conv = small_int if kind == "exact" else (lambda a: np.asarray(a, dtype=np.float32))
            w_scale, x_scale = (1, 1) if kind == "exact" else (256, 32)
            pre = f"{net}_{kind}/"
            for k, v in kw.items():
                out[pre + k] = np.int32(v or 0)
            out[pre + "w_scale"], out[pre + "x_scale"] = np.int32(w_scale), np.int32(x_scale)
            for k, v in sd.items():
                out[pre + "sd/" + k] = small_int(v.numpy() * w_scale) if k.endswith("weight") else conv(v.numpy())
            out[pre + "x"], out[pre + "g"] = small_int(x.numpy() * x_scale), small_int(g.numpy() * x_scale)
            out[pre + "y"], out[pre + "dx"] = conv(y.detach().numpy()), conv(grads[0].numpy())
            for k, gr in zip(params, grads[1:]):
                out[pre + "grad/" + k] = conv(gr.numpy())
    path = os.path.join(ROOT, "tests", "golden", "ref_mlp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
