#!/usr/bin/env python3
"""Generate tests/golden/sinusoidal.npz from the reference's SinusoidalEncoder (examples/radiance_fields/mlp.py), on CPU.

Run from the repo root with the reference checkout (nerfacc 0.5.3) given on the command line:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_sinusoidal_golden.py <reference checkout>

Case i holds c{i}_cfg = (x_dim, min_deg, max_deg, use_identity) as int64, c{i}_x [64, x_dim] float32 and c{i}_y, the
reference's float32 output.  Cases: the four distinct encoders the reference's MLP fields build ((3,0,10) and (3,0,4):
VanillaNeRFRadianceField; (3,0,4) and (1,0,4): TNeRFRadianceField; (2,0,4) and (1,0,4): NDRTNeRFRadianceField) with x
uniform in [-1.5, 1.5], the position encoder (3,0,10) once more with |x| <= 1000, and the two corners of the native
encoding's range, (3,0,16,True) and (4,0,8,False).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
# (cfg, span of x)
CASES = [((3, 0, 10, True), 1.5), ((3, 0, 4, True), 1.5), ((1, 0, 4, True), 1.5), ((2, 0, 4, True), 1.5),
         ((3, 0, 10, True), 1000.0), ((3, 0, 16, True), 1.5), ((4, 0, 8, False), 1.5)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("ref_mlp", os.path.join(sys.argv[1], "examples", "radiance_fields", "mlp.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20240917)
    out = {"n_cases": np.int64(len(CASES))}
    for i, ((D, lo, hi, ident), span) in enumerate(CASES):
        x = rng.uniform(-span, span, size=(N, D)).astype(np.float32)
        enc = ref.SinusoidalEncoder(D, lo, hi, ident)
        with torch.no_grad():
            y = enc(torch.from_numpy(x))
        assert y.shape == (N, enc.latent_dim) and y.dtype == torch.float32
        out.update({f"c{i}_cfg": np.array([D, lo, hi, int(ident)], np.int64), f"c{i}_x": x, f"c{i}_y": y.numpy()})
    path = os.path.join(ROOT, "tests", "golden", "sinusoidal.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
