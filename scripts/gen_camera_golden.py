#!/usr/bin/env python3
"""Generate tests/golden/cameras.npz from the reference's torch camera functions (nerfacc/cameras.py).

Run from the repo root with the reference (leejaeyong7/nerfacc 0.5.3) on the path, as for oracle/gen_golden.py:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python scripts/gen_camera_golden.py

The reference's native undistortion needs its CUDA extension, so the fixture holds the outputs of its torch functions
only: _opencv_lens_undistortion (Newton in torch), _opencv_lens_distortion and _opencv_lens_distortion_fisheye, on CPU.
Inputs stay in a realistic regime where Newton converges: uv in the disc |uv| <= 0.8, |k1| <= 0.1, |k2..k6| <= 0.02,
|p| <= 0.01, fisheye |k| <= 0.05.  Wider draws (uv over the whole [-1, 1] square with every |k| <= 0.1) contain points
that have no undistorted preimage at all -- the radial map x d(|x|^2) stops increasing before it reaches them -- so no
solver can round-trip them (DESIGN.md "Lens undistortion").  The script asserts the round trip distortion(undistortion(uv)) == uv for every case, so a successful run is also the
check that the regime is one the solver handles.

Case i holds: c{i}_uv [*batch, 2], c{i}_params [*pbatch, P] (P in 1/2/4/8, pbatch () or batch = shared or per point),
c{i}_undist (reference undistortion, eps EPS, ITERS steps), c{i}_dist (reference distortion of uv with the parameters
padded to 8), c{i}_fe_params [*pbatch, 4] and c{i}_fe_dist (reference fisheye distortion of uv).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import nerfacc  # the reference  # noqa: E402
from nerfacc import cameras as rc  # noqa: E402

assert nerfacc.__version__ == "0.5.3", nerfacc.__version__
EPS, ITERS = 1e-6, 10
BATCHES = [(7,), (3, 50), (2, 4, 16), (256,)]
COUNTS = [1, 2, 4, 8]


def draw_params(rng, shape, count):
    # {k1, k2, p1, p2, k3, k4, k5, k6}: |k1| <= 0.1, |p| <= 0.01, the higher orders |k| <= 0.02
    full = rng.uniform(-0.02, 0.02, size=shape + (8,))
    full[..., 0] = rng.uniform(-0.1, 0.1, size=shape)
    full[..., 2:4] = rng.uniform(-0.01, 0.01, size=shape + (2,))
    return full[..., :count].astype(np.float32)


def draw_points(rng, batch):
    # uniform in the disc of radius 0.8
    rho = 0.8 * np.sqrt(rng.uniform(0.0, 1.0, size=batch))
    phi = rng.uniform(0.0, 2 * np.pi, size=batch)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi)], -1).astype(np.float32)


def main():
    rng = np.random.default_rng(20240601)
    out = {"eps": np.float32(EPS), "iters": np.int64(ITERS)}
    i = 0
    worst = 0.0
    for batch in BATCHES:
        for count in COUNTS:
            for per_point in (False, True):
                pshape = batch if per_point else ()
                uv = draw_points(rng, batch)
                params = draw_params(rng, pshape, count)
                fe = rng.uniform(-0.05, 0.05, size=pshape + (4,)).astype(np.float32)
                tuv, tp, tfe = torch.from_numpy(uv), torch.from_numpy(params), torch.from_numpy(fe)
                with torch.no_grad():
                    und = rc._opencv_lens_undistortion(tuv, tp, EPS, ITERS)
                    p8 = F.pad(tp, (0, 8 - count))
                    dist = rc._opencv_lens_distortion(tuv, p8)
                    fe_dist = rc._opencv_lens_distortion_fisheye(tuv, tfe)
                    back = rc._opencv_lens_distortion(und, p8)
                err = float((back - tuv).abs().max())
                assert err <= 1e-5, (batch, count, per_point, err)
                worst = max(worst, err)
                out.update({f"c{i}_uv": uv, f"c{i}_params": params, f"c{i}_undist": und.numpy(),
                            f"c{i}_dist": dist.numpy(), f"c{i}_fe_params": fe, f"c{i}_fe_dist": fe_dist.numpy()})
                i += 1
    out["n_cases"] = np.int64(i)
    path = os.path.join(ROOT, "tests", "golden", "cameras.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {i} cases, worst round-trip residual {worst:.3g}")


if __name__ == "__main__":
    sys.exit(main())
