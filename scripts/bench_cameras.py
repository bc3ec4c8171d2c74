#!/usr/bin/env python3
"""Times the lens-undistortion kernels (csrc/camera.hip) with HIP events and prints one JSON line.
    python scripts/bench_cameras.py [--reps 50] [--sizes 20,24]
For 2^k points: OpenCV (8 parameters, Newton, 10 steps) and fisheye (4 parameters), each with one shared parameter set
and with one set per point.  Inputs are in the tests' regime (|uv| <= 0.8, small k), so every Newton loop runs until its
convergence test.  Bytes counted: 8 B read + 8 B written per point, plus the per-point parameters (32 B / 16 B)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="20,24")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cameras.py needs the GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": 10, "eps": 1e-6, "runs": []}
    for log2 in (int(s) for s in args.sizes.split(",")):
        n = 1 << log2
        rho = 0.8 * np.sqrt(rng.uniform(0, 1, n))
        phi = rng.uniform(0, 2 * np.pi, n)
        uv = torch.from_numpy(np.stack([rho * np.cos(phi), rho * np.sin(phi)], -1).astype(np.float32)).to(dev)
        out = torch.empty_like(uv)
        for kind, n_params, fn in (("opencv", 8, "nfa_opencv_lens_undistortion"),
                                   ("fisheye", 4, "nfa_opencv_lens_undistortion_fisheye")):
            for shared in (True, False):
                p = rng.uniform(-0.02, 0.02, (1 if shared else n, n_params)).astype(np.float32)
                p[:, 0] = rng.uniform(-0.1, 0.1, p.shape[0])
                if kind == "opencv":
                    p[:, 2:4] = rng.uniform(-0.01, 0.01, (p.shape[0], 2))
                params = torch.from_numpy(p).to(dev)
                stride = 0 if shared else n_params

                def launch():
                    B.call(fn, B.ptr(uv), B.ptr(params), n, n_params, stride, 1e-6, 10, B.ptr(out), B.stream())

                for _ in range(5):
                    launch()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    launch()
                t1.record()
                torch.cuda.synchronize()
                us = t0.elapsed_time(t1) * 1e3 / args.reps
                nbytes = n * (16 + (0 if shared else 4 * n_params))
                res["runs"].append({"kind": kind, "log2_points": log2, "params": "shared" if shared else "per_point",
                                    "us": round(us, 2), "gpoints_per_s": round(n / us * 1e-3, 2),
                                    "tb_per_s": round(nbytes / us * 1e-6, 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
