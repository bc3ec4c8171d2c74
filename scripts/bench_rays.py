#!/usr/bin/env python3
"""Times nerfacc_amd.rays.generate_rays (csrc/rays.hip) with HIP events against the torch composition it replaces -- the
module's own fallback formulas on CUDA tensors -- on the same inputs in the same run, and prints one JSON line per case.
    python scripts/bench_rays.py [--reps 50] [--rays 1048576]
Cases: 100 cameras with random ids (a training batch; the backward sorts them on the device), the same ids sorted and
marked, and one camera (a test image); int64 pixels, OpenGL convention, normalised directions, no lens; and the 100-camera
case with an 8-parameter pinhole lens.  Forward, and forward + backward to the poses with fixed upstream gradients.
Algorithmic bytes per ray: forward 16 (x, y) [+ 8 camera id] in and 24 out; backward 16 [+ 8 id] [+ 8 order] + 24
(g_origins, g_viewdirs); the camera tables are not counted.  The fraction is of the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd.rays import _generate_rays_torch, _pad8, generate_rays, mark_sorted  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps   # ms


def cameras(n_cameras, dev, g):
    K = torch.zeros(n_cameras, 3, 3, device=dev)
    K[:, 0, 0] = K[:, 1, 1] = 1111.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 400.0, 400.0, 1.0
    q, _ = torch.linalg.qr(torch.randn(n_cameras, 3, 3, generator=g, device=dev))
    pose = torch.cat([q, torch.randn(n_cameras, 3, 1, generator=g, device=dev)], dim=-1).contiguous()
    dist = (torch.rand(n_cameras, 8, generator=g, device=dev) - 0.5) * 0.02
    return K, pose, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rays", type=int, default=1 << 20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rays.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B.load()
    n = args.rays
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randint(0, 800, (n,), generator=g, device=dev)
    y = torch.randint(0, 800, (n,), generator=g, device=dev)
    go, gw = torch.randn(n, 3, generator=g, device=dev), torch.randn(n, 3, generator=g, device=dev)
    K, pose, dist = cameras(100, dev, g)
    random_ids = torch.randint(0, 100, (n,), generator=g, device=dev)
    sorted_ids = mark_sorted(random_ids.sort().values)
    cases = {
        "100_cameras_random_ids": (K[0], pose, random_ids, None),
        "100_cameras_sorted_ids": (K[0], pose, sorted_ids, None),
        "one_camera": (K[0], pose[0].contiguous(), None, None),
        "100_cameras_random_ids_lens8": (K[0], pose, random_ids, dist),
    }
    for name, (Kc, Pc, ids, lens) in cases.items():
        kw = dict(opengl=True, pixel_center=0.5, normalize=True, eps=1e-6, iters=10)
        Pg = Pc.clone().requires_grad_(True)

        def fused(P):
            return generate_rays(x, y, Kc, P, ids, distortion=lens, **kw)

        def composed(P):
            return _generate_rays_torch(x, y, Kc, P, ids, None if lens is None else _pad8(lens), False, *kw.values())

        def fwd(fn):
            with torch.no_grad():
                return fn(Pc)

        def both(fn):
            o, w = fn(Pg)
            return torch.autograd.grad([o, w], [Pg], [go, gw])[0]

        a, b = fwd(fused), fwd(composed)
        ga, gb = both(fused), both(composed)
        fwd_b = 16 + (8 if ids is not None else 0) + 24
        bwd_b = 16 + (8 if ids is not None else 0) + (8 if ids is random_ids else 0) + 24
        row = dict(case=name, n_rays=n, fwd_bytes_per_ray=fwd_b, bwd_bytes_per_ray=bwd_b,
                   viewdirs_max_abs_diff=float((a[1] - b[1]).abs().max()), origins_equal=bool(torch.equal(a[0], b[0])),
                   grad_pose_max_rel_diff=float((ga - gb).abs().max() / gb.abs().max()))
        del a, b, ga, gb
        # alternate the two implementations
        row["fused_fwd_ms"] = timed(lambda: fwd(fused), args.reps)
        row["torch_fwd_ms"] = timed(lambda: fwd(composed), max(3, args.reps // 4))
        row["fused_fwd_bwd_ms"] = timed(lambda: both(fused), args.reps)
        row["torch_fwd_bwd_ms"] = timed(lambda: both(composed), max(3, args.reps // 4))
        row["fused_fwd_ms_again"] = timed(lambda: fwd(fused), args.reps)
        row["fused_bwd_ms"] = row["fused_fwd_bwd_ms"] - row["fused_fwd_ms"]
        row["torch_bwd_ms"] = row["torch_fwd_bwd_ms"] - row["torch_fwd_ms"]
        row["fused_fwd_GBps"] = fwd_b * n / row["fused_fwd_ms"] / 1e6
        row["fused_fwd_frac_hbm_peak"] = row["fused_fwd_GBps"] * 1e9 / HBM_PEAK
        row["fused_bwd_GBps"] = bwd_b * n / row["fused_bwd_ms"] / 1e6
        row["speedup_fwd"] = row["torch_fwd_ms"] / row["fused_fwd_ms"]
        row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["fused_fwd_bwd_ms"]
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
