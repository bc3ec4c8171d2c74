#!/usr/bin/env python3
"""Times nerfacc_amd.photometric.photometric_loss (csrc/photo.hip), forward + backward, with HIP events against the lines of
the reference's loaders and trainers it replaces, restated in torch on the same device in the same process, and prints one
JSON line per case.
    python scripts/bench_photometric.py [--min-exp 10] [--max-exp 20] [--window 0.3]
A step is: the targets of N rays from a uint8 stack of 100 images of 800 x 800 (int64 image_id, y, x), smooth_l1 against
rgb, the loss times a device scale of 1024, and the gradient at rgb.  Cases: C = 4 with a random (3,) background
(nerf_synthetic.py:153,195) and C = 3 (nerf_360_v2.py:327).  The torch side is timed without mse_loss (the trainers compute
it when they log or evaluate) and with it (`torch_with_mse`); the native pass always returns the MSE.  Each side is timed
eagerly, cycling over 4 sets of inputs drawn for the case, and as replays of a captured graph (one set: a graph reads the
tensors it was captured with).  Every timing follows 3 warm-up calls and spans about `--window` seconds; the two sides
alternate, and the native eager timing is repeated at the end (`native_eager_ms_again`) as a measure of the spread.
Algorithmic bytes per ray of the native step: 24 (ids, y, x) + C (the pixel) + 12 (rgb) + 12 (pixels out) forward,
12 + 12 + 12 backward; the fraction is of the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from nerfacc_amd import CapturedStep  # noqa: E402
from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd.photometric import photometric_loss  # noqa: E402

HBM_PEAK = 8.0e12
N_SETS = 4


def timed(fn, window):
    """ms per call over about `window` seconds of calls, after 3 warm-up calls and a pilot that sizes the loop."""
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def span(reps):
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    pilot = span(20)
    return span(int(min(max(window * 1e3 / max(pilot, 1e-3), 50), 5000)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-exp", type=int, default=10)
    ap.add_argument("--max-exp", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B.load()
    g = torch.Generator(device=dev).manual_seed(0)
    n_images, H, W = 100, 800, 800
    scale = torch.tensor(1024.0, device=dev)
    for C in (4, 3):
        stack = torch.randint(0, 256, (n_images, H, W, C), generator=g, device=dev, dtype=torch.uint8)
        bkgd = torch.rand(3, generator=g, device=dev) if C == 4 else None
        for e in range(args.min_exp, args.max_exp + 1):
            n = 1 << e
            sets = [dict(ids=torch.randint(0, n_images, (n,), generator=g, device=dev), x=torch.randint(0, W, (n,), generator=g, device=dev),
                         y=torch.randint(0, H, (n,), generator=g, device=dev),
                         rgb=torch.rand(n, 3, generator=g, device=dev).requires_grad_(True)) for _ in range(N_SETS)]
            turn = [0]

            def next_set():
                turn[0] = (turn[0] + 1) % N_SETS
                return sets[turn[0]]

            def native(s):
                out = photometric_loss(s["rgb"], images=stack, image_ids=s["ids"], x=s["x"], y=s["y"], color_bkgd=bkgd)
                return out.loss, out.mse, torch.autograd.grad(out.loss * scale, s["rgb"])[0]

            def composed(s, with_mse=False):
                rgba = stack[s["ids"], s["y"], s["x"]] / 255.0
                if C == 4:
                    pixels, alpha = torch.split(rgba, [3, 1], dim=-1)
                    pixels = pixels * alpha + bkgd * (1.0 - alpha)
                else:
                    pixels = rgba
                loss = F.smooth_l1_loss(s["rgb"], pixels)
                grad = torch.autograd.grad(loss * scale, s["rgb"])[0]
                mse = F.mse_loss(s["rgb"].detach(), pixels) if with_mse else None
                return loss, mse, grad

            a, b = native(sets[0]), composed(sets[0], True)
            fwd_b, bwd_b = 24 + C + 12 + 12, 36
            row = dict(case=f"C{C}", n_rays=n, bytes_per_ray=fwd_b + bwd_b,
                       loss_rel_diff=float((a[0] - b[0]).abs() / b[0].abs()), mse_rel_diff=float((a[1] - b[1]).abs() / b[1].abs()),
                       grad_max_abs_diff=float((a[2] - b[2]).abs().max()), grad_max_abs=float(b[2].abs().max()))
            del a, b
            row["native_eager_ms"] = timed(lambda: native(next_set()), args.window)
            row["torch_eager_ms"] = timed(lambda: composed(next_set()), args.window)
            row["torch_with_mse_eager_ms"] = timed(lambda: composed(next_set(), True), args.window)
            graph_native = CapturedStep(lambda: native(sets[0]), warmup=3)
            graph_torch = CapturedStep(lambda: composed(sets[0]), warmup=3)
            graph_torch_mse = CapturedStep(lambda: composed(sets[0], True), warmup=3)
            row["native_graph_ms"] = timed(graph_native, args.window)
            row["torch_graph_ms"] = timed(graph_torch, args.window)
            row["torch_with_mse_graph_ms"] = timed(graph_torch_mse, args.window)
            row["native_graph_ms_again"] = timed(graph_native, args.window)
            row["native_eager_ms_again"] = timed(lambda: native(next_set()), args.window)
            del graph_native, graph_torch, graph_torch_mse
            row["speedup_eager"] = row["torch_eager_ms"] / row["native_eager_ms"]
            row["speedup_graph"] = row["torch_graph_ms"] / row["native_graph_ms"]
            row["speedup_eager_with_mse"] = row["torch_with_mse_eager_ms"] / row["native_eager_ms"]
            row["speedup_graph_with_mse"] = row["torch_with_mse_graph_ms"] / row["native_graph_ms"]
            row["native_graph_GBps"] = (fwd_b + bwd_b) * n / row["native_graph_ms"] / 1e6
            row["native_graph_frac_hbm_peak"] = row["native_graph_GBps"] * 1e9 / HBM_PEAK
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
