#!/usr/bin/env python3
"""Times the distortion-loss passes (csrc/segscan.hip: DistortionFwdOp / DistortionBwdOp) with HIP events against the torch
path of nerfacc_amd.losses on the same GPU, and prints one JSON line.
    python scripts/bench_distortion.py [--reps 50] [--rays 1048576]
Input: the bench's cfg 2 size, 2^20 rays and ~32 M samples from a seeded synthetic set (30 % empty rays, the others 1..90
samples), t increasing along each ray.  Roofline bytes: forward reads w, t_starts, t_ends (12 B/sample) and packed_info
(16 B/ray), writes loss, W_tot, S_tot (12 B/ray); backward reads the same 12 B/sample and packed_info, g, W_tot, S_tot
(28 B/ray), writes the three gradients (12 B/sample).  The first midpoint of every ray (two 4 B gathers per non-empty ray,
on lines the pass streams anyway) is not counted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd import losses  # noqa: E402
from nerfacc_amd._segments import tag_trusted  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--torch-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distortion.py needs the GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    R = args.rays
    lengths = np.where(rng.random(R) < 0.3, 0, rng.integers(1, 91, R)).astype(np.int64)
    n = int(lengths.sum())
    counts = torch.from_numpy(lengths).to(dev)
    starts = torch.cumsum(counts, 0) - counts
    packed_info = torch.stack([starts, counts], -1).contiguous()
    seg = tag_trusted(packed_info, n)
    ray_ids = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    gen = torch.Generator(device=dev).manual_seed(0)
    step = torch.rand(n, device=dev, generator=gen) * 0.01 + 1e-3
    c = torch.cumsum(step.double(), 0)
    base = torch.where(starts[ray_ids] > 0, c[(starts[ray_ids] - 1).clamp_min(0)], torch.zeros_like(c))
    te = (c - base).float() + 2.0
    ts = te - step
    w = torch.rand(n, device=dev, generator=gen) / counts.clamp_min(1)[ray_ids]
    loss, w_tot, s_tot = (torch.empty(R, device=dev) for _ in range(3))
    g = torch.rand(R, device=dev, generator=gen)
    gw, gts, gte = (torch.empty_like(w) for _ in range(3))

    def fwd():
        B.call("nfa_distortion_fwd", B.ptr(w), B.ptr(ts), B.ptr(te), B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles,
               R, n, B.ptr(loss), B.ptr(w_tot), B.ptr(s_tot), B.stream())

    def bwd():
        B.call("nfa_distortion_bwd", B.ptr(w), B.ptr(ts), B.ptr(te), B.ptr(w_tot), B.ptr(s_tot), B.ptr(g),
               B.ptr(seg.packed_info), B.ptr(seg.tiles), seg.n_tiles, R, n, B.ptr(gw), B.ptr(gts), B.ptr(gte), B.stream())

    us_f = timed(fwd, args.reps)
    us_b = timed(bwd, args.reps)
    # the torch path (what every non-native input runs), forward + backward on the same GPU
    xs = [t.clone().requires_grad_(True) for t in (w, ts, te)]

    def torch_pair():
        out = losses._distortion_torch(*xs, ray_ids, R)
        torch.autograd.grad(out, xs, g)

    us_t = timed(torch_pair, args.torch_reps)
    # agreement of the two paths at this size
    fwd(); bwd()
    ref = losses._distortion_torch(*xs, ray_ids, R)
    rgw, rts, rte = torch.autograd.grad(ref, xs, g)
    rel = lambda a, b: float((a - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))
    bytes_f = 12 * n + 16 * R + 12 * R
    bytes_b = 12 * n + 28 * R + 12 * n
    res = {"device": torch.cuda.get_device_name(0), "rays": R, "samples": n, "reps": args.reps,
           "fwd_us": round(us_f, 1), "bwd_us": round(us_b, 1), "fwd_gb": round(bytes_f / 1e9, 3), "bwd_gb": round(bytes_b / 1e9, 3),
           "fwd_tb_per_s": round(bytes_f / us_f * 1e-6, 2), "bwd_tb_per_s": round(bytes_b / us_b * 1e-6, 2),
           "torch_fwd_bwd_us": round(us_t, 1), "speedup_vs_torch": round(us_t / (us_f + us_b), 1),
           "max_rel_diff_vs_torch": {"loss": rel(loss, ref), "g_weights": rel(gw, rgw), "g_t_starts": rel(gts, rts),
                                     "g_t_ends": rel(gte, rte)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
