#!/usr/bin/env python3
"""Times the layout conversions of nerfacc_amd.pack (csrc/pack.hip) with HIP events against the torch compositions a user
writes without them, and prints one JSON line.
    python scripts/bench_pack.py [--reps 50] [--rays 1048576] [--per-ray 64]
Input: float32 padded data (R, S, D), D in {1, 3}, and a seeded Bernoulli(0.5) mask; the packed side is pack_data's output
(N ~ R * S / 2 samples).  Algorithmic bytes (rb = 4 D bytes per sample):
  unpack fwd   read N rb + packed_info 16 R, write R S rb                       (nfa_unpack_rows, by counts)
  unpack bwd   read the kept N rb of the padded gradient + 16 R, write N rb  (nfa_pack_rows, by counts)
  pack fwd     read mask R S, data R S rb (kept samples are interleaved at sample granularity: every line is touched),
               write N rb + packed_info 16 R                                     (row counts + cumsum + nfa_pack_rows)
  pack bwd     read mask R S, packed_info 16 R, N rb, write R S rb               (nfa_unpack_rows, by the mask)
pack fwd is timed as the whole op (three launches and the read-back of the total) and its two kernels alone."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nerfacc_amd import _backend as B  # noqa: E402
from nerfacc_amd import pack  # noqa: E402


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


def one(R, S, D, reps, torch_reps, dev):
    gen = torch.Generator(device=dev).manual_seed(D)
    data = torch.rand((R, S, D), device=dev, generator=gen)
    mask = torch.rand((R, S), device=dev, generator=gen) < 0.5
    packed, pi = pack.pack_data(data, mask)
    N, rb = packed.shape[0], 4 * D
    cnts = pi[:, 1].contiguous()
    prefix = torch.arange(S, device=dev)[None, :] < cnts[:, None]
    padded = torch.empty((R, S, D), device=dev)
    g_packed = torch.empty_like(packed)
    cnt_buf = torch.empty(R, dtype=torch.int64, device=dev)
    pi_buf = torch.empty((R, 2), dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = B.cumsum_scratch(R, dev)
    out = torch.empty_like(packed)

    def unpack_fwd():
        B.call("nfa_unpack_rows", B.ptr(packed), B.ptr(pi), None, R, S, N, rb, None, 0, B.ptr(padded), B.stream())

    def unpack_bwd():
        B.call("nfa_pack_rows", B.ptr(padded), B.ptr(pi), None, R, S, N, rb, B.ptr(g_packed), B.stream())

    def counts():
        B.call("nfa_mask_row_counts", B.ptr(mask), R, S, B.ptr(cnt_buf), B.stream())

    def pack_rows():
        B.call("nfa_pack_rows", B.ptr(data), B.ptr(pi), B.ptr(mask), R, S, N, rb, B.ptr(out), B.stream())

    def pack_fwd():
        counts()
        B.call("nfa_exclusive_cumsum_pairs_i64", B.ptr(cnt_buf), R, B.ptr(pi_buf), B.ptr(total), B.ptr(scratch), B.stream())
        int(total.item())
        pack_rows()

    def pack_bwd():
        B.call("nfa_unpack_rows", B.ptr(packed), B.ptr(pi), B.ptr(mask), R, S, N, rb, None, 0, B.ptr(padded), B.stream())

    # torch compositions: repeat_interleave + index_put (unpack), data[mask] (pack), and their reverses
    def t_unpack_fwd():
        pack._unpack_data_torch(pi, packed, S, 0)

    def t_unpack_bwd():
        padded[prefix]

    def t_pack_fwd():
        c = mask.sum(1)
        torch.stack([torch.cumsum(c, 0) - c, c], -1)
        data[mask]

    def t_pack_bwd():
        torch.zeros((R, S, D), device=dev).index_put_((mask,), packed)

    res = {"D": D, "samples": N}
    nbytes = {"unpack_fwd": N * rb + 16 * R + R * S * rb, "unpack_bwd": 2 * N * rb + 16 * R,
              "pack_fwd": R * S + R * S * rb + N * rb + 16 * R, "pack_bwd": R * S + 16 * R + N * rb + R * S * rb}
    for name, fn, tfn in (("unpack_fwd", unpack_fwd, t_unpack_fwd), ("unpack_bwd", unpack_bwd, t_unpack_bwd),
                          ("pack_fwd", pack_fwd, t_pack_fwd), ("pack_bwd", pack_bwd, t_pack_bwd)):
        us, tus = timed(fn, reps), timed(tfn, torch_reps)
        b = nbytes[name]
        res[name] = {"us": round(us, 1), "gb": round(b / 1e9, 3), "tb_per_s": round(b / us * 1e-6, 2),
                     "vs_6tbs": round(us / (b / 6e12 * 1e6), 2), "torch_us": round(tus, 1),
                     "torch_tb_per_s": round(b / tus * 1e-6, 2)}
    for name, fn, b in (("mask_row_counts", counts, R * S + 8 * R), ("pack_rows_masked", pack_rows, nbytes["pack_fwd"] - 8 * R)):
        us = timed(fn, reps)
        res[name] = {"us": round(us, 1), "tb_per_s": round(b / us * 1e-6, 2), "vs_6tbs": round(us / (b / 6e12 * 1e6), 2)}
    # the native results are the torch ones
    unpack_fwd()
    pack_rows()
    res["exact"] = bool(torch.equal(padded, pack._unpack_data_torch(pi, packed, S, 0)) and torch.equal(out, data[mask]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--per-ray", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pack.py needs the GPU"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "per_ray": args.per_ray, "reps": args.reps,
           "cases": [one(args.rays, args.per_ray, D, args.reps, args.torch_reps, dev) for D in (1, 3)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
