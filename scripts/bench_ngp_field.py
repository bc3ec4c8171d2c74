#!/usr/bin/env python3
"""Times the fused Instant-NGP field query (csrc/ngp_field.hip, nerfacc_amd.fields) against the composed chain of the SAME
module (its fused dispatch switched off: normalise, HashGridEncoding, FusedMLP, split, SphericalHarmonicsEncoding, cat,
FusedMLP, activations), under torch.no_grad(), and prints one JSON line per (field, N).
    python scripts/bench_ngp_field.py [--log2n 20 22] [--window-ms 200] [--windows 5] [--check]
Fields: `radiance` (16 levels, 2^19 entries, finest resolution 4096; `density` = query_density, `full` = forward) and
`proposal` (the density field: 5 levels, 2^17 entries, 128).  The points lie along rays through the box (64 consecutive
samples per ray, as scripts/bench_voxgrid.py places them): uniform random points flatter the gathers.  The two paths take
turns window by window in one process; a window is as many calls as fill --window-ms of device time between two HIP events;
`*_us` is the median of the windows' means, `*_spread` their (min, max), `*_ratio` the composed chain's time over the fused
one (above 1: the fused launch is faster).  `*_hbm_us`: the bytes the fused launch must move (density: 12 in, 4 out; full:
24 in, 16 out) over the device-to-device copy rate measured in the same run (`stream_gbps`).
--check compares the fused and the composed outputs at the timed sizes and prints the largest difference in half ulps."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd.fields import NGPDensityField, NGPRadianceField  # noqa: E402

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps   # us


def measure(passes, window_ms, windows):
    times, reps = {k: [] for k in passes}, {}
    for k, fn in passes.items():
        for _ in range(3):
            fn()
        reps[k] = max(3, int(math.ceil(window_ms * 1e3 / timed(fn, 3))))
    for _ in range(windows):
        for k, fn in passes.items():
            times[k].append(timed(fn, reps[k]))
    row = {}
    for k, v in times.items():
        row[k + "_us"] = round(float(np.median(v)), 1)
        row[k + "_spread"] = [round(min(v), 1), round(max(v), 1)]
    return row


def stream_gbps(dev):
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    return 2 * a.numel() * 4 / (timed(lambda: b.copy_(a), 10) * 1e-6) / 1e9


def ray_points(n, dev, gen):
    """n points: 64 consecutive samples on each of n / 64 rays through the box, and the rays' directions per sample."""
    rays = n // 64
    o = torch.rand(rays, 3, generator=gen, device=dev) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=gen, device=dev), dim=-1)
    t = (torch.arange(64, device=dev).float() + 0.5) * (2.0 / 64) - 1.0
    x = (o[:, None, :] * 0.3 + d[:, None, :] * t[None, :, None]).reshape(-1, 3).contiguous()
    return x, d[:, None, :].expand(rays, 64, 3).reshape(-1, 3).contiguous()


def composed(field, fn):
    def run():
        field.fused = False
        try:
            return fn()
        finally:
            field.fused = True
    return run


def half_ulps(a, b, dtype):
    a, b = a.double(), b.double()
    mant = 10 if dtype == torch.float16 else 7
    ulp = torch.exp2(torch.floor(torch.log2(b.abs().clamp_min(2.0 ** -14))) - mant)
    return float(((a - b).abs() / ulp).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    gbps = stream_gbps(dev)
    rad = NGPRadianceField(AABB).to(dev)
    prop = NGPDensityField(AABB).to(dev)
    with torch.no_grad():
        for f in (rad, prop):
            f.encoding.params.uniform_(-0.5, 0.5)
        for log2n in args.log2n:
            n = 1 << log2n
            x, d = ray_points(n, dev, gen)
            queries = {"radiance/density": (rad, lambda: rad.query_density(x), 16), "radiance/full": (rad, lambda: rad(x, d), 40),
                       "proposal/density": (prop, lambda: prop(x), 16)}
            for name, (field, fn, nbytes) in queries.items():
                row = {"query": name, "n": n, "stream_gbps": round(gbps, 1)}
                if args.check:
                    got, want = fn(), composed(field, fn)()
                    if name.endswith("full"):
                        raw_f, raw_c = field.query_raw(x, d), composed(field, lambda: field.query_raw(x, d))()
                        row["raw_rgb_half_ulps"] = round(half_ulps(raw_f[0], raw_c[0], field.dtype), 3)
                        row["raw_sigma_equal"] = bool(torch.equal(raw_f[1], raw_c[1]))
                        got, want = got[1], want[1]
                    row["density_max_rel"] = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
                row.update(measure({"fused": fn, "composed": composed(field, fn)}, args.window_ms, args.windows))
                row["ratio"] = round(row["composed_us"] / row["fused_us"], 2)
                row["hbm_us"] = round(n * nbytes / (gbps * 1e9) * 1e6, 1)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
