#!/usr/bin/env python3
"""Times `nerfacc_amd.optim.FusedAdam` (csrc/optim.hip: `nfa_optim_scan`, `nfa_optim_decide`, `nfa_optim_update`) against
`torch.optim.Adam(foreach=True)` and `torch.optim.Adam(fused=True)`, each also under torch's `GradScaler`, on the same GPU
in the same run, and prints one JSON line per case.
    python scripts/bench_optim.py [--window-ms 200] [--windows 5] [--zero-share 0.75]
Shapes:
  ngp       the table of the default `HashGridEncoding` (NGP's grid) plus the parameter tensors of its two `FusedMLP`s
            (32 -> 64 -> 16 and 32 -> 64 -> 64 -> 3): three tensors;
  propnet   ten tensors, 0.69 M values in all (a proposal network's small tables and matrices): a launch-bound set;
  step      a whole step -- five small fields (`HashGridEncoding` + `FusedMLP`, ten parameter tensors) on 4096 points each,
            squared error, backward, update -- replayed as ONE `CapturedStep` graph with `FusedAdam` + `DeviceGradScaler` +
            `WarmupMultiStepLR` inside, against the graph of forward + backward alone followed by the update outside it:
            `FusedAdam` eager, and torch's `GradScaler.step(Adam(fused=True))` + `update()` (which reads the device).
            `FusedMLP` rebuilds its packed weight images when its masters' version counter has moved, and a graph contains
            that rebuild only if the cache was stale when it was captured; the step function bumps the counter on the host
            before the forward, so every graph holds the same five rebuilds, and `*_follows_updates` records that a replay's
            loss is the eager loss on the parameters as the optimiser left them (the run fails otherwise).
Every variant owns a copy of the parameters and gradients; the variants take turns window by window.  A window is as many
steps as fill `--window-ms` of device time (at least 3; counted from a timed probe after 3 warm-up steps) between two HIP
events; `*_us` is the median of the windows' means, `*_spread` their (min, max).  `*_bytes` is the algorithmic traffic of a
step: 28 B per element (p, m, v read and written, the gradient read), 32 B with `zero_grad` (the gradient written) or with a
scaler (the gradient read twice: the scan), and with `skip_zero_grad` 4 B for an element in a 16-byte piece of zeros; `*_gbps`
is those bytes over the time, beside `copy_gbps`, what `Tensor.copy_` reaches on 256 MB in the same run (read + write).
`zero_pieces`: a share `--zero-share` of the 16-byte pieces zero, at random; `zero_blocks`: the same share as whole
4096-element blocks.  torch's variants are charged the same 28 B whatever they move.  In the `ngp` and `propnet` rows every
scaler, torch's and `DeviceGradScaler`, has scale 1 and never grows: torch unscales the gradients in place, so any other scale
would leave its rows running on zeros after a few steps, and the work does not depend on the scale; in `step` the gradients
are made anew by every backward and the scale is a fixed 2^10.  `*_ratio`: torch's fused Adam over the row."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfacc_amd import CapturedStep  # noqa: E402
from nerfacc_amd.encodings import HashGridEncoding  # noqa: E402
from nerfacc_amd.mlp import FusedMLP  # noqa: E402
from nerfacc_amd.optim import DeviceGradScaler, FusedAdam, WarmupMultiStepLR  # noqa: E402

KW = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=1e-6)   # the reference's NGP trainer
FIXED = 10 ** 9   # a growth interval no run reaches
PROPNET_SIZES = [524288, 131072, 4096, 4096, 1024, 4096, 4096, 64, 16384, 64]


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
        row[k + "_reps"] = reps[k]
    return row


def copies(sizes, dev, seed, zero=None, share=0.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.randn(n, device=dev, generator=g).requires_grad_() for n in sizes]
    for p in params:
        p.grad = torch.randn(p.numel(), device=dev, generator=g)
        if zero == "pieces":
            z = torch.rand((p.numel() + 3) // 4, device=dev, generator=g) < share
            p.grad[z.repeat_interleave(4)[:p.numel()]] = 0.0
        elif zero == "blocks":
            z = torch.rand((p.numel() + 4095) // 4096, device=dev, generator=g) < share
            p.grad[z.repeat_interleave(4096)[:p.numel()]] = 0.0
    return params


def optimiser_passes(sizes, dev, zero_share):
    """name -> (step function, bytes per step)."""
    n = sum(sizes)
    out = {}

    def fused(name, bytes_, zero=None, **kw):
        scale = kw.get("scaler")
        params = copies(sizes, dev, 1, zero, zero_share)
        if scale is not None:
            for p in params:
                p.grad *= scale.init_scale
        opt = FusedAdam(params, **KW, **kw)
        out[name] = (opt.step, bytes_)

    fused("fused", 28 * n)
    fused("fused_zero_grad", 32 * n, zero_grad=True)
    fused("fused_scaler", 32 * n, scaler=DeviceGradScaler(init_scale=1.0, growth_interval=None))
    sparse = int(n * (4 + 24 * (1.0 - zero_share)))
    fused("fused_skip_zero_pieces", sparse, zero="pieces", skip_zero_grad=True)
    fused("fused_skip_zero_blocks", sparse, zero="blocks", skip_zero_grad=True)
    for name, kw in (("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        opt = torch.optim.Adam(copies(sizes, dev, 1), **KW, **kw)
        out[name] = (opt.step, 28 * n)
        opt = torch.optim.Adam(copies(sizes, dev, 1), **KW, **kw)
        scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=FIXED)
        scaler.scale(torch.ones(1, device=dev))

        def scaled(opt=opt, scaler=scaler):
            scaler.step(opt)
            scaler.update()
        out[name + "_gradscaler"] = (scaled, 28 * n)
    return out


def small_fields(dev):
    fields = []
    for k in range(5):
        torch.manual_seed(k)
        grid = HashGridEncoding(n_levels=8, log2_hashmap_size=14, out_dtype=torch.float16).to(dev)
        mlp = FusedMLP(16, 4, n_neurons=64, n_hidden_layers=1, out_dtype=torch.float32).to(dev)
        fields.append((grid, mlp))
    return fields


def step_passes(dev):
    """The whole step as one graph, and forward + backward as a graph with the update outside it.  Returns the passes and, per
    graph variant, a check that its replays follow the updated weights."""
    out, checks = {}, {}
    x = torch.rand(4096, 3, device=dev)
    y = torch.randn(4096, 4, device=dev)

    def build(inside):
        fields = small_fields(dev)
        params = [p for g, m in fields for p in (g.params, m.params)]
        masters = [m.params for _, m in fields]
        if inside == "torch":
            scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=FIXED)
            opt = torch.optim.Adam(params, fused=True, **KW)
        else:
            scaler = DeviceGradScaler(2.0 ** 10, growth_interval=None)
            opt = FusedAdam(params, **KW, zero_grad=True, scaler=scaler, schedule=WarmupMultiStepLR(0.01, 100, (10000, 15000), 0.33))

        def loss_of():
            return sum(((m(g(x)) - y) ** 2).mean() for g, m in fields)

        def fwd_bwd():
            # FusedMLP rebuilds its packed images when the masters' version counter moved.  Bumped here, on the host, every
            # capture sees a stale cache, so EVERY graph below contains the five rebuilds and replays on the weights as its
            # optimiser left them, whether the update is inside the graph or behind it.
            torch.autograd.graph.increment_version(masters)
            loss = loss_of()
            scaler.scale(loss).backward()
            return loss
        return params, scaler, opt, fwd_bwd, (loss_of, masters)

    def follows(step, loss_of, masters):
        """Three more steps, as [eager loss on the parameters as they are before the step, the loss the step returns]: the
        variant follows the updates if each pair agrees, the values are finite and they move from step to step.  (The eager
        forward needs the counter bumped as well: a replay does not repeat step()'s host-side bump, and torch's fused Adam
        under GradScaler leaves the counter alone, so FusedMLP's eager cache would be the stale side of the comparison.)"""
        pairs = []
        for _ in range(3):
            with torch.no_grad():
                torch.autograd.graph.increment_version(masters)
                want = float(loss_of())
            got = step()
            pairs.append([want, float((got[0] if isinstance(got, tuple) else got).detach())])
        ok = all(math.isfinite(g) and abs(g - w) <= 1e-6 * abs(w) for w, g in pairs) and len({g for _, g in pairs}) == 3
        return ok, pairs

    params, scaler, opt, fwd_bwd, loss_of = build("graph")
    whole = CapturedStep(lambda: (fwd_bwd(), opt.step())[0])
    out["graph_whole_step"] = whole
    checks["graph_whole_step"] = lambda: follows(whole, *loss_of)

    params2, scaler2, opt2, fwd_bwd2, loss_of2 = build("eager")
    fwd_bwd2()
    opt2.step()   # the .grad buffers exist (and are zero) before the capture
    part2 = CapturedStep(fwd_bwd2)
    torch._foreach_zero_([p.grad for p in params2])   # (the warm-up runs accumulated)
    out["graph_fwd_bwd_then_fused"] = lambda: (part2(), opt2.step())
    checks["graph_fwd_bwd_then_fused"] = lambda: follows(out["graph_fwd_bwd_then_fused"], *loss_of2)

    params3, scaler3, opt3, fwd_bwd3, loss_of3 = build("torch")
    fwd_bwd3()
    part3 = CapturedStep(fwd_bwd3)
    grads3 = [p.grad for p in params3]
    torch._foreach_zero_(grads3)

    def torch_outside():
        loss = part3()
        scaler3.step(opt3)
        scaler3.update()
        torch._foreach_zero_(grads3)   # in place, as the captured backward accumulates
        return loss
    out["graph_fwd_bwd_then_torch_gradscaler"] = torch_outside
    checks["graph_fwd_bwd_then_torch_gradscaler"] = lambda: follows(torch_outside, *loss_of3)

    params4, scaler4, opt4, fwd_bwd4, _ = build("eager")
    out["eager_whole_step"] = lambda: (fwd_bwd4(), opt4.step())
    return out, checks, sum(p.numel() for p in params)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--zero-share", type=float, default=0.75)
    ap.add_argument("--only", choices=("ngp", "propnet", "step"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on a GPU; none is available")
    dev = torch.device("cuda:0")
    src, dst = torch.empty(1 << 26, device=dev), torch.empty(1 << 26, device=dev)
    copy = measure({"copy": lambda: dst.copy_(src)}, a.window_ms, 3)
    copy_gbps = round(2 * 4 * src.numel() / copy["copy_us"] / 1e3, 1)
    del src, dst
    ngp = [HashGridEncoding().params.numel(), FusedMLP(32, 16, 64, 1).params.numel(), FusedMLP(32, 3, 64, 2).params.numel()]
    for shape, sizes in (("ngp", ngp), ("propnet", PROPNET_SIZES)):
        if a.only not in (None, shape):
            continue
        passes = optimiser_passes(sizes, dev, a.zero_share)
        row = {"shape": shape, "sizes": sizes, "n_values": sum(sizes), "zero_share": a.zero_share, "copy_gbps": copy_gbps,
               "window_ms": a.window_ms, "windows": a.windows}
        row.update(measure({k: v[0] for k, v in passes.items()}, a.window_ms, a.windows))
        for k, (_, b) in passes.items():
            row[k + "_bytes"] = b
            row[k + "_gbps"] = round(b / row[k + "_us"] / 1e3, 1)
            row[k + "_ratio"] = round(row["torch_fused_us"] / row[k + "_us"], 2)
        print(json.dumps(row), flush=True)
        del passes
        torch.cuda.empty_cache()
    if a.only in (None, "step"):
        passes, checks, n_values = step_passes(dev)
        row = {"shape": "step", "n_points": 4096, "n_tensors": 10, "n_values": n_values, "window_ms": a.window_ms, "windows": a.windows}
        row.update(measure(passes, a.window_ms, a.windows))
        for k, check in checks.items():
            row[k + "_follows_updates"], row[k + "_loss_pairs"] = check()
        if not all(row[k + "_follows_updates"] for k in checks):
            print(json.dumps(row), flush=True)
            raise SystemExit("bench_optim.py: a graph variant does not replay on the updated weights; its time is not a step's")
        for k in passes:
            row[k + "_ratio"] = round(row["graph_fwd_bwd_then_torch_gradscaler_us"] / row[k + "_us"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
