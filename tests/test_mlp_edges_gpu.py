"""GPU: the fused MLP kernels (csrc/mlp.hip, csrc/mlp_stream.hip) at the edges of fp16 / bf16 and on non-finite values.  The
tables of tests/mlp_edges_reference.py -- the ones tests/test_mlp_edges_cpu.py runs through the torch path, where the conditions
on them are asserted -- through the modules and through the C entries (every H_l, dZ_l and T_l too, every output between guard
rows), against the float64 restatements by class (NaN, +inf, -inf) and bits; and DeviceGradScaler on an overflow that is born
inside the backward kernel."""
import pytest
import torch

import mlp_edges_reference as E
import test_mlp_grad2_gpu as TG2
import test_mlp_gpu as TG
import test_mlp_stream_gpu as TS
from nerfacc_amd.mlp import wgrad_slices
from test_mlp_edges_cpu import POISON, SCALED, check, check_isolation, dt, ends, make_module, run_module, run_poison, scaler_run, wanted

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run_abi(c, r, x=None, g=None, v=None):
    """The C entries on case ``c``: dict(y, hidden, dz, dx, dp) from the first-order entries, which run on their own H_l, and for
    a case with a second order (t, u, d2p) from nfa_mlp_tangent and the second weight-gradient pass on the restatement ``r``'s
    H_l and dZ_l (one mask and one dZ on both sides)."""
    x, g, v = (c.x if x is None else x), (c.g if g is None else g), (c.v if v is None else v)
    if c.kind == "plain":
        a = TG.run_abi(c.shape, c.dtype, c.ws, x, g, c.out_f32)
        a["dp"] = a.pop("dw")
    elif c.kind == "net":
        a = TS.run_abi(c.shape, c.skip_mask, c.dtype, c.ws, c.bs, x, g, c.out_f32, prefix="nfa_mlp_net_", slices=wgrad_slices)
    else:
        a = TS.run_abi(c.shape, c.skip_mask, c.dtype, c.ws, c.bs, x, g, c.out_f32)
    if c.second:
        s = TG2.run_abi(c.shape, c.dtype, c.ws, v, r.f["hidden"], r.b["dz"], c.out_f32)
        a.update(t=s["t"], u=s["u"], d2p=s["dw"])
    return {k: a[k] for k in ("y", "hidden", "dz", "dx", "dp", "t", "u", "d2p") if k in a}


def wanted_abi(c, r):
    w = dict(y=r.f["y"], hidden=r.f["hidden"], dz=r.b["dz"], dx=r.b["dx"], dp=r.dp)
    if c.second:
        w.update(t=r.s["t"][1:], u=r.s["u"], d2p=r.d2p)
    return w


def check_abi(got, want, tag, rows=None):
    for k, w in want.items():
        if isinstance(w, list):
            assert len(got[k]) == len(w), k
            for l, (a, b) in enumerate(zip(got[k], w)):
                check({f"{k}[{l}]": a}, {f"{k}[{l}]": b}, tag, rows)
        else:
            check({k: got[k]}, {k: w}, tag, rows)


def check_case(c, tag):
    r = E.restate(c)
    check(run_module(make_module(c, DEV), c), wanted(c, r), tag + " (module)")
    check_abi(run_abi(c, r), wanted_abi(c, r), tag + " (C entries)")


@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("net,dtype,which", SCALED, ids=lambda v: v if isinstance(v, str) else dt(v))
def test_scaled(net, dtype, which, f32_ends):
    """Contract items 1, 2, 3 and 5 where the stored values are fp16 subnormals (gradual underflow, ties to even, subnormal MFMA
    operands on both sides) and where they pass MAX of the half type (inf, never saturated)."""
    for i, c in enumerate(E.scaled_cases(net, dtype, which, f32_ends)):
        check_case(c, f"{net} {dt(dtype)} {which}[{i}] {ends(f32_ends)}")


@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
@pytest.mark.parametrize("net", list(E.NETS))
def test_boundary(net, dtype, f32_ends):
    """MAX + ulp/2 becomes inf and one float32 step below it MAX, at every rounding point, with both signs."""
    for probe in E.boundary_probes(net, f32_ends):
        check_case(E.boundary_case(net, dtype, f32_ends, probe), f"{net} {dt(dtype)} {ends(f32_ends)} probe {probe}")


@pytest.mark.parametrize("f32_ends", [False, True], ids=ends)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
@pytest.mark.parametrize("net,target", POISON)
def test_poison(net, target, dtype, f32_ends):
    """Contract item 4: one NaN / +inf / -inf in row p of x, g or v changes row p alone, in y, every H_l, dZ_l and T_l, dx and u
    -- p = N - 1 in a partial tile included, whose clamped loads put that row into lanes that must not store."""
    modules = {}

    def run(c, x, g, v):
        if c.x.shape[0] not in modules:
            modules[c.x.shape[0]] = make_module(c, DEV)
        out = {"module " + k: a for k, a in run_module(modules[c.x.shape[0]], c, x, g, v).items()}
        out.update(run_abi(c, E.restate(c, x, g, v), x, g, v))
        return out

    second = E.has_second_order(net)
    keys = ["module y", "module dx", "y", "hidden", "dz", "dx"] + (["module u", "t", "u"] if second else [])
    for c, r, dirty, p, tag in run_poison(net, dtype, f32_ends, target, run, keys):
        check({k[7:]: a for k, a in dirty.items() if k.startswith("module ")}, wanted(c, r), tag + " (module)", rows=p)
        check_abi(dirty, wanted_abi(c, r), tag + " (C entries)", rows=p)


@pytest.mark.parametrize("dtype", E.DTYPES, ids=dt)
def test_dead_neuron(dtype):
    """Contract item 3: the masks of the backward and of the tangent pass are selects."""
    check_case(E.dead_neuron_case(dtype), f"dead neuron {dt(dtype)}")


def test_scaler_skips_an_overflow_born_in_the_backward():
    """Contract item 6: g * scale is finite in fp16, dZ_0 overflows inside nfa_mlp_bwd_data, dL/dparams carries it, and the
    step is skipped -- as many times in a row as the restatement predicts."""
    scaler_run(DEV)
