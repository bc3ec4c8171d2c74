"""GPU: ``HashGridEncoding(deterministic=True)`` -- the table gradient by sort and segmented sum (nfa_hashgrid_bwd_sorted,
nfa_hashgrid_bwd_bwd_sorted): bit for bit the float32 restatement of tests/hashgrid_sorted_reference.py at both orders and for
fp16 / bf16 gradients, within the derived bound of the float64 sum, exact zeros where nothing arrived, every other result bit
equal to the atomic path's, identical bytes run to run, on a side stream and in a replayed graph, which native calls it
makes, an optimiser run that ends in the same table twice, empty input and the id limit.

The bound is tests/test_hashgrid_sorted_cpu.py's: (cnt + 2) * 2^-23 * sum|term| per entry at first order, (cnt + 8) at second.
Measured on MI355X: every case below is bit-equal to the restatement, so its error is the restatement's own."""
import functools

import numpy as np
import pytest
import torch

import hashgrid_sorted_reference as R
from nerfacc_amd import encodings as E
from nerfacc_amd.graphs import CapturedStep
from test_hashgrid_grad2_gpu import CallLog, second_order

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
KINDS = ["F1_L1", "F1_L32", "F8_L7_edge", "F2_odd_res", "density", "collide", "same_point", "top_digit"]
CASES = [pytest.param(kind, n, id=f"{n}-{kind}") for kind in KINDS for n in R.NS]
ATOMIC = {"nfa_hashgrid_bwd", "nfa_hashgrid_bwd_t", "nfa_hashgrid_bwd_bwd", "nfa_hashgrid_bwd_bwd_t"}


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(grid on the CPU, x, g, v): computed once per (config, n), never modified."""
    enc = R.make_grid(kind)
    return (enc,) + R.make_inputs(kind, n, enc)


def restated(kind, n, order, dtype=torch.float32):
    """(grad float32 [n_params], info) of the restatement, for the gradient rounded to ``dtype`` (not kept: a table of
    2^24 entries is 64 MiB, and every test needs its own once)."""
    enc, x, g, v = case(kind, n)
    return R.sorted_table_grad(x.numpy(), enc, g.to(dtype).float().numpy(), v.numpy() if order == 2 else None)


def pair(kind, dev, out_dtype=None):
    """The sorted and the atomic grid on the device, sharing one parameter tensor."""
    det = R.make_grid(kind, out_dtype, deterministic=True).to(dev)
    atomic = R.make_grid(kind, out_dtype)
    atomic.params = det.params
    return det, atomic


def first_order(enc, x, g):
    dev = enc.params.device
    enc.params.grad = None
    xd = x.to(dev).requires_grad_(True)
    enc(xd).backward(g.to(dev))
    return enc.params.grad, xd.grad


def same_bits(got, want):
    a = got.detach().cpu().numpy().view(np.uint32)
    b = np.asarray(want, dtype=np.float32).view(np.uint32)
    assert a.shape == b.shape
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (int(bad.size), int(bad[0]), float(got.detach().cpu().numpy()[bad[0]]), float(want[bad[0]]))


# ---------------------------------------------------------------- first order
@pytest.mark.parametrize("kind,n", CASES)
def test_first_order(dev, kind, n):
    enc, x, g, _ = case(kind, n)
    want, info = restated(kind, n, 1)
    det, atomic = pair(kind, dev)
    g_p, g_x = first_order(det, x, g)
    g_p, g_x = g_p.clone(), g_x.clone()
    same_bits(g_p, want)
    R.check_bound(g_p.cpu().numpy(), info, enc.n_features_per_level, 2)       # also: exact zeros where nothing arrived
    _, g_x_atomic = first_order(atomic, x, g)
    assert torch.equal(g_x, g_x_atomic)


# ---------------------------------------------------------------- second order
@pytest.mark.parametrize("kind,n", CASES)
def test_second_order(dev, kind, n):
    enc, x, g, v = case(kind, n)
    want, info = restated(kind, n, 2)
    det, atomic = pair(kind, dev)
    x2, g2_p, gg_y, g_x = second_order(det, x, g, v)
    x2, g2_p, gg_y = x2.clone(), g2_p.clone(), gg_y.clone()
    same_bits(g2_p, want)
    R.check_bound(g2_p.cpu().numpy(), info, enc.n_features_per_level, 8)
    x2a, _, gg_ya, g_xa = second_order(atomic, x, g, v)
    assert torch.equal(x2, x2a) and torch.equal(gg_y, gg_ya) and torch.equal(g_x, g_xa)


# ---------------------------------------------------------------- fp16 / bf16 gradients
@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("kind", ["F2_odd_res", "collide"])
@pytest.mark.parametrize("d", HALF)
def test_half_gradients(dev, d, kind, n):
    enc, x, g, v = case(kind, n)
    det, _ = pair(kind, dev, d)
    g_p, _ = first_order(det, x, g.to(d))
    same_bits(g_p, restated(kind, n, 1, d)[0])
    _, g2_p, gg_y, _ = second_order(det, x, g.to(d), v)
    assert gg_y.dtype == d
    same_bits(g2_p, restated(kind, n, 2, d)[0])


# ---------------------------------------------------------------- run to run, side stream
@pytest.mark.parametrize("kind", ["collide", "same_point", "density"])
def test_identical_bytes_run_to_run(dev, kind):
    n = 4097
    _, x, g, v = case(kind, n)
    det, _ = pair(kind, dev)
    first = first_order(det, x, g)[0].clone()
    second = second_order(det, x, g, v)[1].clone()
    for _ in range(2):
        assert torch.equal(first_order(det, x, g)[0], first)
        assert torch.equal(second_order(det, x, g, v)[1], second)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        a = first_order(det, x, g)[0].clone()
        b = second_order(det, x, g, v)[1].clone()
    side.synchronize()
    assert torch.equal(a, first) and torch.equal(b, second)


# ---------------------------------------------------------------- which native calls, and no device reads
def test_one_sorted_call_per_table_gradient(dev, monkeypatch):
    _, x, g, v = case("density", 4097)
    det, _ = pair("density", dev)
    log = CallLog(monkeypatch)
    first_order(det, x, g)
    assert log.names() == ["nfa_hashgrid_fwd", "nfa_hashgrid_bwd_sorted"], log.names()
    args = log.calls[1][1]
    assert args[0] == 0 and args[-5] is not None and args[-3] is not None and args[-2] == R.scratch_bytes(4097, det.n_levels)
    log.calls.clear()
    second_order(det, x, g, v)
    assert all(a[-3] is None for name, a in log.calls if name in ATOMIC), log.names()         # no atomic table gradient
    assert log.names().count("nfa_hashgrid_bwd_bwd_sorted") == 1 and log.names()[-1] == "nfa_hashgrid_bwd_bwd_sorted"
    assert all(a[-5] is not None for name, a in log.calls if name.endswith("_sorted"))      # each forms a table gradient
    # fp16: the same entries, with the element code
    deth, _ = pair("density", dev, torch.float16)
    log.calls.clear()
    first_order(deth, x, g.half())
    assert log.names() == ["nfa_hashgrid_fwd_t", "nfa_hashgrid_bwd_sorted"] and log.calls[1][1][0] == 1
    # no table gradient wanted: the existing entries, unchanged
    det.params.requires_grad_(False)
    log.calls.clear()
    second_order(det, x, g, v)
    assert log.names() == ["nfa_hashgrid_fwd", "nfa_hashgrid_bwd", "nfa_hashgrid_bwd_bwd"], log.names()
    det.params.requires_grad_(True)


def test_captured_step_replays_the_eager_bytes(dev):
    _, x, g, _ = case("density", 4097)
    det, _ = pair("density", dev)
    eager_p, eager_x = first_order(det, x, g)
    eager_p, eager_x = eager_p.clone(), eager_x.clone()
    xs, gs = x.to(dev).requires_grad_(True), g.to(dev)
    step = CapturedStep(lambda: torch.autograd.grad(det(xs), (det.params, xs), gs), warmup=1)
    for _ in range(2):
        for t in step.outputs:
            t.fill_(float("nan"))
        g_p, g_x = step()
        torch.cuda.synchronize()
        assert torch.equal(g_p, eager_p) and torch.equal(g_x, eager_x)


# ---------------------------------------------------------------- end to end
def test_training_twice_gives_the_same_table(dev):
    _, x, _, _ = case("collide", 4097)
    xd = x.to(dev)
    w = torch.randn(4097, 4, generator=torch.Generator().manual_seed(7)).to(dev)
    tables = []
    for _ in range(2):
        enc = R.make_grid("collide", deterministic=True).to(dev)
        opt = torch.optim.Adam([enc.params], lr=1e-2)
        for _ in range(20):
            loss = (enc(xd) * w).square().sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
        tables.append(enc.params.detach().clone())
    assert torch.equal(tables[0], tables[1])
    assert bool(torch.isfinite(tables[0]).all()) and not torch.equal(tables[0], R.make_grid("collide").params.detach().to(dev))


# ---------------------------------------------------------------- empty input, the id limit
def test_empty_input_makes_no_call(dev, monkeypatch):
    det, _ = pair("density", dev)
    log = CallLog(monkeypatch)
    x = torch.zeros(0, 3, device=dev, requires_grad=True)
    g = torch.zeros(0, det.n_output_dims, device=dev, requires_grad=True)
    (g_x,) = torch.autograd.grad(det(x), x, g, create_graph=True)
    g_x.backward(torch.zeros(0, 3, device=dev))
    assert log.names() == []
    assert x.grad.shape == (0, 3) and det.params.grad.shape == det.params.shape and not bool(det.params.grad.any())


def test_id_limit(dev):
    det, _ = pair("collide", dev)
    with pytest.raises(ValueError, match="at most 2\\^29 - 1"):
        E._sorted_scratch(det, 1 << 29, "meta")            # a meta device: no allocation is made
    assert E._sorted_scratch(det, (1 << 29) - 1, "meta").numel() == R.scratch_bytes((1 << 29) - 1, det.n_levels)
