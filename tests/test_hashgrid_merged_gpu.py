"""GPU: ``HashGridEncoding(table_gradient="merged")`` (nfa_hashgrid_bwd_merged) against the float64 per-entry sum of
tests/hashgrid_sorted_reference.py (D = 2, 4: tests/hashgrid_nd_reference.py) within its bound (cnt + 2) 2^-23 sum|term| ((cnt + D) as
tests/test_hashgrid_nd_gpu.py), exact zeros elsewhere; dL/dx bit-equal to the atomic path's; the calls made.  The bound is derived:
a float32 sum of cnt terms in ANY order errs by at most (cnt - 1) 2^-24 sum|term| and a term costs three roundings."""
import copy
import functools

import numpy as np
import pytest
import torch

import hashgrid_nd_reference as ND
import hashgrid_sorted_reference as R
from nerfacc_amd import _backend as B
from nerfacc_amd.encodings import HashGridEncoding
from nerfacc_amd.graphs import CapturedStep
from test_hashgrid_grad2_gpu import CallLog

pytestmark = pytest.mark.gpu

KINDS = ["F1_L1", "F1_L32", "F8_L7_edge", "F2_odd_res", "density", "collide", "same_point"]
NS = [1, 63, 65, 257, 4097]   # below and across a wave of 64 points, a workgroup pass of 256, and several spans


def ray_points(enc, lengths, seed=0):   # rays of `lengths` samples, marched with a step of a quarter of level 0's cell
    gen = torch.Generator().manual_seed(seed)
    o = torch.rand(len(lengths), 3, generator=gen) * 0.5
    d = torch.nn.functional.normalize(torch.rand(len(lengths), 3, generator=gen) + 0.1, dim=-1)
    return torch.cat([o[i] + d[i] * (0.25 / enc.scales[0]) * torch.arange(m)[:, None] for i, m in enumerate(lengths)])


@functools.lru_cache(maxsize=None)
def case(kind, n, points="boundary", dtype=torch.float32):
    """(grid on the CPU, x, g, info of the float64 sum for g rounded to ``dtype``): computed once, never modified."""
    if kind in ND.GRIDS or kind == "d3_smooth":     # Smoothstep at D = 3, D = 2, D = 4 (F = 2) and D = 4 with F = 8 (grouped corners)
        enc = HashGridEncoding(3, *R.configs()["density"], interpolation="Smoothstep") if kind == "d3_smooth" else ND.make_grid(kind)
        enc.table_gradient = "merged"
        x = ND.make_points(n, enc, 1000 + n, same_point=points == "same")
        g = torch.randn(n, enc.n_output_dims, generator=torch.Generator().manual_seed(100 + n))
        ref, cnt, absum, _ = ND.grads(x.numpy(), enc.params.detach().numpy(), ND.table_of(enc), g.numpy(), enc.interp == 1)
        e = np.nonzero(cnt)[0]
        return enc, x, g, dict(entry=e, sum64=ref[e], abs64=absum[e], cnt=cnt[e])
    if kind.startswith("cap"):                      # one level of exactly the LDS cap / of the next legal size above it
        F, entries = int(kind[-1]), B.HG_MERGED_LDS_FLOATS // int(kind[-1])       # a power of two: a hashed level of 2^log2 entries
        res = next(r for r in range(2, 64) if (r ** 3 + 7) // 8 * 8 > entries)
        args = (entries.bit_length() - 1, 64) if kind.startswith("cap_at") else (entries.bit_length(), res)
        enc = HashGridEncoding(3, 1, F, *args, 1.0, table_gradient="merged")
        assert enc.sizes[0] == (entries if kind.startswith("cap_at") else (res ** 3 + 7) // 8 * 8)
    else:
        enc = HashGridEncoding(3, *R.configs()[kind], table_gradient="merged")
    if points == "boundary":
        x, g, _ = R.make_inputs(kind, n, enc)
    else:                                           # runs start and end on lanes 0 and 63 and cross a wave and a pass border;
        tail = ray_points(enc, [1, 1], seed=1).repeat(33, 1)    # then A, B, A, B, ..: equal entries that are never adjacent
        x = torch.cat([ray_points(enc, [64, 63, 1, 65, 2, 130]), tail]) if points == "rays" else ray_points(enc, [130] * 31 + [67])
        g = torch.randn(x.shape[0], enc.n_output_dims, generator=torch.Generator().manual_seed(5))
    return enc, x, g, R.sorted_table_grad(x.numpy(), enc, g.to(dtype).float().numpy())[1]


def both_ways(enc, dev, x, g, dtype=None):   # (merged dL/dparams, merged dL/dx, atomic dL/dx) of a copy of the grid on the device
    m = copy.deepcopy(enc).to(dev)
    m.out_dtype = dtype
    m.params.data.uniform_(-1, 1)
    xd, gd = x.to(dev).requires_grad_(True), (g.to(dtype) if dtype else g).to(dev)
    g_p, g_x = torch.autograd.grad(m(xd), (m.params, xd), gd)
    m.table_gradient = "atomic"
    return g_p, g_x, torch.autograd.grad(m(xd), xd, gd)[0]


HALF = [("F2_odd_res", n, "boundary", d) for n in (65, 4097) for d in (torch.float16, torch.bfloat16)]
CASES = ([(k, n, "boundary", None) for k in KINDS for n in NS] + [(k, 0, "rays", None) for k in ("density", "F2_odd_res")]
         + [(k, 4097, "rays4097", None) for k in ("cap_at_F1", "cap_over_F1", "cap_at_F8", "cap_over_F8")]
         + HALF + [("collide",) + c[1:] for c in HALF]
         + [(k, n, p, None) for k in ("d3_smooth", "d2_boundary", "d4_collide", "d4_edge") for n in (65, 4097) for p in ("spread", "same")])


@pytest.mark.parametrize("kind,n,points,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_table_gradient_within_bound(dev, kind, n, points, dtype):
    enc, x, g, info = case(kind, n, points, dtype or torch.float32)
    g_p, g_x, g_x_atomic = both_ways(enc, dev, x, g, dtype)
    R.check_bound(g_p.cpu().numpy(), info, enc.n_features_per_level, 2 if enc.n_input_dims == 3 else enc.n_input_dims)   # (docstring)
    assert torch.equal(g_x, g_x_atomic)


def test_calls(dev, monkeypatch):
    enc, x, g, _ = case("density", 4097)
    merged, xd, gd = copy.deepcopy(enc).to(dev), x.to(dev), g.to(dev)
    log = CallLog(monkeypatch)

    def calls(x_grad, n=4097):
        log.calls.clear()
        merged.params.grad = None
        merged(xd[:n].clone().requires_grad_(x_grad)).backward(gd[:n])
        return log.names()

    assert calls(False) == ["nfa_hashgrid_fwd", "nfa_hashgrid_bwd_merged"]
    assert sorted(calls(True)) == ["nfa_hashgrid_bwd", "nfa_hashgrid_bwd_merged", "nfa_hashgrid_fwd"] \
        and dict(log.calls)["nfa_hashgrid_bwd"][-3] is None            # grad_params: the plain pass forms dL/dx alone
    assert calls(False, 0) == [] and merged.params.grad.shape == merged.params.shape and not bool(merged.params.grad.any())
    merged.params.requires_grad_(False)                                # frozen table: today's calls exactly
    assert calls(True) == ["nfa_hashgrid_fwd", "nfa_hashgrid_bwd"]


def test_captured_step_replays(dev):
    enc, x, g, info = case("density", 4097, "rays4097")
    merged, xs, gs = copy.deepcopy(enc).to(dev), x.to(dev), g.to(dev)
    step = CapturedStep(lambda: torch.autograd.grad(merged(xs), merged.params, gs), warmup=1)
    for _ in range(2):
        step.outputs[0].fill_(float("nan"))
        (g_p,) = step()
        torch.cuda.synchronize()
        R.check_bound(g_p.cpu().numpy(), info, enc.n_features_per_level, 2)
