"""CPU: nerfacc_amd.losses.distortion -- the signature, the torch path against a float64 pairwise restatement (values and
gradients, packed and batched), and the C ABI's argument checks of nfa_distortion_{fwd,bwd}."""
import inspect

import pytest
import torch


def pairwise_distortion(w, ts, te, ray_ids, n_rays):
    """float64, O(n^2) per ray: sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 s_i (Barron et al. 2022, eq. 15)."""
    w, ts, te = (t.to(torch.float64) for t in (w, ts, te))
    m, s = (ts + te) / 2, te - ts
    same = ray_ids[:, None] == ray_ids[None, :]
    pair = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs() * same).sum(-1)
    return torch.zeros(n_rays, dtype=torch.float64).index_add(0, ray_ids, pair + w * w * s / 3)


def make_packed(lengths, seed=0, offset=0.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    ray_ids = torch.repeat_interleave(torch.arange(len(lengths)), lengths)
    n = int(lengths.sum())
    steps = torch.rand(n, generator=g, dtype=torch.float64) * 0.1 + 1e-3
    # per-ray increasing t: cumulative step lengths restarted at every ray
    c = torch.cumsum(steps, 0)
    starts = torch.cumsum(lengths, 0) - lengths
    base = torch.where(starts[ray_ids] > 0, c[(starts[ray_ids] - 1).clamp_min(0)], torch.zeros_like(c))
    te = c - base + offset
    ts = te - steps * torch.rand(n, generator=g, dtype=torch.float64)
    w = torch.rand(n, generator=g, dtype=torch.float64) * 0.5
    return w.to(dtype), ts.to(dtype), te.to(dtype), ray_ids


def grads(fn, *xs):
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    out = fn(*xs)
    g = torch.linspace(0.5, 1.5, out.numel(), dtype=out.dtype).view(out.shape)
    return out.detach(), torch.autograd.grad(out, xs, g)


def test_module_and_signature():
    import nerfacc_amd
    from nerfacc_amd import losses
    params = list(inspect.signature(losses.distortion).parameters.values())
    assert [(p.name, p.default) for p in params] == [
        ("weights", inspect.Parameter.empty), ("t_starts", inspect.Parameter.empty), ("t_ends", inspect.Parameter.empty),
        ("ray_indices", None), ("n_rays", None), ("packed_info", None)]
    assert "distortion" not in nerfacc_amd.__all__ and "losses" not in nerfacc_amd.__all__


LENGTHS = [0, 1, 5, 0, 17, 2, 1, 40, 0, 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_packed_torch_matches_pairwise(dtype):
    from nerfacc_amd.losses import distortion
    w, ts, te, ri = make_packed(LENGTHS, seed=1, dtype=dtype)
    R = len(LENGTHS)
    got, g_got = grads(lambda a, b, c: distortion(a, b, c, ray_indices=ri, n_rays=R), w, ts, te)
    ref, g_ref = grads(lambda a, b, c: pairwise_distortion(a, b, c, ri, R), w, ts, te)
    tol = 1e-5 if dtype == torch.float32 else 1e-10
    assert got.shape == (R,) and got.dtype == dtype
    torch.testing.assert_close(got.double(), ref, rtol=tol, atol=tol)
    assert float(got[0]) == 0.0 and float(got[3]) == 0.0   # empty rays
    for a, b in zip(g_got, g_ref):
        torch.testing.assert_close(a.double(), b.double(), rtol=tol, atol=tol)
    # packed_info gives the same
    pi = torch.stack([torch.cumsum(torch.tensor(LENGTHS), 0) - torch.tensor(LENGTHS), torch.tensor(LENGTHS)], -1)
    got_pi, g_pi = grads(lambda a, b, c: distortion(a, b, c, packed_info=pi), w, ts, te)
    torch.testing.assert_close(got_pi, got, rtol=0, atol=0)
    for a, b in zip(g_pi, g_got):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_one_sample_rays():
    from nerfacc_amd.losses import distortion
    w, ts, te, ri = make_packed([1, 1, 1], seed=2, dtype=torch.float64)
    got, (gw, gts, gte) = grads(lambda a, b, c: distortion(a, b, c, ray_indices=ri, n_rays=3), w, ts, te)
    s = te - ts
    g = torch.linspace(0.5, 1.5, 3, dtype=torch.float64)
    torch.testing.assert_close(got, w * w * s / 3)
    torch.testing.assert_close(gw, g * 2 * w * s / 3)
    torch.testing.assert_close(gte, g * w * w / 3)
    torch.testing.assert_close(gts, -g * w * w / 3)


def test_unsorted_ray_indices():
    from nerfacc_amd.losses import distortion
    w, ts, te, ri = make_packed(LENGTHS, seed=3, dtype=torch.float64)
    # rays interleaved at random, each ray's samples still in order
    key = torch.rand(w.numel(), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    key = (2.0 * ri + key)[torch.argsort(2.0 * ri + key)] - 2.0 * ri
    perm = torch.argsort(key)
    assert not bool((ri[perm][1:] >= ri[perm][:-1]).all())
    R = len(LENGTHS)
    got, g_got = grads(lambda a, b, c: distortion(a, b, c, ray_indices=ri[perm], n_rays=R), w[perm], ts[perm], te[perm])
    ref, g_ref = grads(lambda a, b, c: pairwise_distortion(a, b, c, ri[perm], R), w[perm], ts[perm], te[perm])
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_got, g_ref):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
    # n_rays defaults to max + 1
    torch.testing.assert_close(distortion(w, ts, te, ray_indices=ri), got[: int(ri.max()) + 1])


def test_batched_torch_matches_pairwise():
    from nerfacc_amd.losses import distortion
    R, S = 6, 9
    w, ts, te, _ = make_packed([S] * R, seed=4, offset=3.0, dtype=torch.float32)
    shape = (2, 3, S)
    got, g_got = grads(lambda a, b, c: distortion(a, b, c), *(t.view(shape) for t in (w, ts, te)))
    ids = torch.arange(R).repeat_interleave(S)
    ref, g_ref = grads(lambda a, b, c: pairwise_distortion(a.reshape(-1), b.reshape(-1), c.reshape(-1), ids, R).view(2, 3),
                       *(t.view(shape) for t in (w, ts, te)))
    assert got.shape == (2, 3)
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-6)
    for a, b in zip(g_got, g_ref):
        assert a.shape == shape
        torch.testing.assert_close(a.double(), b.double(), rtol=1e-5, atol=1e-6)


def test_out_of_order_is_the_linear_formula():
    """Input out of midpoint order is not detected: the result is the O(n) formula's, not the pairwise loss."""
    from nerfacc_amd.losses import distortion
    w = torch.tensor([0.5, 0.5], dtype=torch.float64)
    ts, te = torch.tensor([2.0, 0.0], dtype=torch.float64), torch.tensor([2.0, 0.0], dtype=torch.float64)
    got = distortion(w, ts, te, ray_indices=torch.zeros(2, dtype=torch.int64), n_rays=1)
    # 2 w_1 (m_1 W<1 - S<1) with m = (2, 0): 2 * 0.5 * (0 * 0.5 - 0.5 * 2) = -1 (the pairwise loss is +1)
    torch.testing.assert_close(got, torch.tensor([-1.0], dtype=torch.float64))


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_distortion_fwd": "weights t_starts t_ends packed_info tiles n_tiles n_rays n_elems loss w_tot s_tot stream",
    "nfa_distortion_bwd": "weights t_starts t_ends w_tot s_tot g_loss packed_info tiles n_tiles n_rays n_elems grad_weights "
                          "grad_t_starts grad_t_ends stream",
}
_SCALARS = {"n_tiles": 1, "n_rays": 4, "n_elems": 16}
_TOO_MANY = (1 << 31) - 64


def _cases():
    cases = []
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        cases += [
            (fn, {"n_rays": -1}, f"{nm}: negative size"),
            (fn, {"n_elems": -1}, f"{nm}: negative size"),
            (fn, {"n_rays": _TOO_MANY}, f"{nm}: too many rays"),
            (fn, {"packed_info": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"tiles": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"n_tiles": 0}, f"{nm}: packed_info/tiles is null"),
            (fn, {"n_rays": 0, "n_elems": 0, "all_null": True}, None),
        ]
    cases += [(("nfa_distortion_fwd", {a: None}, "distortion_fwd: null pointer")) for a in "loss w_tot s_tot weights t_starts t_ends".split()]
    cases += [("nfa_distortion_fwd", {"n_rays": 0, "loss": None, "weights": None}, None),
              ("nfa_distortion_fwd", {"n_elems": 0, "weights": None, "t_starts": None, "t_ends": None, "packed_info": P,
                                      "tiles": P, "loss": None}, "distortion_fwd: null pointer")]
    cases += [("nfa_distortion_bwd", {a: None}, "distortion_bwd: null pointer")
              for a in "weights t_starts t_ends w_tot s_tot g_loss".split()]
    cases += [("nfa_distortion_bwd", {"grad_weights": None, "grad_t_starts": None, "grad_t_ends": None},
               "distortion_bwd: null pointer"),
              ("nfa_distortion_bwd", {"n_elems": 0, "weights": None, "g_loss": None}, None)]
    return cases


def test_distortion_argument_errors():
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert lib.nfa_version() == B.ABI_VERSION == 403
    for fn, kw, msg in _cases():
        kw = dict(kw)
        all_null = kw.pop("all_null", False)
        args = [kw[a] if a in kw else _SCALARS[a] if a in _SCALARS else (None if all_null or a == "stream" else P)
                for a in _ARGS[fn].split()]
        assert len(args) == len(B._SIGS[fn])
        lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
        rc = getattr(lib, fn)(*args)
        if msg is None:
            assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
        else:
            assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())
