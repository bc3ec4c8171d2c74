"""CPU: SinusoidalEncoding's torch path against the fixture recorded from the reference's SinusoidalEncoder (bit for bit)
and the float64 restatement of tests/sinusoidal_reference.py, the module's interface and refusals, barf_window, and the
host-side argument checks of the three nfa_sinenc_* entry points."""
import types

import pytest
import torch

import sinusoidal_reference as R
from conftest import load_golden


def _cases():
    g = load_golden("sinusoidal")
    for i in range(int(g["n_cases"])):
        D, lo, hi, ident = (int(v) for v in g[f"c{i}_cfg"])
        yield (D, lo, hi, bool(ident)), torch.from_numpy(g[f"c{i}_x"]), torch.from_numpy(g[f"c{i}_y"])


def test_fixture_covers_the_reference_configs():
    cases = list(_cases())
    cfgs = [c for c, _, _ in cases]
    assert set(R.REFERENCE_CONFIGS) | {(3, 0, 16, True), (4, 0, 8, False)} == set(cfgs)
    spans = [float(x.abs().max()) for _, x, _ in cases]
    assert all(x.shape[0] == 64 for _, x, _ in cases) and max(spans) > 900 and sorted(spans)[-2] <= 1.5


def test_torch_path_is_the_reference_bit_for_bit():
    from nerfacc_amd.encodings import SinusoidalEncoding
    for cfg, x, y in _cases():
        enc = SinusoidalEncoding(*cfg)
        got = enc(x)
        assert got.dtype == torch.float32 and got.shape == (64, enc.latent_dim)
        assert torch.equal(got.view(torch.int32), y.view(torch.int32)), cfg


def test_float64_reference_reproduces_the_fixture_within_the_contract():
    for (D, lo, hi, ident), x, y in _cases():
        want = R.encode(x, lo, hi, ident)
        R.assert_within(y, want, R.forward_bound(x, lo, hi, ident), f"{(D, lo, hi, ident)}")
        if ident:
            assert torch.equal(y[:, :D], x)


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_latent_dim_and_column_order(cfg):
    from nerfacc_amd.encodings import SinusoidalEncoding
    D, lo, hi, ident = cfg
    L = hi - lo
    enc = SinusoidalEncoding(*cfg)
    assert enc.latent_dim == enc.n_output_dims == (int(ident) + 2 * L) * D
    o = D if ident else 0
    for d in range(D):
        x = torch.zeros(1, D)
        x[0, d] = 0.25
        y = enc(x)[0]
        assert y.shape == (enc.latent_dim,)
        sin_cols = {o + k * D + d for k in range(L)}
        lit = {c for c in range(o + L * D) if y[c] != 0}
        assert lit == sin_cols | ({d} if ident else set()), (d, lit)
        for k in range(L):
            xb = 0.25 * 2.0 ** (lo + k)
            tol = 2.0 ** -21 * max(1.0, xb)   # (the torch path keeps the reference's rounded phase)
            assert abs(float(y[o + k * D + d]) - torch.sin(torch.tensor(xb, dtype=torch.float64))) < tol
            assert abs(float(y[o + L * D + k * D + d]) - torch.cos(torch.tensor(xb, dtype=torch.float64))) < tol
        # the cosine block of the other coordinates is cos(0) (the reference's sin(pi / 2) in float32)
        others = [o + L * D + k * D + e for k in range(L) for e in range(D) if e != d]
        assert all(abs(float(y[c]) - 1.0) < 1e-6 for c in others)


def test_no_frequencies_returns_x():
    from nerfacc_amd.encodings import SinusoidalEncoding
    x = torch.randn(5, 3)
    for ident in (True, False):
        enc = SinusoidalEncoding(3, 4, 4, ident)
        assert enc(x) is x and enc.latent_dim == (3 if ident else 0)


def test_leading_dims_out_dtype_var_and_weights():
    from nerfacc_amd.encodings import SinusoidalEncoding, barf_window
    x = R.draw(35, 3, 1).view(5, 7, 3)
    var = torch.rand(5, 7, 3) * 0.1
    w = barf_window(2.4, 4)
    enc = SinusoidalEncoding(3, 0, 4)
    y = enc(x, var, w)
    assert y.shape == (5, 7, 27)
    want = R.encode(x, 0, 4, True, var, w)
    # the torch path keeps the reference's phase rounding: twice the contract's trigonometric part covers it
    R.assert_within(y, want, 2 * R.forward_bound(x, 0, 4, True, var, w), "var and weights")
    assert torch.equal(y[..., :3], x)
    assert torch.equal(enc(x, torch.zeros_like(x), torch.ones(4)), enc(x))
    half = SinusoidalEncoding(3, 0, 4, out_dtype=torch.bfloat16)(x)
    assert half.dtype == torch.bfloat16 and torch.equal(half, enc(x).to(torch.bfloat16))
    y64 = enc(x.double())
    assert y64.dtype == torch.float64 and torch.allclose(y64, R.encode(x, 0, 4), atol=1e-12)


def test_torch_path_gradients():
    from nerfacc_amd.encodings import SinusoidalEncoding
    enc = SinusoidalEncoding(2, -1, 3, False)
    x = R.draw(6, 2, 2).double().requires_grad_(True)
    var = (torch.rand(6, 2, dtype=torch.float64) * 0.1).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: enc(a, b), (x, var))
    w = torch.tensor([1.0, 0.5, 0.0, 0.25])
    y = enc(x, freq_weights=w)
    assert (y[:, 4:6] == 0).all() and (y[:, 12:14] == 0).all()


def test_refusals():
    from nerfacc_amd.encodings import SinusoidalEncoding
    for args, text in [
        ((0, 0, 4), "SinusoidalEncoding: n_input_dims must be in 1..4 (got 0)"),
        ((5, 0, 4), "SinusoidalEncoding: n_input_dims must be in 1..4 (got 5)"),
        ((3, 4, 3), "SinusoidalEncoding: need integers -16 <= min_deg <= max_deg <= 32 (got min_deg=4, max_deg=3)"),
        ((3, -17, 0), "SinusoidalEncoding: need integers -16 <= min_deg <= max_deg <= 32 (got min_deg=-17, max_deg=0)"),
        ((3, 20, 33), "SinusoidalEncoding: need integers -16 <= min_deg <= max_deg <= 32 (got min_deg=20, max_deg=33)"),
        ((3, 0.0, 4), "SinusoidalEncoding: need integers -16 <= min_deg <= max_deg <= 32 (got min_deg=0.0, max_deg=4)"),
        ((3, 0, 17), "SinusoidalEncoding: at most 16 frequencies (got max_deg - min_deg = 17)"),
    ]:
        with pytest.raises(ValueError) as e:
            SinusoidalEncoding(*args)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="out_dtype must be None"):
        SinusoidalEncoding(3, 0, 4, out_dtype=torch.float64)
    assert SinusoidalEncoding(3, 0, 4, out_dtype=torch.float32).out_dtype is None
    enc = SinusoidalEncoding(3, 0, 4)
    x = torch.zeros(2, 3)
    for kw, text in [
        (dict(x=torch.zeros(2, 2)), "SinusoidalEncoding: x must have shape (..., 3) (got (2, 2))"),
        (dict(x=x, var=torch.zeros(2, 1)), "SinusoidalEncoding: var must have x's shape (2, 3) (got (2, 1))"),
        (dict(x=x, freq_weights=torch.ones(3)),
         "SinusoidalEncoding: freq_weights must be a float32 tensor of shape (4,) (got (3,), torch.float32)"),
        (dict(x=x, freq_weights=torch.ones(4, dtype=torch.float64)),
         "SinusoidalEncoding: freq_weights must be a float32 tensor of shape (4,) (got (4,), torch.float64)"),
        (dict(x=x, freq_weights=torch.ones(4, device="meta")),
         "SinusoidalEncoding: freq_weights must be on x's device cpu (got meta)"),
    ]:
        with pytest.raises(ValueError) as e:
            enc(**kw)
        assert str(e.value) == text
    assert "min_deg=0, max_deg=4" in repr(enc)


def test_second_order_with_var_is_refused():
    """The native backward's own backward refuses var before it touches a tensor (a stand-in context: no GPU here)."""
    from nerfacc_amd.encodings import _SinEncBwdFn
    ctx = types.SimpleNamespace(has_var=True, has_fw=False, needs_input_grad=(True,) * 8, saved_tensors=())
    with pytest.raises(NotImplementedError, match=r"^SinusoidalEncoding: the second order "):
        _SinEncBwdFn.backward(ctx, torch.zeros(2, 3), None)
    ctx.has_var = False
    with pytest.raises(NotImplementedError, match=r"^SinusoidalEncoding: the second order "):
        _SinEncBwdFn.backward(ctx, None, torch.zeros(2, 3))
    assert _SinEncBwdFn.backward(ctx, None, None) == (None,) * 8


def test_barf_window():
    from nerfacc_amd.encodings import barf_window
    L = 6
    assert torch.equal(barf_window(0.0, L), torch.zeros(L))
    assert torch.equal(barf_window(float(L), L), torch.ones(L))
    mid = barf_window(L / 2, L)
    assert mid.dtype == torch.float32 and torch.equal(mid, torch.tensor([1.0] * 3 + [0.0] * 3))
    frac = barf_window(2.25, L)
    assert torch.allclose(frac.double(), R.barf_window(2.25, L), atol=2.0 ** -23) and 0 < frac[2] < 0.5 and frac[3] == 0
    assert barf_window(torch.tensor(1.5), 3).shape == (3,)


def test_names_stay_out_of_the_package_namespace():
    import nerfacc_amd
    from nerfacc_amd import encodings
    assert len(nerfacc_amd.__all__) == 22
    assert not {"SinusoidalEncoding", "barf_window"} & set(nerfacc_amd.__all__)
    assert {"SinusoidalEncoding", "barf_window"} <= set(encodings.__all__)


# ----------------------------------------------------------------------------- C ABI argument checks
P = 0x1000   # a stand-in address that is never dereferenced
_ARGS = {
    "nfa_sinenc_fwd": "elem x var freq_weights n_points n_dims min_deg n_freqs identity out stream",
    "nfa_sinenc_bwd": "elem x var freq_weights grad_out n_points n_dims min_deg n_freqs identity grad_x grad_var stream",
    "nfa_sinenc_bwd_bwd": "elem x freq_weights grad_out gg_x n_points n_dims min_deg n_freqs identity grad_grad_out grad_x stream",
}
_SCALARS = {"elem": 0, "n_points": 16, "n_dims": 3, "min_deg": 0, "n_freqs": 4, "identity": 1}


def _abi_cases():
    cases = []
    for fn in _ARGS:
        nm = fn[len("nfa_"):]
        # in the order in which the checks fire: each is also tried together with everything after it
        ordered = [
            ({"elem": 3}, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got 3)"),
            ({"n_dims": 0}, f"{nm}: n_dims must be in 1..4 (got 0)"),
            ({"n_freqs": 17}, f"{nm}: n_freqs must be in 0..16 (got 17)"),
            ({"min_deg": -17}, f"{nm}: min_deg must be in -16..32 - n_freqs (got -17)"),
            ({"n_points": -1}, f"{nm}: negative n_points"),
            ({"x": None}, f"{nm}: null pointer"),
        ]
        for i, (kw, msg) in enumerate(ordered):
            later = {}
            for kw2, _ in ordered[i + 1:]:
                later.update(kw2)
            cases += [(fn, kw, msg), (fn, {**later, **kw}, msg)]
        cases += [
            (fn, {"elem": -1}, f"{nm}: elem must be NFA_ELEM_F32, NFA_ELEM_F16 or NFA_ELEM_BF16 (got -1)"),
            (fn, {"n_dims": 5}, f"{nm}: n_dims must be in 1..4 (got 5)"),
            (fn, {"n_freqs": -1}, f"{nm}: n_freqs must be in 0..16 (got -1)"),
            (fn, {"min_deg": 29}, f"{nm}: min_deg must be in -16..32 - n_freqs (got 29)"),
            (fn, {"n_points": 1 << 31}, f"{nm}: too many points (at most 2^31 - 1)"),
            (fn, {"n_points": 0, "all_null": True}, None),
            (fn, {"n_freqs": 0, "identity": 0, "all_null": True}, None),   # no columns
        ]
    cases += [
        ("nfa_sinenc_fwd", {"out": None}, "sinenc_fwd: null pointer"),
        ("nfa_sinenc_fwd", {"out": P + 8}, "sinenc_fwd: out must be 16-byte aligned"),
        ("nfa_sinenc_bwd", {"grad_out": None}, "sinenc_bwd: null pointer"),
        ("nfa_sinenc_bwd", {"grad_x": None, "grad_var": None}, "sinenc_bwd: null pointer"),
        ("nfa_sinenc_bwd", {"var": None}, "sinenc_bwd: grad_var without var"),
        ("nfa_sinenc_bwd", {"grad_out": P + 4}, "sinenc_bwd: grad_out must be 16-byte aligned"),
        ("nfa_sinenc_bwd_bwd", {"grad_out": None}, "sinenc_bwd_bwd: null pointer"),
        ("nfa_sinenc_bwd_bwd", {"gg_x": None}, "sinenc_bwd_bwd: null pointer"),
        ("nfa_sinenc_bwd_bwd", {"grad_grad_out": None, "grad_x": None}, "sinenc_bwd_bwd: null pointer"),
        ("nfa_sinenc_bwd_bwd", {"grad_grad_out": P + 8}, "sinenc_bwd_bwd: grad_out and grad_grad_out must be 16-byte aligned"),
    ]
    return cases


def test_entry_points_are_bound_and_check_their_arguments():
    from nerfacc_amd import _backend as B
    assert set(_ARGS) <= set(B.EXPORTED_SYMBOLS)
    lib = B.load()
    for fn, kw, msg in _abi_cases():
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
