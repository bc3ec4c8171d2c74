"""CPU: the identity the constant-step (`_cs`) entry points rest on, and their argument checks.

With ``step_size > 0`` and no cone angle every sample of the reference's marcher is ``t_next = t_last + dt`` with
``dt = step`` (grid.cu:213-215), so ``t_ends == fl32(t_starts + fl32(step))`` sample by sample -- across binade crossings and
for per-ray near planes.  Checked here on the oracle's samples with zero mismatches allowed."""
import math

import numpy as np
import pytest


def shell_grid(res, seed=42):
    """bench.py's grid: a shell of radius 0.50 .. 0.66 plus 2 % speckle."""
    rng = np.random.default_rng(seed)
    c = (np.arange(res) + 0.5) / res * 2 - 1
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    return (((r >= 0.50) & (r <= 0.66)) | (rng.random((res, res, res)) < 0.02))[None]


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o, d


AABB = np.array([[-1, -1, -1, 1, 1, 1]], np.float32)
# (rays, grid, step, near plane, jittered per-ray near planes)
SCENES = [
    (4099, 32, 2 * math.sqrt(3) / 1024, 0.0, False),
    (2000, 16, 0.0137, 0.2, False),
    (3000, 32, 1e-3, 0.9, False),
    (3000, 32, 2 * math.sqrt(3) / 1024, 0.0, True),
]


@pytest.mark.parametrize("n_rays,res,step,near,jitter", SCENES)
def test_oracle_t_ends_is_t_starts_plus_step(oracle, n_rays, res, step, near, jitter):
    o, d = random_rays(n_rays, 7 + res)
    if near == 0.9:
        o *= 2.0   # origins further out: distances beyond 4
    t_min = None
    if jitter:   # what stratified sampling does to the near planes
        t_min = (near + np.random.default_rng(3).random(n_rays) * step).astype(np.float32)
    ri, ts, te = oracle.occgrid_sampling(o, d, shell_grid(res), AABB, near_plane=near, t_min=t_min, render_step_size=step)
    assert ts.dtype == np.float32 and te.dtype == np.float32 and ts.size > 2000
    want = ts + np.float32(step)   # float32 + float32: one rounding
    assert want.dtype == np.float32
    assert int((want != te).sum()) == 0, (int((want != te).sum()), ts.size)
    if near == 0.9:
        assert ts.min() < 1.0 and ts.max() > 4.0   # the samples cross the binades at 1, 2 and 4


# The three entry points: argument names in C order and their checks in the order in which they fire (each case is decided
# on the host: the pointers are stand-ins that are never dereferenced).
P = 0x1000
_CS = {
    "nfa_render_visibility_cs": "t_starts step sigmas prefix_trans early_stop_eps alpha_thre packed_info tiles n_tiles n_rays n_elems "
                                "vis vis_cnts stream",
    "nfa_render_fused_fwd_cs": "t_starts step sigmas rgbs packed_info tiles n_tiles n_rays n_elems weights trans alphas colors "
                               "opacities depths stream",
    "nfa_render_fused_bwd_cs": "t_starts step rgbs trans alphas g_colors g_opacities g_depths g_weights g_trans g_alphas packed_info "
                               "tiles n_tiles n_rays n_elems grad_sigmas grad_rgbs stream",
}
_SCALARS = {"step": 0.01, "early_stop_eps": 1e-4, "alpha_thre": 0.0, "n_tiles": 1, "n_rays": 4, "n_elems": 16}
_TOO_MANY = (1 << 31) - 64


def _checks(fn):
    nm = fn[len("nfa_"):]
    bad_step = [({"step": v}, f"{nm}: step must be > 0") for v in (0.0, -0.01, float("inf"), float("nan"))]
    common = [
        ({"n_rays": -1}, f"{nm}: negative size"),
        ({"n_elems": -1}, f"{nm}: negative size"),
        ({"n_rays": _TOO_MANY}, f"{nm}: too many rays"),
        ({"n_rays": 0, "n_elems": 0}, None),            # nothing to do: accepted before anything else is looked at
        ({"packed_info": None}, f"{nm}: packed_info/tiles is null"),
        ({"tiles": None}, f"{nm}: packed_info/tiles is null"),
        ({"n_tiles": 0}, f"{nm}: packed_info/tiles is null"),
        *bad_step,
    ]
    null = lambda names: [({n: None}, f"{nm}: null pointer") for n in names.split()]
    if fn == "nfa_render_visibility_cs":
        # (its n_elems == 0 return comes after a look at the device: in the GPU test)
        return common + null("t_starts sigmas vis")
    if fn == "nfa_render_fused_fwd_cs":
        return common + [({"n_rays": 0, "colors": None}, None)] + null("colors opacities depths t_starts sigmas rgbs")
    return common + [({"n_elems": 0, "t_starts": None}, None)] + null("t_starts rgbs trans alphas") + \
        [({"grad_sigmas": None, "grad_rgbs": None}, f"{nm}: null pointer")]


def _call(lib, fn, kw):
    args = []
    for a in _CS[fn].split():
        if a in kw:
            args.append(kw[a])
        elif a in _SCALARS:
            args.append(_SCALARS[a])
        else:
            args.append(None if a == "stream" else P)
    lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
    return getattr(lib, fn)(*args), lib.nfa_last_error()


@pytest.mark.parametrize("fn", sorted(_CS))
def test_cs_argument_errors_in_order(fn):
    """Each check alone, and each together with the first later check of another outcome: the earlier one decides."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    assert fn in B.EXPORTED_SYMBOLS
    checks = _checks(fn)
    for i, (kw, msg) in enumerate(checks):
        later = next((c[0] for c in checks[i + 1:] if c[1] != msg and c[1] is not None), {})
        for case in (kw, {**later, **kw}):
            rc, err = _call(lib, fn, case)
            if msg is None:
                assert rc == 0, (fn, case, rc, err)
            else:
                assert rc == -1 and err == msg.encode(), (fn, case, rc, err, msg)


def test_tag_needs_the_same_untouched_pair():
    """const_step_of on CPU tensors: never valid (the passes run on the device only), and the tag itself never raises."""
    import torch
    from nerfacc_amd._segments import const_step_of, tag_const_step
    ts = torch.arange(8, dtype=torch.float32)
    te = ts + 0.5
    assert const_step_of(ts, te) is None and const_step_of(None, te) is None and const_step_of(ts, None) is None
    tag_const_step(ts, te, 0.5)
    assert const_step_of(ts, te) is None          # tagged, but not on the device
    assert const_step_of(ts.clone(), te) is None
