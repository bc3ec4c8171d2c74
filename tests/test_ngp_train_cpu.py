"""CPU: the argument checks of the fused training entries (decided before anything reaches a device) and the fallback of
``fused_training=True`` to the composed chain on CPU tensors and on configurations the fused launches do not serve."""
import ctypes as C

import pytest
import torch

from nerfacc_amd import _backend as B
from nerfacc_amd.fields import NGPDensityField, NGPRadianceField

AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
SMALL = dict(log2_hashmap_size=10, base_resolution=4, max_resolution=64)
P = 0x1000   # a stand-in address that is never dereferenced


def test_training_entries_report_argument_errors():
    lib = B.load()
    arr = lambda t, v: (t * len(v))(*v)
    scales, res, sizes = arr(C.c_float, [15.0, 31.0]), arr(C.c_int32, [16, 32]), arr(C.c_int32, [1024, 1024])
    vp = lambda a: C.cast(a, C.c_void_p)

    def call(bwd, full=1, mode=0, n_levels=2, G=3, n=4, save_kw=None, grads_kw=None, null_save=False):
        grid = B.NGPGrid(params=P, n_params=4096, n_levels=n_levels, n_features=2, log2_hashmap_size=10, interp=0, scales_host=vp(scales),
                         resolutions_host=vp(res), sizes_host=vp(sizes))
        inp = B.NGPInput(positions=P, dirs=P)
        sv = B.NGPSaved(**{**dict(enc=P, base_hidden=P, base_out=P, head_x=P, head_hidden=P), **(save_kw or {})})
        gr = B.NGPGrads(**{**dict(g_rgb=P, g_sigma=P, raw_rgb=P, head_dz=P, head_dz_out=P, base_dz=P, base_dz_out=P, grad_table=P),
                           **(grads_kw or {})})
        mid = (C.byref(grid), P, P, G, C.byref(inp), n, None, P, 0, 1, -1.0, None if null_save else C.byref(sv))
        rc = lib.nfa_ngp_train_bwd(1, full, mode, *mid, C.byref(gr), None) if bwd else \
            lib.nfa_ngp_train_fwd(1, full, *mid, P, 0, None, 0, None, None, None, None)
        return rc, lib.nfa_last_error().decode()

    for bwd, nm in ((False, "ngp_train_fwd"), (True, "ngp_train_bwd")):
        for kw, msg in [
            (dict(n_levels=17), f"{nm}: n_levels must be in 1..16 (got 17)"),
            (dict(G=16), f"{nm}: geo_feat_dim must be in 1..15 (got 16)"),
            (dict(null_save=True), f"{nm}: the descriptor of the saved buffers is null"),
            (dict(save_kw=dict(enc=None)), f"{nm}: null pointer (a saved buffer: enc, base_hidden, base_out, head_x, head_hidden)"),
            (dict(full=0, save_kw=dict(base_out=None, head_x=None)), f"{nm}: null pointer (a saved buffer: enc, base_hidden, base_out)"),
            (dict(save_kw=dict(enc=P + 8)), f"{nm}: misaligned pointer (enc and the hidden activations 16, base_out and head_x their element)"),
            (dict(n=0, null_save=False, save_kw=dict(enc=None)), None),
        ]:
            rc, err = call(bwd, **kw)
            assert (rc == 0) if msg is None else (rc == -1 and err == msg), (nm, kw, rc, err)
    for kw, msg in [
        (dict(mode=2), "ngp_train_bwd: mode must be NFA_NGP_GRAD_RAW (0) or NFA_NGP_GRAD_ACTIVATED (1) (got 2)"),
        (dict(grads_kw=dict(g_rgb_elem=2)), "ngp_train_bwd: g_rgb_elem 2: float32 or the networks' type (1)"),
        (dict(grads_kw=dict(base_dz=None)), "ngp_train_bwd: null pointer (base_dz, base_dz_out, head_dz, head_dz_out)"),
        (dict(mode=1, grads_kw=dict(raw_rgb=None)), "ngp_train_bwd: null pointer (raw_rgb: the activated mode forms the sigmoid from it)"),
        (dict(grads_kw=dict(grad_table=P + 4)), "ngp_train_bwd: misaligned pointer (base_dz and head_dz 16, grad_table 8, the others their element)"),
    ]:
        rc, err = call(True, **kw)
        assert rc == -1 and err == msg, (kw, rc, err)
    for args, msg in [
        ((1, 2, P, 16, 15, P, 100), b"ngp_pack_bwd: net must be NFA_NGP_NET_BASE (0) or NFA_NGP_NET_HEAD (1) (got 2)"),
        ((1, 1, P, 16, 0, P, 100), b"ngp_pack_bwd: geo_feat_dim must be in 1..15 (got 0)"),
        ((1, 1, P, 16, 15, P, 100), b"ngp_pack_bwd: the image holds 7168 elements for this shape, got 100"),
    ]:
        assert lib.nfa_ngp_pack_bwd(*args, None) == -1 and lib.nfa_last_error() == msg, args


@pytest.mark.parametrize("kw", [dict(), dict(num_dim=2), dict(n_levels=20, max_resolution=256)])
def test_fused_training_on_cpu_takes_the_composed_chain(kw):
    """CPU tensors (and, there too, an unsupported configuration): the keyword changes nothing, values and gradients."""
    D = kw.get("num_dim", 3)
    f = NGPRadianceField(AABB[:D] + AABB[3:3 + D], geo_feat_dim=7, use_viewdirs=D == 3, **{**SMALL, **kw}, fused_training=True)
    g = NGPDensityField(AABB[:D] + AABB[3:3 + D], num_dim=D, **SMALL, fused_training=True)
    x, d = torch.rand(9, D) - 0.5, torch.nn.functional.normalize(torch.randn(9, 3), dim=-1)
    for m, q in ((f, (lambda m: m(x, d)[0]) if D == 3 else (lambda m: m.query_density(x))), (g, lambda m: m(x))):
        assert m.fused_training and not m._use_train(False, x)
        outs = []
        for flag in (True, False):
            m.fused_training = flag
            y = q(m)
            outs.append((y, torch.autograd.grad(y.sum(), [m.encoding.params, m.mlp_base.params])))
        assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
