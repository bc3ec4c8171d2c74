"""CPU: the C-ABI library loads and exports exactly what include/nerfacc_hip.h declares."""
import os
import re

from conftest import ROOT


def test_header_and_library_agree():
    from nerfacc_amd import _backend as B
    hdr = open(os.path.join(ROOT, "include", "nerfacc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfa_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = B.load()  # builds with hipcc if needed; raises if a bound symbol is missing
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nerfacc_hip.h but not exported"
    assert declared == set(B.EXPORTED_SYMBOLS), declared ^ set(B.EXPORTED_SYMBOLS)
    assert lib.nfa_version() >= 100
    from nerfacc_amd._backend import seg_plan
    assert seg_plan(0) == (1024, 1) and seg_plan(32 * 1024 * 1024)[0] % 256 == 0
    assert seg_plan(2048, 1000) == (1024, 2 + 1000 // 256 + 1)   # a tile also ends after 256 rays


def test_argument_errors_are_reported():
    from nerfacc_amd import _backend as B
    import ctypes as C
    lib = B.load()
    rc = lib.nfa_traverse_grids(None, None)
    assert rc != 0 and b"null args" in lib.nfa_last_error()
    a = B.TraverseArgs()
    a.n_rays = 4
    a.mode = 7
    rc = lib.nfa_traverse_grids(C.byref(a), None)
    assert rc != 0 and b"mode" in lib.nfa_last_error()
    rc = lib.nfa_importance_sampling(None, None, None, 4, 3, 0, 0, 0, 0, None, None, None)
    assert rc != 0 and b">= 1" in lib.nfa_last_error()


# The packed-segment entry points (csrc/segscan.hip): argument names in C order, and the cases that must be rejected
# (or return early) before anything reaches the GPU.  P is a stand-in address that is never dereferenced.
P = 0x1000
_SEG = {
    "nfa_seg_build_tiles": "packed_info n_rays n_elems tile_elems n_tiles tiles flags stream",
    "nfa_packed_scan": "kind reverse packed_info tiles n_tiles n_rays n_elems inputs outputs stream",
    "nfa_packed_scan_generic": "kind reverse normalize packed_info n_rays n_elems inputs outputs stream",
    "nfa_packed_prod_backward": "kind packed_info tiles n_tiles n_rays n_elems inputs outputs grad_outputs grad_inputs stream",
    "nfa_render_from_density_fwd": "t_starts t_ends sigmas prefix_trans packed_info tiles n_tiles n_rays n_elems weights trans alphas stream",
    "nfa_render_from_alpha_fwd": "alphas prefix_trans packed_info tiles n_tiles n_rays n_elems weights trans stream",
    "nfa_render_from_density_bwd": "t_starts t_ends trans alphas g_weights g_trans g_alphas packed_info tiles n_tiles n_rays n_elems "
                                   "grad_sigmas grad_x stream",
    "nfa_density_cdf_rows_fwd": "t_starts t_ends sigmas packed_info tiles n_tiles n_rays n_elems row_len trans alphas cdfs stream",
    "nfa_density_cdf_rows_bwd": "t_starts t_ends trans alphas g_cdfs packed_info tiles n_tiles n_rays n_elems row_len grad_sigmas stream",
    "nfa_render_from_alpha_bwd": "alphas trans g_weights g_trans packed_info tiles n_tiles n_rays n_elems grad_alphas stream",
    "nfa_render_visibility": "t_starts t_ends sigmas_or_alphas prefix_trans early_stop_eps alpha_thre packed_info tiles n_tiles n_rays "
                             "n_elems vis vis_cnts stream",
    "nfa_compact_samples": "vis t_starts t_ends packed_info tiles n_tiles out_starts n_rays n_elems out_ray_indices out_t_starts "
                           "out_t_ends capacity stream",
    "nfa_accumulate_along_rays": "weights values D packed_info tiles n_tiles n_rays n_elems accumulate out stream",
    "nfa_accumulate_along_rays_atomic": "weights values D ray_indices n_rays n_elems out stream",
    "nfa_accumulate_along_rays_bwd": "weights values D g_out packed_info tiles n_tiles n_rays n_elems g_weights g_values stream",
    "nfa_render_accumulate_fwd": "weights rgbs t_starts t_ends packed_info tiles n_tiles n_rays n_elems colors opacities depths stream",
    "nfa_render_accumulate_bwd": "weights rgbs t_starts t_ends g_colors g_opacities g_depths packed_info tiles n_tiles n_rays n_elems "
                                 "g_weights g_rgbs stream",
    "nfa_render_fused_fwd": "t_starts t_ends sigmas rgbs packed_info tiles n_tiles n_rays n_elems weights trans alphas colors opacities "
                            "depths stream",
    "nfa_render_fused_bwd": "t_starts t_ends rgbs trans alphas g_colors g_opacities g_depths g_weights g_trans g_alphas packed_info "
                            "tiles n_tiles n_rays n_elems grad_sigmas grad_rgbs stream",
    "nfa_render_step_accumulate": "t_starts t_ends sigmas rgbs packed_info tiles n_tiles n_rays n_elems alpha_thre colors opacities "
                                  "depths n_visible stream",
}
# arguments that are not pointers, at values every check accepts
_SEG_SCALARS = {"kind": 0, "reverse": 0, "normalize": 0, "n_tiles": 1, "n_rays": 4, "n_elems": 16, "tile_elems": 64,
                "row_len": 4, "early_stop_eps": 1e-4, "alpha_thre": 0.0, "capacity": 16, "D": 2, "accumulate": 0}
_TOO_MANY = (1 << 31) - 64
_ENGINE = [n for n in _SEG if n not in ("nfa_seg_build_tiles", "nfa_packed_scan_generic", "nfa_accumulate_along_rays_atomic")]


def _seg_cases():
    cases = []
    for fn in _ENGINE:
        nm = fn[len("nfa_"):]
        cases += [
            (fn, {"n_rays": -1}, f"{nm}: negative size"),
            (fn, {"n_elems": -1}, f"{nm}: negative size"),
            (fn, {"n_rays": _TOO_MANY}, f"{nm}: too many rays"),
            (fn, {"packed_info": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"tiles": None}, f"{nm}: packed_info/tiles is null"),
            (fn, {"n_tiles": 0}, f"{nm}: packed_info/tiles is null"),
            # nothing to do: accepted before any other argument is looked at
            (fn, {"n_rays": 0, "n_elems": 0, "kind": 7, "D": 0, "row_len": 0, "capacity": -1, "all_null": True}, None),
        ]

    def null(fn, names, msg, **kw):
        return [(fn, {n: None, **kw}, msg) for n in names.split()]

    cases += [
        ("nfa_seg_build_tiles", {"n_rays": -1}, "seg_build_tiles: bad arguments"),
        ("nfa_seg_build_tiles", {"n_elems": -1}, "seg_build_tiles: bad arguments"),
        ("nfa_seg_build_tiles", {"tiles": None}, "seg_build_tiles: bad arguments"),
        ("nfa_seg_build_tiles", {"packed_info": None}, "seg_build_tiles: packed_info is null"),
        ("nfa_seg_build_tiles", {"n_rays": _TOO_MANY}, "seg_build_tiles: too many rays"),
        *[("nfa_seg_build_tiles", kw, "seg_build_tiles: tile_elems must be a multiple of 4 (>= 64) and n_tiles what nfa_seg_plan "
           "returns for (n_elems, n_rays)") for kw in ({"tile_elems": 60}, {"tile_elems": 66}, {"n_tiles": 2}, {"n_tiles": 0})],
        ("nfa_packed_scan", {"kind": 4}, "packed_scan: kind must be 0..3"),
        ("nfa_packed_scan", {"kind": -1, "n_elems": 0}, "packed_scan: kind must be 0..3"),
        ("nfa_packed_scan", {"n_elems": 0, "inputs": None, "outputs": None}, None),
        *null("nfa_packed_scan", "inputs outputs", "packed_scan: null data pointer"),
        ("nfa_packed_scan_generic", {"kind": 4}, "packed_scan_generic: bad arguments"),
        ("nfa_packed_scan_generic", {"n_rays": -1}, "packed_scan_generic: bad arguments"),
        ("nfa_packed_scan_generic", {"n_elems": -1}, "packed_scan_generic: bad arguments"),
        ("nfa_packed_scan_generic", {"n_rays": 0, "packed_info": None}, None),
        *null("nfa_packed_scan_generic", "packed_info inputs outputs", "packed_scan_generic: null pointer"),
        ("nfa_packed_prod_backward", {"kind": 1}, "packed_prod_backward: kind must be 2 or 3"),
        ("nfa_packed_prod_backward", {"kind": 4, "n_elems": 0}, "packed_prod_backward: kind must be 2 or 3"),
        ("nfa_packed_prod_backward", {"kind": 2, "n_elems": 0, "inputs": None}, None),
        *null("nfa_packed_prod_backward", "inputs outputs grad_outputs grad_inputs", "packed_prod_backward: null data pointer", kind=3),
        ("nfa_render_from_density_fwd", {"n_elems": 0, "t_starts": None}, None),
        *null("nfa_render_from_density_fwd", "t_starts t_ends sigmas", "render_from_density_fwd: null input"),
        *null("nfa_render_from_alpha_fwd", "alphas", "render_from_alpha_fwd: null input"),
        *null("nfa_render_from_density_bwd", "t_starts t_ends trans alphas", "render_from_density_bwd: null pointer"),
        ("nfa_render_from_density_bwd", {"grad_sigmas": None, "grad_x": None}, "render_from_density_bwd: null pointer"),
        *null("nfa_density_cdf_rows_fwd", "t_starts t_ends sigmas cdfs", "density_cdf_rows_fwd: null pointer", row_len=3),
        *[("nfa_density_cdf_rows_fwd", {"row_len": r}, "density_cdf_rows_fwd: n_elems must be n_rays * row_len") for r in (0, -4, 3)],
        *null("nfa_density_cdf_rows_bwd", "t_starts t_ends trans g_cdfs grad_sigmas", "density_cdf_rows_bwd: null pointer", row_len=3),
        ("nfa_density_cdf_rows_bwd", {"alphas": None, "row_len": 3}, "density_cdf_rows_bwd: n_elems must be n_rays * row_len"),
        ("nfa_density_cdf_rows_bwd", {"row_len": 0}, "density_cdf_rows_bwd: n_elems must be n_rays * row_len"),
        *null("nfa_render_from_alpha_bwd", "alphas trans grad_alphas", "render_from_alpha_bwd: null pointer"),
        *null("nfa_render_visibility", "sigmas_or_alphas vis", "render_visibility: null pointer"),
        ("nfa_render_visibility", {"t_ends": None}, "render_visibility: t_ends is null"),
        *null("nfa_compact_samples", "vis t_starts t_ends out_starts", "compact_samples: null input", capacity=-1),
        ("nfa_compact_samples", {"capacity": -1}, "compact_samples: negative capacity"),
        *[("nfa_accumulate_along_rays", kw, "accumulate_along_rays: bad D")
          for kw in ({"D": 0}, {"D": -3}, {"D": 2, "values": None}, {"D": 0, "n_rays": 0})],
        ("nfa_accumulate_along_rays", {"n_rays": 0, "out": None, "weights": None}, None),
        *null("nfa_accumulate_along_rays", "out weights", "accumulate_along_rays: null pointer"),
        ("nfa_accumulate_along_rays_atomic", {"D": 0}, "accumulate_along_rays_atomic: bad arguments"),
        ("nfa_accumulate_along_rays_atomic", {"D": 3, "values": None}, "accumulate_along_rays_atomic: bad arguments"),
        ("nfa_accumulate_along_rays_atomic", {"n_rays": -1}, "accumulate_along_rays_atomic: bad arguments"),
        ("nfa_accumulate_along_rays_atomic", {"n_elems": 0, "weights": None}, None),
        *null("nfa_accumulate_along_rays_atomic", "weights ray_indices out", "accumulate_along_rays_atomic: null pointer"),
        *[("nfa_accumulate_along_rays_bwd", kw, "accumulate_along_rays_bwd: bad D")
          for kw in ({"D": 0}, {"D": 2, "values": None}, {"D": 0, "n_elems": 0})],
        ("nfa_accumulate_along_rays_bwd", {"n_elems": 0, "weights": None}, None),
        *null("nfa_accumulate_along_rays_bwd", "weights g_out", "accumulate_along_rays_bwd: null pointer"),
        ("nfa_accumulate_along_rays_bwd", {"g_weights": None, "g_values": None}, "accumulate_along_rays_bwd: null pointer"),
        ("nfa_render_accumulate_fwd", {"n_rays": 0, "colors": None}, None),
        *null("nfa_render_accumulate_fwd", "colors opacities depths weights rgbs t_starts t_ends", "render_accumulate_fwd: null pointer"),
        *null("nfa_render_accumulate_bwd", "weights rgbs t_starts t_ends", "render_accumulate_bwd: null pointer"),
        ("nfa_render_accumulate_bwd", {"g_weights": None, "g_rgbs": None}, "render_accumulate_bwd: null pointer"),
        ("nfa_render_fused_fwd", {"n_rays": 0, "colors": None}, None),
        *null("nfa_render_fused_fwd", "colors opacities depths t_starts t_ends sigmas rgbs", "render_fused_fwd: null pointer"),
        *null("nfa_render_fused_bwd", "t_starts t_ends rgbs trans alphas", "render_fused_bwd: null pointer"),
        ("nfa_render_fused_bwd", {"grad_sigmas": None, "grad_rgbs": None}, "render_fused_bwd: null pointer"),
        ("nfa_render_step_accumulate", {"n_elems": 0, "colors": None}, None),
        *null("nfa_render_step_accumulate", "t_starts t_ends sigmas rgbs colors opacities depths", "render_step_accumulate: null pointer"),
    ]
    return cases


def test_segscan_argument_errors():
    """Every packed-segment entry point checks its arguments in a fixed order and reports the first failure with a fixed
    text: the cases below are all decided on the host, before a launch."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn, kw, msg in _seg_cases():
        kw = dict(kw)
        all_null = kw.pop("all_null", False)
        args = []
        for a in _SEG[fn].split():
            if a in kw:
                args.append(kw[a])
            elif a in _SEG_SCALARS:
                args.append(_SEG_SCALARS[a])
            else:
                args.append(None if all_null or a == "stream" else P)
        lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
        rc = getattr(lib, fn)(*args)
        if msg is None:
            assert rc == 0, (fn, kw, rc, lib.nfa_last_error())
        else:
            assert rc == -1 and lib.nfa_last_error() == msg.encode(), (fn, kw, rc, lib.nfa_last_error())
