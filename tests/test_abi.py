"""CPU: the C-ABI library loads and exports exactly what include/nerfacc_hip.h declares."""
import os
import re

import pytest

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


def test_every_header_is_in_the_content_hash():
    """A header under csrc/ that `_deps()` leaves out would let a stale library survive an edit to it."""
    from nerfacc_amd import _build
    headers = {os.path.join(_build.CSRC, f) for f in os.listdir(_build.CSRC) if f.endswith(".h")}
    assert headers, "no headers found"
    deps = set(_build._deps())
    assert headers <= deps, sorted(headers - deps)
    assert {os.path.join(_build.CSRC, s) for s in _build.SOURCES} <= deps


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


# The traversal entry points (csrc/grid.hip, csrc/walk.hip): arguments in C order, and for each one its checks in the
# order in which they fire: (what is wrong, the error text), None = the call returns NFA_OK without a launch.  Names of
# nfa_traverse_args fields go into the struct when the entry point takes one.
_TRAV = {
    "nfa_traverse_grids": "args stream",
    "nfa_traverse_runs": "args bits run_cnts runs max_runs overflow_count near_hint ray_order n_order stream",
    "nfa_traverse_cone_walk": "args bits run_cnts runs max_runs overflow_count arena arena_capacity ray_order n_order stream",
    "nfa_traverse_cone_runs": "args run_cnts runs max_runs overflow_count ray_order n_order stream",
    "nfa_pack_walk_bits": "binaries n_grids res bits stream",
    "nfa_ray_events": "rays_o rays_d n_rays aabbs n_aabbs t_sorted t_indices hits stream",
    "nfa_expand_cone_arena": "arena n_entries step_size cone_angle packed_info t_starts t_ends ray_indices stream",
}
# arguments that are not (required) pointers, at values every check accepts
_TRAV_SCALARS = {"max_runs": 8, "near_hint": float("nan"), "ray_order": None, "n_order": 0, "arena_capacity": 0,
                 "n_grids": 1, "res": (8, 8, 8), "n_rays": 4, "n_aabbs": 1, "n_entries": 4, "step_size": 0.01, "cone_angle": 0.001}
# a struct every check of nfa_traverse_runs accepts (one grid, intersection in the kernel, count pass); steps_limit_dev is
# set so that nfa_traverse_runs makes no HIP call before its checks
_ARGS_BASE = dict(n_rays=4, rays_o=P, rays_d=P, n_grids=1, res=(8, 8, 8), binaries=P, aabbs=P, near_planes=P, far_planes=P,
                  step_size=0.01, cone_angle=0.0, traverse_steps_limit=0, mode=0, sm_cnts=P, steps_limit_dev=P)
_EVENTS = dict(hits=P, t_sorted=P, t_indices=P)
_HUGE = dict(res=(512, 512, 512), n_grids=16, **_EVENTS)   # 16 levels of 2^27 cells: 2^31 bits


def _nulls(names, msg, **kw):
    return [({n: None, **kw}, msg) for n in names.split()]


def _run_record_checks(nm, cone, mode_words, beyond, inputs, null_msg):
    """The checks nfa_traverse_runs, nfa_traverse_cone_walk and nfa_traverse_cone_runs have in common, in their order."""
    angle = "cone_angle > 0" if cone else "cone_angle == 0"
    return [
        ({"step_size": 0.0}, f"{nm}: needs step_size > 0 and {angle}"),
        ({"cone_angle": 0.0 if cone else 0.1}, f"{nm}: needs step_size > 0 and {angle}"),
        ({"mode": 1}, f"{nm}: mode must be 0 (all rays) or 2 ({mode_words})"),
        ({"mode": 2}, "traverse_steps_limit must be > 0 when over_allocate is true"),
        *_nulls(inputs + " run_cnts runs", null_msg),
        ({"max_runs": 0}, f"{nm}: max_runs must be in [1, 32]"),
        ({"max_runs": 33}, f"{nm}: max_runs must be in [1, 32]"),
        ({"n_grids": 0}, f"{nm}: bad grid shape"),
        ({"res": (8, 0, 8)}, f"{nm}: bad grid shape"),
        beyond,
        ({"hits": P}, f"{nm}: t_sorted, t_indices and hits must be given together"),
        ({"t_sorted": P, "t_indices": P}, f"{nm}: t_sorted, t_indices and hits must be given together"),
        ({"n_grids": 2, "hits": None, "t_sorted": None, "t_indices": None}, f"{nm}: in-kernel intersection supports one grid"),
    ]


def _order_checks(nm):
    return [
        ({"ray_order": P, "n_order": -1}, f"{nm}: n_order out of range"),
        ({"ray_order": P, "n_order": 5}, f"{nm}: n_order out of range"),
        ({"ray_order": P, "n_order": 0}, None),
    ]


_WALK_INPUTS = "rays_o rays_d aabbs near_planes far_planes sm_cnts bits"
_TRAV_CHECKS = {
    "nfa_traverse_grids": [
        ({"args": None}, "traverse_grids: null args"),
        ({"n_rays": -1}, "traverse_grids: n_rays out of range"),
        ({"n_rays": 1 << 31}, "traverse_grids: n_rays out of range"),
        ({"n_rays": 0}, None),
        ({"mode": 3}, "traverse_grids: mode must be 0, 1 or 2"),
        ({"mode": -1}, "traverse_grids: mode must be 0, 1 or 2"),
        *_nulls("rays_o rays_d binaries aabbs near_planes far_planes", "traverse_grids: null input pointer"),
        ({"n_grids": 0}, "traverse_grids: bad grid shape"),
        ({"res": (8, 8, 0)}, "traverse_grids: bad grid shape"),
        ({"res": (2048, 1024, 1024)}, "traverse_grids: grid level too large"),
        ({"hits": P}, "traverse_grids: t_sorted, t_indices and hits must be given together"),
        ({"n_grids": 2}, "traverse_grids: in-kernel intersection supports one grid; pass t_sorted/t_indices/hits"),
        ({"mode": 2}, "traverse_steps_limit must be > 0 when over_allocate is true"),
        ({"sm_cnts": None}, "traverse_grids: nothing to compute", "alone"),   # (the next case asks for intervals: that would heal it)
        ({"mode": 1, "iv_cnts": P}, "traverse_grids: interval outputs missing"),
        ({"mode": 1, "sm_starts": None}, "traverse_grids: sample starts missing"),
        ({"mode": 1, "sm_starts": P, "sm_t_starts": P}, "traverse_grids: direct emission needs sm_t_starts, sm_t_ends and no intervals"),
        ({"mode": 1, "sm_starts": P}, "traverse_grids: sample outputs missing"),
    ],
    "nfa_traverse_runs": [
        ({"args": None}, "traverse_runs: null args"),
        ({"n_rays": -1}, "traverse_runs: n_rays out of range"),
        ({"n_rays": 1 << 31}, "traverse_runs: n_rays out of range"),
        ({"overflow_count": None}, "traverse_runs: overflow_count is null"),
        ({"n_rays": 0}, None),
        *_run_record_checks("traverse_runs", False, "rays_mask + limit",
                            ({"res": (513, 8, 8)}, "traverse_runs: at most 512 cells per axis (use nfa_traverse_grids beyond)"),
                            _WALK_INPUTS, "traverse_runs: null pointer"),
        (_HUGE, "traverse_runs: grid too large"),
        *_order_checks("traverse_runs"),
    ],
    "nfa_traverse_cone_walk": [
        ({"args": None}, "traverse_cone_walk: null args"),
        ({"n_rays": -1}, "traverse_cone_walk: n_rays out of range"),
        ({"n_rays": 1 << 31}, "traverse_cone_walk: n_rays out of range"),
        ({"overflow_count": None}, "traverse_cone_walk: overflow_count is null"),
        # ---- from here on overflow_count has been cleared on the device
        ({"arena_capacity": -16}, "traverse_cone_walk: arena_capacity must be a multiple of 16"),
        ({"arena": P, "arena_capacity": 24}, "traverse_cone_walk: arena_capacity must be a multiple of 16"),
        ({"n_rays": 0}, None),
        *_run_record_checks("traverse_cone_walk", True, "rays_mask + traverse_steps_limit",
                            ({"res": (8, 8, 513)}, "traverse_cone_walk: at most 512 cells per axis (use nfa_traverse_cone_runs beyond)"),
                            _WALK_INPUTS, "traverse_cone_walk: null pointer (or interval outputs requested)"),
        ({"res": (2, 2, 2)}, "traverse_cone_walk: a level of the grid copy must be a whole number of 64-bit words (at least 4 cells per axis) "
                             "and the copy below 2^31 bits"),
        (_HUGE, "traverse_cone_walk: a level of the grid copy must be a whole number of 64-bit words (at least 4 cells per axis) "
                "and the copy below 2^31 bits"),
        *_order_checks("traverse_cone_walk"),
    ],
    "nfa_traverse_cone_runs": [
        ({"args": None}, "traverse_cone_runs: null args"),
        ({"n_rays": -1}, "traverse_cone_runs: n_rays out of range"),
        ({"n_rays": 1 << 31}, "traverse_cone_runs: n_rays out of range"),
        ({"overflow_count": None}, "traverse_cone_runs: overflow_count is null"),
        # ---- from here on overflow_count has been cleared on the device
        ({"n_rays": 0}, None),
        *_run_record_checks("traverse_cone_runs", True, "rays_mask + traverse_steps_limit",
                            ({"res": (2048, 1024, 1024)}, "traverse_cone_runs: grid level too large"),
                            "rays_o rays_d binaries aabbs near_planes far_planes sm_cnts",
                            "traverse_cone_runs: null pointer (or interval outputs requested)"),
        *_order_checks("traverse_cone_runs"),
    ],
    "nfa_pack_walk_bits": [
        *_nulls("binaries res bits", "pack_walk_bits: bad arguments"),
        ({"n_grids": 0}, "pack_walk_bits: bad arguments"),
        ({"res": (0, 8, 8)}, "pack_walk_bits: 1..512 cells per axis"),
        ({"res": (8, 513, 8)}, "pack_walk_bits: 1..512 cells per axis"),
        ({"res": (512, 512, 512), "n_grids": 16}, "pack_walk_bits: grid too large"),
    ],
    "nfa_ray_events": [
        ({"n_rays": -1}, "ray_events: 1..NFA_MAX_EVENT_LEVELS boxes"),
        ({"n_aabbs": 0}, "ray_events: 1..NFA_MAX_EVENT_LEVELS boxes"),
        ({"n_aabbs": 9}, "ray_events: 1..NFA_MAX_EVENT_LEVELS boxes"),
        ({"n_rays": 0}, None),
        *_nulls("rays_o rays_d aabbs t_sorted t_indices hits", "ray_events: null pointer"),
    ],
    "nfa_expand_cone_arena": [
        ({"n_entries": -1}, "expand_cone_arena: negative n_entries"),
        ({"n_entries": 0}, None),
        *_nulls("arena packed_info t_starts t_ends ray_indices", "expand_cone_arena: null pointer"),
        ({"step_size": 0.0}, "expand_cone_arena: step_size and cone_angle must be > 0"),
        ({"cone_angle": 0.0}, "expand_cone_arena: step_size and cone_angle must be > 0"),
    ],
}
# leading checks that are decided before the entry point makes its first HIP call (the others: all of them)
_TRAV_HOST_ONLY = {"nfa_traverse_cone_walk": 4, "nfa_traverse_cone_runs": 4}


# No case may get as far as a launch (the pointers are stand-ins).  Each case has something wrong with it, but two of them
# merged can heal each other, so whatever passes every check still ends without a launch: an empty ray list for the
# run-record entry points (their last early return), a fill pass without outputs for nfa_traverse_grids (its last checks).
_TRAV_LAST_RESORT = {fn: {"ray_order": P, "n_order": 0} for fn in ("nfa_traverse_runs", "nfa_traverse_cone_walk", "nfa_traverse_cone_runs")}


def _trav_args(fn):
    if fn == "nfa_traverse_grids":
        return {**_ARGS_BASE, "mode": 1}
    return {**_ARGS_BASE, "cone_angle": 0.0 if fn == "nfa_traverse_runs" else 0.001}


def _trav_call(lib, fn, kw, args_base, call_base):
    import ctypes as C
    from nerfacc_amd import _backend as B
    names = _TRAV[fn].split()
    takes_struct = names[0] == "args"
    fields = {f[0] for f in B.TraverseArgs._fields_}
    st = dict(args_base)
    call = dict(call_base)
    for k, v in kw.items():
        (st if takes_struct and k in fields else call)[k] = v
    a = B.TraverseArgs()
    for k, v in st.items():
        setattr(a, k, (C.c_int32 * 3)(*v) if k == "res" else v)
    args = []
    for n in names:
        if n == "args":
            args.append(C.byref(a) if call.get("args", 1) is not None else None)
        elif n in call:
            args.append(call[n])
        elif n in _TRAV_SCALARS:
            args.append(_TRAV_SCALARS[n])
        else:
            args.append(None if n == "stream" else P)
    if not takes_struct and "res" in names:
        i = names.index("res")
        args[i] = (C.c_int32 * 3)(*args[i]) if args[i] is not None else None
    lib.nfa_set_tuning(b"", None)  # leaves a known error text behind
    return getattr(lib, fn)(*args), lib.nfa_last_error()


def _trav_check(lib, fn, checks, first, last, args_over=None, call_base=None):
    """checks[first:last], each alone, and each together with the first later check of another outcome: the earlier one fires."""
    args_base = {**_trav_args(fn), **(args_over or {})}
    call_base = {**_TRAV_LAST_RESORT.get(fn, {}), **(call_base or {})}
    for i in range(first, last):
        kw, msg, *alone = checks[i]
        later = {} if alone else next((c[0] for c in checks[i + 1:] if c[1] != msg), {})
        for case in (kw, {**later, **kw}):
            rc, err = _trav_call(lib, fn, case, args_base, call_base)
            if msg is None:
                assert rc == 0, (fn, case, rc, err)
            else:
                assert rc == -1 and err == msg.encode(), (fn, case, rc, err, msg)


def test_traversal_argument_errors():
    """Every traversal entry point checks its arguments in a fixed order and reports the first failure with a fixed text.
    Here: the checks that are decided on the host before the entry point's first HIP call (nfa_traverse_cone_walk and
    nfa_traverse_cone_runs clear overflow_count on the device after their fourth; the rest of theirs is in the GPU test)."""
    from nerfacc_amd import _backend as B
    lib = B.load()
    for fn, checks in _TRAV_CHECKS.items():
        _trav_check(lib, fn, checks, 0, _TRAV_HOST_ONLY.get(fn, len(checks)))


@pytest.mark.gpu
def test_traversal_argument_errors_after_the_memset(dev):
    """The checks of the run-record entry points that follow the clearing of overflow_count (a real device buffer here:
    the stand-in address must not reach hipMemsetAsync), and which words of it each entry point clears."""
    import torch
    from nerfacc_amd import _backend as B
    lib = B.load()
    ovf = torch.empty(2, dtype=torch.int32, device=dev)
    for fn, cleared, args_over in (("nfa_traverse_cone_walk", [0, 0], None), ("nfa_traverse_cone_runs", [0, 7], None),
                                   ("nfa_traverse_runs", [0, 0], {"steps_limit_dev": None})):
        checks = _TRAV_CHECKS[fn]
        call_base = {"overflow_count": ovf.data_ptr()}
        _trav_check(lib, fn, checks, 0, len(checks), args_over, call_base)
        # the clearing comes before every check behind "overflow_count is null", the n_rays == 0 return included
        for kw in ({"n_rays": 0}, {"step_size": 0.0}, {"ray_order": P, "n_order": 0}):
            ovf.fill_(7)
            torch.cuda.synchronize()
            _trav_call(lib, fn, kw, {**_trav_args(fn), **(args_over or {})}, {**_TRAV_LAST_RESORT[fn], **call_base})
            torch.cuda.synchronize()
            assert ovf.tolist() == cleared, (fn, kw, ovf.tolist())
    # a device-driven call (steps_limit_dev set) leaves overflow_count to nfa_testmode_begin
    lim = torch.ones(1, dtype=torch.int32, device=dev)
    ovf.fill_(7)
    torch.cuda.synchronize()
    rc, err = _trav_call(lib, "nfa_traverse_runs", {"step_size": 0.0}, {**_ARGS_BASE, "steps_limit_dev": lim.data_ptr()},
                         {**_TRAV_LAST_RESORT["nfa_traverse_runs"], "overflow_count": ovf.data_ptr()})
    torch.cuda.synchronize()
    assert rc == -1 and err == b"traverse_runs: needs step_size > 0 and cone_angle == 0" and ovf.tolist() == [7, 7]
