"""GPU: every form of the grid traversal on exact scenes -- DDA ties, midpoints on a threshold, spans that start on the near plane.

The other traversal tests draw random float32 rays, on which two boundary distances of the cell walk are never equal and a
sample's midpoint never equals the distance it is compared with.  The rays of ``traversal_reference`` ride cell edges and
corners (a fifth of their cell steps are two-way ties, a twentieth three-way ties in the dyadic scenes), a fifth of them start
their span on the near plane, and with the directed near planes half of them put a midpoint exactly on a cell's exit
(test_traversal_exact_cpu.py asserts those shares on the same keys and checks the counting restatement against the C oracle).
The rays whose slab test forms 0 * inf are removed before anything reaches the device.

Every comparison is ``==`` with ``oracle.traverse_grids`` / ``oracle.occgrid_sampling`` / ``oracle.ray_aabb_intersect``: values,
``packed_info``, ``ray_indices``, ``is_left`` / ``is_right`` / ``is_valid`` and termination planes.  ``CallLog`` shows which native
entry ran and what it was given (the near-plane hint, the ray list).

What each form is compared on, summed over the two one-level scenes and the three steps, counted by the restatement (the
two- and three-level scenes add 4352 and 4288 rays per run whose finest level alone has 8720 and 8161 tie steps; their
midpoint events are not counted):

    form                                               planes                   ray traversals  tie steps  midpoint equalities
    ray_aabb_intersect, ray_events                     -                        17239 rays (all four scenes)
    traverse_grids constant, cone, over_allocate       zero, common, directed   77391           92396      50349
    traverse_grids per cell (step 0)                   zero, common, directed   25797           31335      -
    sampler, lattice walk                              zero, common             51594           56637      1097
    sampler, marcher / binned / mask + limit (each)    common, directed         51594           60761      50349
    sampler, off-lattice repeat                        common + 7 directed      25797           25002      1097
    sampler, cone walk / cone runs / serial (each)     zero, common, directed   77391           92396      50349
    OccGridEstimator.sampling                          common, t_min directed   51594           60761      50349

(With a step limit a ray stops early and meets fewer of its events.  Up to a distance of 4 a cone angle of 2^-8 leaves the step
at its minimum, so inside the finest box the cone forms march like the constant-step ones; beyond it, in the nested levels,
their step grows.)
"""
import math

import numpy as np
import pytest
import torch

import nerfacc_amd as na
import traversal_reference as TR
from nerfacc_amd import _backend as B

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(TR.SCENES)
CONE = 2.0 ** -8
_REF, _DEV = {}, {}


class CallLog:
    """Records every native call (name, arguments) while installed, as test_pdf_variants_gpu.CallLog does."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = B.call
        monkeypatch.setattr(B, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self):
        return [n for n, _ in self.calls]

    def of(self, name):
        return [a for n, a in self.calls if n == name]

    def clear(self):
        del self.calls[:]


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)     # (a copy: the helper's arrays are read-only)


def N(t):
    return t.detach().cpu().numpy()


def scene_on(dev, scene):
    """The scene's rays and grid on the device (made once)."""
    if scene not in _DEV:
        o, d, b, ab, _ = TR.case(scene)
        _DEV[scene] = (T(o, dev), T(d, dev), T(b, dev), T(ab, dev))
    return _DEV[scene]


def reference(oracle, scene, near, far, step, cone=0.0, limit=None, mask=None, key=None):
    """``oracle.traverse_grids`` (computed once per ``key``): (intervals, samples, termination planes)."""
    if key is None or key not in _REF:
        o, d, b, ab, _ = TR.case(scene)
        kw = dict(near_planes=near, far_planes=far, step_size=step, cone_angle=cone)
        if limit is not None:
            kw.update(traverse_steps_limit=limit, over_allocate=True, rays_mask=np.ones(o.shape[0], bool) if mask is None else mask)
        out = oracle.traverse_grids(o, d, b, ab, **kw)
        if key is None:
            return out
        _REF[key] = out
    return _REF[key]


def assert_samples(got, ref, what, masked=False):
    """The sampler's (ray_indices, t_starts, t_ends, packed_info, terminate planes) against the oracle's streams."""
    riv, rsm, rterm = ref
    keep = rsm["is_valid"] if masked else np.ones(rsm["ray_indices"].shape[0], bool)
    ri, ts, te, pi, term = (N(x) for x in got)
    assert np.array_equal(pi, rsm["packed_info"]), (what, "packed_info", int((pi != rsm["packed_info"]).any(-1).sum()))
    assert np.array_equal(ri, rsm["ray_indices"][keep]), (what, "ray_indices")
    assert np.array_equal(ts, riv["vals"][riv["is_left"]]), (what, "t_starts")
    assert np.array_equal(te, riv["vals"][riv["is_right"]]), (what, "t_ends")
    assert np.array_equal(term, rterm), (what, "terminate planes", int((term != rterm).sum()))


def assert_traversal(res, ref, what):
    """``na.traverse_grids``' three outputs against the oracle's, field by field."""
    iv, sm, term = res
    riv, rsm, rterm = ref
    assert np.array_equal(N(iv.packed_info), riv["packed_info"]), (what, "interval packed_info")
    assert np.array_equal(N(sm.packed_info), rsm["packed_info"]), (what, "sample packed_info")
    assert np.array_equal(N(iv.vals), riv["vals"]), (what, "interval vals")
    assert np.array_equal(N(iv.is_left), riv["is_left"]) and np.array_equal(N(iv.is_right), riv["is_right"]), (what, "is_left / is_right")
    assert np.array_equal(N(iv.ray_indices), riv["ray_indices"]), (what, "interval ray_indices")
    assert np.array_equal(N(sm.vals), rsm["vals"]), (what, "sample vals")
    assert np.array_equal(N(sm.ray_indices), rsm["ray_indices"]), (what, "sample ray_indices")
    assert np.array_equal(N(sm.is_valid), rsm["is_valid"]), (what, "is_valid")
    assert np.array_equal(N(term), rterm), (what, "terminate planes")


def mask_of(scene, share):
    o = TR.case(scene)[0]
    return TR.case_rng(3, SCENE_NAMES.index(scene), int(share * 100)).random(o.shape[0]) < share


# ----------------------------------------------------------------------------- a. intersection and events
@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_intersection_and_events(dev, oracle, monkeypatch, scene):
    o, d, b, ab, _ = TR.case(scene)
    to, td, _, tab = scene_on(dev, scene)
    log = CallLog(monkeypatch)
    # the family has what random rays never have: hits of length zero, origins on the face they leave through
    tmin, tmax, hit = oracle.ray_aabb_intersect(o, d, ab)
    grazing = hit & (tmin == tmax)
    leaving = (((o == 1) & (d > 0)) | ((o == -1) & (d < 0))).any(-1)
    assert grazing[:, 0].sum() >= 10 and leaving.sum() >= 100 and not hit[leaving, 0].any()
    for near, far, miss in ((-math.inf, math.inf, math.inf), (TR.NEAR_COMMON, TR.FAR_COMMON, -1.0), (0.0, 0.75, math.inf)):
        rmin, rmax, rhit = oracle.ray_aabb_intersect(o, d, ab, near, far, miss)
        gmin, gmax, ghit = na.ray_aabb_intersect(to, td, tab, near, far, miss)
        assert np.array_equal(N(ghit), rhit), (near, far, int((N(ghit) != rhit).sum()))
        assert np.array_equal(N(gmin), rmin) and np.array_equal(N(gmax), rmax), (near, far)
    assert log.names() == ["nfa_ray_aabb_intersect"] * 3
    log.clear()
    ts, ti, th = na.grid.ray_events(to, td, tab)
    assert log.names() == ["nfa_ray_events"]
    rs, rix = oracle.sort_intersections(tmin, tmax)
    assert np.array_equal(N(th), hit)
    assert np.array_equal(N(ts), rs), int((N(ts) != rs).any(-1).sum())
    assert np.array_equal(N(ti), rix), int((N(ti) != rix).any(-1).sum())       # equal distances keep their order (a stable sort)


# ----------------------------------------------------------------------------- b. the API: intervals + samples
@pytest.mark.parametrize("scene", SCENE_NAMES)
@pytest.mark.parametrize("form", ["constant", "cone", "per_cell", "over_allocate"])
def test_traverse_grids_api(dev, oracle, monkeypatch, scene, form):
    to, td, tb, tab = scene_on(dev, scene)
    log = CallLog(monkeypatch)
    n_samples = 0
    steps = {"per_cell": {"0": 0.0}}.get(form, TR.STEPS)
    for step_name, step in steps.items():
        for mode in ("zero", "common", "directed"):
            near, far = TR.planes(scene, "2^-6" if form == "per_cell" else step_name, mode)
            what = (scene, form, step_name, mode)
            log.clear()
            if form == "over_allocate":
                mask = mask_of(scene, 0.6)
                res = na.traverse_grids(to, td, tb, tab, T(near, dev), T(far, dev), step, 0.0, traverse_steps_limit=7,
                                        over_allocate=True, rays_mask=T(mask, dev))
                ref = reference(oracle, scene, near, far, step, limit=7, mask=mask, key=(scene, step_name, mode, "limit7"))
                assert log.names().count("nfa_traverse_grids") == 1 and "nfa_traverse_runs" not in log.names(), what
            else:
                cone = CONE if form == "cone" else 0.0
                planes = {} if mode == "zero" else dict(near_planes=T(near, dev), far_planes=T(far, dev))   # zero: the API's defaults
                res = na.traverse_grids(to, td, tb, tab, step_size=step, cone_angle=cone, **planes)
                ref = reference(oracle, scene, near, far, step, cone, key=(scene, step_name, mode, cone))
                if form == "constant":      # the run-length walk and its two expansions; the serial kernel only for rays with > MAX_RUNS runs
                    runs = log.of("nfa_traverse_runs")
                    assert len(runs) == 1 and "nfa_expand_runs" in log.names() and "nfa_expand_intervals" in log.names(), what
                    assert (runs[0][6] == 0.0) if mode == "zero" else math.isnan(runs[0][6]), what
                else:                       # grid.hip's traverse_kernel: a count and a fill launch
                    assert log.names().count("nfa_traverse_grids") == 2 and "nfa_traverse_runs" not in log.names(), what
            assert_traversal(res, ref, what)
            n_samples += int(res[1].vals.numel())
    assert n_samples > 10_000


# ----------------------------------------------------------------------------- c. the sampler's constant-step forms
@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_sampler_constant_step_forms(dev, oracle, monkeypatch, scene):
    to, td, tb, tab = scene_on(dev, scene)
    log = CallLog(monkeypatch)
    n = to.shape[0]
    assert n >= 4096

    def run(near, far, step, **kw):
        log.clear()
        return na.grid._traverse_samples(to, td, tb, tab, T(near, dev), T(far, dev), step, 0.0, return_terminate=True, **kw)

    for step_name, step in TR.STEPS.items():
        zero, common, directed = (TR.planes(scene, step_name, m) for m in ("zero", "common", "directed"))
        ref = {m: reference(oracle, scene, *TR.planes(scene, step_name, m), step, key=(scene, step_name, m, 0.0))
               for m in ("zero", "common", "directed")}
        # one near plane for the launch: the lattice walk, once
        for mode, hint, pl in (("zero", 0.0, zero), ("common", TR.NEAR_COMMON, common)):
            got = run(*pl, step, near_hint=hint)
            runs = log.of("nfa_traverse_runs")
            assert len(runs) == 1 and runs[0][6] == hint and runs[0][7] is None, (scene, step_name, mode, len(runs))
            assert_samples(got, ref[mode], (scene, step_name, mode, "lattice"))
        # per-ray near planes: the marcher
        got = run(*directed, step, near_hint=None)
        runs = log.of("nfa_traverse_runs")
        assert len(runs) == 1 and math.isnan(runs[0][6]), (scene, step_name)
        assert_samples(got, ref["directed"], (scene, step_name, "marcher"))
        got = run(*common, step, near_hint=None)
        assert_samples(got, ref["common"], (scene, step_name, "marcher, common planes"))
        # a hint that a handful of rays do not follow: the walk reports them and the traversal is repeated with the marcher
        near = common[0].copy()
        sampled = ref["directed"][1]["packed_info"][:, 1] > 0
        odd = np.flatnonzero(sampled & (directed[0] != np.float32(TR.NEAR_COMMON)))
        odd = odd[:: max(1, odd.size // 7)][:7]
        near[odd] = directed[0][odd]
        got = run(near, common[1], step, near_hint=TR.NEAR_COMMON)
        runs = log.of("nfa_traverse_runs")
        assert len(odd) >= 5 and len(runs) == 2 and runs[0][6] == TR.NEAR_COMMON and math.isnan(runs[1][6]), (scene, step_name, len(runs))
        assert_samples(got, reference(oracle, scene, near, common[1], step), (scene, step_name, "off-lattice repeat"))
        # the binned lane assignment
        for mode, hint, pl in (("common", TR.NEAR_COMMON, common), ("directed", None, directed)):
            got = run(*pl, step, near_hint=hint, bin_rays=True)
            assert "nfa_bin_rays" in log.names() and log.of("nfa_traverse_runs")[0][7] is not None, (scene, step_name, mode)
            assert_samples(got, ref[mode], (scene, step_name, mode, "binned"))
        # mask + step limit (the test-mode loop's call): all rays walked, or only the listed alive ones
        for share, limit in ((0.5, 5), (0.9, 9)):
            mask = mask_of(scene, share)
            n_alive = int(mask.sum())
            listed = n_alive < na.grid.ALIVE_LIST_FRACTION * n
            assert listed == (share == 0.5)
            for mode, hint, pl in (("common", TR.NEAR_COMMON, common), ("directed", None, directed)):
                got = run(*pl, step, near_hint=hint, rays_mask=T(mask, dev), traverse_steps_limit=limit, n_alive=n_alive)
                runs = log.of("nfa_traverse_runs")
                assert len(runs) == 1, (scene, step_name, mode, share)
                assert (runs[0][7] is not None and runs[0][8] == n_alive) if listed else runs[0][7] is None
                mref = reference(oracle, scene, *pl, step, limit=limit, mask=mask, key=(scene, step_name, mode, "mask", share, limit))
                assert_samples(got, mref, (scene, step_name, mode, "mask", share, limit), masked=True)


# ----------------------------------------------------------------------------- d. the sampler's cone-angle forms
@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_sampler_cone_angle_forms(dev, oracle, monkeypatch, scene):
    to, td, tb, tab = scene_on(dev, scene)
    log = CallLog(monkeypatch)
    saved = (na.grid.CONE_WALK, na.grid.CONE_RUNS)
    forms = {"walk": (True, True, "nfa_traverse_cone_walk"), "bricks": (False, True, "nfa_traverse_cone_runs"),
             "serial": (True, False, "nfa_traverse_grids")}
    try:
        for step_name, step in TR.STEPS.items():
            for mode, hint in (("common", TR.NEAR_COMMON), ("directed", None), ("zero", 0.0)):
                near, far = TR.planes(scene, step_name, mode)
                ref = reference(oracle, scene, near, far, step, CONE, key=(scene, step_name, mode, CONE))
                for form, (walk, runs, entry) in forms.items():
                    na.grid.CONE_WALK, na.grid.CONE_RUNS = walk, runs
                    log.clear()
                    got = na.grid._traverse_samples(to, td, tb, tab, T(near, dev), T(far, dev), step, CONE, return_terminate=True,
                                                    near_hint=hint)
                    names = log.names()
                    others = {e for _, _, e in forms.values()} - {entry}
                    assert names.count(entry) == (2 if form == "serial" else 1) and not others & set(names), (scene, form, names)
                    assert_samples(got, ref, (scene, step_name, mode, form))
                assert ref[1]["ray_indices"].size > 3_000
            # ... and with a step limit (the refilling kernels of both walks)
            mask = mask_of(scene, 0.6)
            near, far = TR.planes(scene, step_name, "directed")
            mref = reference(oracle, scene, near, far, step, CONE, limit=6, mask=mask, key=(scene, step_name, "directed", CONE, "limit6"))
            for form, (walk, runs, entry) in forms.items():
                na.grid.CONE_WALK, na.grid.CONE_RUNS = walk, runs
                log.clear()
                got = na.grid._traverse_samples(to, td, tb, tab, T(near, dev), T(far, dev), step, CONE, return_terminate=True,
                                                rays_mask=T(mask, dev), traverse_steps_limit=6)
                assert entry in log.names(), (scene, form, log.names())
                assert_samples(got, mref, (scene, step_name, form, "limit 6"), masked=True)
    finally:
        na.grid.CONE_WALK, na.grid.CONE_RUNS = saved


# ----------------------------------------------------------------------------- e. the estimator
@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_estimator_sampling(dev, oracle, monkeypatch, scene):
    o, d, b, ab, _ = TR.case(scene)
    to, td, tb, tab = scene_on(dev, scene)
    res, levels = TR.SCENES[scene]
    est = na.OccGridEstimator(roi_aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=list(res), levels=levels).to(dev)
    est.binaries = tb
    assert np.array_equal(N(est.aabbs), ab)
    log = CallLog(monkeypatch)
    for step_name, step in TR.STEPS.items():
        directed = TR.planes(scene, step_name, "directed")[0]
        for cone in (0.0, CONE):
            log.clear()
            ri, ts, te = est.sampling(to, td, near_plane=TR.NEAR_COMMON, far_plane=TR.FAR_COMMON, render_step_size=step, cone_angle=cone)
            assert ("nfa_traverse_runs" if cone == 0.0 else "nfa_traverse_cone_walk") in log.names()
            ori, ots, ote = oracle.occgrid_sampling(o, d, b, ab, near_plane=TR.NEAR_COMMON, far_plane=TR.FAR_COMMON,
                                                    render_step_size=step, cone_angle=cone)
            assert np.array_equal(N(ri), ori) and np.array_equal(N(ts), ots) and np.array_equal(N(te), ote), (scene, step_name, cone, "common")
            log.clear()
            ri, ts, te = est.sampling(to, td, t_min=T(directed, dev), render_step_size=step, cone_angle=cone)
            if cone == 0.0:         # the hint is the estimator's near plane, 0: the rays with a plane of their own force the repeat
                runs = log.of("nfa_traverse_runs")
                assert len(runs) == 2 and runs[0][6] == 0.0 and math.isnan(runs[1][6]), (scene, step_name, len(runs))
            ori, ots, ote = oracle.occgrid_sampling(o, d, b, ab, t_min=directed, render_step_size=step, cone_angle=cone)
            assert np.array_equal(N(ri), ori) and np.array_equal(N(ts), ots) and np.array_equal(N(te), ote), (scene, step_name, cone, "t_min")
            assert ori.size > 10_000
