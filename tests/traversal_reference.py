"""Exact scenes for the grid traversal: rays that ride cell edges and corners, samples whose midpoint sits on a threshold.

Test helper (no conftest, nothing of ``nerfacc_amd`` is imported).  Random float32 rays never make two of the DDA's three
boundary distances equal, never put a sample's midpoint ``t_last + dt / 2`` exactly on the distance it is compared with
by ``>=``, and never start a span on the near plane.  The rays of :func:`exact_rays` have dyadic origins and directions
on a grid with dyadic cells, so they do all of that all the time; :func:`directed_near_planes` then aims each ray's
sample lattice at one of its own cell exits.

:func:`traverse_ray` is a float32 scalar restatement of one ray of ``oracle/nerfacc_oracle.c:traverse_one_ray`` (one
level, constant step or the per-cell mode ``step_size == 0``; no cone angle, no sample limit): the same operations in the
same order, every intermediate rounded to float32.  Beside the samples it counts the events the tests are about
(:class:`Events`).  tests/test_traversal_exact_cpu.py checks it against the C oracle bit for bit and asserts the shares of
those events on the very inputs the GPU tests use (same keys).
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

F = np.float32
EPS = F(1e-6)          # setup_traversal's eps (nerfacc_oracle.c:147)
HALF = F(0.5)

DIR_VALUES = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, 2.0], np.float32)
ORG_VALUES = np.array([-1.5, -1.0, -0.5, -0.125, 0.0, 0.0625, 0.5, 1.0], np.float32)


def case_rng(*key):
    """The generator of a test case: the CPU checks and the GPU tests draw the same inputs from the same key."""
    return np.random.default_rng([11, *key])


def exact_rays(key, n) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(origins (n, 3), directions (n, 3), zero_times_inf (n,) bool)``: components of the directions from
    ``DIR_VALUES`` (not all zero, not normalised: 342 directions), of the origins from ``ORG_VALUES`` (512 origins), drawn
    with the generator of ``key``.  ``zero_times_inf`` marks the rays with a zero direction component whose origin lies
    exactly on that axis' plane of the base box [-1, 1]^3: the reference's slab test forms 0 * inf = NaN for them; they are
    out of scope and must be removed before a comparison."""
    rng = case_rng(*key)
    dirs = np.stack(np.meshgrid(DIR_VALUES, DIR_VALUES, DIR_VALUES, indexing="ij"), -1).reshape(-1, 3)
    dirs = dirs[(dirs != 0).any(-1)]
    orgs = np.stack(np.meshgrid(ORG_VALUES, ORG_VALUES, ORG_VALUES, indexing="ij"), -1).reshape(-1, 3)
    assert dirs.shape[0] == 342 and orgs.shape[0] == 512
    d = np.ascontiguousarray(dirs[rng.integers(0, dirs.shape[0], n)])
    o = np.ascontiguousarray(orgs[rng.integers(0, orgs.shape[0], n)])
    zero_times_inf = ((d == 0) & (np.abs(o) == 1)).any(-1)
    return o, d, zero_times_inf


def exact_scene(key, res, levels=1, occ=0.5) -> Tuple[np.ndarray, np.ndarray]:
    """``(binaries (levels, *res) bool, aabbs (levels, 6) float32)``: random cells of share ``occ``, nested boxes +-2^i."""
    rng = case_rng(*key)
    res = (res,) * 3 if np.isscalar(res) else tuple(res)
    binaries = rng.random((levels, *res)) < occ
    aabbs = np.stack([np.concatenate([-(2.0 ** i) * np.ones(3), (2.0 ** i) * np.ones(3)]) for i in range(levels)])
    return binaries, aabbs.astype(np.float32)


@dataclass
class Events:
    cell_steps: int = 0        # executions of single_traversal's axis choice (nerfacc_oracle.c:257)
    ties2: int = 0             # ... at which exactly two of the three boundary distances share the minimum
    ties3: int = 0             # ... at which all three are equal
    mid_eq_occ: int = 0        # t_last + dt / 2 == t_traverse in the occupied-cell loop (:218)
    mid_eq_skip: int = 0       # t_last + dt / 2 == t_traverse when fast-forwarding over an empty cell (:132 from :209)
    mid_eq_span: int = 0       # t_last + dt / 2 == this_tmin when fast-forwarding to the span (:132 from :180)
    next_eq: int = 0           # t_next == t_traverse (:253)
    starts_on_near: int = 0    # the first sample starts on the near plane (no whole step was skipped before it)
    n_intervals: int = 0       # interval edges: a sample that continues the previous one adds one, any other two (:222-241)
    occupied_exits: List[float] = field(default_factory=list)   # t_traverse of every occupied cell visited

    @property
    def mid_eq_cell(self):
        """midpoint equalities with a cell's exit distance"""
        return self.mid_eq_occ + self.mid_eq_skip

    @property
    def mid_eq(self):
        return self.mid_eq_occ + self.mid_eq_skip + self.mid_eq_span


def _slab(o, d, inv, bmin, bmax):
    """nerfacc_oracle.c:61-80 with near = -inf, far = inf (what traverse_grids' preamble asks for)."""
    def axis(a):
        if inv[a] >= 0:
            return (bmin[a] - o[a]) * inv[a], (bmax[a] - o[a]) * inv[a]
        return (bmax[a] - o[a]) * inv[a], (bmin[a] - o[a]) * inv[a]
    tmin, tmax = axis(0)
    for a in (1, 2):
        lo, hi = axis(a)
        if tmin > hi or lo > tmax:
            return False, F(0), F(0)
        if lo > tmin:
            tmin = lo
        if hi < tmax:
            tmax = hi
    if tmax <= 0:
        return False, F(0), F(0)
    return True, tmin, tmax


def _fast_forward(t_last, target, step, ev, kind, strict=False):
    """nerfacc_oracle.c:127-138 with a constant step."""
    if step <= 0:
        return target
    half = step * HALF
    while True:
        mid = t_last + half
        if (mid > target) if strict else (mid >= target):
            if mid == target:
                setattr(ev, kind, getattr(ev, kind) + 1)
            return t_last
        t_new = t_last + step
        if t_new == t_last:
            return target
        t_last = t_new


VARIANTS = (None, "ties_x_first", "mid_strict")


def traverse_ray(o, d, binaries, aabb, near=0.0, far=np.inf, step_size=2.0 ** -6, variant=None):
    """One ray through one level: ``(samples [(t_start, t_end)], terminate_plane, Events)``.  ``binaries`` (rx, ry, rz) bool,
    ``aabb`` (6,).  Restates nerfacc_oracle.c:140-267 (``traverse_one_ray``) line by line in float32.

    ``variant``: a plausible WRONG rule instead of the reference's, to show that the exact scenes tell them apart (random rays
    do not): ``ties_x_first`` steps the lowest axis among equal boundary distances (the reference: z over y over x, :257),
    ``mid_strict`` ends a march at ``t_mid > threshold`` instead of ``>=`` (:132, :218)."""
    assert variant in VARIANTS
    with np.errstate(all="ignore"):
        return _traverse_ray(np.asarray(o, F), np.asarray(d, F), binaries, np.asarray(aabb, F), F(near), F(far), F(step_size), variant)


def _traverse_ray(o, d, binaries, aabb, near, far, step, variant=None):
    ev = Events()
    samples = []
    res = binaries.shape
    bmin, bmax = aabb[:3], aabb[3:]
    one = F(1)
    inv = [one / d[a] for a in range(3)]
    t_last = near
    hit, tmin, tmax = _slab(o, d, inv, bmin, bmax)
    if not hit:
        return samples, t_last, ev
    this_tmin = max(tmin, near)
    this_tmax = min(tmax, far)
    if this_tmin >= this_tmax:
        return samples, t_last, ev
    strict = variant == "mid_strict"
    t_last = _fast_forward(t_last, this_tmin, step, ev, "mid_eq_span", strict)
    on_near = t_last == near

    tdist, delta, stp, cur, overflow = [None] * 3, [None] * 3, [0] * 3, [0] * 3, [0] * 3
    for a in range(3):
        resf = F(res[a])
        voxel = (bmax[a] - bmin[a]) / resf
        ray_start = o[a] + d[a] * (this_tmin + EPS)
        ray_end = o[a] + d[a] * (this_tmax - EPS)
        cur[a] = min(max(int(((ray_start - bmin[a]) / (bmax[a] - bmin[a])) * resf), 0), res[a] - 1)
        fin = min(max(int(((ray_end - bmin[a]) / (bmax[a] - bmin[a])) * resf), 0), res[a] - 1)
        start_index = cur[a] + (1 if d[a] > 0 else 0)
        tmax_a = ((bmin[a] + ((F(start_index) * voxel) - ray_start)) * inv[a]) + this_tmin
        step_f = F(0) if d[a] == 0 else (F(1) if d[a] > 0 else F(-1))
        tdist[a] = this_tmax if d[a] == 0 else tmax_a
        stp[a] = int(step_f)
        delta[a] = this_tmax if d[a] == 0 else voxel * inv[a] * step_f
        overflow[a] = fin + stp[a]

    continuous = False
    half = step * HALF
    cells_left = res[0] + res[1] + res[2] + 3
    while True:
        t_traverse = min(min(tdist[0], min(tdist[1], tdist[2])), this_tmax)
        if not binaries[cur[0], cur[1], cur[2]]:
            t_last = _fast_forward(t_last, t_traverse, step, ev, "mid_eq_skip", strict)
            continuous = False
        else:
            ev.occupied_exits.append(float(t_traverse))
            while True:
                if step <= 0:
                    t_next = t_traverse
                else:
                    mid = t_last + half
                    if mid == t_traverse:
                        ev.mid_eq_occ += 1
                    if (mid > t_traverse) if strict else (mid >= t_traverse):
                        break
                    t_next = t_last + step
                    if t_next == t_last:
                        break
                if not samples and on_near and t_last == near:
                    ev.starts_on_near += 1
                samples.append((t_last, t_next))
                ev.n_intervals += 1 if continuous else 2
                continuous = True
                t_last = t_next
                if t_next == t_traverse:
                    ev.next_eq += 1
                if t_next >= t_traverse:
                    break
        # single_traversal (:257)
        if variant == "ties_x_first":
            a = 0 if (tdist[0] <= tdist[1] and tdist[0] <= tdist[2]) else (1 if tdist[1] <= tdist[2] else 2)
        else:
            a = 0 if (tdist[0] < tdist[1] and tdist[0] < tdist[2]) else (1 if tdist[1] < tdist[2] else 2)
        ev.cell_steps += 1
        m = min(tdist)
        n_min = sum(1 for t in tdist if t == m)
        ev.ties2 += n_min == 2
        ev.ties3 += n_min == 3
        cur[a] += stp[a]
        tdist[a] = tdist[a] + delta[a]
        if cur[a] == overflow[a]:
            break
        cells_left -= 1
        if cells_left <= 0:
            break
    return samples, t_last, ev


def traverse_rays(o, d, binaries, aabb, near=None, far=None, step_size=2.0 ** -6, variant=None):
    """:func:`traverse_ray` over a batch (one level): ``(ray_indices, t_starts, t_ends, terminate_planes, [Events])``."""
    n = o.shape[0]
    near = np.zeros(n, F) if near is None else np.broadcast_to(np.asarray(near, F), (n,))
    far = np.full(n, np.inf, F) if far is None else np.broadcast_to(np.asarray(far, F), (n,))
    ri, ts, te, term, evs = [], [], [], np.empty(n, F), []
    for r in range(n):
        s, term[r], ev = traverse_ray(o[r], d[r], binaries, aabb, near[r], far[r], step_size, variant)
        ri += [r] * len(s)
        ts += [a for a, _ in s]
        te += [b for _, b in s]
        evs.append(ev)
    return np.asarray(ri, np.int64), np.asarray(ts, F), np.asarray(te, F), term, evs


def directed_near_planes(o, d, binaries, aabb, step_size) -> np.ndarray:
    """Per-ray near planes that put a sample's midpoint exactly on one of the ray's own cell exits: with ``tt`` the exit
    distance of the ray's second occupied cell (its first when there is only one; from the restatement's cell walk with a
    near plane of 0), the plane is ``fl(tt - dt / 2)`` walked back by whole steps while it stays >= 0.  For a dyadic step
    the walk back and the march forward are exact, so the march from the plane stands on ``tt - dt / 2`` again; for other
    steps it may.  Rays without an occupied cell keep 0.  (Rays that start inside the box take the plane as their span
    start, which moves their cell exits by an ulp or so: what equalities remain is measured, not assumed.)"""
    step = F(step_size)
    near = np.zeros(o.shape[0], F)
    for r in range(o.shape[0]):
        _, _, ev = traverse_ray(o[r], d[r], binaries, aabb, 0.0, np.inf, 0.0)     # per-cell mode: the cell walk alone
        if not ev.occupied_exits:
            continue
        tt = F(ev.occupied_exits[min(1, len(ev.occupied_exits) - 1)])
        t = tt - step * HALF
        if not (t >= 0):
            continue
        while t - step >= 0:
            t = t - step
        near[r] = t
    return near


# ----------------------------------------------------------------------------- the cases of the CPU checks and the GPU tests
N_RAYS = 4800                     # drawn per scene; about 10 % are 0 * inf rays, and the binned walk wants 4096 kept ones
SCENES = {                        # name: (resolution, levels)
    "16": ((16, 16, 16), 1),
    "16x2": ((16, 16, 16), 2),
    "16x8x32x3": ((16, 8, 32), 3),     # unequal index bits per axis: the irregular cell layout of the walk
    "12": ((12, 12, 12), 1),          # a voxel of 1/6: not dyadic, ties come from symmetric rays only
}
STEPS = {                         # name: step
    "2^-6": 2.0 ** -6,
    "3*2^-8": 3 * 2.0 ** -8,
    "2^-6+2^-25": 2.0 ** -6 + 2.0 ** -25,   # k + 1/2 ulps in [0.5, 1): no stable increment in that binade
}
NEAR_COMMON, FAR_COMMON = 2.0 ** -7, 1.25
PLANE_MODES = ("zero", "common", "directed", "directed_far")
_CASES, _PLANES, _EVENTS = {}, {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def case(scene):
    """``(origins, directions, binaries, aabbs, share of 0 * inf rays)`` of a scene of ``SCENES``, the 0 * inf rays removed.
    Computed once; the arrays are read-only."""
    if scene not in _CASES:
        idx = list(SCENES).index(scene)
        res, levels = SCENES[scene]
        o, d, bad = exact_rays((1, idx), N_RAYS)
        b, ab = exact_scene((2, idx), res, levels, 0.5)
        _CASES[scene] = (_frozen(o[~bad]), _frozen(d[~bad]), _frozen(b), _frozen(ab), float(bad.mean()))
    return _CASES[scene]


def planes(scene, step_name, mode):
    """``(near_planes, far_planes)`` float32 per kept ray: ``zero`` (0, inf), ``common`` (2^-7, 1.25), ``directed``
    (:func:`directed_near_planes` on the scene's finest level, inf), ``directed_far`` (the same, 1.25)."""
    key = (scene, step_name, mode)
    if key not in _PLANES:
        o, d, b, ab, _ = case(scene)
        n = o.shape[0]
        if mode in ("directed", "directed_far"):
            dkey = (scene, step_name, "directed")
            if dkey not in _PLANES:
                _PLANES[dkey] = (_frozen(directed_near_planes(o, d, b[0], ab[0], STEPS[step_name])), _frozen(np.full(n, np.inf, F)))
            near = _PLANES[dkey][0]
            far = np.full(n, np.inf if mode == "directed" else FAR_COMMON, F)
        elif mode == "common":
            near, far = np.full(n, NEAR_COMMON, F), np.full(n, FAR_COMMON, F)
        else:
            assert mode == "zero"
            near, far = np.zeros(n, F), np.full(n, np.inf, F)
        _PLANES[key] = (_frozen(near), _frozen(far))
    return _PLANES[key]


def restated(scene, step_name, mode):
    """:func:`traverse_rays` of a one-level scene with the planes of ``mode``, computed once."""
    key = (scene, step_name, mode)
    if key not in _EVENTS:
        o, d, b, ab, _ = case(scene)
        assert b.shape[0] == 1
        near, far = planes(scene, step_name, mode)
        _EVENTS[key] = traverse_rays(o, d, b[0], ab[0], near, far, STEPS[step_name])
    return _EVENTS[key]


def totals(evs) -> dict:
    """Sums and ray counts over a batch's events."""
    return dict(
        rays=len(evs),
        cell_steps=sum(e.cell_steps for e in evs), ties2=sum(e.ties2 for e in evs), ties3=sum(e.ties3 for e in evs),
        mid_eq_occ=sum(e.mid_eq_occ for e in evs), mid_eq_skip=sum(e.mid_eq_skip for e in evs),
        mid_eq_span=sum(e.mid_eq_span for e in evs), next_eq=sum(e.next_eq for e in evs),
        starts_on_near=sum(e.starts_on_near for e in evs),
        rays_mid_eq_cell=sum(e.mid_eq_cell > 0 for e in evs), rays_mid_eq=sum(e.mid_eq > 0 for e in evs))
