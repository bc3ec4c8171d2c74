"""Inputs of the test-mode loop's boundary tests (tests/test_testmode_cpu.py, tests/test_testmode_gpu.py), in numpy, with
the matching torch callbacks.

The exact field: ``sigma = SIGMA_OPAQUE`` for the rays with ``ri % mod != 0``, else ``keep_sigma`` (default 0);
``rgb = (0.25, 0.25 * (ri % 4), 0.5)``.  With ``sigma * dt >= 60`` the alpha of an opaque sample is exactly ``1.0f``
(``expf(-60) < 2^-25``), so every opacity is exactly 0 or 1: no ray comes near the early-termination threshold, and the
sample count and the schedule of any correct loop EQUAL the oracle's.  Every value is exact in fp16 and bf16.

Scenes (background (0.2, 0.4, 0.6), near plane 0.05, early_stop_eps 1e-3, level-0 box [-1, 1]^3):

* ``full``     an all-occupied 16^3 grid, step 0.05, rays from inside.  With ``mod = 1`` every ray is transparent and uses its
               whole budget, so ``n_alive * n_samples == n_rays`` whenever ``n_alive`` divides ``n_rays``: the padded loop's
               sample arrays are full to the last slot.  With ``mod = 3`` and ``max_samples = 6`` the schedule overshoots
               ``max_samples`` as the reference's ``while`` does.
* ``checker``  a 256^3 checkerboard, step one cell: rays that cross the box meet a new run every other cell, more than
               MAX_RUNS (32) of them within 64 steps -- the fill pass of the traversal, in two successive iterations (the
               second from termination planes that are no longer the initial near plane).  The rays that live that long are
               the transparent ones, whose samples weigh nothing: ``checker(0.5)`` gives them a small density, so that the
               depth image depends on every sample position the fill pass writes (no ray comes near an opacity of 1).
* ``multi``    two nested 48^3 levels at 25 % occupancy and 2 * 8192 + 77 rays: the alive list is built by three
               workgroups in the first iteration and by one later on.
* ``miss``     rays that never meet the box.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

SIGMA_OPAQUE = 16384.0
MAX_RUNS = 32                  # nerfacc_amd.grid.MAX_RUNS' default (asserted by the GPU tests)
ALIVE_PER_WG = 8192            # rays per workgroup of nfa_alive_rays (csrc/traverse2.hip)
BKGD = np.array([0.2, 0.4, 0.6], np.float32)
NEAR_PLANE, FAR_PLANE, EARLY_STOP_EPS = 0.05, 1e10, 1e-3
FULL_SIZES = (1, 3, 5, 96, 128)
FULL_SETTINGS = ((1, 600), (3, 6))          # (mod, max_samples)
MULTI_RAYS = 2 * ALIVE_PER_WG + 77


@dataclass(frozen=True, eq=False)
class Scene:
    name: str
    rays_o: np.ndarray
    rays_d: np.ndarray
    binaries: np.ndarray       # (levels, res, res, res) bool
    step: float
    mod: int
    max_samples: int
    keep_sigma: float = 0.0
    aabbs: np.ndarray = field(init=False)

    def __post_init__(self):
        levels = self.binaries.shape[0]
        ab = np.stack([np.concatenate([-(2.0 ** i) * np.ones(3), (2.0 ** i) * np.ones(3)]) for i in range(levels)])
        object.__setattr__(self, "aabbs", ab.astype(np.float32))
        assert SIGMA_OPAQUE * self.step >= 60.0    # alpha == 1.0f exactly

    @property
    def n_rays(self) -> int:
        return self.rays_o.shape[0]

    @property
    def resolution(self) -> int:
        return self.binaries.shape[1]

    @property
    def levels(self) -> int:
        return self.binaries.shape[0]


def _unit(rng, n):
    d = rng.standard_normal((n, 3)).astype(np.float32)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def full(n_rays: int, mod: int, max_samples: int) -> Scene:
    rng = np.random.default_rng(1)
    o = rng.random((n_rays, 3)).astype(np.float32) - np.float32(0.5)
    d = _unit(rng, n_rays)
    return Scene(f"full-{n_rays}-{mod}", o, d, np.ones((1, 16, 16, 16), bool), 0.05, mod, max_samples)


@functools.lru_cache(maxsize=None)
def checker(keep_sigma: float = 0.0) -> Scene:
    rng = np.random.default_rng(2)
    n, res = 2100, 256
    d = _unit(rng, n)
    o = np.float32(-1.6) * d + (rng.random((n, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(0.3)
    i = np.arange(res)
    b = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0)[None]
    return Scene(f"checker-{keep_sigma:g}", o.astype(np.float32), d, b, 2.0 / res, 70, 600, float(keep_sigma))


@functools.lru_cache(maxsize=None)
def multi(keep_sigma: float = 0.0) -> Scene:
    rng = np.random.default_rng(3)
    o = (rng.random((MULTI_RAYS, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(3.0)
    d = _unit(rng, MULTI_RAYS)
    b = np.random.default_rng(4).random((2, 48, 48, 48)) < 0.25
    return Scene(f"multi-{keep_sigma:g}", o, d, b, 6e-3, 3, 600, float(keep_sigma))


@functools.lru_cache(maxsize=None)
def miss() -> Scene:
    base = full(200, 3, 600)
    return Scene("miss", base.rays_o + np.float32(10.0), np.abs(base.rays_d), base.binaries, base.step, 3, 600)


def all_scenes():
    """Every scene of the loop tests with opacities that are exactly 0 or 1."""
    out = [full(n, mod, ms) for n in FULL_SIZES for mod, ms in FULL_SETTINGS]
    return out + [checker(), multi(), miss()]


# ----------------------------------------------------------------------------- the exact field
def field_np(scene: Scene):
    mod, keep = int(scene.mod), np.float32(scene.keep_sigma)

    def fn(ts, te, ri):
        ri = np.asarray(ri)
        sig = np.where(ri % mod != 0, np.float32(SIGMA_OPAQUE), keep).astype(np.float32)
        rgbs = np.stack([np.full(ri.shape, 0.25, np.float32), np.float32(0.25) * (ri % 4).astype(np.float32),
                         np.full(ri.shape, 0.5, np.float32)], -1)
        return rgbs, sig
    return fn


def field_torch(scene: Scene):
    """Elementwise in the samples and free of host synchronisation (the padded loop's contract)."""
    mod, keep = int(scene.mod), float(scene.keep_sigma)

    def fn(ts, te, ri):
        sig = torch.where(ri % mod != 0, torch.full_like(ts, SIGMA_OPAQUE), torch.full_like(ts, keep))
        rgbs = torch.stack([torch.full_like(ts, 0.25), 0.25 * (ri % 4).to(ts.dtype), torch.full_like(ts, 0.5)], -1)
        return rgbs, sig
    return fn


# ----------------------------------------------------------------------------- the oracle's run, with a trace
def count_long_run_rays(ts, te, ri, step, max_runs=MAX_RUNS) -> int:
    """Rays of one iteration with more than ``max_runs`` run records.  A run is broken where the gap to the ray's previous
    sample exceeds half a step (the walk also breaks runs where the increment's rounding changes: this can only undercount)."""
    if len(ri) == 0:
        return 0
    new_ray = np.ones(len(ri), bool)
    new_ray[1:] = ri[1:] != ri[:-1]
    gap = np.zeros(len(ri), bool)
    gap[1:] = (ts[1:] - te[:-1]) > 0.5 * step
    runs = np.bincount(ri, weights=(new_ray | gap).astype(np.float64))
    return int((runs > max_runs).sum())


@functools.lru_cache(maxsize=None)
def _reference(scene: Scene, alpha_thre: float, guard: float):
    from oracle import oracle as O
    O.build()
    fn = field_np(scene)
    trace = []          # per iteration that produced samples: (samples, rays with more than MAX_RUNS runs, alive rays)
    n, exact = scene.n_rays, scene.keep_sigma == 0.0
    alive = [n]         # alive rays at the start of the iteration (exact field: a ray lives on iff it is transparent and used
                        # its whole budget; an iteration without samples ends the loop, so every iteration before it is seen here)

    def recording(ts, te, ri):
        trace.append((len(ri), count_long_run_rays(ts, te, ri, scene.step), alive[0] if exact else None))
        if exact:
            ns = max(min(n // alive[0], 64), 1)
            alive[0] = int(((np.bincount(ri, minlength=n) == ns) & (np.arange(n) % scene.mod == 0)).sum())
        return fn(ts, te, ri)

    rgb, opa, dep, total, info = O.test_mode_loop(
        scene.max_samples, recording, scene.rays_o, scene.rays_d, scene.binaries, scene.aabbs, NEAR_PLANE, FAR_PLANE, scene.step,
        BKGD, 0.0, alpha_thre, EARLY_STOP_EPS, guard=guard)
    for a in (rgb, opa, dep):
        a.setflags(write=False)
    return rgb, opa, dep, int(total), dict(info, trace=tuple(trace))


def reference(scene: Scene, alpha_thre: float = 0.0, guard: float = 1e-5):
    """``oracle.test_mode_loop`` on the scene, computed once and shared (read-only): ``(rgb, opacity, depth, total, info)``
    with ``info["trace"]``: ``(samples, rays with more than MAX_RUNS runs, alive rays at its start -- exact field only)`` of
    every iteration that produced samples."""
    return _reference(scene, float(alpha_thre), float(guard))
