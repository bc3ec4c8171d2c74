"""GPU: the test-mode loop's bookkeeping kernels (nfa_alive_rays, nfa_testmode_begin, nfa_testmode_alive:
csrc/traverse2.hip) against plain numpy / Python -- integers and comparisons, so every comparison is exact -- and the four
forms of the loop (nerfacc_amd/marching.py: two host reads per iteration, one read, the padded loop with and without a
hipGraph) on the boundary scenes of tests/testmode_scenes.py: bit-identical to each other, the oracle's sample count,
iteration count and opacities, its colours and depths within the tolerances of test_test_mode_marching_loop.

What the scenes reach that the random 25 % grids of tests/test_gpu_parity.py do not (asserted on the oracle alone in
tests/test_testmode_cpu.py): iterations whose samples fill the padded loop's arrays to the last slot, fewer than 64 and fewer
than 4 rays, an exhausted ``max_samples``, rays with more than MAX_RUNS run records (the padded loop's fill pass, which reads
its own copy of the near planes), an alive list built by three workgroups, iterations without any sample, and callbacks that
return fp16, bf16 or non-contiguous float32.
"""
import numpy as np
import pytest
import torch

import nerfacc_amd as na
import nerfacc_amd.marching as marching
import testmode_scenes as S
from conftest import assert_close
from nerfacc_amd import _backend as B
from nerfacc_amd import grid as G
from nerfacc_amd.marching import PaddedTestModeLoop, render_rays_test_mode

pytestmark = pytest.mark.gpu

THRE = np.float32(1 - 1e-3)                     # opacity_max of the loop tests (early_stop_eps 1e-3)
ABOVE = np.nextafter(THRE, np.float32(2))
WG = S.ALIVE_PER_WG


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------- nfa_alive_rays / nfa_testmode_alive
N_SAMPLES = 5
ALIVE_SIZES = (1, 7, 64, WG - 1, WG, WG + 1, 3 * WG + 5)


def alive_case(n, kind, seed):
    """opacity from {0, thre, the float above thre, 1}: ``<=`` is met from both sides; samples taken from {n_samples,
    n_samples - 1, 0}; packed_info is a consistent (exclusive start, count) table."""
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        opacity = rng.choice(np.array([0, THRE, ABOVE, 1], np.float32), n)
        cnt = rng.choice(np.array([N_SAMPLES, N_SAMPLES - 1, 0], np.int64), n)
    elif kind == "alive":
        opacity = rng.choice(np.array([0, THRE], np.float32), n)
        cnt = np.full(n, N_SAMPLES, np.int64)
    else:
        opacity = rng.choice(np.array([ABOVE, 1], np.float32), n)
        cnt = rng.choice(np.array([N_SAMPLES, N_SAMPLES - 1, 0], np.int64), n)
        cnt[::2], opacity[::2] = N_SAMPLES - 1, 0        # ... and rays that are transparent but stopped early
    packed = np.stack([np.cumsum(cnt) - cnt, cnt], -1)
    want = (opacity <= THRE) & (cnt == N_SAMPLES)
    return opacity, packed, want


def alive_buffers(n, dev):
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)                # (a value the kernel never writes)
    alive = torch.full((n + 8,), -1, dtype=torch.int32, device=dev)
    return mask, alive


def check_alive(n, want, mask, alive, count):
    mask, alive = mask.cpu().numpy(), alive.cpu().numpy()
    assert np.array_equal(mask, want.astype(np.uint8))
    assert count == int(want.sum())
    listed = alive[:count]
    assert np.array_equal(np.sort(listed), np.nonzero(want)[0])
    assert (alive[count:] == -1).all()
    # the header's promise: a workgroup's stretch of ray ids is appended as one ascending block
    stretch = listed // WG
    same = stretch[1:] == stretch[:-1]
    assert (np.diff(listed)[same] > 0).all()
    assert int((~same).sum()) == max(len(np.unique(stretch)) - 1, 0)


@pytest.mark.parametrize("kind", ["mixed", "alive", "dead"])
@pytest.mark.parametrize("n", ALIVE_SIZES)
def test_alive_rays(dev, n, kind):
    opacity, packed, want = alive_case(n, kind, 100 + n)
    if kind == "mixed" and n >= 64:
        assert ((opacity == THRE) & want).any() and (opacity == ABOVE).any() and 0 < want.sum() < n
    if kind == "alive":
        assert want.all()
    if kind == "dead":
        assert not want.any()
    t_op, t_pi = T(opacity, dev), T(packed, dev)
    mask, alive = alive_buffers(n, dev)
    count = torch.full((1,), 12345, dtype=torch.int64, device=dev)
    B.call("nfa_alive_rays", B.ptr(t_op), B.ptr(t_pi), N_SAMPLES, float(THRE), n, B.ptr(mask), B.ptr(alive), B.ptr(count), B.stream())
    check_alive(n, want, mask, alive, int(count.item()))


def call_testmode_alive(dev, opacity, packed, state, count_samples, count0=0):
    n = opacity.shape[0]
    t_op, t_pi = T(opacity, dev), T(packed, dev)
    mask, alive = alive_buffers(n, dev)
    t_state = T(np.asarray(state, np.int32), dev)
    count = torch.tensor([count0, 4242], dtype=torch.int64, device=dev)      # [1] belongs to nfa_testmode_begin
    B.call("nfa_testmode_alive", B.ptr(t_op), B.ptr(t_pi), B.ptr(t_state), float(THRE), n, B.ptr(mask), B.ptr(alive), B.ptr(count),
           int(count_samples), B.stream())
    return mask, alive, count.cpu().numpy(), t_state.cpu().numpy()


def state_words(n_samples, counted):
    """state[0] the step limit, [1..3] and [6..7] sentinels, [4..5] the int64 sample counter."""
    st = np.array([n_samples, 301, 302, 303, 0, 0, 306, 307], np.int32)
    st[4:6] = np.array([counted], np.int64).view(np.int32)
    return st


@pytest.mark.parametrize("n", ALIVE_SIZES)
def test_testmode_alive_equals_alive_rays(dev, n):
    """nfa_alive_rays with n_samples = state[0]; with count_samples the int64 in state[4..5] grows by the iteration's samples
    (the last row of packed_info: start + count), across 2^31 and with the carry into state[5] across 2^32."""
    opacity, packed, want = alive_case(n, "mixed", 200 + n)
    total = int(packed[-1].sum())
    for start in (0, 2 ** 31 - 3, 2 ** 32 - 3, 5 * 2 ** 32 + 11):
        st = state_words(N_SAMPLES, start)
        mask, alive, count, got = call_testmode_alive(dev, opacity, packed, st, 1)
        check_alive(n, want, mask, alive, int(count[0]))
        assert count[1] == 4242
        assert int(got[4:6].view(np.int64)[0]) == start + total
        assert np.array_equal(got[[0, 1, 2, 3, 6, 7]], st[[0, 1, 2, 3, 6, 7]])
    assert total >= 3 or n < 7                       # (so the two starts above do cross their boundary)
    st = state_words(N_SAMPLES, 2 ** 31 - 3)
    mask, alive, count, got = call_testmode_alive(dev, opacity, packed, st, 0)
    check_alive(n, want, mask, alive, int(count[0]))
    assert np.array_equal(got, st)                   # count_samples = 0: the counter is somebody else's


@pytest.mark.parametrize("n", [1, WG + 1, 3 * WG + 5])
@pytest.mark.parametrize("count_samples", [0, 1])
def test_testmode_alive_does_nothing_after_the_last_iteration(dev, n, count_samples):
    opacity, packed, want = alive_case(n, "alive", 300 + n)
    packed[:, 1] = 0                                 # samples taken == state[0] == 0 everywhere: "alive" if the kernel ran
    st = state_words(0, 2 ** 31 - 3)
    mask, alive, count, got = call_testmode_alive(dev, opacity, packed, st, count_samples, count0=0)
    assert (mask.cpu().numpy() == 7).all() and (alive.cpu().numpy() == -1).all()
    assert count.tolist() == [0, 4242] and np.array_equal(got, st)


# ----------------------------------------------------------------------------- nfa_testmode_begin
def begin_reference(n_rays, n_alive, handed_out, min_samples, max_samples):
    """examples/utils.py:330-340: ``while iter_samples < max_samples``, ``if n_alive == 0: break``,
    ``n_samples = max(min(num_rays // n_alive, 64), min_samples)``, ``iter_samples += n_samples``."""
    if n_alive == 0 or handed_out >= max_samples:
        return 0, handed_out, 0
    n_samples = max(min(n_rays // n_alive, 64), min_samples)
    return n_samples, handed_out + n_samples, 1


BEGIN_STRIDE = 2048 * 256                       # threads of the largest launch: more rays need a second trip of the zeroing loop
BEGIN_CASES = [
    # (n_rays, alive_count[0], state[1], min_samples, max_samples)
    (100, 0, 0, 1, 600),                        # nobody alive
    (100, 0, 600, 1, 600),
    (100, 100, 600, 1, 600),                    # the budget is spent exactly
    (100, 100, 599, 1, 600),                    # one sample left: a whole iteration, overshooting as the reference's while
    (6400, 10, 599, 1, 600),
    (100, 100, 601, 1, 600),
    (100, 150, 0, 1, 600),                      # n_rays // n_alive == 0: clamped up to min_samples
    (100, 150, 0, 4, 600),
    (100, 100, 0, 1, 600),                      # quotient 1
    (100, 51, 17, 1, 600),
    (100, 50, 17, 1, 600),                      # 2
    (6300 + 99, 100, 0, 1, 600),                # 63
    (6400, 100, 0, 1, 600),                     # 64
    (6500, 100, 0, 1, 600),                     # 65: clamped down to 64
    (6500, 1, 3, 1, 600),                       # 6500
    (100, 100, 0, 4, 600),                      # min_samples 4 (the cone-angle loop's)
    (100, 25, 0, 4, 600),                       # quotient == min_samples
    (100, 10, 0, 4, 600),                       # quotient above it
    (100, 100, 597, 4, 600),
    (1, 1, 0, 1, 1),
    (3, 2, 0, 1, 6),
    (BEGIN_STRIDE - 1, BEGIN_STRIDE - 1, 0, 1, 600),
    (BEGIN_STRIDE + 3, BEGIN_STRIDE + 3, 5, 1, 600),     # second trip of the grid-stride loop
    (BEGIN_STRIDE + 3, 0, 5, 1, 600),
]


@pytest.mark.parametrize("n_rays,n_alive,handed_out,min_samples,max_samples", BEGIN_CASES)
def test_testmode_begin(dev, n_rays, n_alive, handed_out, min_samples, max_samples):
    n_zero = 8
    alive_count = torch.tensor([n_alive, 999], dtype=torch.int64, device=dev)
    state0 = np.array([77, handed_out, 5, 1003, 1004, 1005, 1006, 1007], np.int32)
    state = T(state0, dev)
    # one guard element on each side of what the kernel zeroes
    sm_cnts = torch.full((n_rays + 2,), 7, dtype=torch.int64, device=dev)
    run_cnts = torch.full((n_rays + 2,), 7, dtype=torch.int32, device=dev)
    zero_words = torch.full((n_zero + 2,), 7, dtype=torch.int64, device=dev)
    B.call("nfa_testmode_begin", B.ptr(alive_count), B.ptr(state), n_rays, min_samples, max_samples, B.ptr(sm_cnts[1:]),
           B.ptr(run_cnts[1:]), B.ptr(zero_words[1:]), n_zero, B.stream())
    n_samples, handed_out_after, ran = begin_reference(n_rays, n_alive, handed_out, min_samples, max_samples)
    got = state.cpu().numpy()
    assert got[:3].tolist() == [n_samples, handed_out_after, 5 + ran], got
    assert np.array_equal(got[3:], state0[3:])
    assert alive_count.tolist() == [0, n_alive]
    for buf in (sm_cnts, run_cnts, zero_words):
        assert buf[0].item() == 7 and buf[-1].item() == 7
        assert not buf[1:-1].any().item()


def test_begin_cases_cover_the_schedule():
    """The table above reaches every branch of the schedule."""
    quotients = {n // a for n, a, *_ in BEGIN_CASES if a}
    assert {0, 1, 63, 64, 65} <= quotients
    assert any(a == 0 for _, a, *_ in BEGIN_CASES)
    assert any(a and h == mx for _, a, h, _, mx in BEGIN_CASES) and any(a and h == mx - 1 for _, a, h, _, mx in BEGIN_CASES)
    assert any(mn == 4 for *_, mn, _ in BEGIN_CASES) and any(n > BEGIN_STRIDE for n, *_ in BEGIN_CASES)


# ----------------------------------------------------------------------------- the loop, every form
_DEVICE_SCENES: dict = {}
_FORMS: dict = {}
FORM_NAMES = ("two_reads", "one_read", "exact", "graph_1", "graph_2", "no_graph")


def device_scene(dev, scene):
    """(estimator, rays_o, rays_d, background) on the device, built once per scene."""
    got = _DEVICE_SCENES.get(scene.name)
    if got is None:
        est = na.OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=scene.resolution, levels=scene.levels).to(dev)
        est.binaries = T(scene.binaries, dev)
        assert np.array_equal(est.aabbs.cpu().numpy(), scene.aabbs)
        got = _DEVICE_SCENES[scene.name] = (est, T(scene.rays_o, dev), T(scene.rays_d, dev), T(S.BKGD, dev))
    return got


def run_forms(dev, scene, fn, alpha_thre=0.0):
    """``{form: (rgb, opacity, depth, total, iterations or None)}`` of the four forms of the loop (the padded one with a
    graph twice, and render_exact on a loop object for its iteration count)."""
    assert G.MAX_RUNS == S.MAX_RUNS
    est, o, d, bk = device_scene(dev, scene)
    kw = dict(near_plane=S.NEAR_PLANE, far_plane=S.FAR_PLANE, render_step_size=scene.step, alpha_thre=alpha_thre,
              early_stop_eps=S.EARLY_STOP_EPS)
    out = {}
    marching.ONE_READ = False
    try:
        out["two_reads"] = (*render_rays_test_mode(scene.max_samples, fn, est, o, d, render_bkgd=bk, **kw), None)
    finally:
        marching.ONE_READ = True
    out["one_read"] = (*render_rays_test_mode(scene.max_samples, fn, est, o, d, render_bkgd=bk, **kw), None)
    loops = {g: PaddedTestModeLoop(scene.max_samples, fn, est, o, d, S.NEAR_PLANE, S.FAR_PLANE, scene.step, alpha_thre,
                                   S.EARLY_STOP_EPS, use_graph=g) for g in (False, True)}
    out["exact"] = (*loops[False].render_exact(bk), loops[False].iterations_run)
    for name, g in (("graph_1", True), ("graph_2", True), ("no_graph", False)):
        out[name] = (*loops[g].render(bk), loops[g].iterations_run)
    assert tuple(out) == FORM_NAMES
    return out


def float32_forms(dev, scene, alpha_thre=0.0):
    """The forms with the scene's float32 callback: computed once, shared, never written to."""
    key = (scene.name, float(alpha_thre))
    if key not in _FORMS:
        _FORMS[key] = run_forms(dev, scene, S.field_torch(scene), alpha_thre)
    return _FORMS[key]


def assert_forms_identical(forms, want, what):
    for name, got in forms.items():
        assert got[3] == want[3], (what, name, got[3], want[3])
        for a, w, part in zip(got[:3], want[:3], ("rgb", "opacity", "depth")):
            assert a.dtype == torch.float32 and torch.equal(a, w), (what, name, part)


def assert_matches_oracle(scene, forms, alpha_thre=0.0, guard=1e-5):
    orgb, oopa, odep, ototal, info = S.reference(scene, alpha_thre, guard)
    assert not info["guard_rays"].any()
    assert_forms_identical(forms, forms["one_read"], scene.name)
    rgb, opa, dep, total, _ = forms["one_read"]
    assert total == ototal, (total, ototal)
    for name in ("exact", "graph_1", "graph_2", "no_graph"):
        assert forms[name][4] == info["iterations"], (name, forms[name][4], info["iterations"])
    if scene.keep_sigma == 0:
        assert np.array_equal(opa.cpu().numpy(), oopa)           # exactly 0 or 1
    else:
        assert_close(opa, oopa, atol=2e-5, rtol=1e-5)
    assert_close(rgb, orgb, atol=2e-5, rtol=1e-5)
    assert_close(dep, odep, atol=1e-4, rtol=1e-4)
    return info


@pytest.mark.parametrize("alpha_thre", [0.0, 0.5])
@pytest.mark.parametrize("mod,max_samples", S.FULL_SETTINGS)
@pytest.mark.parametrize("n_rays", S.FULL_SIZES)
def test_loop_full(dev, oracle, n_rays, mod, max_samples, alpha_thre):
    """Iterations whose samples fill the arrays to the last slot (mod 1), fewer rays than a wave and than the smallest
    capacity, ``max_samples`` spent with rays alive (mod 3); with ``alpha_thre`` the total comes from the device's counter of
    visible samples (alphas are exactly 0 or 1)."""
    scene = S.full(n_rays, mod, max_samples)
    info = assert_matches_oracle(scene, float32_forms(dev, scene, alpha_thre), alpha_thre)
    if mod == 1 and alpha_thre == 0:
        assert any(t[0] == n_rays for t in info["trace"])


def test_loop_checker(dev, oracle):
    """Rays with more than MAX_RUNS run records in two successive iterations: the fill pass of every form."""
    scene = S.checker()
    info = assert_matches_oracle(scene, float32_forms(dev, scene))
    assert sum(1 for t in info["trace"] if t[1] >= 10) >= 2


def test_loop_checker_with_a_density(dev, oracle):
    """The same rays with a small density on the long-lived ones: their samples weigh something, so the depth image depends
    on every position the fill pass writes -- in the padded loop from its own copy of the iteration's near planes.  No ray
    comes near the termination threshold (asserted), so counts and schedule still equal the oracle's."""
    scene = S.checker(0.5)
    info = assert_matches_oracle(scene, float32_forms(dev, scene), guard=2e-6)
    assert sum(1 for t in info["trace"] if t[1] >= 10) >= 2


def test_loop_multi(dev, oracle):
    """2 * 8192 + 77 rays through two nested levels: the alive list comes from three workgroups, then from one."""
    scene = S.multi()
    info = assert_matches_oracle(scene, float32_forms(dev, scene))
    assert info["iterations"] >= 20


def test_loop_miss(dev, oracle):
    scene = S.miss()
    forms = float32_forms(dev, scene)
    assert_matches_oracle(scene, forms)
    for name, (rgb, opa, dep, total, _) in forms.items():
        assert total == 0, name
        assert not opa.any().item() and not dep.any().item(), name
        assert torch.equal(rgb, T(S.BKGD, dev).expand(scene.n_rays, 3)), name


def test_loop_multi_general_field(dev, oracle):
    """``keep_sigma = 8``: opacities between 0 and 1, the weights' general arithmetic.  Rays that end an iteration within
    2e-6 of the early-termination threshold may live one iteration longer on one side (at most 64 samples each), as in
    test_test_mode_marching_loop; every other ray agrees, and the forms agree bit for bit."""
    scene = S.multi(8.0)
    forms = float32_forms(dev, scene)
    assert_forms_identical(forms, forms["one_read"], scene.name)
    orgb, oopa, odep, ototal, info = S.reference(scene, guard=2e-6)
    g = info["guard_rays"]
    assert g.mean() < 0.1
    rgb, opa, dep, total, _ = forms["one_read"]
    assert abs(total - ototal) <= 64 * int(g.sum())
    if not g.any():
        assert forms["exact"][4] == forms["graph_1"][4] == forms["no_graph"][4] == info["iterations"]
    k = torch.from_numpy(~g).to(dev)
    assert_close(opa[k], oopa[~g], atol=2e-5, rtol=1e-5); assert_close(rgb[k], orgb[~g], atol=2e-5, rtol=1e-5)
    assert_close(dep[k], odep[~g], atol=1e-4, rtol=1e-4)


# ----------------------------------------------------------------------------- half-precision and strided callbacks
def returns_dtype(fn, dtype):
    def wrapped(ts, te, ri):
        rgbs, sigmas = fn(ts, te, ri)
        return rgbs.to(dtype), sigmas.to(dtype)
    return wrapped


def returns_transposed_rgbs(fn):
    def wrapped(ts, te, ri):
        rgbs, sigmas = fn(ts, te, ri)
        return rgbs.t().contiguous().t(), sigmas      # float32 (N, 3), the transpose of a contiguous (3, N) tensor
    return wrapped


HALF_SCENES = {"full": lambda: S.full(128, 3, 6), "multi": S.multi}
CALLBACK_WRAPS = {"fp16": lambda fn: returns_dtype(fn, torch.float16), "bf16": lambda fn: returns_dtype(fn, torch.bfloat16),
                  "transposed": returns_transposed_rgbs}


@pytest.mark.parametrize("wrap", list(CALLBACK_WRAPS))
@pytest.mark.parametrize("scene_name", list(HALF_SCENES))
def test_loop_callback_dtype_and_layout(dev, scene_name, wrap):
    """A callback that returns fp16 or bf16 (an autocast field; the field's values are exact in both) or a strided float32
    view: every form converts to contiguous float32 before the accumulation pass, so the image equals the float32
    callback's bit for bit."""
    scene = HALF_SCENES[scene_name]()
    fn = CALLBACK_WRAPS[wrap](S.field_torch(scene))
    probe = fn(torch.zeros(8, device=dev), torch.ones(8, device=dev), torch.arange(8, device=dev))
    if wrap == "transposed":
        assert probe[0].dtype == torch.float32 and probe[0].shape == (8, 3) and not probe[0].is_contiguous()
    else:
        assert probe[0].dtype == probe[1].dtype != torch.float32
    want = float32_forms(dev, scene)["one_read"]
    assert want[3] > 0
    assert_forms_identical(run_forms(dev, scene, fn), want, (scene.name, wrap))
