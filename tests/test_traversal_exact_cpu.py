"""CPU: tests/traversal_reference.py against the C oracle, and the shares of ties and equalities in the exact scenes.

test_traversal_exact_gpu.py compares the traversal kernels with ``oracle.traverse_grids`` on the rays of
``traversal_reference.case`` / ``planes``: rays through cell edges and corners, samples whose midpoint sits exactly on the
distance it is compared with.  Whether a batch contains such events cannot be seen from the oracle's outputs; the float32
restatement ``traversal_reference.traverse_ray`` counts them.  Here, without a GPU and on the same keys:

* the restatement equals ``oracle.traverse_grids`` bit for bit (ray ids, t_starts, t_ends, termination planes) on every
  kept ray of every one-level scene, for every step and every choice of planes;
* the shares below are asserted, so the GPU tests cannot quietly turn into random tests.

Measured (4800 rays drawn per scene, 4321 / 4278 kept in the 16^3 / 12^3 scene; every run prints the figures, ``pytest -s``
shows them).  Shares of cell steps for ties, of kept rays for the rest:

    scene, step           planes         two-way  three-way  cell-exit equality  any midpoint equality  rays with samples
    16^3  2^-6            zero           22.2 %   4.8 %      0                   0                      49.0 %
    16^3  2^-6            common         20.8 %   3.9 %      1.0 %               8.1 %                  47.7 %
    16^3  2^-6            directed       25.7 %   7.6 %      49.4 %              49.4 %                 49.0 %
    16^3  2^-6            directed_far   24.8 %   7.2 %      48.7 %              48.7 %                 47.7 %
    16^3  3*2^-8          directed       25.7 %   7.6 %      49.4 %              49.4 %                 49.0 %
    16^3  2^-6+2^-25      directed       22.6 %   5.5 %      15.2 %              15.2 %                 49.1 %
    12^3  2^-6            zero            9.1 %   0.7 %      0                   0                      49.6 %
    12^3  2^-6            common          8.6 %   0.7 %      10.4 %              15.4 %                 48.4 %
    12^3  2^-6            directed        9.2 %   0.7 %      43.9 %              43.9 %                 49.8 %
    12^3  3*2^-8          directed        9.2 %   0.7 %      36.6 %              36.6 %                 49.8 %
    12^3  2^-6+2^-25      directed        9.1 %   0.6 %      28.0 %              28.0 %                 49.8 %

0 * inf rays: 10.0 %, 9.3 %, 10.7 %, 10.9 % of the four scenes' draws.  Two levels (16^3): 98.0 % of the kept rays have samples.
With the common planes and the step 3*2^-8 no midpoint meets a threshold, but 22 (16^3) and 252 (12^3) samples END on their
cell's exit (``t_next == t_traverse``).  920 / 947 rays start their first span on the near plane.

The floors of the 16^3 scene with the step 2^-6 are the ones the family was designed for (22 %, 4 %, 52 %, 8 %, 10.2 %, 51 %,
98 % measured on 600 rays of it: floors 15 %, 2 %, 30 %, 4 %, 12 % ceiling, 45 %, 90 %); every other floor is two thirds of the
share in the table.
"""
import numpy as np
import pytest

import traversal_reference as TR

ONE_LEVEL = [s for s, (_, levels) in TR.SCENES.items() if levels == 1]


def shares(scene, step_name, mode):
    ri, ts, te, term, evs = TR.restated(scene, step_name, mode)
    t = TR.totals(evs)
    n, cs = t["rays"], max(t["cell_steps"], 1)
    return dict(t, samples=int(ri.size), ties2_share=t["ties2"] / cs, ties3_share=t["ties3"] / cs,
                mid_eq_cell_share=t["rays_mid_eq_cell"] / n, mid_eq_share=t["rays_mid_eq"] / n,
                sampled_share=np.unique(ri).size / n)


def show(scene, step_name, mode, s):
    print(f"{scene:>4} {step_name:>10} {mode:>12}: rays {s['rays']} samples {s['samples']} cell steps {s['cell_steps']} "
          f"ties2 {s['ties2']} ({s['ties2_share']:.3f}) ties3 {s['ties3']} ({s['ties3_share']:.3f}) "
          f"mid==exit occupied {s['mid_eq_occ']} skipped {s['mid_eq_skip']} span start {s['mid_eq_span']} next==exit {s['next_eq']} "
          f"starts on near {s['starts_on_near']} | rays with a cell-exit equality {s['mid_eq_cell_share']:.3f}, any {s['mid_eq_share']:.3f}, "
          f"with samples {s['sampled_share']:.3f}")


@pytest.mark.parametrize("scene", ONE_LEVEL)
@pytest.mark.parametrize("step_name", list(TR.STEPS))
def test_restatement_equals_oracle(oracle, scene, step_name):
    o, d, b, ab, _ = TR.case(scene)
    for mode in TR.PLANE_MODES:
        near, far = TR.planes(scene, step_name, mode)
        ri, ts, te, term, evs = TR.restated(scene, step_name, mode)
        iv, sm, oterm = oracle.traverse_grids(o, d, b, ab, near_planes=near, far_planes=far, step_size=TR.STEPS[step_name])
        assert np.array_equal(ri, sm["ray_indices"]), (scene, step_name, mode)
        assert np.array_equal([e.n_intervals for e in evs], iv["packed_info"][:, 1]), (scene, step_name, mode)
        assert np.array_equal(ts, iv["vals"][iv["is_left"]]) and np.array_equal(te, iv["vals"][iv["is_right"]]), (scene, step_name, mode)
        assert np.array_equal(term, oterm), (scene, step_name, mode)
        show(scene, step_name, mode, shares(scene, step_name, mode))


def test_restatement_per_cell_mode_equals_oracle(oracle):
    """step_size == 0: one sample per occupied cell -- the cell walk alone, which is what directed_near_planes reads."""
    for scene in ONE_LEVEL:
        o, d, b, ab, _ = TR.case(scene)
        for mode in ("zero", "common"):
            near, far = TR.planes(scene, "2^-6", mode)
            ri, ts, te, term, evs = TR.traverse_rays(o, d, b[0], ab[0], near, far, 0.0)
            iv, sm, oterm = oracle.traverse_grids(o, d, b, ab, near_planes=near, far_planes=far, step_size=0.0)
            assert np.array_equal(ri, sm["ray_indices"]) and np.array_equal(term, oterm)
            assert np.array_equal(ts, iv["vals"][iv["is_left"]]) and np.array_equal(te, iv["vals"][iv["is_right"]])
            assert sum(len(e.occupied_exits) for e in evs) == ri.size


def test_family_shares():
    for scene in TR.SCENES:
        o, d, b, ab, bad_share = TR.case(scene)
        print(f"{scene}: {o.shape[0]} kept rays, 0 * inf share {bad_share:.3f}")
        assert bad_share <= 0.12
        assert o.shape[0] >= 4096                       # the binned walk needs that many
        assert not np.isnan(o).any() and (d != 0).any(-1).all()


# floors: two thirds of the measured share (module docstring), or the issue's floor where that is lower
FLOORS_16 = dict(ties2=0.15, ties3=0.02, directed_eq=0.30, common_eq=0.04, sampled=0.45)


def test_tie_and_equality_shares_dyadic_scene():
    z = shares("16", "2^-6", "zero")
    assert z["ties2_share"] >= FLOORS_16["ties2"] and z["ties3_share"] >= FLOORS_16["ties3"]
    assert z["sampled_share"] >= FLOORS_16["sampled"]
    assert z["starts_on_near"] >= 0.1 * z["rays"]            # origins inside the box: the span starts on the near plane
    c = shares("16", "2^-6", "common")
    assert c["mid_eq_share"] >= FLOORS_16["common_eq"]
    assert c["ties2_share"] >= FLOORS_16["ties2"] and c["ties3_share"] >= FLOORS_16["ties3"]
    for mode in ("directed", "directed_far"):
        s = shares("16", "2^-6", mode)
        assert s["mid_eq_cell_share"] >= FLOORS_16["directed_eq"]
        assert s["mid_eq_occ"] > 0 and s["mid_eq_skip"] > 0
        assert s["ties2_share"] >= FLOORS_16["ties2"] and s["ties3_share"] >= FLOORS_16["ties3"]


# (scene, step): (two-way ties, three-way ties with zero planes; cell-exit equality rays with directed planes) -- two thirds of
# the measured shares
FLOORS_OTHER = {
    ("16", "3*2^-8"): (0.15, 0.02, 0.30),
    ("16", "2^-6+2^-25"): (0.15, 0.02, 0.10),
    ("12", "2^-6"): (0.06, 0.004, 0.29),
    ("12", "3*2^-8"): (0.06, 0.004, 0.24),
    ("12", "2^-6+2^-25"): (0.06, 0.004, 0.18),
}


@pytest.mark.parametrize("scene,step_name", list(FLOORS_OTHER))
def test_tie_and_equality_shares_other_cases(scene, step_name):
    t2, t3, eq = FLOORS_OTHER[(scene, step_name)]
    z = shares(scene, step_name, "zero")
    assert z["ties2_share"] >= t2 and z["ties3_share"] >= t3 and z["sampled_share"] >= 0.45
    for mode in ("directed", "directed_far"):
        s = shares(scene, step_name, mode)
        assert s["mid_eq_cell_share"] >= eq * (1.0 if mode == "directed" else 0.9), (mode, s["mid_eq_cell_share"])
        assert s["mid_eq_occ"] > 0 and s["mid_eq_skip"] > 0
    if step_name == "3*2^-8":
        assert shares(scene, step_name, "common")["next_eq"] >= 10       # samples that end exactly on their cell's exit
    if (scene, step_name) == ("12", "2^-6"):
        assert shares(scene, step_name, "common")["mid_eq_share"] >= 0.10


def differing_rays(scene, step_name, mode, variant, n=1200):
    """Rays (of the scene's first ``n``) on which a wrong rule changes the samples, the interval edges or the termination
    plane -- what the GPU tests compare."""
    o, d, b, ab, _ = TR.case(scene)
    near, far = TR.planes(scene, step_name, mode)
    step = TR.STEPS.get(step_name, 0.0)
    ri, ts, te, term, evs = TR.traverse_rays(o[:n], d[:n], b[0], ab[0], near[:n], far[:n], step)
    vri, vts, vte, vterm, vevs = TR.traverse_rays(o[:n], d[:n], b[0], ab[0], near[:n], far[:n], step, variant)
    diff = term != vterm
    diff |= np.array([e.n_intervals != v.n_intervals for e, v in zip(evs, vevs)])
    cnt, vcnt = np.bincount(ri, minlength=n), np.bincount(vri, minlength=n)
    diff |= cnt != vcnt
    first, vfirst = np.cumsum(cnt) - cnt, np.cumsum(vcnt) - vcnt
    for r in np.flatnonzero(~diff):
        a, va = slice(first[r], first[r] + cnt[r]), slice(vfirst[r], vfirst[r] + cnt[r])
        diff[r] = not (np.array_equal(ts[a], vts[va]) and np.array_equal(te[a], vte[va]))
    return int(diff.sum())


def test_exact_scenes_tell_wrong_rules_apart():
    """The point of the exact scenes: a traversal that breaks ties in another order, or compares a midpoint or a sample's end
    with ``>`` where the reference has ``>=``, gives other outputs on them.  (On random rays none of these variants changes
    anything: the equalities never occur.)  Floors: a third of the measured counts (of 1200 rays: 120 and 345 for the tie order
    with the step 2^-6 and in the per-cell mode, 598 for the midpoint).  The third ``>=`` of the reference, ``t_next >=
    t_traverse`` (:253), cannot be told from ``>`` by any input: after a sample that ends on the exit the midpoint test ends the
    cell anyway."""
    n = differing_rays("16", "2^-6", "zero", "ties_x_first")
    n0 = differing_rays("16", "per_cell", "zero", "ties_x_first")
    print(f"ties_x_first: {n} rays differ with the step 2^-6, {n0} in the per-cell mode")
    assert n >= 40 and n0 >= 115
    m = differing_rays("16", "2^-6", "directed", "mid_strict")
    print(f"mid_strict: {m} rays differ with the directed near planes")
    assert m >= 200
    assert differing_rays("16", "2^-6", "zero", "mid_strict", n=300) == 0      # ... and without the planes nothing tells them apart


def test_two_level_scene_sample_share(oracle):
    o, d, b, ab, _ = TR.case("16x2")
    _, sm, _ = oracle.traverse_grids(o, d, b, ab, step_size=TR.STEPS["2^-6"])
    share = (sm["packed_info"][:, 1] > 0).mean()
    print(f"16x2: rays with samples {share:.3f}")
    assert share >= 0.90
