"""GPU tests of damped junctions in groups (Junction.of(shared=True, damped=True) -> Scene.render_damped_groups -> RenderModalDampedGroups ->
mh_bank_render_damped_groups -> k_bank_modes_grouped<Real, OBSERVE, true, true>; contract: include/modalhip.h, step 4g).

Scenes and shapes are those of tests/test_bank_groups_gpu.py: objects of 32, 130 and 256 modes, T60 2 s, noise drives; a star of three on
the 130-mode hub, a chain, four exciter junctions on the 32-mode object, two junctions between one pair.  Members all damped (even
members Hertz, odd ones linear), or mixed: member 0 damped Hertz, 1 plain Hertz, 2 damped linear, 3 linear and bilateral.  Three blocks of
128 frames, so the carry crosses two boundaries; one run in blocks of 77 for the tile tail.

1. Fails without the feature: a damped member of a star, linear or Hertz, has status 1 and a row that is not zero through
   render_damped_groups, status 0 through render_mixed.
2. A call without a damped junction in a group is render_mixed bit for bit: rows, reads, C, statuses, carries, unconverged, samples, states.
3. Force rows, samples, C_ii and carries against the numpy.longdouble restatement (tests/damped_group_harness.py) under a steered approach
   with the carry passed on, and 4. the law where it is solved, from advance-1 pickups at every member's sides in the same call.
5. The carry matters: a NaN in its place at a boundary moves the rows away by far more than the bound.
6. Bit-exact: a second run, 1 against 4 renderers, bystanders, one block against two halves with the carry passed (128 = 64 + 64 and
   231 = 3 x 77), a dead group against silent members, gating.
7. Replay: the returned rows as drives on a twin move an object that carries one replayed row bit for bit in fp32.
8. The kinds still left out have the bits of the call without them; a refused group has the bits of K = 0 and NaN carries.
9. Every junction launch in one call -- lone, linear group, Hertz-member group, damped-member group, tapped waves, the main launch -- has
   the bits of four calls with one kind each."""
import numpy as np
import pytest

from tests import bank_harness as bh
from tests import damped_group_harness as dg
from tests import drive_harness as dh
from tests import group_harness as gh
from tests import observed_harness as oh
from tests import pickup_harness as ph
from tests import test_bank_groups_gpu as groups_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
BOUND = 4  # x the working-precision restatement's own deviation: the suite's standing bound
FRAMES, BLOCKS = 128, 3
MODES, T60, SIZES = groups_suite.MODES, groups_suite.T60, groups_suite.SIZES
_shape, _drive_args, _noise_rows, _states, _same = groups_suite._shape, groups_suite._drive_args, groups_suite._noise_rows, groups_suite._states, groups_suite._same
FREE = 2e-5  # the size of a member's free deflection under the noise drives, as tests/test_bank_groups_gpu.py takes it
RATE = np.float32(bh.SAMPLE_RATE)


def _rate(lam):
    """(D in s/m as the binding takes it, l per frame as the bank forms it: float32(D) * float32(sample rate))."""
    d = np.float32(lam) / RATE
    return np.float32(d), np.float32(d * RATE)


def _laws(name, mixed):
    """(hertz, bilateral, damped) per member."""
    n = SIZES[name]
    if not mixed:
        return [i % 2 == 0 for i in range(n)], [False] * n, [True] * n
    return [i < 2 for i in range(n)], [i == 3 for i in range(n)], [i % 2 == 0 for i in range(n)]


def _specs(name, k, mixed, single_points=False):
    hertz, bilateral, damped = _laws(name, mixed)
    return [dg.spec(s[0], s[1], s[2], bilateral[i], hertz[i], damped[i]) for i, s in enumerate(_shape(name, k, single_points))]


def _stiffness(comp, hertz, kc, scale):
    """K with K C_ii sqrt(scale) = kc on a Hertz member and K C_ii = kc on a linear one."""
    return [kc / (c * np.sqrt(s)) if h else kc / c for c, h, s in zip(comp, hertz, scale)]


def _approach(n, frames, blocks, amp=3.0, period=100.0, phase=0.9):
    t = np.arange(blocks * frames)
    return np.array([(amp * FREE * (np.sin(2 * np.pi * t / period - phase * j) + 0.1)).astype(np.float32) for j in range(n)])


def _call(sc, entry, out, rows, pickups, specs, u, rates, carry):
    """One block: (reads, forces, comp, status, carry, unconverged)."""
    got = getattr(sc, entry)(out, *_drive_args(rows, len(out)), ph.records(list(pickups)), dg.records(specs), u, rates, carry)
    return got[0], got[2], got[3], got[4], got[5], got[6]


def _run(use_double, specs, u, rates, renderers=1, entry="render_damped_groups", blocks=BLOCKS, frames=FRAMES, pickups=(), modes=MODES, forget=()):
    """Noise drives on every object (the signal of 3 x 128 frames, cut into the blocks), the given junctions and approach rows, the carry
    passed from block to block -- replaced by NaN ahead of the blocks in `forget`.  Returns (forces, reads, comp, status, unconverged,
    carries per block, [out, states, object state])."""
    sc, _ = dh.device_scene(modes, T60, renderers, use_double)
    total = blocks * frames
    noise = _noise_rows(modes, 0, 1, total)
    rows_f, rows_r, outs, carries, counts = [], [], [], [], np.zeros(len(specs), np.uint64)
    carry = None
    for b in range(blocks):
        out = np.zeros(frames, sc.dtype)
        rows = [(o, p, d, f[b * frames:(b + 1) * frames]) for (o, p, d, f) in noise]
        if b in forget:
            carry = None
        reads, forces, comp, status, carry, bad = _call(sc, entry, out, rows, list(pickups), specs, u[:, b * frames:(b + 1) * frames], rates, carry)
        rows_f.append(forces.copy()), rows_r.append(reads.copy()), outs.append(out), carries.append(carry.copy())
        counts += bad
    result = np.concatenate(rows_f, axis=1), np.concatenate(rows_r, axis=1), comp, status, counts, carries, [np.concatenate(outs)] + _states(sc) + list(sc.object_state())
    sc.close()
    return result


def _comp(name, use_double):
    return groups_suite._compliances(name, use_double)


def _star(use_double, mixed=False, kc=10.0, k_scale=(1, 1, 1), lam_x=1.0):
    """(specs, D per member) of the star with K C sqrt(FREE) or K C = kc and l FREE = lam_x."""
    hertz, _, _ = _laws("star", mixed)
    k = _stiffness(_comp("star", use_double), hertz, kc, [FREE] * 3)
    return _specs("star", [a * b for a, b in zip(k, k_scale)], mixed), np.full(3, _rate(lam_x / FREE)[0], np.float32)


# ---- 1. the feature ----
@PRECISIONS
def test_a_damped_member_of_a_group_is_solved(use_double):
    """The all-damped star: member 0 and 2 are damped Hertz junctions, member 1 a damped linear one."""
    (specs, rates), u = _star(use_double), _approach(3, FRAMES, BLOCKS)
    forces, _, comp, status, bad, carries, _ = _run(use_double, specs, u, rates)
    assert list(status) == [1, 1, 1], list(status)
    assert (np.abs(forces).max(axis=1) > 0).all() and np.isfinite(forces).all() and (forces >= 0).all()
    assert np.array_equal(comp, _comp("star", use_double)) and not bad.any()
    assert all(np.isfinite(c).all() for c in carries)
    old, _, _, old_status, _, old_carries, _ = _run(use_double, specs, u, rates, entry="render_mixed")
    assert list(old_status) == [1, 0, 0] and not old[1:].any() and np.abs(old[0]).max() > 0
    assert all(np.isnan(c[1:]).all() for c in old_carries)


# ---- 2. the entry without a damped junction in a group ----
@PRECISIONS
@pytest.mark.parametrize("renderers", [1, 4])
def test_without_a_damped_junction_in_a_group_it_is_render_mixed(use_double, renderers):
    """A linear group (the four exciter junctions on the 32-mode object, one bilateral), a Hertz group (two exciter junctions on the hub),
    a lone damped junction, a lone flagged damped Hertz junction and an unflagged bystander on objects of their own; advance-1 pickups at
    every side."""
    modes = MODES + [64, 64]
    comp = _comp("four", use_double)
    specs = [s + (False,) for s in _shape("four", [10.0 / c for c in comp])]
    specs[3] = dg.spec(specs[3][0], None, specs[3][2], bilateral=True)
    specs += [dg.spec(gh.side(1, 1, direction=groups_suite.NORMAL), None, 2e9, hertz=True), dg.spec(gh.side(1, 3, direction=(0.5, 0.5, -1.0)), None, 1e9, hertz=True)]
    specs += [gh.spec(gh.side(2, 1, direction=(1.0, 0.0, 0.5)), None, 1e5, shared=False) + (True,), dg.spec(gh.side(3, 2, direction=(0.0, 1.0, 0.25)), None, 2e9, hertz=True, damped=True),
              gh.spec(gh.side(4, 0, direction=(1.0, 0.5, 0.0)), None, 1e5, shared=False) + (False,)]
    u = _approach(len(specs), FRAMES, BLOCKS)
    rates = np.full(len(specs), _rate(1.0 / FREE)[0], np.float32)
    pickups = [p for _, p in oh.side_pickups(specs)]
    new = _run(use_double, specs, u, rates, renderers, pickups=pickups, modes=modes)
    old = _run(use_double, specs, u, rates, renderers, entry="render_mixed", pickups=pickups, modes=modes)
    assert list(new[3]) == [1] * 9 and (np.abs(new[0]).max(axis=1) > 0).sum() >= 8 and np.abs(new[1]).max() > 0
    for a, b in zip(new[:5], old[:5]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(new[5], old[5])) and np.isfinite(new[5][-1][[6, 7]]).all() and np.isnan(new[5][-1][:6]).all()
    assert _same(new[6], old[6]) and not new[4].any()


# ---- 3. and 4. accuracy, and the law where it is solved ----
_RESTATED = {}
PAIRS = ((1.0, 0.1), (30.0, 1.0), (1.0, 10.0), (30.0, 0.1), (1.0, 1.0), (30.0, 10.0))  # (K C, l d)


_Steer = dg.Steer


def _restated(name, mixed, use_double, kc, lam_x, forget=()):
    """The longdouble and working-precision runs of a shape over the three blocks with the carry passed on (forgotten ahead of the blocks
    in `forget`), once per case."""
    key = (name, mixed, use_double, kc, lam_x, tuple(forget))
    if key in _RESTATED:
        return _RESTATED[key]
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    exact, working, scout = (dg.Restatement(sc, MODES, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    sc.close()
    n = SIZES[name]
    hertz, bilateral, damped = _laws(name, mixed)
    noise = _noise_rows(MODES, 0, 1, BLOCKS * FRAMES)
    all_rows = [[(o, p, d, f[b * FRAMES:(b + 1) * FRAMES]) for (o, p, d, f) in noise] for b in range(BLOCKS)]
    trace = {}
    scout.render_grouped(all_rows[0], _shape(name, [0.0] * n), np.zeros((n, FRAMES), np.float32), FRAMES, trace)  # the size of the free deflection
    scale = np.sqrt((trace["d"] ** 2).mean(axis=1))
    specs = _specs(name, _stiffness(_comp(name, use_double), hertz, kc, scale), mixed)
    both = [_rate(lam_x / s) for s in scale]
    rates, lam = np.array([r[0] for r in both], np.float32), np.array([r[1] for r in both], np.float32)
    C, K = exact.compliance_matrix(specs), [np.float32(s[2]) for s in specs]
    steer = _Steer(n, C, K, hertz, damped, lam, scale, 3 if n == 4 else 6, lam_x)
    runs, sets = [], []
    nothing = np.full(n, np.nan)
    carry_exact, carry_work = nothing, nothing
    for b in range(BLOCKS):
        t_exact, t_work = {}, {}
        steer.first = b * FRAMES
        if b in forget:
            carry_exact, carry_work = nothing, nothing
        want = exact.render_damped_groups(all_rows[b], specs, steer, lam, carry_exact, FRAMES, t_exact)
        plain = working.render_damped_groups(all_rows[b], specs, t_exact["u"], lam, carry_work, FRAMES, t_work)
        carry_exact, carry_work = want[5], plain[5]
        sets.append(t_exact["sets"])
        runs.append((t_exact["u"], want, plain, t_work["read1"]))
    c_exact = np.diag(exact.compliance_matrix(specs)).astype(np.longdouble)
    c_plain = np.diag(working.compliance_matrix(specs)).astype(np.longdouble)
    _RESTATED[key] = (specs, rates, lam, all_rows, runs, c_exact, c_plain, np.concatenate(sets))
    return _RESTATED[key]


def _law_figure(specs, lam, forces, u, reach, before):
    """The largest |f[s] - K phi(y'[s]) max(1 + l (y'[s] - y'[s - 1]), 0)| over a row's peak, y' = u - reach, reach [n][frames] the sum of
    the advance-1 reads at the member's sides; before: y' of the frame ahead of the block (None: the first block, where frame 0 has no
    history and is skipped on a damped member).  Returns (figure, y' of the last frame)."""
    T = forces.dtype.type
    worst = 0.0
    y_all = u.astype(T) - reach.astype(T)
    for i, s in enumerate(specs):
        y = y_all[i]
        pos = np.where(y > 0, y, T(0))
        law = T(np.float32(s[2])) * (pos * np.sqrt(pos) if s[4] else (y if s[3] else pos))
        first = 0
        if s[6]:
            prev = np.concatenate([[before[i] if before is not None else y[0]], y[:-1]]).astype(T)
            m = T(1) + T(lam[i]) * (y - prev)
            law = law * np.where(m > 0, m, T(0))
            first = 0 if before is not None else 1
        peak = float(np.abs(forces[i]).max())
        if peak > 0:
            worst = max(worst, float(np.abs(forces[i].astype(np.longdouble) - law.astype(np.longdouble))[first:].max()) / peak)
    return worst, y_all[:, -1]


@PRECISIONS
@pytest.mark.parametrize("mixed", [False, True], ids=["damped", "mixed"])
@pytest.mark.parametrize("name", ["star", "chain", "four", "pair"])
def test_forces_samples_carries_and_the_law_match_a_longdouble_restatement(use_double, mixed, name):
    """K from the returned C_ii so that K C sqrt(d) (Hertz; d the rms free deflection) or K C (linear) = 1 and 30, l d = 0.1, 1 and 10: the
    six pairs (PAIRS) are dealt round over the eight groups, two each, so that the all-damped groups see all six and the mixed groups do
    -- the longdouble restatement is what a case's time goes to --, one with 1 renderer and one with 4, alternating; 3 blocks of 128
    frames with the carry passed on.  The approach is steered from the longdouble run's own free
    prediction (_Steer): six frames per active set (three with four members), the empty set and the full one a quarter of the frames
    each.  Conditions on the inputs, asserted on the longdouble run: the empty and the full set hold 15 % of the frames each or more, and
    at both block boundaries a damped member is compressed in the frame before and the frame after.
    Figures: the largest deviation of a force row / of the samples from the longdouble restatement's over the row's peak, the relative
    deviation of C_ii, the largest deviation of a carry over all blocks and members over the largest carry, and the law -- |f - K phi(y')
    max(1 + l (y'[s] - y'[s - 1]), 0)|, y' = u - the sum of the advance-1 reads at the member's sides, over the row's peak -- of the device
    and of the working-precision restatement in the same run.  Bound: 4 x.  unconverged is 0 on the device and in the restatement.

    The yardsticks are asserted to say something (below 1e7 eps).  The largest by far are the law and the carry of the four mixed
    members at K C = 30, l d = 10: 1e6 eps, 0.12 and 0.18 of the peak in fp32 -- C df is 30 times the compression there --, so that in
    fp32 those two figures of that one case bound little; its force rows (5e-3) and samples (6e-5) and every other case's law and carry
    (at most 1e-2 of the peak in fp32, 3e-11 in fp64) are the check.
    Measured on an MI355X (this test prints the figures): force rows 0.13 - 0.96 x, samples 0.12 - 0.71 x, C_ii
    0.14 - 0.48 x, carries 0.02 - 1.13 x, the law 0.16 - 1.55 x the restatement's deviation."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    n = SIZES[name]
    at = 2 * (2 * ["star", "chain", "four", "pair"].index(name) + int(mixed))
    first = 1 if (at // 2) % 2 == 0 else 4  # (the renderer counts alternate from group to group, so neither always meets the same pairs)
    for (kc, lam_x), renderers in ((PAIRS[at % 6], first), (PAIRS[(at + 1) % 6], 5 - first)):
        specs, rates, lam, all_rows, runs, c_exact, c_plain, sets = _restated(name, mixed, use_double, kc, lam_x)
        one_way = sum(1 << j for j, s in enumerate(specs) if not s[3])
        damped_mask = sum(1 << j for j, s in enumerate(specs) if s[6])
        assert ((sets & one_way) == 0).mean() >= 0.15 and ((sets & one_way) == one_way).mean() >= 0.15, (name, kc, lam_x, np.bincount(sets))
        for b in range(1, BLOCKS):
            assert sets[b * FRAMES - 1] & damped_mask and sets[b * FRAMES] & damped_mask, (name, kc, lam_x, b)
        picks = oh.side_pickups(specs)
        sc, _ = dh.device_scene(MODES, T60, renderers, use_double)
        fig = {"force": [0.0, 0.0], "out": [0.0, 0.0], "C": [0.0, 0.0], "law": [0.0, 0.0], "carry": [0.0, 0.0]}
        carry, before, before_plain, top = None, None, None, 0.0
        for b in range(BLOCKS):
            ub, (want_out, want, _, _, _, want_carry), (plain_out, plain, _, _, plain_bad, plain_carry), plain_reach = runs[b]
            out = np.zeros(FRAMES, sc.dtype)
            reads, forces, c_dev, status, carry, bad = _call(sc, "render_damped_groups", out, all_rows[b], [p for _, p in picks], specs, ub, rates, carry)
            assert list(status) == [1] * n and not bad.any() and plain_bad == 0
            for got, yard, key, ref in ((forces, plain, "force", want), (out[None, :], plain_out[None, :], "out", want_out[None, :])):
                fig[key][0] = max(fig[key][0], gh.row_figure(got, ref))
                fig[key][1] = max(fig[key][1], gh.row_figure(yard, ref))
            fig["C"][0] = max(fig["C"][0], float(np.abs((c_dev.astype(np.longdouble) - c_exact) / c_exact).max()))
            fig["C"][1] = max(fig["C"][1], float(np.abs((c_plain - c_exact) / c_exact).max()))
            is_damped = np.array([bool(s[6]) for s in specs])
            assert np.isnan(carry[~is_damped]).all() and np.isfinite(carry[is_damped]).all()
            top = max(top, float(np.abs(want_carry[is_damped]).max()))
            fig["carry"][0] = max(fig["carry"][0], float(np.abs(carry[is_damped].astype(np.longdouble) - want_carry[is_damped]).max()))
            fig["carry"][1] = max(fig["carry"][1], float(np.abs(plain_carry[is_damped].astype(np.longdouble) - want_carry[is_damped]).max()))
            reach = np.zeros((n, FRAMES), sc.dtype)
            for q, (j, _) in enumerate(picks):
                reach[j] = reach[j] + reads[q]
            law_dev, before = _law_figure(specs, lam, forces, ub, reach, before)
            law_plain, before_plain = _law_figure(specs, lam, plain, ub, plain_reach, before_plain)
            fig["law"][0], fig["law"][1] = max(fig["law"][0], law_dev), max(fig["law"][1], law_plain)
        sc.close()
        fig["carry"] = [v / top for v in fig["carry"]]
        print("%s, %s %s, K C = %g, l d = %g, %d renderers: " % ("fp64" if use_double else "fp32", name, "mixed" if mixed else "damped", kc, lam_x, renderers) +
              ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()))
        for key, (device, yardstick) in fig.items():
            assert 0 < yardstick < 1e7 * eps, (key, yardstick)  # (a yardstick that says something: the largest is 1.4e6 eps, law and carry of the four mixed members at K C = 30, l d = 10)
            assert device <= BOUND * yardstick, (name, kc, lam_x, key, device, yardstick)


# ---- 5. the carry matters ----
@PRECISIONS
def test_forgetting_the_carry_at_a_boundary_moves_the_rows(use_double):
    """The all-damped star, K C = 1, l d = 10, under the steered approach of the accuracy test: with a NaN in the carry's place ahead of
    block 1 the rows of that block leave the rows of the run that kept it by at least 10 x the bound (4 x the working-precision
    restatement's deviation from the longdouble one), on the device as in the restatement.  The factor is printed; measured: 2.5e-3 of the peak, 37 x the fp32 bound (section 3f measured 93 x or more on a lone
    junction)."""
    specs, rates, lam, all_rows, runs, _, _, _ = _restated("star", False, use_double, 1.0, 10.0)
    bound = BOUND * max(gh.row_figure(runs[b][2][1], runs[b][1][1]) for b in range(BLOCKS))
    got = {}
    for forget in ((), (1,)):
        sc, _ = dh.device_scene(MODES, T60, 1, use_double)
        carry, rows = None, []
        for b in range(2):
            if b in forget:
                carry = None
            out = np.zeros(FRAMES, sc.dtype)
            _, forces, _, status, carry, bad = _call(sc, "render_damped_groups", out, all_rows[b], [], specs, runs[b][0], rates, carry)
            assert list(status) == [1, 1, 1] and not bad.any()
            rows.append(forces.copy())
        sc.close()
        got[forget] = rows
    assert np.array_equal(got[()][0], got[(1,)][0])
    moved = gh.row_figure(got[(1,)][1], got[()][1].astype(np.longdouble))
    print("%s: forgetting the carry moves the rows by %.3e of the peak, %.0f x the bound %.3e" % ("fp64" if use_double else "fp32", moved, moved / bound, bound))
    assert moved >= 10 * bound, (moved, bound)


# ---- 6. bit-exact properties ----
@PRECISIONS
def test_a_damped_group_is_deterministic_and_local(use_double):
    (specs, rates), u = _star(use_double, mixed=True), _approach(3, FRAMES, BLOCKS)
    first, again, four = _run(use_double, specs, u, rates), _run(use_double, specs, u, rates), _run(use_double, specs, u, rates, renderers=4)
    assert (np.abs(first[0]).max(axis=1) > 0).all() and not first[4].any()
    same_carries = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[2], again[2]) and same_carries(first[5], again[5]) and _same(first[6], again[6])
    # (the block's samples are summed per renderer: with another renderer count they differ in rounding, as everywhere in the bank)
    assert np.array_equal(first[0], four[0]) and np.array_equal(first[2], four[2]) and same_carries(first[5], four[5]) and _same(first[6][1:], four[6][1:])


@PRECISIONS
def test_a_bystander_does_not_see_the_group(use_double):
    """The all-damped pair on objects 0 and 1: object 2 has the bits it has with every K = 0."""
    hertz, _, _ = _laws("pair", False)
    u = _approach(2, FRAMES, BLOCKS)
    rates = np.full(2, _rate(1.0 / FREE)[0], np.float32)
    live = _run(use_double, _specs("pair", _stiffness(_comp("pair", use_double), hertz, 10.0, [FREE] * 2), False), u, rates)
    dead = _run(use_double, _specs("pair", [0.0, 0.0], False), u, rates)
    assert (np.abs(live[0]).max(axis=1) > 0).all()
    first = sum(MODES[:2])
    for a, b in zip(live[6][1:3], dead[6][1:3]):  # the state columns
        assert np.array_equal(a[first:], b[first:]) and not np.array_equal(a[:first], b[:first])


@PRECISIONS
@pytest.mark.parametrize("frames, parts", [(128, 2), (231, 3)], ids=["128=2x64", "231=3x77"])
def test_one_block_is_its_parts_with_the_carry_passed(use_double, frames, parts):
    """The solve keeps no state but the carry: one block, and the same frames in `parts` blocks with the carry handed on, give the same
    force rows, carries and states.  77 is no multiple of the turn-around tile (32 / 16 samples)."""
    (specs, rates), u = _star(use_double, mixed=False, lam_x=3.0), _approach(3, frames, 1) + np.float32(4 * FREE)  # (raised: the members are compressed at the boundaries)
    whole = _run(use_double, specs, u, rates, blocks=1, frames=frames)
    split = _run(use_double, specs, u, rates, blocks=parts, frames=frames // parts)
    assert (np.abs(whole[0]).max(axis=1) > 0).all() and not whole[4].any() and not split[4].any()
    assert np.array_equal(whole[0], split[0]) and np.array_equal(whole[5][-1], split[5][-1]) and _same(whole[6][1:3], split[6][1:3])
    forgot = _run(use_double, specs, u, rates, blocks=parts, frames=frames // parts, forget=(1,))
    assert not np.array_equal(whole[0], forgot[0])


@PRECISIONS
def test_a_dead_group_is_the_linear_dead_group(use_double):
    """Every K = 0, or every exciter far away (u = -1e30): zero rows, status 1, and the bits of the same members, linear and undamped,
    with K = 0 through render_mixed (which the older suites tie to silent drives in their places)."""
    u = _approach(3, FRAMES, BLOCKS)
    (specs, rates), (zero, _) = _star(use_double), _star(use_double, k_scale=(0, 0, 0))
    linear = _run(use_double, [s + (False,) for s in _shape("star", [0.0] * 3)], u, rates, entry="render_mixed")
    for got in (_run(use_double, zero, u, rates), _run(use_double, specs, np.full_like(u, np.float32(-1e30)), rates)):
        assert list(got[3]) == [1, 1, 1] and not got[0].any() and not got[4].any()
        assert np.array_equal(got[2], linear[2]) and _same(got[6], linear[6])


@PRECISIONS
def test_a_member_near_with_the_others_far_acts_alone(use_double):
    (specs, rates), u = _star(use_double), _approach(3, FRAMES, BLOCKS)
    far = u.copy()
    far[1:] = np.float32(-1e30)
    lone, _ = _star(use_double, k_scale=(1, 0, 0))
    alone = _run(use_double, lone, u, rates)
    for got in (_run(use_double, specs, far, rates), _run(use_double, lone, far, rates)):
        assert list(got[3]) == [1, 1, 1] and np.abs(got[0][0]).max() > 0 and not got[0][1:].any() and not got[4].any()
        assert np.array_equal(got[0], alone[0]) and _same(got[6], alone[6])
        assert all(np.array_equal(a[:1], b[:1]) for a, b in zip(got[5], alone[5]))


# ---- 7. replay ----
@pytest.mark.parametrize("name", ["star", "chain"])
def test_the_rows_replayed_as_drives_move_the_leaves_alike(name):
    """Two identical fp32 scenes rung up by noise drives for two blocks; then three blocks in which scene A carries the all-damped group
    (single-point sides) through render_damped_groups with the carry passed on, and scene B the returned rows as drives.  An object with
    one side of one member carries one replayed row in B: its state is array_equal block after block -- the rows returned are the forces
    step 5 applied."""
    n = SIZES[name]
    hertz, _, _ = _laws(name, False)
    specs = _specs(name, _stiffness(_comp(name, False), hertz, 10.0, [FREE] * n), False, single_points=True)
    rates = np.full(n, _rate(1.0 / FREE)[0], np.float32)
    a, _ = dh.device_scene(MODES, T60, 1, False)
    b, _ = dh.device_scene(MODES, T60, 1, False)
    for blk in range(2):
        rows = _noise_rows(MODES, blk, 2, FRAMES)
        for sc in (a, b):
            sc.render_driven(np.zeros(FRAMES, np.float32), *_drive_args(rows, FRAMES))
    u = _approach(n, FRAMES, 3)
    sides = [[sd for sd in (s[0], s[1]) if sd is not None] for s in specs]
    count = {}
    for group in sides:
        for sd in group:
            count[sd[0]] = count.get(sd[0], 0) + 1
    leaves = [o for o, c in count.items() if c == 1]
    assert leaves
    starts = np.cumsum([0] + MODES)
    carry, pressed = None, np.zeros(n)
    for blk in range(3):
        out_a, out_b = np.zeros(FRAMES, np.float32), np.zeros(FRAMES, np.float32)
        _, forces, _, status, carry, bad = _call(a, "render_damped_groups", out_a, [], [], specs, u[:, blk * FRAMES:(blk + 1) * FRAMES], rates, carry)
        assert list(status) == [1] * n and not bad.any()
        pressed += (forces != 0).sum(axis=1)
        replay = [(sd[0], sd[1][0], sd[3], forces[j].astype(np.float32)) for j, group in enumerate(sides) for sd in group]
        b.render_driven(out_b, *_drive_args(replay, FRAMES))
        for o in leaves:
            for col_a, col_b in zip(_states(a), _states(b)):
                assert np.array_equal(col_a[starts[o]:starts[o + 1]], col_b[starts[o]:starts[o + 1]]), (blk, o)
    a.close()
    b.close()
    assert (pressed > 0).all(), pressed


# ---- 8. left out and refused ----
@PRECISIONS
def test_what_a_damped_group_cannot_hold_is_left_out(use_double):
    """Each kind: status 0, a zero row, C = 0, a NaN carry, and for everything else the bits of the call without that junction."""
    def run(specs, rates):
        sc, _ = dh.device_scene(MODES, T60, 1, use_double)
        out = np.zeros(FRAMES, sc.dtype)
        got = _call(sc, "render_damped_groups", out, _noise_rows(MODES, 0, 1, FRAMES), [], specs, _approach(len(specs), FRAMES, 1), rates, None)
        result = got[1:] + ([out] + _states(sc) + list(sc.object_state()),)
        sc.close()
        return result

    (star, star_rates) = _star(use_double)
    hertz4, _, _ = _laws("four", False)
    four = _specs("four", _stiffness(_comp("four", use_double), hertz4, 10.0, [FREE] * 4), False)
    d = star_rates[0]
    stray_side = gh.side(1, 0, direction=(0.0, 1.0, 0.25))
    cases = {"damped with bilateral": (star[:2], dg.spec(stray_side, None, 2e5, bilateral=True, damped=True), d),
             "a damping that is not finite": (star[:2], dg.spec(stray_side, None, 2e5, damped=True), np.float32(np.inf)),
             "a damping below 0": (star[:2], dg.spec(stray_side, None, 2e5, damped=True), np.float32(-1e-3)),
             "Hertz with bilateral": (star[:2], dg.spec(stray_side, None, 2e9, bilateral=True, hertz=True), d),
             "a fifth member": (four, dg.spec(gh.side(0, 2, direction=(1.0, 0.0, 0.0)), None, 2e5, damped=True), d),
             "a flagged junction on an unflagged one's object": ([gh.spec(gh.side(2, 1, direction=(1.0, 0.0, 0.5)), None, 1e5, shared=False) + (False,)] + star[:1], dg.spec(gh.side(2, 3, direction=(0.0, 1.0, 0.25)), None, 2e5, damped=True), d)}
    for kind, (kept, stray, rate) in cases.items():
        at = len(kept)
        forces, comp, status, carry, bad, rest = run(kept + [stray], np.array([d] * at + [rate], np.float32))
        want = run(kept, np.full(at, d, np.float32))
        assert status[at] == 0 and comp[at] == 0 and not forces[at].any() and np.isnan(carry[at]) and not bad.any(), kind
        assert list(status[:at]) == [1] * at and np.abs(forces[:at]).max() > 0, kind
        assert np.array_equal(forces[:at], want[0]) and np.array_equal(comp[:at], want[1]) and np.array_equal(carry[:at], want[3], equal_nan=True) and _same(rest, want[5]), kind
    # a ninth wave: the chain's objects take 1 + 2 + 2 = 5 waves; a third member to a fourth object of 512 modes would make them 9
    modes = MODES + [512]

    def wide(specs, rates):
        sc, _ = dh.device_scene(modes, T60, 1, use_double)
        out = np.zeros(FRAMES, sc.dtype)
        got = _call(sc, "render_damped_groups", out, _noise_rows(modes, 0, 1, FRAMES), [], specs, _approach(len(specs), FRAMES, 1), rates, None)
        result = got[1:] + ([out] + _states(sc) + list(sc.object_state()),)
        sc.close()
        return result
    hertz2, _, _ = _laws("chain", False)
    chain = _specs("chain", _stiffness(_comp("chain", use_double), hertz2, 10.0, [FREE] * 2), False)
    stray = dg.spec(gh.side(2, 0, direction=(1.0, 0.0, 0.5)), gh.side(3, 1, direction=(-1.0, 0.0, -0.5)), 2e5, damped=True)
    forces, comp, status, carry, bad, rest = wide(chain + [stray], np.full(3, d, np.float32))
    want = wide(chain, np.full(2, d, np.float32))
    assert list(status) == [1, 1, 0] and not forces[2].any() and np.isnan(carry[2])
    assert np.array_equal(forces[:2], want[0]) and np.array_equal(carry[:2], want[3]) and _same(rest, want[5])


@PRECISIONS
def test_a_refused_group_has_the_bits_of_k_0_and_nan_carries(use_double):
    """A negative coupling on both sides of the chain's second member makes its C_ii negative: with a damped member the group is refused
    whatever K is -- status 2 and a zero row on every member, C_ii returned, NaN carries, the bits of the same members, linear and
    undamped, with K = 0.  In
    fp32 an l of 1e30 puts C_ij K_j l_j out of the range the elimination needs: refused as well; fp64 solves it with finite rows."""
    def make(k, plain=False):
        specs = _specs("chain", k, False)
        a, b = specs[1][0], specs[1][1]
        if plain:
            return [dg.spec(specs[0][0], specs[0][1], specs[0][2]), dg.spec(a[:4] + (-2.0,), b[:4] + (-2.0,), specs[1][2])]
        return [specs[0], dg.spec(a[:4] + (-2.0,), b[:4] + (-2.0,), specs[1][2], hertz=specs[1][4], damped=True)]

    u = np.full((2, BLOCKS * FRAMES), 1e-5, np.float32)
    rates = np.full(2, _rate(1.0 / FREE)[0], np.float32)
    zero = _run(use_double, make([0.0, 0.0], plain=True), u, rates)
    assert list(zero[3]) == [1, 1] and zero[2][0] > 0 and zero[2][1] < 0
    refused = _run(use_double, make([1e9, 1e5]), u, rates)
    assert list(refused[3]) == [2, 2] and not refused[0].any() and np.array_equal(refused[2], zero[2]) and not refused[4].any()
    assert all(np.isnan(c).all() for c in refused[5]) and _same(refused[6], zero[6])
    hertz, _, _ = _laws("chain", False)
    chain = _specs("chain", _stiffness(_comp("chain", use_double), hertz, 10.0, [FREE] * 2), False)
    u = _approach(2, FRAMES, BLOCKS)
    huge = _run(use_double, chain, u, np.full(2, np.float32(1e30) / RATE, np.float32))
    if use_double:
        assert list(huge[3]) == [1, 1] and np.isfinite(huge[0]).all() and not huge[4].any()
    else:
        dead = _run(use_double, _specs("chain", [0.0, 0.0], False), u, rates)
        assert list(huge[3]) == [2, 2] and not huge[0].any() and all(np.isnan(c).all() for c in huge[5]) and _same(huge[6], dead[6])


# ---- 9. every junction launch in one call ----
@PRECISIONS
@pytest.mark.parametrize("renderers", [1, 4])
def test_every_junction_launch_in_one_call_is_the_four_calls_with_one_kind_each(use_double, renderers):
    """One render_damped_groups call with a lone damped Hertz junction (the first 64-mode object), a linear group of two (the 32-mode
    object), a group of two with a Hertz member (the 130-mode hub: two waves) and a group of two with a damped member (the 256-mode
    object), all exciter junctions, named in an order that interleaves the kinds; an advance-1 pickup on the object of each, and one on
    the second 64-mode object, which no junction names; noise drives on all five.  Two blocks of 40 frames with the carry passed on: 40
    frames are one full and one partial turn-around tile in fp32 (32 samples), two full and one partial in fp64 (16).
    Four further calls on fresh scenes hold one kind each, with its pickup and the same drives: every junction's force row, compliance,
    status, carry and unconverged count, and every junction-object pickup row, equal theirs bit for bit -- a launch's place behind the
    others (its groups' offset in the list, first_wave, its gain rows, the taps' indices) changes nothing."""
    frames, blocks = 40, 2
    modes = MODES + [64, 64]
    comp = _comp("four", use_double)
    four = _shape("four", [10.0 / c for c in comp])
    kinds = {"lone": [dg.spec(gh.side(3, 2, direction=(0.0, 1.0, 0.25)), None, 2e9, hertz=True, damped=True)],
             "linear": [four[0] + (False,), four[1] + (False,)],
             "hertz": [dg.spec(gh.side(1, 1, direction=groups_suite.NORMAL), None, 2e9, hertz=True), dg.spec(gh.side(1, 3, direction=(0.5, 0.5, -1.0)), None, 1e5)],
             "damped": [dg.spec(gh.side(2, 1, direction=(1.0, 0.0, 0.5)), None, 2e9, hertz=True, damped=True), dg.spec(gh.side(2, 3, direction=(0.0, 1.0, 0.25)), None, 1e5)]}
    order = [("damped", 0), ("linear", 0), ("lone", 0), ("hertz", 0), ("linear", 1), ("damped", 1), ("hertz", 1)]
    specs = [kinds[k][i] for k, i in order]
    u = _approach(len(specs), frames, blocks) + np.float32(4 * FREE)  # (raised: every member is compressed in most frames)
    rates = np.full(len(specs), _rate(1.0 / FREE)[0], np.float32)
    picked = ["damped", "linear", "lone", "hertz"]
    pickups = [oh.side_pickup(kinds[k][0][0]) for k in picked]
    off = ph.spec(4, 1, direction=(0.0, 1.0, 0.5), advance=1)
    every = _run(use_double, specs, u, rates, renderers, blocks=blocks, frames=frames, pickups=pickups + [off], modes=modes)
    assert list(every[3]) == [1] * len(specs) and (np.abs(every[0]).max(axis=1) > 0).all()
    assert (np.abs(every[1]).max(axis=1) > 0).all()
    is_damped = np.array([bool(s[6]) for s in specs])
    assert all(np.isfinite(c[is_damped]).all() and np.isnan(c[~is_damped]).all() for c in every[5])
    for kind in kinds:
        at = [j for j, (k, _) in enumerate(order) if k == kind]
        one = _run(use_double, [specs[j] for j in at], u[at], rates[at], renderers, blocks=blocks, frames=frames, pickups=[pickups[picked.index(kind)]], modes=modes)
        assert np.array_equal(every[0][at], one[0]) and np.array_equal(every[2][at], one[2]) and np.array_equal(every[3][at], one[3]), kind
        assert np.array_equal(every[4][at], one[4]) and all(np.array_equal(a[at], b, equal_nan=True) for a, b in zip(every[5], one[5])), kind
        assert np.array_equal(every[1][picked.index(kind)], one[1][0]), kind
