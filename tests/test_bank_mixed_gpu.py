"""GPU tests of Hertz junctions in groups (Junction.of(shared=True, hertz=True) -> Scene.render_mixed -> RenderModalMixed ->
mh_bank_render_mixed -> k_bank_modes_grouped<Real, OBSERVE, true>; contract: include/modalhip.h, step 4m).

Scenes and shapes are those of tests/test_bank_groups_gpu.py: objects of 32, 130 and 256 modes, T60 2 s, noise drives; a star of three on
the 130-mode hub, a chain, four exciter junctions on the 32-mode object, two junctions between one pair.  Members all Hertz, or mixed
(even members Hertz, odd ones linear, the last linear one of the four bilateral).

1. Fails without the feature: a Hertz member of a group has status 1 and a row that is not zero through render_mixed, status 0 through
   render_observed.
2. A call without a Hertz junction in a group is render_observed bit for bit, pickups included; unconverged is all zero.
3. Force rows, samples and C_ii against the numpy.longdouble restatement (tests/mixed_harness.py) under a steered approach, and the law
   where it is solved, from advance-1 pickups at every member's sides in the same call; unconverged is 0.
4. Gating: one member near, the others far -- the bits of the call with the others at K = 0.
5. A dead group (every K = 0) has the bits of the same group of linear members with K = 0 through render_observed.
6. A second run, 1 against 4 renderers, and bystanders are bit-exact; permuting the members changes roundings only.
7. The kinds still left out have the bits of the call without them; C_ii < 0 on a Hertz member, and a C_ij K_j out of range, are refused
   with the bits of K = 0.
8. Replay: the returned rows as drives on a twin move an object with one replayed row bit for bit, the hub within rounding."""
import numpy as np
import pytest

from tests import drive_harness as dh
from tests import group_harness as gh
from tests import mixed_harness as mh
from tests import observed_harness as oh
from tests import pickup_harness as ph
from tests import test_bank_groups_gpu as groups_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
BOUND = 4  # x the working-precision restatement's own deviation: the suite's standing bound
FRAMES, BLOCKS = 128, 2
MODES, T60, SIZES = groups_suite.MODES, groups_suite.T60, groups_suite.SIZES
_shape, _drive_args, _noise_rows, _states, _same = groups_suite._shape, groups_suite._drive_args, groups_suite._noise_rows, groups_suite._states, groups_suite._same
FREE = 2e-5  # the size of a member's free deflection under the noise drives, as tests/test_bank_groups_gpu.py takes it


def _laws(name, mixed):
    """(hertz, bilateral) per member."""
    n = SIZES[name]
    hertz = [not mixed or i % 2 == 0 for i in range(n)]
    bilateral = [mixed and name == "four" and i == n - 1 for i in range(n)]
    return hertz, bilateral


def _specs(name, k, mixed):
    hertz, bilateral = _laws(name, mixed)
    plain = _shape(name, k)
    return [mh.spec(s[0], s[1], s[2], bilateral[i], hertz[i]) for i, s in enumerate(plain)]


def _stiffness(comp, hertz, kc, scale):
    """K with K C_ii sqrt(scale) = kc on a Hertz member and K C_ii = kc on a linear one."""
    return [kc / (c * np.sqrt(s)) if h else kc / c for c, h, s in zip(comp, hertz, scale)]


def _approach(n, frames, blocks, amp=3.0, period=100.0, phase=0.9):
    t = np.arange(blocks * frames)
    return np.array([(amp * FREE * (np.sin(2 * np.pi * t / period - phase * j) + 0.1)).astype(np.float32) for j in range(n)])


def _call(sc, entry, out, rows, pickups, specs, u):
    """One block through render_mixed or render_observed: (reads, forces, comp, status, unconverged)."""
    got = getattr(sc, entry)(out, *_drive_args(rows, len(out)), ph.records(list(pickups)), gh.records(specs), u)
    reads, _, forces, comp, status = got[:5]
    return reads, forces, comp, status, (got[6] if entry == "render_mixed" else np.zeros(len(specs), np.uint32))


def _run(use_double, specs, u, renderers=1, entry="render_mixed", blocks=BLOCKS, frames=FRAMES, pickups=()):
    """Noise drives on every object, the given junctions and approach rows.  Returns (forces, reads, comp, status, unconverged, [out, states, object state])."""
    sc, _ = dh.device_scene(MODES, T60, renderers, use_double)
    rows_f, rows_r, outs, counts = [], [], [], np.zeros(len(specs), np.uint64)
    for b in range(blocks):
        out = np.zeros(frames, sc.dtype)
        reads, forces, comp, status, bad = _call(sc, entry, out, _noise_rows(MODES, b, blocks, frames), list(pickups), specs, u[:, b * frames:(b + 1) * frames])
        rows_f.append(forces.copy()), rows_r.append(reads.copy()), outs.append(out)
        counts += bad
    result = np.concatenate(rows_f, axis=1), np.concatenate(rows_r, axis=1), comp, status, counts, [np.concatenate(outs)] + _states(sc) + list(sc.object_state())
    sc.close()
    return result


def _comp(name, use_double):
    return groups_suite._compliances(name, use_double)


def _hertz_star(use_double, kc=10.0, k_scale=(1, 1, 1)):
    comp = _comp("star", use_double)
    k = _stiffness(comp, [True] * 3, kc, [FREE] * 3)
    return _specs("star", [a * b for a, b in zip(k, k_scale)], False)


# ---- 1. the feature ----
@PRECISIONS
def test_a_hertz_member_of_a_group_is_solved(use_double):
    specs, u = _hertz_star(use_double), _approach(3, FRAMES, BLOCKS)
    forces, _, comp, status, bad, _ = _run(use_double, specs, u)
    assert list(status) == [1, 1, 1], list(status)
    assert (np.abs(forces).max(axis=1) > 0).all() and np.isfinite(forces).all() and (forces >= 0).all()
    assert np.array_equal(comp, _comp("star", use_double)) and not bad.any()
    old, _, _, old_status, _, _ = _run(use_double, specs, u, entry="render_observed")
    assert list(old_status) == [1, 0, 0] and not old[1:].any() and np.abs(old[0]).max() > 0


# ---- 2. the entry without a Hertz junction in a group ----
@PRECISIONS
@pytest.mark.parametrize("renderers", [1, 4])
def test_without_a_hertz_junction_in_a_group_it_is_render_observed(use_double, renderers):
    """The four linear exciter junctions on the 32-mode object (one bilateral), a lone flagged Hertz junction on the hub and an unflagged
    linear one on the 256-mode object, advance-1 pickups at every side."""
    comp = _comp("four", use_double)
    specs = _shape("four", [10.0 / c for c in comp])
    specs[3] = gh.spec(specs[3][0], None, specs[3][2], bilateral=True)
    specs += [gh.spec(gh.side(1, 3, direction=groups_suite.NORMAL), None, 2e9, hertz=True), gh.spec(gh.side(2, 1, direction=(1.0, 0.0, 0.5)), None, 1e5, shared=False)]
    u = _approach(len(specs), FRAMES, BLOCKS)
    pickups = [p for _, p in oh.side_pickups(specs)]
    new = _run(use_double, specs, u, renderers, pickups=pickups)
    old = _run(use_double, specs, u, renderers, entry="render_observed", pickups=pickups)
    assert list(new[3]) == [1] * 6 and (np.abs(new[0]).max(axis=1) > 0).sum() >= 5 and np.abs(new[1]).max() > 0
    for a, b in zip(new[:4], old[:4]):
        assert np.array_equal(a, b)
    assert _same(new[5], old[5]) and not new[4].any()


# ---- 3. accuracy, and the law where it is solved ----
_RESTATED = {}


def _restated(name, mixed, use_double, kc):
    key = (name, mixed, use_double, kc)
    if key in _RESTATED:
        return _RESTATED[key]
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    exact, working, scout = (mh.Restatement(sc, MODES, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    sc.close()
    n = SIZES[name]
    hertz, _ = _laws(name, mixed)
    all_rows = [_noise_rows(MODES, b, BLOCKS, FRAMES) for b in range(BLOCKS)]
    trace = {}
    scout.render_grouped(all_rows[0], _shape(name, [0.0] * n), np.zeros((n, FRAMES), np.float32), FRAMES, trace)  # the size of the free deflection
    scale = np.sqrt((trace["d"] ** 2).mean(axis=1))
    specs = _specs(name, _stiffness(_comp(name, use_double), hertz, kc, scale), mixed)
    C, K = exact.compliance_matrix(specs), [np.float32(s[2]) for s in specs]
    runs, touching, sets = [], [], []
    hold = 4 if n == 4 else 8  # (a round through every set of four members is 4 x 14 holds: it has to fit into the two blocks)
    for b in range(BLOCKS):
        t_exact, t_work = {}, {}
        want = exact.render_mixed(all_rows[b], specs, mh.steered(n, C, K, hertz, scale, b * FRAMES, hold), FRAMES, t_exact)
        plain = working.render_mixed(all_rows[b], specs, t_exact["u"], FRAMES, t_work)
        touching.append(t_exact["touching"])
        sets.append(t_exact["sets"])
        runs.append((t_exact["u"], want, plain, t_work["read1"]))
    c_exact = np.diag(exact.compliance_matrix(specs)).astype(np.longdouble)
    c_plain = np.diag(working.compliance_matrix(specs)).astype(np.longdouble)
    _RESTATED[key] = (specs, all_rows, runs, np.concatenate(touching), c_exact, c_plain, np.concatenate(sets))
    return _RESTATED[key]


def _law_figure(specs, forces, u, reach):
    """The largest |f - law(u - reach)| over a row's peak: reach [n][frames] is the sum of the advance-1 reads at the member's sides."""
    T = forces.dtype.type
    worst = 0.0
    for i, s in enumerate(specs):
        y = u[i].astype(T) - reach[i].astype(T)
        pos = np.where(y > 0, y, T(0))
        law = T(np.float32(s[2])) * (pos * np.sqrt(pos) if s[4] else (y if s[3] else pos))
        peak = float(np.abs(forces[i]).max())
        if peak > 0:
            worst = max(worst, float(np.abs(forces[i].astype(np.longdouble) - law.astype(np.longdouble)).max()) / peak)
    return worst


@PRECISIONS
@pytest.mark.parametrize("mixed", [False, True], ids=["hertz", "mixed"])
@pytest.mark.parametrize("name", ["star", "chain", "four", "pair"])
def test_forces_samples_and_the_law_match_a_longdouble_restatement(use_double, mixed, name):
    """K from the returned C_ii so that K C sqrt(d) (Hertz; d the rms free deflection) or K C (linear) = 1 and 30; 2 blocks of 128 frames,
    1 and 4 renderers.  The approach is steered from the longdouble run's own free prediction (tests/mixed_harness.steered): eight frames
    per active set, the empty set and the full one a quarter of the frames each.  Conditions on the inputs, asserted on the longdouble run:
    no member touches in at least 15 % of the frames, every member in at least 15 %, two or more in at least 10 %, and every active set
    of the unilateral members occurs (the per-frame masks of the longdouble run; four members are held four frames per set, not eight).
    Figures: the largest deviation of a force row / of the samples from the longdouble restatement's over the row's peak, the relative
    deviation of C_ii, and the law -- |f - K phi(u - the sum of the advance-1 reads at the member's sides)| over the row's peak -- of the
    device and of the working-precision restatement in the same run.  Bound: 4 x.  unconverged is 0 on the device and in the restatement.

    Measured on an MI355X: see DESIGN.md section 3h (this test prints the figures)."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    n = SIZES[name]
    for kc in (1.0, 30.0):
        specs, all_rows, runs, touching, c_exact, c_plain, sets = _restated(name, mixed, use_double, kc)
        bilateral = sum(1 for s in specs if s[3])
        # the steering visits every active set of the unilateral members, on the longdouble run
        one_way = sum(1 << j for j, s in enumerate(specs) if not s[3])
        seen = {int(m) & one_way for m in np.unique(sets)}
        assert seen == {m for m in range(1 << n) if m & one_way == m}, (name, kc, sorted(seen))
        assert (touching <= bilateral).mean() >= 0.15 and (touching == n).mean() >= 0.15 and (touching >= 2).mean() >= 0.10, (name, kc, np.bincount(touching))
        picks = oh.side_pickups(specs)
        for renderers in (1, 4):
            sc, _ = dh.device_scene(MODES, T60, renderers, use_double)
            fig = {"force": [0.0, 0.0], "out": [0.0, 0.0], "C": [0.0, 0.0], "law": [0.0, 0.0]}
            for b in range(BLOCKS):
                ub, (want_out, want, _, _, _), (plain_out, plain, _, _, plain_bad), plain_reach = runs[b]
                out = np.zeros(FRAMES, sc.dtype)
                reads, forces, c_dev, status, bad = _call(sc, "render_mixed", out, all_rows[b], [p for _, p in picks], specs, ub)
                assert list(status) == [1] * n and not bad.any() and plain_bad == 0
                for got, yard, key, ref in ((forces, plain, "force", want), (out[None, :], plain_out[None, :], "out", want_out[None, :])):
                    fig[key][0] = max(fig[key][0], gh.row_figure(got, ref))
                    fig[key][1] = max(fig[key][1], gh.row_figure(yard, ref))
                fig["C"][0] = max(fig["C"][0], float(np.abs((c_dev.astype(np.longdouble) - c_exact) / c_exact).max()))
                fig["C"][1] = max(fig["C"][1], float(np.abs((c_plain - c_exact) / c_exact).max()))
                reach = np.zeros((n, FRAMES), sc.dtype)
                for q, (j, _) in enumerate(picks):
                    reach[j] = reach[j] + reads[q]
                fig["law"][0] = max(fig["law"][0], _law_figure(specs, forces, ub, reach))
                fig["law"][1] = max(fig["law"][1], _law_figure(specs, plain, ub, plain_reach))
            sc.close()
            print("%s, %s %s, K C = %g, %d renderers: " % ("fp64" if use_double else "fp32", name, "mixed" if mixed else "hertz", kc, renderers) +
                  ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()) +
                  "; members touching " + " ".join("%d:%.2f" % (m, v) for m, v in enumerate(np.bincount(touching, minlength=n + 1) / len(touching))))
            for key, (device, yardstick) in fig.items():
                assert 0 < yardstick < 1e6 * eps, (key, yardstick)
                assert device <= BOUND * yardstick, (name, kc, key, device, yardstick)


# ---- 4. gating ----
@PRECISIONS
def test_a_member_near_with_the_others_far_acts_alone(use_double):
    specs, u = _hertz_star(use_double), _approach(3, FRAMES, BLOCKS)
    far = u.copy()
    far[1:] = np.float32(-1e30)
    alone = _run(use_double, _hertz_star(use_double, k_scale=(1, 0, 0)), u)
    for got in (_run(use_double, specs, far), _run(use_double, _hertz_star(use_double, k_scale=(1, 0, 0)), far)):
        assert list(got[3]) == [1, 1, 1] and np.abs(got[0][0]).max() > 0 and not got[0][1:].any() and not got[4].any()
        assert np.array_equal(got[0], alone[0]) and _same(got[5], alone[5])


# ---- 5. dead groups ----
@PRECISIONS
def test_a_dead_group_is_the_linear_dead_group(use_double):
    """Every K = 0: the free step, the sums and step 5 are section 3e's, so the bits are those of the same members, linear, with K = 0
    through render_observed (which tests/test_bank_groups_gpu.py ties to silent drives in their places); likewise with every exciter far."""
    u = _approach(3, FRAMES, BLOCKS)
    linear = _run(use_double, _shape("star", [0.0] * 3), u, entry="render_observed")
    dead = _run(use_double, _hertz_star(use_double, k_scale=(0, 0, 0)), u)
    far = _run(use_double, _hertz_star(use_double), np.full_like(u, np.float32(-1e30)))
    for got in (dead, far):
        assert list(got[3]) == [1, 1, 1] and not got[0].any() and not got[4].any()
        assert np.array_equal(got[2], linear[2]) and _same(got[5], linear[5])


# ---- 6. reproducibility ----
@PRECISIONS
def test_a_mixed_group_is_deterministic_and_local(use_double):
    comp = _comp("chain", use_double)
    hertz, _ = _laws("chain", True)
    specs = _specs("chain", _stiffness(comp, hertz, 10.0, [FREE] * 2), True)
    u = _approach(2, FRAMES, BLOCKS)
    first, again, four = _run(use_double, specs, u), _run(use_double, specs, u), _run(use_double, specs, u, renderers=4)
    assert (np.abs(first[0]).max(axis=1) > 0).all() and not first[4].any()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[2], again[2]) and _same(first[5], again[5])
    # (the block's samples are summed per renderer: with another renderer count they differ in rounding, as everywhere in the bank)
    assert np.array_equal(first[0], four[0]) and np.array_equal(first[2], four[2]) and _same(first[5][1:], four[5][1:])
    # the order of the members changes roundings only
    swapped = _run(use_double, specs[::-1], u[::-1])
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    assert gh.row_figure(swapped[0][::-1], first[0].astype(np.longdouble)) < 1e4 * eps


@PRECISIONS
def test_a_bystander_does_not_see_the_group(use_double):
    """The pair on objects 0 and 1: object 2 has the bits it has with every K = 0."""
    comp = _comp("pair", use_double)
    u = _approach(2, FRAMES, BLOCKS)
    live = _run(use_double, _specs("pair", _stiffness(comp, [True, True], 10.0, [FREE] * 2), False), u)
    dead = _run(use_double, _specs("pair", [0.0, 0.0], False), u)
    assert (np.abs(live[0]).max(axis=1) > 0).all()
    first = sum(MODES[:2])
    for a, b in zip(live[5][1:3], dead[5][1:3]):  # the state columns
        assert np.array_equal(a[first:], b[first:]) and not np.array_equal(a[:first], b[:first])


# ---- 7. left out and refused ----
@PRECISIONS
def test_what_a_mixed_group_cannot_hold_is_left_out(use_double):
    """Each kind: status 0, a zero row, C = 0, and for everything else the bits of the call without that junction."""
    def run(specs, rates=None):
        sc, _ = dh.device_scene(MODES, T60, 1, use_double)
        out = np.zeros(FRAMES, sc.dtype)
        u = _approach(len(specs), FRAMES, 1)
        got = sc.render_mixed(out, *_drive_args(_noise_rows(MODES, 0, 1, FRAMES), FRAMES), [], gh.records(specs), u, rates)
        result = (got[2], got[3], got[4], [out] + _states(sc) + list(sc.object_state()), got[6])
        sc.close()
        return result

    from mesheditor_amd import bank as hipbank
    star = _hertz_star(use_double)
    four = _specs("four", _stiffness(_comp("four", use_double), [True] * 4, 10.0, [FREE] * 4), False)
    stray_side = gh.side(1, 0, direction=(0.0, 1.0, 0.25))
    cases = {"Hertz with bilateral": (star[:2], mh.spec(stray_side, None, 2e9, bilateral=True, hertz=True), None),
             "a fifth member": (four, mh.spec(gh.side(0, 2, direction=(1.0, 0.0, 0.0)), None, 2e9, hertz=True), None)}
    for kind, (kept, stray, rates) in cases.items():
        forces, comp, status, rest, bad = run(kept + [stray], rates)
        want = run(kept)
        at = len(kept)
        assert status[at] == 0 and comp[at] == 0 and not forces[at].any() and not bad.any(), kind
        assert list(status[:at]) == [1] * at and np.abs(forces[:at]).max() > 0, kind
        assert np.array_equal(forces[:at], want[0]) and np.array_equal(comp[:at], want[1]) and _same(rest, want[3]), kind
    # a damped junction joining a group
    kept = star[:2]
    records = (hipbank.Junction * 3)(*[gh.record(s) for s in kept], hipbank.Junction.of(stray_side, None, 2e5, shared=True, damped=True))
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    out = np.zeros(FRAMES, sc.dtype)
    got = sc.render_mixed(out, *_drive_args(_noise_rows(MODES, 0, 1, FRAMES), FRAMES), [], records, _approach(3, FRAMES, 1), np.full(3, 1e-4, np.float32))
    rest = [out] + _states(sc) + list(sc.object_state())
    sc.close()
    want = run(kept)
    assert got[4][2] == 0 and not got[2][2].any() and list(got[4][:2]) == [1, 1]
    assert np.array_equal(got[2][:2], want[0]) and _same(rest, want[3])


@PRECISIONS
def test_a_negative_compliance_on_a_hertz_member_is_refused(use_double):
    """A negative coupling on both sides of the chain's second member makes its C_ii negative.  As a Hertz member of a group that is
    refused whatever K is: every member has status 2 and a zero row, C_ii is returned, and the run has the bits of the same members,
    linear, with K = 0 through render_observed."""
    def make(k, hertz):
        specs = _shape("chain", k)
        a, b, stiffness = specs[1][:3]
        return [mh.spec(specs[0][0], specs[0][1], specs[0][2], hertz=hertz), mh.spec(a[:4] + (-2.0,), b[:4] + (-2.0,), stiffness, hertz=hertz)]

    u = np.full((2, BLOCKS * FRAMES), 1e-5, np.float32)
    zero = _run(use_double, make([0.0, 0.0], False), u, entry="render_observed")
    assert list(zero[3]) == [1, 1] and zero[2][0] > 0 and zero[2][1] < 0
    refused = _run(use_double, make([1e9, 1e9], True), u)
    assert list(refused[3]) == [2, 2] and not refused[0].any() and np.array_equal(refused[2], zero[2]) and not refused[4].any()
    assert _same(refused[5], zero[5])



@PRECISIONS
def test_numbers_out_of_range_on_a_hertz_member_are_refused(use_double):
    """K = 1e30 on the chain's Hertz members: C_ij K_j is about 1e23, above the square root of float32's largest number -- refused in
    fp32 (status 2, zero rows, the bits of K = 0), inside the range and solved with finite rows in fp64.  A coupling of 1e25 on the second
    member's sides makes its C_ii some 1e18: with K = 1e5 the product leaves the range in fp32 and the group is refused, with the C_ii and
    the bits of the same call with K = 0, which is solved."""
    u = _approach(2, FRAMES, BLOCKS)
    zero = _run(use_double, _specs("chain", [0.0, 0.0], False), u)
    stiff = _run(use_double, _specs("chain", [1e30, 1e30], False), u)
    assert list(zero[3]) == [1, 1] and not stiff[4].any()
    if use_double:
        assert list(stiff[3]) == [1, 1] and np.isfinite(stiff[0]).all() and np.abs(stiff[0]).max() > 0 and all(np.isfinite(v).all() for v in stiff[5][:3])
    else:
        assert list(stiff[3]) == [2, 2] and not stiff[0].any() and np.array_equal(stiff[2], zero[2]) and _same(stiff[5], zero[5])

        def huge(k):
            specs = _specs("chain", k, False)
            a, b, stiffness = specs[1][:3]
            return [specs[0], mh.spec(a[:4] + (1e25,), b[:4] + (1e25,), stiffness, hertz=True)]
        free, pressed = _run(use_double, huge([0.0, 0.0]), u), _run(use_double, huge([1e5, 1e5]), u)
        assert list(free[3]) == [1, 1] and list(pressed[3]) == [2, 2] and not pressed[0].any() and np.array_equal(pressed[2], free[2]) and pressed[2][1] > 1e15 and _same(pressed[5], free[5])


# ---- 8. replay ----
@PRECISIONS
@pytest.mark.parametrize("mixed", [False, True], ids=["hertz", "mixed"])
@pytest.mark.parametrize("name", ["star", "chain"])
def test_the_rows_replayed_as_drives_move_the_objects_alike(use_double, mixed, name):
    """Two identical scenes rung up by noise drives for two blocks; then three blocks in which scene A carries the group (single-point
    sides) through render_mixed and nothing else, and scene B the returned rows as drives, side by side.  An object with one side of one
    member carries one replayed row in B: (z c + +0) + a f there and (z c + (+0 + f g)) here are the same bits, so its state is
    array_equal block after block -- the rows returned are the forces step 5 applied.  The hub adds its members' a_i f_i one after
    another where the drives' products are summed first: its state and the samples are compared within rounding,
    an ulp of the peak per frame."""
    n = SIZES[name]
    hertz, bilateral = _laws(name, mixed)
    plain = _shape(name, _stiffness(_comp(name, use_double), hertz, 10.0, [FREE] * n), single_points=True)
    specs = [mh.spec(s[0], s[1], s[2], bilateral[i], hertz[i]) for i, s in enumerate(plain)]
    a, _ = dh.device_scene(MODES, T60, 1, use_double)
    b, _ = dh.device_scene(MODES, T60, 1, use_double)
    T = a.dtype
    for blk in range(2):
        rows = _noise_rows(MODES, blk, 2, FRAMES)
        for sc in (a, b):
            sc.render_driven(np.zeros(FRAMES, T), *_drive_args(rows, FRAMES))
    assert _same(_states(a), _states(b))
    u = _approach(n, FRAMES, 3)
    sides = [[sd for sd in (s[0], s[1]) if sd is not None] for s in specs]
    count = {}
    for group in sides:
        for sd in group:
            count[sd[0]] = count.get(sd[0], 0) + 1
    leaves, hubs = [o for o, c in count.items() if c == 1], [o for o, c in count.items() if c > 1]
    assert leaves and hubs
    starts = np.cumsum([0] + MODES)
    eps = float(np.finfo(T).eps)
    pressed = np.zeros(n)
    for blk in range(3):
        ub = u[:, blk * FRAMES:(blk + 1) * FRAMES]
        out_a, out_b = np.zeros(FRAMES, T), np.zeros(FRAMES, T)
        got = a.render_mixed(out_a, [], np.zeros((0, FRAMES), np.float32), [], gh.records(specs), ub)
        forces, status, bad = got[2], got[4], got[6]
        assert list(status) == [1] * n and not bad.any()
        pressed += (forces != 0).sum(axis=1)
        replay = [(sd[0], sd[1][0], sd[3], forces[j].astype(np.float32)) for j, group in enumerate(sides) for sd in group]
        if use_double:  # a drive's signal is float32: a float64 row replays only where it is one
            assert T == np.float64
            forces32 = forces.astype(np.float32).astype(T)
            exact_rows = np.array_equal(forces32, forces)
        else:
            exact_rows = True
        b.render_driven(out_b, *_drive_args(replay, FRAMES))
        for o in leaves:
            for col_a, col_b in zip(_states(a), _states(b)):
                sa, sb = col_a[starts[o]:starts[o + 1]], col_b[starts[o]:starts[o + 1]]
                if exact_rows:
                    assert np.array_equal(sa, sb), (blk, o)
                else:
                    assert np.abs(sa - sb).max() <= 3 * FRAMES * float(np.finfo(np.float32).eps) * np.abs(sa).max(), (blk, o)
        tol = eps if exact_rows else float(np.finfo(np.float32).eps)
        for o in hubs:
            for col_a, col_b in zip(_states(a), _states(b)):
                sa, sb = col_a[starts[o]:starts[o + 1]], col_b[starts[o]:starts[o + 1]]
                assert np.abs(sa - sb).max() <= 3 * FRAMES * tol * np.abs(sa).max(), (blk, o)
        assert np.abs(out_a - out_b).max() <= 3 * FRAMES * tol * np.abs(out_a).max()
    a.close()
    b.close()
    assert (pressed > 0).all(), pressed
