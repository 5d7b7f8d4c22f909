"""GPU tests of the Hertz law of the contact junctions (Junction.of(..., hertz=True) -> RenderModalCoupled -> mh_bank_render_coupled ->
k_bank_modes_coupled_hertz; contract: include/modalhip.h, MH_JUNCTION_HERTZ).  Scenes, junctions and approach signals are those of
tests/test_bank_junctions_gpu.py with the flag set; K is chosen from the returned C and the approach's peak x0 so that
sigma = K C sqrt(x0) takes the named values.

1. The flag selects the law: same scene, same K, with and without it.
2. A linear junction beside a Hertz one is untouched: the linear branch of the Hertz entry against the linear entry, bit for bit.
3. Dead Hertz junctions observe: K = 0, and u = -1e30, are zero-signal drives in the junctions' place, bit for bit.
4. Replay and the law on the device: the force rows replayed as drives give the coupled run, and f[s] = K max(u[s] - read1[s], 0)^1.5.
5. Force rows, the block's samples and C against a numpy.longdouble restatement (tests/hertz_harness.py), sigma = 0.1 ... 100.
6. Determinism and locality.
7. Left out and refused: Hertz + bilateral, C < 0, C = 0, a sample of u that is not finite.
f is finite and >= 0 in every run of this file (_checked)."""
import numpy as np
import pytest

from tests import drive_harness as dh
from tests import hertz_harness as hh
from tests import pickup_harness as ph
from tests import test_bank_junctions_gpu as junctions_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
BOUND = junctions_suite.BOUND  # x the working-precision restatement's own deviation
FRAMES = junctions_suite.FRAMES
REST_MODES, REST_T60, NORMAL = junctions_suite.REST_MODES, junctions_suite.REST_T60, junctions_suite.NORMAL
_signal, _drive_args, _states, _same = junctions_suite._signal, junctions_suite._drive_args, junctions_suite._states, junctions_suite._same
_ring_up, _approach, _compliances = junctions_suite._ring_up, junctions_suite._approach, junctions_suite._compliances


def _with_law(specs, hertz):
    """The junction suite's specs (side a, side b, K, bilateral) with the law field; hertz: one flag per junction."""
    return [hh.spec(s[0], s[1], s[2], s[3], h) for s, h in zip(specs, hertz)]


def _contact_specs(stiffness, hertz=(True, True)):
    """junctions_suite._contact_specs: a one-sided junction on object 1, a two-sided one between objects 0 and 2; object 3 is a bystander."""
    return _with_law(junctions_suite._contact_specs(stiffness), hertz)


def _rest_specs(stiffness, hertz=(True, True)):
    """junctions_suite._rest_specs: a two-sided junction between objects 0 and 1 (side a blended), a one-sided one on object 2."""
    return _with_law(junctions_suite._rest_specs(stiffness), hertz)


def _stiffness(sigma, comp, x0):
    """K with K C sqrt(x0) = sigma, per junction."""
    return [sigma / (float(c) * np.sqrt(float(x))) for c, x in zip(comp, x0)]


def _checked(forces):
    assert np.isfinite(forces).all() and (forces >= 0).all()
    return forces


def _coupled(sc, out, rows, specs, u, pickups=()):
    """One coupled block: (forces, C, status), the force rows checked for f >= 0 and finite."""
    _, _, forces, comp, status = sc.render_coupled(out, *_drive_args(rows, len(out)), ph.records(list(pickups)), hh.records(specs), u)
    return _checked(forces), comp, status


def _free_deflection(sc, working, specs, frames):
    """The size of the free deflection at each contact (largest |d| of one block without contact), from a float64 restatement started at
    `working`'s state."""
    probe = hh.Restatement(sc, working.mode_counts, np.float64, working.bank_dtype)
    probe.z = [(re.astype(np.float64), im.astype(np.float64)) for re, im in working.z]
    trace = {}
    probe.render_coupled([], [hh.spec(s[0], s[1], 0.0, False, False) for s in specs], np.zeros((len(specs), frames), np.float32), frames, trace)
    return np.abs(trace["d"]).max(axis=1)


# ---- 4 (and 1). replay, and the law on the device ----
def _replay_run(renderers, frames, sigma, blocks, hertz=(True, True)):
    """Two identical fp32 scenes (a replayed row has to fit a drive's float signal), rung up by noise drives for two blocks.  Then `blocks`
    blocks in which scene A carries the two junctions of _contact_specs (and a drive on the bystander), and scene B the returned force
    rows as drives, with an advance-1 pickup on each side.
    out, every state and object_state() are array_equal block after block (asserted here).  Returns the force rows, the law's figures
    (device, yardstick: largest deviation of f[s] from K max(u[s] - sum_sides read1[s], 0)^p over the row's peak, p = 1.5 or 1, of the
    device and of the working-precision restatement of the same run) and the share of frames in contact per junction."""
    T = np.float32
    comp = _compliances(REST_MODES, REST_T60, False, junctions_suite._contact_specs, 2)
    a, _ = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    b, _ = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    working = hh.Restatement(a, REST_MODES, T, T)
    _ring_up(a, [working], frames, 2)
    _ring_up(b, [], frames, 2)
    assert _same(_states(a), _states(b))
    u = _approach(_free_deflection(a, working, _contact_specs([0.0, 0.0]), frames), frames, blocks, amp=1.0)
    specs = _contact_specs(_stiffness(sigma, comp, u.max(axis=1)), hertz)
    pickups = []
    for s in specs:
        pickups += [sd + (1,) for sd in (s[0], s[1]) if sd is not None]
    device, yardstick, contact, rows_out = 0.0, 0.0, [], []
    for blk in range(blocks):
        rows = [(3,) + dh.row_direction(3) + (_signal("sweep", 3, blocks * frames)[blk * frames:(blk + 1) * frames],)]
        ub = u[:, blk * frames:(blk + 1) * frames]
        out_a, out_b = np.zeros(frames, T), np.zeros(frames, T)
        forces, _, status = _coupled(a, out_a, rows, specs, ub)
        assert list(status) == [1, 1]
        rows_out.append(forces.copy())
        replay = list(rows)
        for j, s in enumerate(specs):
            replay += [(o, p, d, forces[j]) for (o, p, *d) in hh.replay_drives(s)]
        reads, flags = b.render_read(out_b, *_drive_args(replay, frames), ph.records(pickups))
        assert (flags == 1).all()
        assert np.array_equal(out_a, out_b), blk
        assert _same(_states(a), _states(b)) and _same(a.object_state(), b.object_state()), blk
        read1 = [reads[0].astype(np.longdouble), reads[1].astype(np.longdouble) + reads[2].astype(np.longdouble)]
        trace = {}
        _, plain, _, _ = working.render_coupled(rows, specs, ub, frames, trace)
        for j, s in enumerate(specs):
            k, p = np.longdouble(np.float32(s[2])), np.longdouble(1.5 if s[4] else 1.0)
            law_plain = k * np.maximum(ub[j].astype(np.longdouble) - trace["read1"][j].astype(np.longdouble), 0) ** p
            peak = np.abs(forces[j]).max()
            contact.append(float((forces[j] > 0).mean()))
            if peak == 0 or np.abs(plain[j]).max() == 0:  # a block the contact stays open in: nothing to hold to the law but f = 0 itself
                continue
            law = k * np.maximum(ub[j].astype(np.longdouble) - read1[j], 0) ** p
            device = max(device, float(np.abs(forces[j].astype(np.longdouble) - law).max() / peak))
            yardstick = max(yardstick, float(np.abs(plain[j].astype(np.longdouble) - law_plain).max() / np.abs(plain[j]).max()))
    a.close()
    b.close()
    return np.concatenate(rows_out, axis=1), device, yardstick, [float(np.mean(contact[j::2])) for j in range(2)]


@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
@pytest.mark.parametrize("sigma", [1.0, 30.0])
def test_the_force_rows_replayed_as_drives_give_the_coupled_run_and_meet_the_law(renderers, frames, sigma):
    """junctions_suite's replay test under the Hertz law (fp32, as there): four blocks, the
    coupled run and its replay array_equal in out, states and object_state(); with the advance-1 pickups of the replay,
    f[s] against K max(u[s] - sum_sides read1[s], 0)^1.5 in longdouble, largest deviation over the row's peak: device <= 4 x the same
    figure of the float32 restatement of the same run.  Both junctions make and break (5 % ... 80 % of the frames in contact).

    Measured on an MI355X: see DESIGN.md section 3d (this test prints the figures)."""
    _, device, yardstick, contact = _replay_run(renderers, frames, sigma, 4)
    print("the Hertz law on the device, sigma = %g, %d renderers, %d frames: device %.3e, float32 restatement %.3e (%.2f x); in contact %s" %
          (sigma, renderers, frames, device, yardstick, device / yardstick if yardstick else float("inf"), ["%.2f" % c for c in contact]))
    assert all(0.05 < c < 0.8 for c in contact), contact
    assert 0 < yardstick < 1e5 * float(np.finfo(np.float32).eps)
    assert device <= BOUND * yardstick, (device, yardstick)


# ---- 1. the flag selects the law ----
@RENDERERS
def test_the_flag_selects_the_law(renderers):
    """The replay scene with the same K, with and without the flag: both solved (asserted inside), the force rows differ, and each run's
    rows meet its own law (exponent 1.5 / 1) by the bound of the replay test."""
    hertz, dev_h, yard_h, contact_h = _replay_run(renderers, 333, 1.0, 2)
    linear, dev_l, yard_l, contact_l = _replay_run(renderers, 333, 1.0, 2, hertz=(False, False))
    print("the flag, %d renderers: Hertz device %.3e / restatement %.3e, linear device %.3e / restatement %.3e; in contact %s / %s" %
          (renderers, dev_h, yard_h, dev_l, yard_l, contact_h, contact_l))
    assert all(c > 0.05 for c in contact_h + contact_l)
    assert all((hertz[j] != linear[j]).mean() > 0.05 for j in range(2))
    assert 0 < yard_h and dev_h <= BOUND * yard_h and 0 < yard_l and dev_l <= BOUND * yard_l


# ---- 2. a linear junction beside a Hertz one is untouched ----
def _beside_run(use_double, renderers, frames, specs, keep, u, blocks=3):
    """The rung-up scene under the junctions specs[j], j in keep (u goes with the junction).  Returns per block (forces, C, status) of the
    kept junctions in keep's order, and the final state columns."""
    sc, _ = dh.device_scene(REST_MODES, REST_T60, renderers, use_double)
    _ring_up(sc, [], frames, 2)
    per_block = []
    for blk in range(blocks):
        rows = [(3,) + dh.row_direction(3) + (_signal("sweep", 3, blocks * frames)[blk * frames:(blk + 1) * frames],)]
        forces, comp, status = _coupled(sc, np.zeros(frames, sc.dtype), rows, [specs[j] for j in keep], u[list(keep), blk * frames:(blk + 1) * frames])
        per_block.append((forces.copy(), comp.copy(), status.copy()))
    cols = _states(sc)
    sc.close()
    return per_block, cols


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_a_linear_junction_beside_a_hertz_one_is_untouched(use_double, renderers, frames):
    """Junction 0 (one-sided, object 1) and junction 1 (two-sided, objects 0 and 2), one of them linear and the other Hertz, against the
    call with the linear one alone: the linear junction's force row, C and status, its objects' states and the bystander's (object 3) are
    array_equal -- the linear branch of k_bank_modes_coupled_hertz against k_bank_modes_coupled."""
    comp = _compliances(REST_MODES, REST_T60, use_double, junctions_suite._contact_specs, 2)
    u = np.array([(3e-5 * (np.sin(2 * np.pi * np.arange(3 * frames) / (400.0 + 90 * j)) + 0.1)).astype(np.float32) for j in range(2)])
    first = np.cumsum([0] + REST_MODES)
    objects_of = {0: [1], 1: [0, 2]}
    for linear in (0, 1):
        k = _stiffness(3.0, comp, u.max(axis=1))
        k[linear] = 10.0 / float(comp[linear])  # the linear one: K C = 10
        specs = _contact_specs(k, hertz=tuple(j != linear for j in range(2)))
        both, cols_both = _beside_run(use_double, renderers, frames, specs, (0, 1), u)
        alone, cols_alone = _beside_run(use_double, renderers, frames, specs, (linear,), u)
        for blk, (b, a) in enumerate(zip(both, alone)):
            assert list(b[2]) == [1, 1] and list(a[2]) == [1]
            assert np.abs(b[0]).max(axis=1).min() > 0, blk  # both push
            assert np.array_equal(b[0][linear], a[0][0]) and b[1][linear] == a[1][0], (linear, blk)
        for o in objects_of[linear] + [3]:
            sl = slice(first[o], first[o + 1])
            assert np.array_equal(cols_both[0][sl], cols_alone[0][sl]) and np.array_equal(cols_both[1][sl], cols_alone[1][sl]), (linear, o)
        o = objects_of[1 - linear][0]  # (and the Hertz junction did move its own objects)
        assert not np.array_equal(cols_both[0][first[o]:first[o + 1]], cols_alone[0][first[o]:first[o + 1]])


# ---- 3. dead Hertz junctions observe ----
DEAD_T60 = 0.01  # 480 frames: four blocks without excitation silence an object
DEAD_PLAN = "JJPPPPJJJJ"  # J: a block with the junctions (six in all); P: a plain block -- the junctions' objects fall silent in them


def _run_dead(use_double, renderers, frames, variant):
    """variant 'drive': zero-signal drives in the junctions' place; 'k0': Hertz junctions of stiffness 0 under a lively approach; 'open':
    stiff Hertz junctions whose exciter is far away (u = -1e30).  Objects 0 - 2 carry the junctions of _rest_specs and a noise drive each in
    the first two blocks; object 3 is driven throughout."""
    sc, _ = dh.device_scene(REST_MODES, DEAD_T60, renderers, use_double)
    blocks = len(DEAD_PLAN)
    specs = _rest_specs([0.0, 0.0] if variant == "k0" else [1e9, 1e9])
    sig, states, silent_before = np.zeros(blocks * frames, sc.dtype), [], []
    for b, kind in enumerate(DEAD_PLAN):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in (range(4) if b < 2 else (3,))]
        out = sig[b * frames:(b + 1) * frames]
        if kind == "J":
            silent_before.append([int(r) for r in sc.object_state()[2][:3]])
        if kind == "P":
            sc.render_driven(out, *_drive_args(rows, frames))
        elif variant == "drive":
            for s in specs:
                rows += [(sd[0], sd[1][0], sd[3], np.zeros(frames, np.float32)) for sd in (s[0], s[1]) if sd is not None]
            sc.render_driven(out, *_drive_args(rows, frames))
        else:
            u = np.array([_signal("noise", 40 + j, blocks * frames)[b * frames:(b + 1) * frames] for j in range(2)], np.float32) if variant == "k0" \
                else np.full((2, frames), -1e30, np.float32)
            forces, comp, status = _coupled(sc, out, rows, specs, u)
            assert list(status) == [1, 1], (b, list(status))
            assert (forces == 0).all() and (comp > 0).all(), b
        states.append([a.copy() for a in sc.object_state()])
    cols = _states(sc)
    sc.close()
    return sig, states, cols, silent_before


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_dead_hertz_junctions_observe(use_double, renderers, frames):
    ref, ref_states, ref_cols, ringing = _run_dead(use_double, renderers, frames, "drive")
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    assert ringing[1] == [1, 1, 1] and ringing[2] == [0, 0, 0], ringing  # junction blocks on ringing objects, and one on objects that have gone silent
    for variant in ("k0", "open"):
        got, states, cols, _ = _run_dead(use_double, renderers, frames, variant)
        assert np.array_equal(ref, got), variant
        for b in range(len(DEAD_PLAN)):
            assert _same(ref_states[b], states[b]), (variant, b)
        assert _same(ref_cols, cols), variant


# ---- 5. against longdouble ----
APPROACH_AMP, APPROACH_PERIOD = 3.0, 400.0  # of _approach (junctions_suite's own values)


def _against_longdouble(use_double, renderers, kind, sigma, comp, blocks=2, frames=FRAMES):
    sc, _ = dh.device_scene(REST_MODES[:3], REST_T60, renderers, use_double)
    modes = REST_MODES[:3]
    exact, working, scout = (hh.Restatement(sc, modes, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    all_rows = [[(o,) + dh.row_direction(o) + (_signal(kind, o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))] for b in range(blocks)]
    trace = {}
    scout.render_coupled(all_rows[0], _rest_specs([0.0, 0.0], (False, False)), np.zeros((2, frames), np.float32), frames, trace)  # the size of the free deflection
    u = _approach(np.sqrt((trace["d"] ** 2).mean(axis=1)), frames, blocks, amp=APPROACH_AMP, period=APPROACH_PERIOD)
    specs = _rest_specs(_stiffness(sigma, comp, u.max(axis=1)))
    fig = {"force": [0.0, 0.0], "out": [0.0, 0.0], "C": [0.0, 0.0]}
    contact = []
    for b in range(blocks):
        ub = u[:, b * frames:(b + 1) * frames]
        out = np.zeros(frames, sc.dtype)
        forces, c_dev, status = _coupled(sc, out, all_rows[b], specs, ub)
        assert list(status) == [1, 1]
        tuned, live, ring = sc.object_state()
        assert (ring == 1).all() and np.array_equal(tuned, live)
        want_out, want, c_want, _ = exact.render_coupled(all_rows[b], specs, ub, frames)
        plain_out, plain, c_plain, _ = working.render_coupled(all_rows[b], specs, ub, frames)
        contact.append([float((np.asarray(want[j]) > 0).mean()) for j in range(2)])
        c_exact = np.array([exact.compliance(s[:4]) for s in specs])
        for got, yard, key, ref in ((forces, plain, "force", want), (out[None, :], plain_out[None, :], "out", want_out[None, :])):
            fig[key][0] = max(fig[key][0], hh.row_figure(got, ref))
            fig[key][1] = max(fig[key][1], hh.row_figure(yard, ref))
        fig["C"][0] = max(fig["C"][0], float(np.abs((c_dev.astype(np.longdouble) - c_exact) / c_exact).max()))
        fig["C"][1] = max(fig["C"][1], float(np.abs((np.array([working.compliance(s[:4]) for s in specs]).astype(np.longdouble) - c_exact) / c_exact).max()))
    sc.close()
    return fig, [float(c) for c in np.mean(contact, axis=0)]  # per junction, over the run


@PRECISIONS
@RENDERERS
def test_forces_and_samples_match_a_longdouble_restatement(use_double, renderers):
    """junctions_suite's test of the same name under the Hertz law: objects of 32, 130 and 256 modes, a noise or swept-sine drive on each
    in every block, a two-sided junction between the first two (side a at a blend of three points) and a one-sided one on the third,
    sigma = K C sqrt(x0) = 0.1, 1, 10, 100 with x0 the approach's peak; 2 blocks of 512 frames.  The longdouble run (Newton to a fixed
    point) is in contact between 10 % and 60 % of the run's frames at either junction (asserted).  Figures: the largest deviation of a
    force row / of the block's samples from the longdouble restatement's over that row's peak, and the relative deviation of C -- of the
    device, and of the working-precision restatement (every operation rounded, numpy.cbrt, four steps) in the same run.  Bound: 4 x.

    Measured on an MI355X: see DESIGN.md section 3d (this test prints the figures)."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    comp = _compliances(REST_MODES[:3], REST_T60, use_double, junctions_suite._rest_specs, 2)
    for kind in ("noise", "sweep"):
        for sigma in (0.1, 1.0, 10.0, 100.0):
            fig, contact = _against_longdouble(use_double, renderers, kind, sigma, comp)
            print("%s, %s, sigma = %g, %d renderers: " % ("fp64" if use_double else "fp32", kind, sigma, renderers) +
                  ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()) +
                  "; in contact " + " ".join("%.2f" % c for c in contact))
            assert all(0.10 <= c <= 0.60 for c in contact), contact
            for key, (device, yardstick) in fig.items():
                assert 0 < yardstick < 1e6 * eps, (key, yardstick)
                assert device <= BOUND * yardstick, (kind, sigma, key, device, yardstick)


# ---- 6. determinism and locality ----
def _exact_specs(k):
    return [hh.spec(hh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), hh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), k[0]),
            hh.spec(hh.side(2, (3, 0, 1), (0.5, 0.25, 0.25), NORMAL, 2.0), None, k[1])]


U_EXACT = 2e-5  # the approach's amplitude in the exact runs


def _exact_compliances(use_double):
    return _compliances([130, 64, 256], 0.5, use_double, lambda k: [s[:4] for s in _exact_specs(k)], 2)


def _exact_run(use_double, renderers, comp, bystanders=False, blocks=3, frames=FRAMES):
    """Objects 0 (130 modes) and 1 (64) joined by a two-sided Hertz junction, object 2 (256) under a one-sided one, every one driven;
    sigma = 10.  bystanders: further objects with a (linear) junction, drives and a pickup of their own.  Returns (forces, states of
    objects 0 - 2)."""
    modes = [130, 64, 256] + ([37, 200, 129] if bystanders else [])
    sc, _ = dh.device_scene(modes, 0.5, renderers, use_double)
    specs = _exact_specs(_stiffness(10.0, comp, [U_EXACT, U_EXACT]))
    pickups = []
    if bystanders:
        specs = [hh.spec(hh.side(4, 0, direction=NORMAL), hh.side(5, 1, direction=NORMAL), 3.0 / comp[0], False, False)] + specs
        pickups = [ph.spec(3, 1, direction=NORMAL, advance=1)]
    rows_f = []
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise" if o % 2 else "sweep", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))]
        # (a junction's approach goes with the junction: the two under test are the last two whatever stands before them)
        u = np.array([(U_EXACT * np.sin(2 * np.pi * (np.arange(frames) + b * frames) / (500.0 + 100 * (len(specs) - 1 - j)))).astype(np.float32) for j in range(len(specs))])
        forces, _, status = _coupled(sc, np.zeros(frames, sc.dtype), rows, specs, u, pickups)
        assert (status == 1).all()
        rows_f.append(forces[-2:].copy())
    n = sum(modes[:3])
    cols = [c[:n] for c in _states(sc)]
    sc.close()
    return np.concatenate(rows_f, axis=1), cols


@PRECISIONS
def test_a_hertz_junction_is_local_and_deterministic(use_double):
    comp = _exact_compliances(use_double)
    f, cols = _exact_run(use_double, 1, comp)
    assert (np.abs(f).max(axis=1) > 0).all() and ((f == 0).mean(axis=1) > 0.05).all()  # both make and break
    for what, (g, c) in (("a second run", _exact_run(use_double, 1, comp)), ("four renderers", _exact_run(use_double, 4, comp)),
                         ("bystanders", _exact_run(use_double, 1, comp, bystanders=True)), ("bystanders, four renderers", _exact_run(use_double, 4, comp, bystanders=True))):
        assert np.array_equal(f, g) and _same(cols, c), what


@PRECISIONS
def test_objects_off_a_hertz_junction_do_not_see_its_stiffness(use_double):
    comp = _exact_compliances(use_double)
    runs = []
    for sigma in (0.0, 10.0, 1000.0):
        sc, _ = dh.device_scene([130, 64, 256, 200], 0.5, 1, use_double)
        for b in range(2):
            rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, 2 * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(4)]
            spec = _exact_specs(_stiffness(sigma, comp, [1e-5, 1e-5]))[0]
            _coupled(sc, np.zeros(FRAMES, sc.dtype), rows, [spec], 1e-5 * np.ones((1, FRAMES), np.float32))
        runs.append(_states(sc))
        sc.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0][194:], other[0][194:]) and np.array_equal(runs[0][1][194:], other[1][194:])
    assert not np.array_equal(runs[0][0][:194], runs[2][0][:194])


# ---- 7. left out and refused ----
def _small_run(use_double, specs, u, blocks=2, modes=(64, 130, 37)):
    """Objects of 64, 130 and 37 modes, each under a noise drive, and the given junctions.  Returns (out, forces, C, status, states,
    object_state) of the run; forces block after block."""
    sc, _ = dh.device_scene(list(modes), 0.5, 1, use_double)
    out, rows_f = np.zeros(blocks * FRAMES, sc.dtype), []
    comp = status = None
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(len(modes))]
        forces, comp, status = _coupled(sc, out[b * FRAMES:(b + 1) * FRAMES], rows, specs, u[:, b * FRAMES:(b + 1) * FRAMES])
        rows_f.append(forces.copy())
    result = (out, np.concatenate(rows_f, axis=1), comp, status, _states(sc), sc.object_state())
    sc.close()
    return result


def _slow_sine(n, amp=2e-5):
    return np.array([(amp * np.sin(2 * np.pi * np.arange(2 * FRAMES) / (300.0 + 50 * j))).astype(np.float32) for j in range(n)])


@PRECISIONS
def test_hertz_with_bilateral_is_left_out(use_double):
    good = hh.spec(hh.side(0, 1, direction=NORMAL, coupling=2.0), None, 1e9)
    stray = hh.spec(hh.side(1, 2, direction=(1.0, 0.5, 0.0)), hh.side(2, 0, direction=(-1.0, -0.5, 0.0)), 1e9, bilateral=True)
    u = _slow_sine(2)
    ref = _small_run(use_double, [good], u[:1])
    assert list(ref[3]) == [1] and np.abs(ref[1]).max() > 0
    for specs, at, rows in (([good, stray], 1, u), ([stray, good], 0, u[::-1])):
        out, forces, comp, status, cols, state = _small_run(use_double, specs, rows)
        assert status[at] == 0 and comp[at] == 0 and (forces[at] == 0).all() and status[1 - at] == 1
        assert np.array_equal(forces[1 - at], ref[1][0]) and comp[1 - at] == ref[2][0]
        assert np.array_equal(out, ref[0]) and _same(cols, ref[4]) and _same(state, ref[5])


@PRECISIONS
def test_a_hertz_junction_with_negative_compliance_is_refused(use_double):
    """A negative coupling makes C negative: status 2, a zero row and the bits of the K = 0 call -- with K = -2 / C, and with K = -0.01 / C,
    where 1 + K C = 0.99 > 0 and the linear law solves."""
    make = lambda k, hertz: [hh.spec(hh.side(0, 1, direction=NORMAL, coupling=-2.0), hh.side(1, 2, direction=NORMAL, coupling=-1.0), k, False, hertz)]
    u = 1e-5 * np.ones((1, 2 * FRAMES), np.float32)
    zero = _small_run(use_double, make(0.0, False), u)
    c = float(zero[2][0])
    assert zero[3][0] == 1 and c < 0
    for k in (-2.0 / c, -0.01 / c):
        out, forces, comp, status, cols, state = _small_run(use_double, make(k, True), u)
        assert status[0] == 2 and comp[0] == zero[2][0] and (forces == 0).all(), k
        assert np.array_equal(out, zero[0]) and _same(cols, zero[4]) and _same(state, zero[5]), k
    linear = _small_run(use_double, make(-0.01 / c, False), u)
    assert linear[3][0] == 1 and np.abs(linear[1]).max() > 0
    k0 = _small_run(use_double, make(0.0, True), u)  # K = 0 with C < 0: refused as well, and the same bits
    assert k0[3][0] == 2 and np.array_equal(k0[0], zero[0]) and _same(k0[4], zero[4])


@PRECISIONS
def test_a_side_that_reads_nothing_is_solved_with_the_rigid_law(use_double):
    """A zero direction vector: every gain of the side is 0, C = 0 exactly, d = 0, and the solve returns f = K x^1.5 with x = u -- three
    roundings (K y, sqrt, their product): within 2 eps of the longdouble value.  The force moves nothing (a = 0): the bits of the K = 0 call."""
    T = np.float64 if use_double else np.float32
    make = lambda k: [hh.spec(hh.side(0, 1, direction=(0.0, 0.0, 0.0), coupling=2.0), None, k)]
    u = _slow_sine(1, amp=0.25)
    out, forces, comp, status, cols, state = _small_run(use_double, make(40.0), u)
    assert status[0] == 1 and comp[0] == 0
    x = np.maximum(u[0].astype(np.longdouble), 0)
    want = np.longdouble(40.0) * x * np.sqrt(x)
    assert (forces[0][u[0] <= 0] == 0).all() and (want > 0).mean() > 0.3
    closed = want > 0
    assert float((np.abs(forces[0].astype(np.longdouble) - want)[closed] / want[closed]).max()) <= 2 * float(np.finfo(T).eps)
    zero = _small_run(use_double, make(0.0), u)
    assert np.array_equal(out, zero[0]) and _same(cols, zero[4]) and _same(state, zero[5])


@PRECISIONS
def test_a_sample_of_the_approach_that_is_not_finite_counts_as_zero(use_double):
    comp = _compliances([64, 130, 37], 0.5, use_double, lambda k: [s[:4] for s in _pair(k)], 1)
    u = _slow_sine(1) + np.float32(1e-5)
    specs = _pair(_stiffness(3.0, comp, u.max(axis=1)))
    holes = u.copy()
    holes[0, 5::7] = 0
    ref = _small_run(use_double, specs, holes)
    assert ref[3][0] == 1 and np.abs(ref[1]).max() > 0
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        holes[0, 5 + 7 * i::21] = bad
    got = _small_run(use_double, specs, holes)
    assert not np.isfinite(holes).all() and got[3][0] == 1
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0]) and _same(got[4], ref[4])


def _pair(k):
    return [hh.spec(hh.side(0, 1, direction=NORMAL, coupling=2.0), hh.side(1, 2, direction=(-0.25, 1.0, -0.5), coupling=1.0), k[0])]
