"""GPU tests of the contact damping of the junctions (Junction.of(..., damped=True) -> Scene.render_damped -> RenderModalDamped ->
mh_bank_render_damped -> k_bank_modes_coupled_damped; contract: include/modalhip.h, MH_JUNCTION_DAMPED).  Scenes, junctions and drives
are those of tests/test_bank_junctions_gpu.py and tests/test_bank_hertz_gpu.py with the flag set; K is chosen from the returned C and
the approach's peak x0 so that sigma = K C (Hertz: K C sqrt(x0)) takes the named values, and the damping so that l x0 does.

1. The flag selects the law: the rows of a flagged junction with l > 0 are the damped restatement's, not the undamped run's.
2. An unflagged linear or Hertz junction beside a damped one keeps its bits.
3. Dead damped junctions observe: K = 0, and u = -1e30, are zero-signal drives in the junctions' place, bit for bit.
4. Replay and the law on the device: the force rows replayed as drives give the coupled run, and f[s] is the law on the measured
   compressions of frames s + 1 and s.
5. Force rows, samples and the final carry against a numpy.longdouble restatement over three blocks with the carry passed on; with the
   carry dropped at the boundaries the run leaves the bound.
6. Determinism and locality.  7. Scaling.  8. Left out and refused.  9. The carry is the restatement's.
f is finite and >= 0 in every run of this file (_checked)."""
import numpy as np
import pytest

from tests import bank_harness as bh
from tests import damped_harness as dd
from tests import drive_harness as dh
from tests import pickup_harness as ph
from tests import test_bank_hertz_gpu as hertz_suite
from tests import test_bank_junctions_gpu as junctions_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
SHAPES = pytest.mark.parametrize("renderers,frames", [(1, 512), (4, 333)])
BOUND = junctions_suite.BOUND  # x the working-precision restatement's own deviation
FRAMES = junctions_suite.FRAMES
REST_MODES, REST_T60, NORMAL = junctions_suite.REST_MODES, junctions_suite.REST_T60, junctions_suite.NORMAL
_signal, _drive_args, _states, _same = junctions_suite._signal, junctions_suite._drive_args, junctions_suite._states, junctions_suite._same
_ring_up, _compliances = junctions_suite._ring_up, junctions_suite._compliances
_checked = hertz_suite._checked
RATE = np.float32(bh.SAMPLE_RATE)


def _rate(lam):
    """(D, l): the damping in s/m, a float, whose per-frame l = float(D) * float(sample rate) is the float nearest `lam`, and that l."""
    d = np.float32(lam) / RATE
    return float(d), np.float32(d * RATE)


def _laws(specs, hertz, damped):
    """The junction suite's specs (side a, side b, K, bilateral) with a law and a damping flag per junction."""
    return [dd.spec(s[0], s[1], s[2], s[3], h, d) for s, h, d in zip(specs, hertz, damped)]


def _stiffness(sigma, comp, x0, hertz):
    """K with K C = sigma, or K C sqrt(x0) = sigma for a Hertz junction."""
    return [sigma / (float(c) * (np.sqrt(float(x)) if h else 1.0)) for c, x, h in zip(comp, x0, hertz)]


def _damped(sc, out, rows, specs, u, lam, carry=None, pickups=()):
    """One block through render_damped: (forces, C, status, carry); lam: the per-frame l aimed at, per junction."""
    _, _, forces, comp, status, carry = sc.render_damped(out, *_drive_args(rows, len(out)), ph.records(list(pickups)), dd.records(specs), u, [_rate(v)[0] for v in lam], carry)
    return _checked(forces), comp, status, carry


def _l(lam):
    return [_rate(v)[1] for v in lam]


# ---- 5 (and 1). against longdouble, three blocks with the carry passed on ----
def _press(x0, frames, blocks):
    """Per junction an approach of peak x0 that closes the contact in the first frame of every block: within each block u falls from x0 to
    -x0 / 4 (the contact opens) and comes back to x0 / 2 by the block's end; the next block begins with a step to x0 (_against_longdouble
    then moves that one sample to x0 above the frame's free prediction), which closes the contact whatever the surface did before
    (x = u - d, and d does not see the frame's own force).  So the first frame of a block is
    solved against what the last frame of the block before left -- a compression, or a gap where the surface had bounced off: what the
    carry is for.  (A step in the block's LAST frame was tried instead: from sigma = 1 on the surface gives way within that one frame and
    the next block begins open, where a dropped carry changes nothing.)"""
    t = np.arange(frames) / float(frames)
    shape = np.where(t < 0.6, 1.0 - 1.25 * t / 0.6, -0.25 + 0.75 * (t - 0.6) / 0.4)
    return np.array([np.tile((x * shape).astype(np.float32), blocks) for x in x0])


def _pressed_scene(sc, frames, blocks):
    """(rows block by block, u) of the runs against longdouble: a noise drive on each of the three objects, and _press at x0 = 4 x the
    largest free deflection at each junction of _rest_specs over the run (from a float64 restatement without contact): the block's last
    frame, at x0 / 2, is twice that deflection inside the surface."""
    modes = REST_MODES[:3]
    all_rows = [[(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))] for b in range(blocks)]
    scout, free = dd.Restatement(sc, modes, np.float64, sc.dtype), np.zeros(2)
    for rows in all_rows:
        trace = {}
        scout.render_coupled(rows, junctions_suite._rest_specs([0.0, 0.0]), np.zeros((2, frames), np.float32), frames, trace)
        free = np.maximum(free, np.abs(trace["d"]).max(axis=1))
    return all_rows, _press(4.0 * free, frames, blocks)


def _against_longdouble(use_double, renderers, frames, sigma, lx0, comp, hertz=(False, True), blocks=3):
    """Objects of 32, 130 and 256 modes under noise drives, the two-sided junction of _rest_specs linear and damped, the one-sided one
    Hertz and damped (`hertz`).  Returns the figures {key: (device, working-precision restatement, device with the carry dropped at every
    boundary)} against the longdouble restatement -- force rows and samples over the row's peak; every block's returned carry over the
    peak of the block's row of compressions y, whose last sample it is, the largest over blocks and junctions --, the device's rows, and the share of frames in contact of the longdouble run with what it does at the boundaries."""
    modes = REST_MODES[:3]
    sc, _ = dh.device_scene(modes, REST_T60, renderers, use_double)
    cut, _ = dh.device_scene(modes, REST_T60, renderers, use_double)  # the same run with the carry replaced by NaN at each boundary
    exact, working = (dd.Restatement(sc, modes, t, sc.dtype) for t in (np.longdouble, sc.dtype))
    all_rows, u = _pressed_scene(sc, frames, blocks)
    x0 = u.max(axis=1)
    specs = _laws(junctions_suite._rest_specs(_stiffness(sigma, comp, x0, hertz)), hertz, (True, True))
    lam = [lx0 / float(x) for x in x0]
    fig = {"force": [0.0, 0.0, 0.0], "out": [0.0, 0.0, 0.0], "carry": [0.0, 0.0, 0.0]}
    contact, across, rows_out = [], [], []
    carry = {"device": None, "exact": None, "working": None}
    for b in range(blocks):
        # the block's first sample of u is chosen on the longdouble restatement: x0 above the free prediction d of that frame (one frame
        # rendered ahead and taken back), so that the block begins compressed by x0 whatever the surface is doing
        ahead, held = {}, list(exact.z)
        exact.render_damped(all_rows[b], specs, np.zeros((2, 1), np.float32), _l(lam), carry["exact"], 1, ahead)
        exact.z = held
        u[:, b * frames] = (np.asarray(ahead["d"][:, 0], np.float64) + x0).astype(np.float32)
        ub = u[:, b * frames:(b + 1) * frames]
        out, out_cut = np.zeros(frames, sc.dtype), np.zeros(frames, sc.dtype)
        forces, _, status, carry["device"] = _damped(sc, out, all_rows[b], specs, ub, lam, carry["device"])
        forces_cut, _, _, end_cut = _damped(cut, out_cut, all_rows[b], specs, ub, lam, None)
        assert list(status) == [1, 1] and np.isfinite(carry["device"]).all()
        trace = {}
        want_out, want, _, _, carry["exact"] = exact.render_damped(all_rows[b], specs, ub, _l(lam), carry["exact"], frames, trace)
        plain_out, plain, _, _, carry["working"] = working.render_damped(all_rows[b], specs, ub, _l(lam), carry["working"], frames)
        contact.append([float((np.asarray(want[j]) > 0).mean()) for j in range(2)])
        across.append([(bool(trace["y"][j][0] > 0), bool(trace["y"][j][-1] > 0)) for j in range(2)])  # compressed: y > 0 (the force may be clamped to 0 there)
        rows_out.append(forces.copy())
        for i, (f, o, c) in enumerate(((forces, out, carry["device"]), (plain, plain_out, carry["working"]), (forces_cut, out_cut, end_cut))):
            fig["force"][i] = max(fig["force"][i], dd.row_figure(f, want))
            fig["out"][i] = max(fig["out"][i], dd.row_figure(o[None, :], want_out[None, :]))
            # every block's carry, the same statistic for all three: its deviation from the longdouble carry over the peak of the block's y row
            fig["carry"][i] = max(fig["carry"][i], float((np.abs(np.asarray(c, np.longdouble) - carry["exact"]) / np.abs(trace["y"]).max(axis=1)).max()))
    sc.close()
    cut.close()
    return fig, np.concatenate(rows_out, axis=1), [float(c) for c in np.mean(contact, axis=0)], across, u


@PRECISIONS
@SHAPES
@pytest.mark.parametrize("sigma", [0.1, 1.0, 10.0, 100.0])
def test_forces_samples_and_carry_match_a_longdouble_restatement(use_double, renderers, frames, sigma):
    """Three blocks, the carry passed on, l x0 = 0.1, 1, 10, against the longdouble restatement, which is handed its own carry in longdouble
    and so runs one continuous loop.  Figures: the largest deviation of a force row / of the samples over the row's peak -- of the device,
    and of the working-precision restatement of the same run.  The carry: every block's returned carry (three blocks, two junctions, the
    three l x0: 18 values) against the longdouble restatement's, each deviation over the peak of its block's row of compressions, the
    largest of the device's 18 against the largest of the working-precision restatement's 18 -- the same statistic on both sides.  Bound:
    4 x throughout.  Every block begins compressed at both junctions (asserted on the longdouble run: its y > 0 there), so the carry enters
    the solve at every boundary, and the same device run with the carry replaced by NaN at each boundary leaves the bound.  At one or more
    of a run's four boundaries (two per junction) the frame before is compressed as well (asserted; the count is printed) -- these objects
    ring (T60 2 s) and a contact on them chatters, so it is not all four; where the frame before was open, the carry is a gap.

    Measured on an MI355X: see DESIGN.md section 3f (this test prints the figures)."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    comp = _compliances(REST_MODES[:3], REST_T60, use_double, junctions_suite._rest_specs, 2)
    carries = [0.0, 0.0]  # device, working-precision restatement: over the three runs
    for lx0 in (0.1, 1.0, 10.0):
        fig, _, contact, across, _ = _against_longdouble(use_double, renderers, frames, sigma, lx0, comp)
        carries = [max(a, b) for a, b in zip(carries, fig["carry"][:2])]
        print("%s, sigma = %g, l x0 = %g, %d renderers, %d frames: " % ("fp64" if use_double else "fp32", sigma, lx0, renderers, frames) +
              ", ".join("%s device %.3e / restatement %.3e (%.2f x), carry dropped %.3e" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf"), v[2]) for k, v in fig.items()) +
              "; in contact " + " ".join("%.2f" % c for c in contact))
        assert all(first for block in across for (first, _) in block), across  # compressed in the first frame of every block: the carry is used at every boundary
        both = sum(across[b][j][0] and across[b - 1][j][1] for b in range(1, len(across)) for j in range(2))
        print("    boundaries compressed on both sides: %d of %d" % (both, 2 * (len(across) - 1)))
        assert both > 0, across
        assert all(c > 0.05 for c in contact), contact
        for key in ("force", "out"):
            device, yardstick, _ = fig[key]
            assert 0 < yardstick < 1e6 * eps, (key, yardstick)
            assert device <= BOUND * yardstick, (lx0, key, device, yardstick)
        assert any(fig[key][2] > BOUND * fig[key][1] for key in ("force", "out")), (lx0, fig)
    print("%s, sigma = %g, %d renderers, %d frames: the 18 carries, device %.3e / restatement %.3e (%.2f x)" %
          ("fp64" if use_double else "fp32", sigma, renderers, frames, carries[0], carries[1], carries[0] / carries[1] if carries[1] else float("inf")))
    assert 0 < carries[1] < 1e6 * eps, carries
    assert carries[0] <= BOUND * carries[1], carries


@SHAPES
def test_the_flag_selects_the_law(renderers, frames):
    """The flag is what makes the law (on a tree without the feature it is ignored): sigma = 1, l x0 = 1, fp32.  The rows of the flagged
    junctions meet the damped longdouble restatement by the bound; the same junctions without the flag, through the same entry, differ from
    them in more than 5 % of the frames and miss that restatement by far more than the bound."""
    comp = _compliances(REST_MODES[:3], REST_T60, False, junctions_suite._rest_specs, 2)
    fig, rows, _, _, u = _against_longdouble(False, renderers, frames, 1.0, 1.0, comp)
    assert fig["force"][0] <= BOUND * fig["force"][1]
    # the undamped run: the same scene, K, approach and entry, the flag off
    modes = REST_MODES[:3]
    sc, _ = dh.device_scene(modes, REST_T60, renderers, False)
    exact = dd.Restatement(sc, modes, np.longdouble, sc.dtype)
    all_rows, pressed = _pressed_scene(sc, frames, 3)
    x0 = pressed.max(axis=1)
    k = _stiffness(1.0, comp, x0, (False, True))
    lam = [1.0 / float(x) for x in x0]
    plain, want, carry, carry_exact = [], [], None, None
    for b in range(3):
        rows_b = all_rows[b]
        ub = u[:, b * frames:(b + 1) * frames]
        forces, _, status, carry = _damped(sc, np.zeros(frames, sc.dtype), rows_b, _laws(junctions_suite._rest_specs(k), (False, True), (False, False)), ub, lam, carry)
        assert list(status) == [1, 1] and np.isnan(carry).all()
        plain.append(forces.copy())
        _, f, _, _, carry_exact = exact.render_damped(rows_b, _laws(junctions_suite._rest_specs(k), (False, True), (True, True)), ub, _l(lam), carry_exact, frames)
        want.append(f)
    sc.close()
    plain, want = np.concatenate(plain, axis=1), np.concatenate(want, axis=1)
    assert all((plain[j] != rows[j]).mean() > 0.05 for j in range(2))
    assert dd.row_figure(plain, want) > 100 * BOUND * fig["force"][1], (dd.row_figure(plain, want), fig)


# ---- 2. an unflagged junction beside a damped one is untouched ----
def _beside_run(use_double, renderers, frames, specs, u, lam, blocks=2):
    sc, _ = dh.device_scene(REST_MODES, REST_T60, renderers, use_double)
    _ring_up(sc, [], frames, 2)
    per_block, carry = [], None
    for blk in range(blocks):
        rows = [(3,) + dh.row_direction(3) + (_signal("sweep", 3, blocks * frames)[blk * frames:(blk + 1) * frames],)]
        forces, comp, status, carry = _damped(sc, np.zeros(frames, sc.dtype), rows, specs, u[:, blk * frames:(blk + 1) * frames], lam, carry)
        per_block.append((forces.copy(), comp.copy(), status.copy(), carry.copy()))
    cols = _states(sc)
    sc.close()
    return per_block, cols


@PRECISIONS
@SHAPES
def test_an_unflagged_junction_beside_a_damped_one_is_untouched(use_double, renderers, frames):
    """Junction 0 (one-sided, object 1) and junction 1 (two-sided, objects 0 and 2): one of them damped (linear), the other an unflagged
    linear or Hertz junction, against the same call without the damped one's flag (which launches the kernels of mh_bank_render_coupled).
    The unflagged junction's force row, C and status, its objects' states and the bystander's (object 3) are array_equal; its carry is NaN."""
    comp = _compliances(REST_MODES, REST_T60, use_double, junctions_suite._contact_specs, 2)
    u = np.array([(3e-5 * (np.sin(2 * np.pi * np.arange(2 * frames) / (400.0 + 90 * j)) + 0.1)).astype(np.float32) for j in range(2)])
    first = np.cumsum([0] + REST_MODES)
    objects_of = {0: [1], 1: [0, 2]}
    lam = [2.0 / float(x) for x in u.max(axis=1)]
    for plain in (0, 1):  # the unflagged junction: one-sided, then two-sided
        for law in (False, True):  # linear, Hertz
            hertz = tuple(law and j == plain for j in range(2))
            k = _stiffness(3.0, comp, u.max(axis=1), hertz)
            base = junctions_suite._contact_specs(k)
            both, cols_both = _beside_run(use_double, renderers, frames, _laws(base, hertz, tuple(j != plain for j in range(2))), u, lam)
            bare, cols_bare = _beside_run(use_double, renderers, frames, _laws(base, hertz, (False, False)), u, lam)
            for blk, (b, a) in enumerate(zip(both, bare)):
                assert list(b[2]) == [1, 1] and list(a[2]) == [1, 1]
                assert np.abs(b[0]).max(axis=1).min() > 0, blk  # both push
                assert np.array_equal(b[0][plain], a[0][plain]) and b[1][plain] == a[1][plain], (plain, law, blk)
                assert not np.array_equal(b[0][1 - plain], a[0][1 - plain])  # (and the damped one is damped)
                assert np.isnan(b[3][plain]) and np.isfinite(b[3][1 - plain]) and np.isnan(a[3]).all()
            for o in objects_of[plain] + [3]:
                sl = slice(first[o], first[o + 1])
                assert np.array_equal(cols_both[0][sl], cols_bare[0][sl]) and np.array_equal(cols_both[1][sl], cols_bare[1][sl]), (plain, law, o)


# ---- 3. dead damped junctions observe ----
def _run_dead(use_double, renderers, frames, variant, hertz):
    """hertz_suite._run_dead with damped junctions (l = 1e4 per frame) and the carry passed from junction block to junction block."""
    sc, _ = dh.device_scene(REST_MODES, hertz_suite.DEAD_T60, renderers, use_double)
    plan = hertz_suite.DEAD_PLAN
    blocks = len(plan)
    specs = _laws(junctions_suite._rest_specs([0.0, 0.0] if variant == "k0" else [1e9, 1e9]), (hertz, hertz), (True, True))
    sig, states, carry = np.zeros(blocks * frames, sc.dtype), [], None
    for b, kind in enumerate(plan):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in (range(4) if b < 2 else (3,))]
        out = sig[b * frames:(b + 1) * frames]
        if kind == "P":
            sc.render_driven(out, *_drive_args(rows, frames))
        elif variant == "drive":
            for s in specs:
                rows += [(sd[0], sd[1][0], sd[3], np.zeros(frames, np.float32)) for sd in (s[0], s[1]) if sd is not None]
            sc.render_driven(out, *_drive_args(rows, frames))
        else:
            u = np.array([_signal("noise", 40 + j, blocks * frames)[b * frames:(b + 1) * frames] for j in range(2)], np.float32) if variant == "k0" \
                else np.full((2, frames), -1e30, np.float32)
            forces, comp, status, carry = _damped(sc, out, rows, specs, u, [1e4, 1e4], carry)
            assert list(status) == [1, 1], (b, list(status))
            assert (forces == 0).all() and (comp > 0).all() and np.isfinite(carry).all(), b
        states.append([a.copy() for a in sc.object_state()])
    cols = _states(sc)
    sc.close()
    return sig, states, cols


@PRECISIONS
@SHAPES
def test_dead_damped_junctions_observe(use_double, renderers, frames):
    ref, ref_states, ref_cols = _run_dead(use_double, renderers, frames, "drive", False)
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    assert list(ref_states[5][2][:3]) == [0, 0, 0], ref_states[5][2]  # the junctions' objects have gone silent before the later junction blocks
    for variant in ("k0", "open"):
        for hertz in (False, True):
            got, states, cols = _run_dead(use_double, renderers, frames, variant, hertz)
            assert np.array_equal(ref, got), (variant, hertz)
            for b in range(len(hertz_suite.DEAD_PLAN)):
                assert _same(ref_states[b], states[b]), (variant, hertz, b)
            assert _same(ref_cols, cols), (variant, hertz)


# ---- 4. replay, and the law on the device ----
@SHAPES
@pytest.mark.parametrize("sigma,lx0", [(1.0, 1.0), (30.0, 10.0)])
def test_the_force_rows_replayed_as_drives_give_the_damped_run_and_meet_the_law(renderers, frames, sigma, lx0):
    """hertz_suite's replay test under damping (fp32): the one-sided junction linear and damped, the two-sided one Hertz and damped; four
    blocks with the carry passed on; the damped run and its replay array_equal in out, states and object_state().  With the advance-1
    pickups of the replay, y[s] = u[s] - sum_sides read1[s] is the measured compression of frame s + 1, and f[s] is held against
    K phi(y[s]) max(1 + l (y[s] - y[s-1]), 0) in longdouble (the run's first frame has no history: l = 0), largest deviation over the
    row's peak: device <= 4 x the same figure of the float32 restatement of the same run on its own trace."""
    T, blocks, hertz = np.float32, 4, (False, True)
    comp = _compliances(REST_MODES, REST_T60, False, junctions_suite._contact_specs, 2)
    a, _ = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    b, _ = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    working = dd.Restatement(a, REST_MODES, T, T)
    _ring_up(a, [working], frames, 2)
    _ring_up(b, [], frames, 2)
    assert _same(_states(a), _states(b))
    u = junctions_suite._approach(hertz_suite._free_deflection(a, working, hertz_suite._contact_specs([0.0, 0.0]), frames), frames, blocks, amp=1.0)
    x0 = u.max(axis=1)
    specs = _laws(junctions_suite._contact_specs(_stiffness(sigma, comp, x0, hertz)), hertz, (True, True))
    lam = [lx0 / float(x) for x in x0]
    pickups = []
    for s in specs:
        pickups += [sd + (1,) for sd in (s[0], s[1]) if sd is not None]
    carry, carry_plain = None, None
    y_dev, y_plain, f_dev, f_plain = [], [], [], []
    for blk in range(blocks):
        rows = [(3,) + dh.row_direction(3) + (_signal("sweep", 3, blocks * frames)[blk * frames:(blk + 1) * frames],)]
        ub = u[:, blk * frames:(blk + 1) * frames]
        out_a, out_b = np.zeros(frames, T), np.zeros(frames, T)
        forces, _, status, carry = _damped(a, out_a, rows, specs, ub, lam, carry)
        assert list(status) == [1, 1]
        replay = list(rows)
        for j, s in enumerate(specs):
            replay += [(o, p, d, forces[j]) for (o, p, *d) in dd.replay_drives(s)]
        reads, flags = b.render_read(out_b, *_drive_args(replay, frames), ph.records(pickups))
        assert (flags == 1).all()
        assert np.array_equal(out_a, out_b), blk
        assert _same(_states(a), _states(b)) and _same(a.object_state(), b.object_state()), blk
        read1 = [reads[0].astype(np.longdouble), reads[1].astype(np.longdouble) + reads[2].astype(np.longdouble)]
        trace = {}
        _, plain, _, _, carry_plain = working.render_damped(rows, specs, ub, _l(lam), carry_plain, frames, trace)
        y_dev.append([ub[j].astype(np.longdouble) - read1[j] for j in range(2)])
        y_plain.append([ub[j].astype(np.longdouble) - trace["read1"][j].astype(np.longdouble) for j in range(2)])
        f_dev.append(forces.copy())
        f_plain.append(plain.copy())
    a.close()
    b.close()
    device = yardstick = 0.0
    contact = []
    for j, s in enumerate(specs):
        k, l = np.longdouble(np.float32(s[2])), np.longdouble(_l(lam)[j])
        for ys, fs, which in ((y_dev, f_dev, "device"), (y_plain, f_plain, "plain")):
            y = np.concatenate([blk[j] for blk in ys])
            f = np.concatenate([blk[j] for blk in fs]).astype(np.longdouble)
            law = np.concatenate([[dd.law(y[0], 0, 0, k, s[4])], dd.law(y[1:], y[:-1], l, k, s[4])])
            figure = float(np.abs(f - law).max() / np.abs(f).max())
            if which == "device":
                device = max(device, figure)
                contact.append(float((f > 0).mean()))
            else:
                yardstick = max(yardstick, figure)
    print("the damped law on the device, sigma = %g, l x0 = %g, %d renderers, %d frames: device %.3e, float32 restatement %.3e (%.2f x); in contact %s" %
          (sigma, lx0, renderers, frames, device, yardstick, device / yardstick if yardstick else float("inf"), ["%.2f" % c for c in contact]))
    assert all(0.05 < c < 0.8 for c in contact), contact
    assert 0 < yardstick < 1e5 * float(np.finfo(np.float32).eps)
    assert device <= BOUND * yardstick, (device, yardstick)


# ---- 6, 7. determinism, locality, scaling ----
def _exact_specs(k, hertz=(False, True)):
    return _laws([s[:4] for s in hertz_suite._exact_specs(k)], hertz, (True, True))


def _exact_run(use_double, renderers, comp, bystanders=False, scale=1.0, hertz=(False, True), blocks=3, frames=FRAMES, drop=False):
    """hertz_suite._exact_run with damped junctions (the two-sided one linear, the one-sided one Hertz; sigma = 10, l x0 = 2) and the
    carry passed on.  scale: of u and of every drive, with l divided by it.  Returns (forces, carries block by block, states of objects 0 - 2)."""
    modes = [130, 64, 256] + ([37, 200, 129] if bystanders else [])
    sc, _ = dh.device_scene(modes, 0.5, renderers, use_double)
    x0 = hertz_suite.U_EXACT
    specs = _exact_specs(_stiffness(10.0, comp, [x0, x0], hertz), hertz)
    lam = [2.0 / x0 / scale] * 2
    pickups = []
    if bystanders:
        specs = [dd.spec(dd.side(4, 0, direction=NORMAL), dd.side(5, 1, direction=NORMAL), 3.0 / comp[0], damped=False)] + specs
        lam = [0.0] + lam
        pickups = [ph.spec(3, 1, direction=NORMAL, advance=1)]
    rows_f, carries, carry = [], [], None
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (np.float32(scale) * _signal("noise" if o % 2 else "sweep", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))]
        u = np.float32(scale) * np.array([(x0 * np.sin(2 * np.pi * (np.arange(frames) + b * frames) / (500.0 + 100 * (len(specs) - 1 - j)))).astype(np.float32) for j in range(len(specs))])
        forces, _, status, carry = _damped(sc, np.zeros(frames, sc.dtype), rows, specs, u, lam, None if drop else carry, pickups)
        assert (status == 1).all() and np.isfinite(carry[-2:]).all()
        rows_f.append(forces[-2:].copy())
        carries.append(carry[-2:].copy())
    n = sum(modes[:3])
    cols = [c[:n] for c in _states(sc)]
    sc.close()
    return np.concatenate(rows_f, axis=1), np.array(carries), cols


@PRECISIONS
def test_a_damped_junction_is_local_and_deterministic(use_double):
    comp = hertz_suite._exact_compliances(use_double)
    f, carries, cols = _exact_run(use_double, 1, comp)
    assert (np.abs(f).max(axis=1) > 0).all() and ((f == 0).mean(axis=1) > 0.05).all()  # both make and break
    for what, (g, k, c) in (("a second run", _exact_run(use_double, 1, comp)), ("four renderers", _exact_run(use_double, 4, comp)),
                            ("bystanders", _exact_run(use_double, 1, comp, bystanders=True)), ("bystanders, four renderers", _exact_run(use_double, 4, comp, bystanders=True))):
        assert np.array_equal(f, g) and np.array_equal(carries, k) and _same(cols, c), what
    g, _, _ = _exact_run(use_double, 1, comp, drop=True)  # (and the carry matters here)
    assert not np.array_equal(f, g)


@PRECISIONS
def test_scaling_the_excitation_by_two_with_half_the_damping_scales_the_linear_law_by_two(use_double):
    """A scene excited by drives only, both junctions linear and damped: u and every drive signal times 2 with l halved gives f, the carry
    and the states times 2, bit for bit -- the halved D is exact in float (a power of two), so is float(D) * float(rate), and then every
    operation of the closed form scales exactly (l (y - y_p), c l x, B and m are unchanged; x, r - B over 2 c l and y double)."""
    comp = hertz_suite._exact_compliances(use_double)
    f1, k1, cols1 = _exact_run(use_double, 1, comp, hertz=(False, False))
    f2, k2, cols2 = _exact_run(use_double, 1, comp, hertz=(False, False), scale=2.0)
    assert _rate(2.0 / hertz_suite.U_EXACT / 2.0)[1] * np.float32(2) == _rate(2.0 / hertz_suite.U_EXACT)[1]
    assert np.abs(f1).max() > 0 and np.array_equal(f2, f1 * 2) and np.array_equal(k2, k1 * 2)
    assert all(np.array_equal(b, a * 2) for a, b in zip(cols1, cols2))


# ---- 8, 9. left out and refused; the carry ----
def _small_run(use_double, specs, u, lam, blocks=2, modes=(64, 130, 37)):
    """hertz_suite._small_run through render_damped with the carry passed on: (out, forces, C, status, states, object_state, last carry)."""
    sc, _ = dh.device_scene(list(modes), 0.5, 1, use_double)
    out, rows_f = np.zeros(blocks * FRAMES, sc.dtype), []
    comp = status = carry = None
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(len(modes))]
        forces, comp, status, carry = _damped(sc, out[b * FRAMES:(b + 1) * FRAMES], rows, specs, u[:, b * FRAMES:(b + 1) * FRAMES], lam, carry)
        rows_f.append(forces.copy())
    result = (out, np.concatenate(rows_f, axis=1), comp, status, _states(sc), sc.object_state(), carry)
    sc.close()
    return result


def _same_run(a, b):
    return np.array_equal(a[0], b[0]) and _same(a[4], b[4]) and _same(a[5], b[5])


@PRECISIONS
@pytest.mark.parametrize("hertz", [False, True], ids=["linear", "hertz"])
def test_what_the_damped_law_cannot_take_is_left_out(use_double, hertz):
    """Status 0, a zero row, C = 0, a NaN carry and the bits of the call without the junction: damped + bilateral; l NaN, inf, below 0; a
    damped junction that would join another junction's component; a junction that would join a damped junction's component.  A lone
    damped junction with the shared flag is an ordinary damped junction."""
    good = dd.spec(dd.side(0, 1, direction=NORMAL, coupling=2.0), None, 1e9, hertz=hertz)
    u = hertz_suite._slow_sine(2)
    lam = 2.0 / 2e-5
    ref = _small_run(use_double, [good], u[:1], [lam])
    assert list(ref[3]) == [1] and np.abs(ref[1]).max() > 0 and np.isfinite(ref[6][0])
    stray = lambda bilateral: dd.spec(dd.side(1, 2, direction=(1.0, 0.5, 0.0)), dd.side(2, 0, direction=(-1.0, -0.5, 0.0)), 1e9, bilateral=bilateral, hertz=hertz)
    for bad, bad_lam in ((stray(True), lam), (stray(False), np.nan), (stray(False), np.inf), (stray(False), -1.0)):
        for specs, at, rows, lams in (([good, bad], 1, u, [lam, bad_lam]), ([bad, good], 0, u[::-1], [bad_lam, lam])):
            got = _small_run(use_double, specs, rows, lams)
            assert got[3][at] == 0 and got[2][at] == 0 and (got[1][at] == 0).all() and np.isnan(got[6][at]) and got[3][1 - at] == 1, (bad_lam, at)
            assert np.array_equal(got[1][1 - at], ref[1][0]) and got[2][1 - at] == ref[2][0] and got[6][1 - at] == ref[6][0] and _same_run(got, ref), (bad_lam, at)
    # components: the binding's records, so that the shared flag can be set
    from mesheditor_amd import bank as hipbank
    sd = lambda s: hipbank.JunctionSide.of(*s)
    a_side, b1, b2 = dd.side(0, 1, direction=NORMAL, coupling=2.0), dd.side(0, 3, direction=(1.0, 0.5, 0.0)), dd.side(1, 0, direction=(-1.0, -0.5, 0.0))  # object 0 on both

    def run(junctions, rows, lams):
        sc, _ = dh.device_scene([64, 130, 37], 0.5, 1, use_double)
        out, carry, result = np.zeros(2 * FRAMES, sc.dtype), None, None
        for b in range(2):
            drives = [(o,) + dh.row_direction(o) + (_signal("noise", o, 2 * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(3)]
            _, _, forces, comp, status, carry = sc.render_damped(out[b * FRAMES:(b + 1) * FRAMES], *_drive_args(drives, FRAMES), [], (hipbank.Junction * len(junctions))(*junctions),
                                                                rows[:, b * FRAMES:(b + 1) * FRAMES], [_rate(v)[0] for v in lams], carry)
            result = (_checked(forces), comp, status, carry)
        got = (out,) + result[:3] + (_states(sc), sc.object_state(), result[3])
        sc.close()
        return got

    lone = run([hipbank.Junction.of(sd(a_side), None, 1e9, hertz=hertz, shared=True, damped=True)], u[:1], [lam])
    assert lone[3][0] == 1 and np.array_equal(lone[1], ref[1][:, FRAMES:]) and lone[6][0] == ref[6][0] and _same_run(lone, ref)  # the flag on a lone junction changes nothing
    # a damped junction first, a shared one on its object after it: the second is left out
    got = run([hipbank.Junction.of(sd(a_side), None, 1e9, hertz=hertz, shared=True, damped=True), hipbank.Junction.of(sd(b1), sd(b2), 1e9, shared=True)], u, [lam, 0.0])
    assert list(got[3]) == [1, 0] and (got[1][1] == 0).all() and got[2][1] == 0 and np.isnan(got[6][1]) and got[6][0] == ref[6][0] and _same_run(got, ref)
    # a shared junction first, a damped one on its object after it: the damped one is left out, and the first is the call with it alone
    first = hipbank.Junction.of(sd(b1), sd(b2), 1e6, shared=True)
    alone = run([first], u[1:], [0.0])
    got = run([first, hipbank.Junction.of(sd(a_side), None, 1e9, hertz=hertz, shared=True, damped=True)], u[::-1], [0.0, lam])
    assert list(got[3]) == [1, 0] and (got[1][1] == 0).all() and got[2][1] == 0 and np.isnan(got[6]).all()
    assert np.array_equal(got[1][0], alone[1][0]) and _same_run(got, alone)


@PRECISIONS
@pytest.mark.parametrize("hertz", [False, True], ids=["linear", "hertz"])
def test_what_the_damped_law_cannot_solve_is_refused(use_double, hertz):
    """Status 2, a zero row, a NaN carry and the bits of the K = 0 call: C < 0 (a negative coupling), whatever 1 + K C is; and, in fp32,
    K C l that is not finite while K C is."""
    make = lambda k, damped, coupling=-2.0: [dd.spec(dd.side(0, 1, direction=NORMAL, coupling=coupling), dd.side(1, 2, direction=NORMAL, coupling=coupling / 2), k, False, hertz and damped, damped)]
    u = 1e-5 * np.ones((1, 2 * FRAMES), np.float32)
    zero = _small_run(use_double, make(0.0, False), u, [0.0])
    c = float(zero[2][0])
    assert zero[3][0] == 1 and c < 0
    for k in (-2.0 / c, -0.01 / c):
        got = _small_run(use_double, make(k, True), u, [1e4])
        assert got[3][0] == 2 and got[2][0] == zero[2][0] and (got[1] == 0).all() and np.isnan(got[6][0]), k
        assert _same_run(got, zero), k
    if not use_double:
        zero = _small_run(False, make(0.0, False, 2.0), u, [0.0])
        c = float(zero[2][0])
        assert c > 0
        got = _small_run(False, make(1e20 / c, True, 2.0), u, [1e30])
        assert got[3][0] == 2 and (got[1] == 0).all() and np.isnan(got[6][0]) and _same_run(got, zero)
        solved = _small_run(False, make(1e20 / c, True, 2.0), u, [1.0])
        assert solved[3][0] == 1 and np.isfinite(solved[6][0])


@PRECISIONS
@pytest.mark.parametrize("hertz", [False, True], ids=["linear", "hertz"])
def test_the_carry_and_the_rows_of_a_side_that_reads_nothing_are_the_restatements(use_double, hertz):
    """(The carry of a solve with C > 0 is held against the longdouble restatement's in
    test_forces_samples_and_carry_match_a_longdouble_restatement: the device's sums reach it in another order, so it cannot be bit-exact.)
    A zero direction vector: every gain of the side is 0, C = 0 and d = 0 exactly, so x = u and no sum stands between the device and the
    working-precision restatement: force rows and the carry are its bits (the solves' operations are correctly rounded ones and, with
    c = 0, exp2, log2 and cbrt decide nothing).  The carry is the last frame's y = u, in contact or not; with l = 0 and the flag the
    junction is solved and returns a carry as well."""
    T = np.float64 if use_double else np.float32
    specs = [dd.spec(dd.side(0, 1, direction=(0.0, 0.0, 0.0), coupling=2.0), None, 40.0, hertz=hertz)]
    u = hertz_suite._slow_sine(1, amp=0.25)
    for lam in (0.0, 6.0):
        sc, _ = dh.device_scene([64, 130, 37], 0.5, 1, use_double)
        rest = dd.Restatement(sc, [64, 130, 37], T, T)
        carry, want_carry = None, None
        for b in range(2):
            ub = u[:, b * FRAMES:(b + 1) * FRAMES]
            forces, comp, status, carry = _damped(sc, np.zeros(FRAMES, T), [], specs, ub, [lam], carry)
            _, want, _, want_status, want_carry = rest.render_damped([], specs, ub, _l([lam]), want_carry, FRAMES)
            assert status[0] == 1 and want_status[0] == 1 and comp[0] == 0
            assert np.array_equal(forces, want) and carry[0] == want_carry[0] == T(ub[0, -1]), (lam, b)
            assert (forces[0][ub[0] <= 0] == 0).all() and (forces[0] > 0).mean() > 0.3
        sc.close()


def test_one_block_against_two_halves_is_recorded():
    """Recorded, not asserted: whether one 512-frame block and two of 256 (with the carry passed on) give the same bits -- first for the
    undamped junctions, then for the damped ones."""
    comp = hertz_suite._exact_compliances(False)
    for name, damped in (("undamped", (False, False)), ("damped", (True, True))):
        runs = []
        for frames, blocks in ((512, 1), (256, 2)):
            sc, _ = dh.device_scene([130, 64, 256], 0.5, 1, False)
            x0 = hertz_suite.U_EXACT
            specs = _laws([s[:4] for s in hertz_suite._exact_specs(_stiffness(10.0, comp, [x0, x0], (False, True)))], (False, True), damped)
            rows_f, carry = [], None
            for b in range(blocks):
                rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, 512)[b * frames:(b + 1) * frames],) for o in range(3)]
                u = np.array([(x0 * np.sin(2 * np.pi * (np.arange(frames) + b * frames) / (500.0 + 100 * j))).astype(np.float32) for j in range(2)])
                forces, _, _, carry = _damped(sc, np.zeros(frames, sc.dtype), rows, specs, u, [2.0 / x0] * 2, carry)
                rows_f.append(forces.copy())
            runs.append((np.concatenate(rows_f, axis=1), _states(sc)))
            sc.close()
        print("one block of 512 against two of 256, %s: force rows %s, states %s" %
              (name, "the same bits" if np.array_equal(runs[0][0], runs[1][0]) else "differ", "the same bits" if _same(runs[0][1], runs[1][1]) else "differ"))
