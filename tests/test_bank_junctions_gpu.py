"""GPU tests of contact junctions (Scene.render_coupled -> RenderModalCoupled -> mh_bank_render_coupled -> k_bank_modes_coupled).

1. No junction, no change: render_coupled without junctions is render_read, bit for bit, over the 72-block scenes of the drive tests.
2. A dead junction is an observer: K = 0, and separately u = -1e30 (unilateral), give a zero force row, and the run is bit for bit the
   run with a zero-signal drive on each side's object in the junction's place, whatever else excites the objects.
3. Replay (fp32): the returned force rows, passed as drives through render_driven on a second identical scene, reproduce the coupled run
   bit for bit.  (In the replayed blocks the junctions' objects carry no other row: the contract adds a*f to the stepped state,
   (z c + e) + a f, a drive joins the excitation sum, z c + (e + a f) -- the same bits exactly when e is +0.)
4. The law holds on the device: with an advance-1 pickup per side in that replay, f[s] = K max(u[s] - sum_sides read1[s], 0).
5. Force rows, the block's samples and C against a numpy.longdouble restatement (tests/junction_harness.py), K C = 0.1 ... 100.
6. Exact properties: scaling by 2, renderer count, a second run, bystanders, a mirrored pair.
7. What cannot be solved is left out or refused; pickups on a side's object are left out; a live retune reaches C."""
import numpy as np
import pytest

from tests import bank_harness as bh
from tests import drive_harness as dh
from tests import junction_harness as jh
from tests import pickup_harness as ph
from tests import test_bank_drives_gpu as drives_suite
from tests import test_bank_pickups_gpu as pickups_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
BOUND = 4  # x the working-precision restatement's own deviation: the project's bound for drives and pickups
FRAMES = 512
_signal = drives_suite._signal


def _drive_args(rows, frames):
    """(drives, signals) of restatement rows (object, ex_pos, direction, signal)."""
    return [(o, p) + tuple(float(v) for v in d) for (o, p, d, f) in rows], np.array([f for (_, _, _, f) in rows], np.float32).reshape(len(rows), frames)


def _states(sc):
    return [sc.column("StateRe"), sc.column("StateIm")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. no junction, no change ----
def _run_mixed(use_double, renderers, frames, blocks, coupled):
    """The 'mixed' run of the drive tests with 1 + (object % 10) pickups on every object, through render_read or through render_coupled
    with an empty junction list."""
    from mesheditor_amd import bank as hipbank
    sc, slots = dh.device_scene(drives_suite.MODES, drives_suite.T60, renderers, use_double)
    probes = ph.records([pickups_suite._some_pickup(slots[o], i) for o in range(len(slots)) for i in range(1 + o % 10)])
    sig, states, reads = np.zeros(blocks * frames, sc.dtype), [], []
    for b in range(blocks):
        drives, signals, seen = [], [], set()
        for (o, p, d, gamma) in drives_suite._rows_of(b):
            if o not in seen:
                assert sc.enqueue(dh.one_sample_impact(hipbank.Event, slots[o], p, d, gamma))
            else:
                drives.append((slots[o], p) + tuple(float(v) for v in d))
                signals.append(dh.impulse_row(gamma, frames))
            seen.add(o)
        out = sig[b * frames:(b + 1) * frames]
        signals = np.array(signals, np.float32).reshape(len(drives), frames)
        if coupled:
            got = sc.render_coupled(out, drives, signals, probes, [], np.zeros((0, frames), np.float32))
            assert got[2].shape == (0, frames) and len(got[3]) == 0 and len(got[4]) == 0
        else:
            got = sc.render_read(out, drives, signals, probes)
        reads.append((got[0].copy(), got[1].copy()))
        states.append([a.copy() for a in sc.object_state()])
    cols = _states(sc)
    sc.close()
    return sig, states, cols, reads


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_no_junction_no_change(use_double, renderers, frames):
    blocks = drives_suite.BLOCKS
    ref, ref_states, ref_cols, ref_reads = _run_mixed(use_double, renderers, frames, blocks, False)
    assert np.abs(ref).max() > 0 and max(np.abs(r).max() for r, _ in ref_reads) > 0
    got, states, cols, reads = _run_mixed(use_double, renderers, frames, blocks, True)
    assert np.array_equal(ref, got)
    for b in range(blocks):
        assert _same(ref_states[b], states[b]) and _same(ref_reads[b], reads[b]), b
    assert _same(ref_cols, cols)


# ---- 2. a dead junction is an observer ----
# Objects of the drive tests' scene (rows per object 1, 2, 3, 8, 5, 12, 14, 10, 4, 2; modes 64, 37, 130, 256, 300, 128, 64, 200, 8, 129): junctions on
# objects with 14 and 4, 8, 5 and 2, 2, and 1 further rows in the excited blocks and 0 in the others; objects 2, 5 and 7 stay in the main launch.
DEAD = [jh.spec(jh.side(6, 1, direction=(1.0, 0.5, 0.25)), jh.side(8, 2, direction=(-1.0, -0.5, -0.25)), 1.0),
        jh.spec(jh.side(3, 0, direction=(0.25, -1.0, 0.5), coupling=2.0), None, 1.0),
        jh.spec(jh.side(4, 3, direction=(0.5, 0.5, -1.0)), jh.side(9, 1, direction=(-0.5, -0.5, 1.0)), 1.0),
        jh.spec(jh.side(1, 2, direction=(0.0, 1.0, 0.0)), None, 1.0),
        jh.spec(jh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.0, -0.5)), None, 1.0)]
JUNCTION_ON = {0, 1, 2, 14, 15, 30, 56, 57, 58}  # with the strikes, after them, on objects that have gone silent, and not at all in between


def _run_dead(use_double, renderers, frames, blocks, variant):
    """variant 'drive': zero-signal drives in the junctions' place; 'k0': junctions of stiffness 0 under a lively approach signal; 'open':
    stiff junctions whose exciter is far away (u = -1e30, unilateral)."""
    from mesheditor_amd import bank as hipbank
    sc, slots = dh.device_scene(drives_suite.MODES, drives_suite.T60, renderers, use_double)
    assert slots == list(range(len(slots)))
    junctions = [jh.spec(a, b, 0.0 if variant == "k0" else 1e4) for (a, b, _, _) in DEAD]
    sig, states = np.zeros(blocks * frames, sc.dtype), []
    for b in range(blocks):
        drives, signals, seen = [], [], set()
        for (o, p, d, gamma) in drives_suite._rows_of(b):
            if o not in seen:
                assert sc.enqueue(dh.one_sample_impact(hipbank.Event, slots[o], p, d, gamma))
            else:
                drives.append((slots[o], p) + tuple(float(v) for v in d))
                signals.append(dh.impulse_row(gamma, frames))
            seen.add(o)
        out = sig[b * frames:(b + 1) * frames]
        if b not in JUNCTION_ON:
            sc.render_driven(out, drives, np.array(signals, np.float32).reshape(len(drives), frames))
        elif variant == "drive":
            for s in junctions:
                for v in jh.replay_drives((s[0][:2] + ((1.0, 0.0, 0.0),) + s[0][3:], None if s[1] is None else s[1][:2] + ((1.0, 0.0, 0.0),) + s[1][3:])):
                    drives.append(v)
                    signals.append(np.zeros(frames, np.float32))
            sc.render_driven(out, drives, np.array(signals, np.float32).reshape(len(drives), frames))
        else:
            u = np.array([_signal("noise", 40 + j, blocks * frames)[b * frames:(b + 1) * frames] for j in range(len(junctions))], np.float32) if variant == "k0" \
                else np.full((len(junctions), frames), -1e30, np.float32)
            _, _, forces, comp, status = sc.render_coupled(out, drives, np.array(signals, np.float32).reshape(len(drives), frames), [], jh.records(junctions), u)
            assert list(status) == [1] * len(junctions), (b, list(status))
            assert (forces == 0).all() and (comp > 0).all(), b
        states.append([a.copy() for a in sc.object_state()])
    cols = _states(sc)
    sc.close()
    return sig, states, cols


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_a_dead_junction_is_an_observer(use_double, renderers, frames):
    blocks = drives_suite.BLOCKS
    ref, ref_states, ref_cols = _run_dead(use_double, renderers, frames, blocks, "drive")
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    ring = np.array([s[2] for s in ref_states])
    assert any((s[1][s[2] != 0] < s[0][s[2] != 0]).any() for s in ref_states)  # culling ...
    assert ((ring[:-1] == 1) & (ring[1:] == 0)).any() and ((ring[:-1] == 0) & (ring[1:] == 1)).any()  # ... silence and re-excitation
    for variant in ("k0", "open"):
        got, states, cols = _run_dead(use_double, renderers, frames, blocks, variant)
        bad = np.flatnonzero(ref != got)
        assert np.array_equal(ref, got), (variant, len(bad), bad[:4])
        for b in range(blocks):
            assert _same(ref_states[b], states[b]), (variant, b)
        assert _same(ref_cols, cols), variant


# ---- 3, 4. replay, and the law on the device ----
REST_MODES, REST_T60 = [32, 130, 256, 64], 2.0
NORMAL = (0.25, -1.0, 0.5)


def _contact_specs(stiffness):
    """A one-sided junction on object 1 and a two-sided one between objects 0 and 2 (side b pushed the opposite way); object 3 is a bystander."""
    return [jh.spec(jh.side(1, 2, direction=NORMAL, coupling=2.0), None, stiffness[0]),
            jh.spec(jh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), jh.side(2, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), stiffness[1], False)]


def _compliances(modes, t60, use_double, make_specs, n):
    """The C each junction of make_specs(stiffnesses) returns, from a scene of its own (one block with K = 0)."""
    sc, _ = dh.device_scene(modes, t60, 1, use_double)
    _, _, _, comp, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), [], np.zeros((0, FRAMES), np.float32), [], jh.records(make_specs([0.0] * n)), np.zeros((n, FRAMES), np.float32))
    sc.close()
    assert (status == 1).all() and (comp > 0).all(), (status, comp)
    return comp


def _approach(free, frames, blocks, amp=3.0, period=400.0):
    """A slow sine per junction, `amp` times its free deflection `free` and raised a little: the exciter dips in and out of the surface.
    (A stiff contact pushes the surface away and closes for a shorter time than a soft one: with these numbers the restatement of test 5
    is in contact for 15 % ... 43 % of the frames over K C = 0.1 ... 100.)"""
    t = np.arange(blocks * frames)
    return np.array([(amp * a * (np.sin(2 * np.pi * t / (period + 90 * j)) + 0.1)).astype(np.float32) for j, a in enumerate(free)])


def _ring_up(sc, rest, frames, blocks):
    """Noise drives on every object for `blocks` blocks (render_driven; the same on the restatements): what the junctions then act on."""
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(REST_MODES))]
        sc.render_driven(np.zeros(frames, sc.dtype), *_drive_args(rows, frames))
        for r in rest:
            r.render_coupled(rows, [], np.zeros((0, frames), np.float32), frames)


@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
@pytest.mark.parametrize("kc", [1.0, 30.0])
def test_the_force_rows_replayed_as_drives_give_the_coupled_run_and_meet_the_law(renderers, frames, kc):
    """Two identical fp32 scenes, rung up by noise drives for two blocks.  Then four blocks in which scene A carries the two junctions (and a
    drive on the bystander), and scene B the returned force rows as drives: side a at its point along its direction, side b at its point
    along its own (opposite) direction.  out, every state and object_state() are array_equal block after block.  In scene B an advance-1
    pickup sits on each side (same point, direction and coupling): f[s] against K max(u[s] - sum_sides read1[s], 0), largest deviation
    over the row's peak, against the same figure of the float32 restatement of the same run (bound 4 x)."""
    comp = _compliances(REST_MODES, REST_T60, False, _contact_specs, 2)
    specs = _contact_specs([kc / c for c in comp])
    a, slots = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    b, _ = dh.device_scene(REST_MODES, REST_T60, renderers, False)
    working = jh.Restatement(a, REST_MODES, np.float32, np.float32)
    _ring_up(a, [working], frames, 2)
    _ring_up(b, [], frames, 2)
    assert _same(_states(a), _states(b))
    # the size of the free deflection at each contact: the restatement's prediction of the first coupled frame's neighbourhood
    probe = jh.Restatement(a, REST_MODES, np.float64, np.float32)
    probe.z = [(re.astype(np.float64), im.astype(np.float64)) for re, im in working.z]
    trace = {}
    probe.render_coupled([], [jh.spec(s[0], s[1], 0.0) for s in specs], np.zeros((2, frames), np.float32), frames, trace)
    u = _approach(np.abs(trace["d"]).max(axis=1), frames, 4, amp=1.0)
    pickups = []
    for s in specs:
        pickups += [sd + (1,) for sd in (s[0], s[1]) if sd is not None]
    device, yardstick, contact = 0.0, 0.0, []
    for blk in range(4):
        rows = [(3,) + dh.row_direction(3) + (_signal("sweep", 3, 4 * frames)[blk * frames:(blk + 1) * frames],)]
        ub = u[:, blk * frames:(blk + 1) * frames]
        out_a, out_b = np.zeros(frames, np.float32), np.zeros(frames, np.float32)
        _, _, forces, _, status = a.render_coupled(out_a, *_drive_args(rows, frames), [], jh.records(specs), ub)
        assert list(status) == [1, 1]
        replay = list(rows)
        for j, s in enumerate(specs):
            replay += [(o, p, d, forces[j]) for (o, p, *d) in jh.replay_drives(s)]
        reads, flags = b.render_read(out_b, *_drive_args(replay, frames), ph.records(pickups))
        assert (flags == 1).all()
        assert np.array_equal(out_a, out_b), blk
        assert _same(_states(a), _states(b)) and _same(a.object_state(), b.object_state()), blk
        trace = {}
        _, plain, _, _ = working.render_coupled(rows, specs, ub, frames, trace)
        read1 = [reads[0].astype(np.longdouble), reads[1].astype(np.longdouble) + reads[2].astype(np.longdouble)]
        for j, s in enumerate(specs):
            k = np.longdouble(np.float32(s[2]))
            law = k * np.maximum(ub[j].astype(np.longdouble) - read1[j], 0)
            law_plain = k * np.maximum(ub[j].astype(np.longdouble) - trace["read1"][j].astype(np.longdouble), 0)
            peak = np.abs(forces[j]).max()
            contact.append(float((forces[j] > 0).mean()))
            if peak == 0 or np.abs(plain[j]).max() == 0:  # a block the contact stays open in: nothing to hold to the law but f = 0 itself
                continue
            device = max(device, float(np.abs(forces[j].astype(np.longdouble) - law).max() / peak))
            yardstick = max(yardstick, float(np.abs(plain[j].astype(np.longdouble) - law_plain).max() / np.abs(plain[j]).max()))
    a.close()
    b.close()
    print("the law on the device, K C = %g, %d renderers, %d frames: device %.3e, float32 restatement %.3e (%.2f x); in contact %s" %
          (kc, renderers, frames, device, yardstick, device / yardstick, ["%.2f" % c for c in contact]))
    assert 0.05 < np.mean(contact[0::2]) < 0.8 and 0.05 < np.mean(contact[1::2]) < 0.8  # both junctions make and break
    assert 0 < yardstick < 1e5 * float(np.finfo(np.float32).eps)
    assert device <= BOUND * yardstick, (device, yardstick)


# ---- 5. against longdouble ----
def _rest_specs(stiffness):
    """A two-sided junction between objects 0 (32 modes) and 1 (130), one point blended, and a one-sided one on object 2 (256)."""
    return [jh.spec(jh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.5, -0.25), 1.5), jh.side(1, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5), stiffness[0]),
            jh.spec(jh.side(2, 1, direction=NORMAL, coupling=2.0), None, stiffness[1])]


def _against_longdouble(use_double, renderers, kind, kc, comp, blocks=2, frames=FRAMES):
    sc, slots = dh.device_scene(REST_MODES[:3], REST_T60, renderers, use_double)
    modes = REST_MODES[:3]
    exact, working, scout = (jh.Restatement(sc, modes, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    specs = _rest_specs([kc / c for c in comp])
    all_rows = [[(o,) + dh.row_direction(o) + (_signal(kind, o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))] for b in range(blocks)]
    trace = {}
    scout.render_coupled(all_rows[0], [jh.spec(s[0], s[1], 0.0) for s in specs], np.zeros((2, frames), np.float32), frames, trace)  # the size of the free deflection
    u = _approach(np.sqrt((trace["d"] ** 2).mean(axis=1)), frames, blocks)
    fig = {"force": [0.0, 0.0], "out": [0.0, 0.0], "C": [0.0, 0.0]}
    contact = []
    for b in range(blocks):
        ub = u[:, b * frames:(b + 1) * frames]
        out = np.zeros(frames, sc.dtype)
        _, _, forces, c_dev, status = sc.render_coupled(out, *_drive_args(all_rows[b], frames), [], jh.records(specs), ub)
        assert list(status) == [1, 1]
        tuned, live, ring = sc.object_state()
        assert (ring == 1).all() and np.array_equal(tuned, live)
        want_out, want, c_want, _ = exact.render_coupled(all_rows[b], specs, ub, frames)
        plain_out, plain, c_plain, _ = working.render_coupled(all_rows[b], specs, ub, frames)
        contact.append([float((np.asarray(want[j]) > 0).mean()) for j in range(2)])
        c_exact = np.array([exact.compliance(s) for s in specs])
        for got, yard, key, ref in ((forces, plain, "force", want), (out[None, :], plain_out[None, :], "out", want_out[None, :])):
            fig[key][0] = max(fig[key][0], jh.row_figure(got, ref))
            fig[key][1] = max(fig[key][1], jh.row_figure(yard, ref))
        fig["C"][0] = max(fig["C"][0], float(np.abs((c_dev.astype(np.longdouble) - c_exact) / c_exact).max()))
        fig["C"][1] = max(fig["C"][1], float(np.abs((np.array([working.compliance(s) for s in specs]).astype(np.longdouble) - c_exact) / c_exact).max()))
    sc.close()
    return fig, [float(c) for c in np.mean(contact, axis=0)]  # per junction, over the run


@PRECISIONS
@RENDERERS
def test_forces_and_samples_match_a_longdouble_restatement(use_double, renderers):
    """Objects of 32, 130 and 256 modes (longest T60 2 s), a noise or swept-sine drive on each in every block, a two-sided junction between
    the first two (side a at a blend of three points) and a one-sided one on the third, K chosen from the returned C so that K C = 0.1, 1,
    10, 100; u a slow sine of the size of the free deflection; 2 blocks of 512 frames.  The longdouble run is in contact between 10 % and
    60 % of the run's frames at either junction (asserted).  Figures: the largest deviation of a force row / of the block's samples
    from the longdouble restatement's over that row's peak, and the relative deviation of C -- of the device, and of the working-precision
    restatement (every operation rounded to the bank's format, sums sequential) in the same run.  Bound: 4 x.

    Measured on an MI355X: see DESIGN.md section 3c (this test prints them)."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    comp = _compliances(REST_MODES[:3], REST_T60, use_double, _rest_specs, 2)
    for kind in ("noise", "sweep"):
        for kc in (0.1, 1.0, 10.0, 100.0):
            fig, contact = _against_longdouble(use_double, renderers, kind, kc, comp)
            print("%s, %s, K C = %g, %d renderers: " % ("fp64" if use_double else "fp32", kind, kc, renderers) +
                  ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()) +
                  "; in contact " + " ".join("%.2f" % c for c in contact))
            assert all(0.10 <= c <= 0.60 for c in contact), contact
            for key, (device, yardstick) in fig.items():
                assert 0 < yardstick < 1e6 * eps, (key, yardstick)
                assert device <= BOUND * yardstick, (kind, kc, key, device, yardstick)


# ---- 6. exact properties ----
def _exact_run(use_double, renderers, scale=1.0, bystanders=False, blocks=3, frames=FRAMES, comp=None, mirrored=False):
    """Objects 0 (130 modes) and 1 (64) joined by a two-sided junction, object 2 (256) under a one-sided one, every one driven; K C = 10.
    bystanders: further objects with a junction, drives and pickups of their own.  Returns (forces, out, states of objects 0 - 2)."""
    modes = [130, 64, 256] + ([37, 200, 129] if bystanders else [])
    sc, slots = dh.device_scene(modes, 0.5, renderers, use_double)
    specs = [jh.spec(jh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), jh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), 10.0 / comp[0]),
             jh.spec(jh.side(2, (3, 0, 1), (0.5, 0.25, 0.25), NORMAL, 2.0), None, 10.0 / comp[1], True)]
    pickups = []
    if bystanders:
        specs = [jh.spec(jh.side(4, 0, direction=NORMAL), jh.side(5, 1, direction=NORMAL), 3.0 / comp[0])] + specs
        pickups = [ph.spec(3, 1, direction=NORMAL, advance=1)]
    rows_f, outs = [], []
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (np.float32(scale) * _signal("noise" if o % 2 else "sweep", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))]
        # (a junction's approach goes with the junction: the two under test are the last two whatever stands before them)
        u = np.float32(scale) * np.array([(2e-5 * np.sin(2 * np.pi * (np.arange(frames) + b * frames) / (500.0 + 100 * (len(specs) - 1 - j)))).astype(np.float32) for j in range(len(specs))])
        out = np.zeros(frames, sc.dtype)
        _, _, forces, _, status = sc.render_coupled(out, *_drive_args(rows, frames), ph.records(pickups), jh.records(specs), u)
        assert (status == 1).all()
        rows_f.append(forces[-2:].copy())
        outs.append(out)
    n = sum(modes[:3])
    cols = [c[:n] for c in _states(sc)]
    sc.close()
    return np.concatenate(rows_f, axis=1), np.concatenate(outs), cols


def _exact_compliances(use_double):
    def make(k):
        return [jh.spec(jh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), jh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), k[0]),
                jh.spec(jh.side(2, (3, 0, 1), (0.5, 0.25, 0.25), NORMAL, 2.0), None, k[1], True)]
    return _compliances([130, 64, 256], 0.5, use_double, make, 2)


@PRECISIONS
def test_scaling_the_excitation_by_two_scales_everything_by_two(use_double):
    """A scene excited by drives only: u and every drive signal times 2 gives f, out and the states times 2, bit for bit (a power of two
    commutes with every rounding of the recurrence and of the solve, and max(2x, 0) = 2 max(x, 0))."""
    comp = _exact_compliances(use_double)
    f1, out1, cols1 = _exact_run(use_double, 1, 1.0, comp=comp)
    f2, out2, cols2 = _exact_run(use_double, 1, 2.0, comp=comp)
    assert np.abs(f1).max(axis=1).min() > 0 and ((f1[0] == 0).mean() > 0.05)  # the unilateral one makes and breaks
    assert np.array_equal(2 * f1, f2) and np.array_equal(2 * out1, out2)
    assert np.array_equal(2 * cols1[0], cols2[0]) and np.array_equal(2 * cols1[1], cols2[1])


@PRECISIONS
def test_a_junction_is_local_and_deterministic(use_double):
    comp = _exact_compliances(use_double)
    f, out, cols = _exact_run(use_double, 1, comp=comp)
    assert np.abs(f).max() > 0 and np.isfinite(f).all()
    for what, (g, _, c) in (("a second run", _exact_run(use_double, 1, comp=comp)), ("four renderers", _exact_run(use_double, 4, comp=comp)),
                            ("bystanders", _exact_run(use_double, 1, bystanders=True, comp=comp)), ("bystanders, four renderers", _exact_run(use_double, 4, bystanders=True, comp=comp))):
        assert np.array_equal(f, g) and _same(cols, c), what
    _, out4, _ = _exact_run(use_double, 4, comp=comp)
    assert np.abs(out4 - out).max() <= 1e-3 * np.abs(out).max()  # (the mix of four renderers adds in another order: not bit-equal, and not asked to be)


@PRECISIONS
def test_objects_off_the_junction_do_not_see_its_stiffness(use_double):
    comp = _exact_compliances(use_double)
    runs = []
    for k in (0.0, 10.0, 1000.0):
        sc, slots = dh.device_scene([130, 64, 256, 200], 0.5, 1, use_double)
        for b in range(2):
            rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, 2 * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(4)]
            spec = jh.spec(jh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), jh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), k / comp[0])
            sc.render_coupled(np.zeros(FRAMES, sc.dtype), *_drive_args(rows, FRAMES), [], jh.records([spec]), 1e-5 * np.ones((1, FRAMES), np.float32))
        runs.append(_states(sc))
        sc.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0][194:], other[0][194:]) and np.array_equal(runs[0][1][194:], other[1][194:])
    assert not np.array_equal(runs[0][0][:194], runs[2][0][:194])


@PRECISIONS
def test_a_mirrored_pair_moves_as_one(use_double):
    """Two identical objects (one body, added twice) under identical drives, joined by a junction whose two sides are the same record but
    for the object: both objects' states are equal bit for bit after every block."""
    from mesheditor_amd import bank as hipbank
    n = 130
    sc = hipbank.Scene(bh.SAMPLE_RATE, 0, use_double)
    mo = bh.make_modes(n, 0.5)
    for o in range(2):
        slot = sc.add_object(o, mo["shapes"], mo["positions"], mo["indices"])
        sc.tune_object(slot, mo["freqs"], mo["t60s"])
        sc.set_gains(slot, 1.0, 1.0)
    sc.install()
    sc.render(np.zeros(FRAMES, sc.dtype))
    make = lambda k: [jh.spec(jh.side(0, 2, direction=NORMAL, coupling=2.0), jh.side(1, 2, direction=NORMAL, coupling=2.0), k)]
    _, _, _, comp, _ = sc.render_coupled(np.zeros(FRAMES, sc.dtype), [], np.zeros((0, FRAMES), np.float32), [], jh.records(make(0.0)), np.zeros((1, FRAMES), np.float32))
    moved = False
    for b in range(3):
        f = _signal("noise", 1, 3 * FRAMES)[b * FRAMES:(b + 1) * FRAMES]
        rows = [(o,) + dh.row_direction(1) + (f,) for o in range(2)]
        u = (3e-5 * np.sin(2 * np.pi * np.arange(FRAMES) / 300.0)).astype(np.float32)[None, :]
        _, _, forces, _, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), *_drive_args(rows, FRAMES), [], jh.records(make(10.0 / comp[0])), u)
        assert status[0] == 1
        moved = moved or np.abs(forces).max() > 0
        re, im = _states(sc)
        assert np.array_equal(re[:n], re[n:]) and np.array_equal(im[:n], im[n:]) and np.abs(re).max() > 0, b
    sc.close()
    assert moved


# ---- 7. left out, refused, pickups, retune ----
ODD_MODES = (64, 130, 0, 600, 520)


def _odd_scene(use_double):
    """Objects of 64, 130, 0, 600 and 520 modes (the last two together: ten waves, more than a junction's workgroup holds)."""
    from mesheditor_amd import bank as hipbank
    sc = hipbank.Scene(bh.SAMPLE_RATE, 0, use_double)
    for o, n in enumerate(ODD_MODES):
        mo = bh.make_modes(n, 0.5, freq_scale=1.0 + 0.013 * o)
        slot = sc.add_object(o, mo["shapes"], mo["positions"], mo["indices"])
        assert slot == o
        sc.tune_object(slot, mo["freqs"], mo["t60s"])
        sc.set_gains(slot, 1.0, 1.0)
    sc.install()
    sc.render(np.zeros(bh.BLOCK, sc.dtype))
    return sc


@PRECISIONS
def test_what_cannot_be_solved_is_left_out(use_double):
    frames, blocks = FRAMES, 2
    good = [jh.spec(jh.side(0, 1, direction=NORMAL, coupling=2.0), None, 2e6), jh.spec(jh.side(1, 2, direction=(1.0, 0.5, 0.0)), jh.side(3, 0, direction=(-1.0, -0.5, 0.0)), 1e6)]
    free = jh.side(4, 0, direction=NORMAL)  # an object no good junction uses
    P = ph.POINTS
    bad = {"no such object": jh.spec(jh.side(5, 0), None, 1.0), "no such object on side b": jh.spec(free, jh.side(77, 0), 1.0), "an object without modes": jh.spec(jh.side(2, 0), None, 1.0),
           "side b without modes": jh.spec(free, jh.side(2, 0), 1.0), "first point beyond the shapes": jh.spec(jh.side(4, (P, 0, 0)), None, 1.0),
           "second point beyond": jh.spec(jh.side(4, (0, 2 ** 31, 0)), None, 1.0), "third point beyond": jh.spec(jh.side(4, (0, 0, P)), None, 1.0),
           "weight nan": jh.spec(jh.side(4, 0, (1.0, np.nan, 0.0)), None, 1.0), "weight inf": jh.spec(jh.side(4, 0, (np.inf, 0.0, 0.0)), None, 1.0),
           "direction nan": jh.spec(jh.side(4, 0, direction=(1.0, 0.0, np.nan)), None, 1.0), "direction inf": jh.spec(jh.side(4, 0, direction=(-np.inf, 0.0, 0.0)), None, 1.0),
           "scale nan": jh.spec(jh.side(4, 0, coupling=np.nan), None, 1.0), "scale inf": jh.spec(jh.side(4, 0, coupling=np.inf), None, 1.0),
           "stiffness nan": jh.spec(free, None, np.nan), "stiffness inf": jh.spec(free, None, np.inf), "stiffness negative": jh.spec(free, None, -1.0),
           "both sides one object": jh.spec(free, jh.side(4, 1), 1.0), "an object of an earlier junction": jh.spec(free, jh.side(0, 2), 1.0),
           "more modes than a workgroup holds": jh.spec(jh.side(4, 0, direction=NORMAL), jh.side(3, 1, direction=NORMAL), 1.0)}

    def run(specs):
        sc = _odd_scene(use_double)
        out, rows, status = np.zeros(blocks * frames, sc.dtype), [], None
        for b in range(blocks):
            drives = [(0, 1, 1.0, 0.5, 0.0), (1, 2, 0.5, 0.0, 1.0), (4, 0, 0.5, 0.5, 0.0)]
            sig = np.array([_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames] for o in (0, 1, 4)], np.float32)
            u = np.array([(2e-5 * np.sin(2 * np.pi * np.arange(frames) / (300.0 + 50 * s[0][0]))).astype(np.float32) for s in specs])  # (it goes with the junction, not with its place)
            _, _, forces, comp, status = sc.render_coupled(out[b * frames:(b + 1) * frames], drives, sig, [], jh.records(specs), u)
            rows.append(forces)
        state = sc.object_state(), _states(sc)
        sc.close()
        return out, np.concatenate(rows, axis=1), status, comp, state

    ref_out, ref_rows, ref_status, _, ref_state = run(good)
    assert list(ref_status) == [1, 1] and (np.abs(ref_rows).max(axis=1) > 0).all()
    for name, stray in bad.items():
        specs = [good[0], good[1], stray] if name in ("an object of an earlier junction", "more modes than a workgroup holds") else [good[0], stray, good[1]]
        at = specs.index(stray)
        if name == "more modes than a workgroup holds":  # (object 3 must be free for it to be the mode count that decides)
            specs, at = [good[0], stray], 1
            want_out, want_rows, _, _, want_state = run([good[0]])
        else:
            want_out, want_rows, want_state = ref_out, ref_rows, ref_state
        out, rows, status, comp, state = run(specs)
        assert status[at] == 0 and comp[at] == 0 and (rows[at] == 0).all(), name
        assert list(np.delete(status, at)) == [1] * (len(specs) - 1), name
        assert np.array_equal(np.delete(rows, at, axis=0), want_rows), name
        assert np.array_equal(out, want_out) and _same(state[0], want_state[0]) and _same(state[1], want_state[1]), name


@PRECISIONS
def test_a_junction_that_would_amplify_is_refused(use_double):
    """A negative coupling makes C negative; with K >= -1 / C the denominator 1 + K C is not above 0: status 2, a zero row, and the bits of
    the K = 0 call.  With K below -1 / C it is solved."""
    make = lambda k: [jh.spec(jh.side(0, 1, direction=NORMAL, coupling=-2.0), jh.side(1, 2, direction=NORMAL, coupling=-1.0), k[0])]
    sc, _ = dh.device_scene([64, 130], 0.5, 1, use_double)
    _, _, _, comp, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), [], np.zeros((0, FRAMES), np.float32), [], jh.records(make([0.0])), np.zeros((1, FRAMES), np.float32))
    sc.close()
    assert status[0] == 1 and comp[0] < 0
    results = {}
    for name, k in (("zero", 0.0), ("refused", -2.0 / comp[0]), ("at the edge", -1.0 / comp[0] * 1.001), ("solved", -0.01 / comp[0])):
        sc, _ = dh.device_scene([64, 130], 0.5, 1, use_double)
        out = np.zeros(2 * FRAMES, sc.dtype)
        for b in range(2):
            rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, 2 * FRAMES)[b * FRAMES:(b + 1) * FRAMES],) for o in range(2)]
            _, _, forces, _, status = sc.render_coupled(out[b * FRAMES:(b + 1) * FRAMES], *_drive_args(rows, FRAMES), [], jh.records(make([k])), 1e-5 * np.ones((1, FRAMES), np.float32))
        results[name] = (out, forces, status[0], _states(sc), sc.object_state())
        sc.close()
    for name in ("refused", "at the edge"):
        out, forces, status, cols, state = results[name]
        assert status == 2 and (forces == 0).all(), name
        assert np.array_equal(out, results["zero"][0]) and _same(cols, results["zero"][3]) and _same(state, results["zero"][4]), name
    assert results["zero"][2] == 1 and results["solved"][2] == 1 and np.abs(results["solved"][1]).max() > 0


@PRECISIONS
def test_a_pickup_on_a_junctions_object_is_left_out(use_double):
    sc, _ = dh.device_scene([64, 130, 37], 0.5, 1, use_double)
    rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, FRAMES),) for o in range(3)]
    pickups = [ph.spec(0, 1, direction=NORMAL), ph.spec(1, 1, direction=NORMAL, advance=1), ph.spec(2, 1, direction=NORMAL)]
    junction = [jh.spec(jh.side(0, 1, direction=NORMAL), jh.side(1, 2, direction=NORMAL), 1e5)]
    reads, flags, forces, _, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), *_drive_args(rows, FRAMES), ph.records(pickups), jh.records(junction), np.zeros((1, FRAMES), np.float32))
    assert status[0] == 1 and list(flags) == [0, 0, 1] and (reads[:2] == 0).all() and np.abs(reads[2]).max() > 0
    reads, flags = sc.render_read(np.zeros(FRAMES, sc.dtype), *_drive_args(rows, FRAMES), ph.records(pickups))  # and read again once the junction is gone
    assert list(flags) == [1, 1, 1] and (np.abs(reads).max(axis=1) > 0).all()
    sc.close()


@PRECISIONS
def test_a_live_retune_reaches_the_next_blocks_compliance(use_double):
    """tune_object(..., live=True) with other frequencies and radius_scale 2 between two blocks: the returned C follows the new columns --
    held to the restatement rebuilt from them by the yardstick of test 5 -- and is far from the old one."""
    modes = [130, 64]
    sc, _ = dh.device_scene(modes, REST_T60, 1, use_double)
    mo = bh.make_modes(modes[0], REST_T60)
    spec = jh.spec(jh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), NORMAL, 2.0), jh.side(1, 2, direction=NORMAL), 1e4)
    comps = []
    for b in range(2):
        if b == 1:
            sc.tune_object(0, mo["freqs"] * np.float32(1.0625), mo["t60s"], radius_scale=2.0, live=True)
        _, _, _, comp, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), [], np.zeros((0, FRAMES), np.float32), [], jh.records([spec]), np.zeros((1, FRAMES), np.float32))
        assert status[0] == 1
        comps.append(float(comp[0]))
        exact, working = jh.Restatement(sc, modes, np.longdouble, sc.dtype), jh.Restatement(sc, modes, sc.dtype, sc.dtype)
        c_exact, c_plain = exact.compliance(spec), np.longdouble(working.compliance(spec))
        device, yardstick = float(abs(np.longdouble(comps[-1]) - c_exact) / c_exact), float(abs(c_plain - c_exact) / c_exact)
        print("%s, block %d: C device %.17g, deviation %.3e, working-precision restatement %.3e" % ("fp64" if use_double else "fp32", b, comps[-1], device, yardstick))
        assert yardstick > 0 and device <= BOUND * yardstick, (b, device, yardstick)
    sc.close()
    assert abs(comps[1] - comps[0]) > 0.05 * abs(comps[0])
