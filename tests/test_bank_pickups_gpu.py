"""GPU tests of deflection pickups (Scene.render_read -> RenderModalRead -> mh_bank_render_read -> k_bank_modes_read).

1. A pickup observes: the 72-block scenes of tests/test_bank_drives_gpu.py (impacts and drives mixed, culling, silence, re-excitation)
   through render_read with 1 ... 10 pickups on every object are, bit for bit, what render_driven gives.
2. A pickup's row is local and deterministic: the same bits alone, among others, beside drives elsewhere, for 1 and 4 renderers, twice.
3. Rows against a numpy.longdouble restatement (tests/pickup_harness.py), bounded by 4 x the deviation of the working-precision
   restatement (numpy float32 / float64, modes added in order, no contraction) from the same longdouble rows in the same run.
4. advance is a free advance of the read.
5. What cannot be read is left out; an object at rest reads zeros; a live retune reaches the next block's pickup."""
import numpy as np
import pytest

from tests import bank_harness as bh
from tests import drive_harness as dh
from tests import pickup_harness as ph
from tests import test_bank_drives_gpu as drives_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
BOUND = 4  # x the working-precision restatement's own deviation (see test 3)


def _signal(kind, row, n):
    return drives_suite._signal(kind, row, n)


def _some_pickup(obj, i):
    """Pickup i of an object: positions, blends, directions and advances that differ from one to the next."""
    p, d = dh.row_direction(i + 2 * obj)
    if i % 3 == 2:
        return ph.spec(obj, (p, (p + 1) % ph.POINTS, (p + 2) % ph.POINTS), (0.5, 0.25, 0.25), d, 1.0 + 0.5 * i, i % 3)
    return ph.spec(obj, p, direction=d, coupling=1.0 + 0.5 * i, advance=i % 3)


# ---- 1. observer ----
def _run_mixed(use_double, renderers, frames, blocks, watched):
    """The 'mixed' run of tests/test_bank_drives_gpu.py (an object's first row an impact, the rest drives), through render_driven or,
    `watched`, through render_read with 1 + (object % 10) pickups on every object."""
    from mesheditor_amd import bank as hipbank
    sc, slots = dh.device_scene(drives_suite.MODES, drives_suite.T60, renderers, use_double)
    specs = [_some_pickup(slots[o], i) for o in range(len(slots)) for i in range(1 + o % 10)]
    probes = ph.records(specs)
    sig, states, loudest, flags = np.zeros(blocks * frames, sc.dtype), [], 0.0, None
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
        if watched:
            reads, flags = sc.render_read(out, drives, signals, probes)
            assert np.isfinite(reads).all()
            loudest = max(loudest, float(np.abs(reads).max()))
        else:
            sc.render_driven(out, drives, signals)
        states.append([a.copy() for a in sc.object_state()])
    cols = [sc.column("StateRe"), sc.column("StateIm")]
    sc.close()
    return sig, states, cols, loudest, flags, specs


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_a_pickup_observes(use_double, renderers, frames):
    blocks = drives_suite.BLOCKS
    ref, ref_states, ref_cols, _, _, _ = _run_mixed(use_double, renderers, frames, blocks, False)
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    ring = np.array([s[2] for s in ref_states])
    assert any((s[1][s[2] != 0] < s[0][s[2] != 0]).any() for s in ref_states)  # culling ...
    assert ((ring[:-1] == 1) & (ring[1:] == 0)).any() and ((ring[:-1] == 0) & (ring[1:] == 1)).any()  # ... silence and re-excitation
    got, states, cols, loudest, flags, specs = _run_mixed(use_double, renderers, frames, blocks, True)
    assert loudest > 0  # the pickups did read something
    per_object = {}
    for s, f in zip(specs, flags):  # the first eight of an object are read, the ninth and tenth are beyond the cap
        per_object[s[0]] = per_object.get(s[0], 0) + 1
        assert f == (1 if per_object[s[0]] <= 8 else 0)
    bad = np.flatnonzero(ref != got)
    assert np.array_equal(ref, got), (len(bad), bad[:4])
    for b, (want, have) in enumerate(zip(ref_states, states)):
        for a, c in zip(want, have):
            assert np.array_equal(a, c), b
    assert np.array_equal(ref_cols[0], cols[0]) and np.array_equal(ref_cols[1], cols[1])


# ---- 2. locality and determinism ----
LOCAL_MODES = [130, 64, 256, 37]


def _local_run(use_double, renderers, others_on_object, elsewhere, drives_elsewhere, blocks=5, frames=512):
    """Object 0 is struck in block 0 and driven in every block; the pickup under test sits on it, optionally among seven others, with
    pickups on the other objects, with drives on the other objects.  Returns its rows, block after block."""
    from mesheditor_amd import bank as hipbank
    sc, slots = dh.device_scene(LOCAL_MODES, 0.4, renderers, use_double)
    target = ph.spec(slots[0], (3, 0, 1), (0.5, 0.25, 0.25), (0.25, -1.0, 0.5), 3.0, 1)
    specs = [target]
    if others_on_object:
        specs = [_some_pickup(slots[0], i) for i in range(3)] + [target] + [_some_pickup(slots[0], i) for i in range(3, 7)]
    at = specs.index(target)
    if elsewhere:
        specs = [_some_pickup(slots[2], 1)] + specs + [_some_pickup(slots[o], i) for o in (1, 2, 3) for i in range(3)]
        at += 1
    full = {o: _signal("noise" if o % 2 else "sweep", o, blocks * frames) for o in range(len(slots))}
    for o in range(len(slots)):  # every object struck, so that the others ring whether they are driven or not
        assert sc.enqueue(hipbank.Event(0, slots[o], o % ph.POINTS, 1.0, 0.5, 0.0, 1.0 / 300.0, 20.0, 0.0, 0.0, 0.0, 0.0))
    rows = []
    for b in range(blocks):
        driven = [0] + ([1, 2, 3] if drives_elsewhere else [])
        drives = [(slots[o], (o + 1) % ph.POINTS, 1.0, 0.5, 0.25) for o in driven]
        reads, flags = sc.render_read(np.zeros(frames, sc.dtype), drives, np.array([full[o][b * frames:(b + 1) * frames] for o in driven], np.float32), ph.records(specs))
        assert flags[at] == 1
        rows.append(reads[at].copy())
    sc.close()
    return np.concatenate(rows)


@PRECISIONS
def test_a_pickups_row_is_local_and_deterministic(use_double):
    alone = _local_run(use_double, 1, False, False, False)
    assert np.abs(alone).max() > 0 and np.isfinite(alone).all()
    for what, other in (("a second run", _local_run(use_double, 1, False, False, False)),
                        ("seven others on its object", _local_run(use_double, 1, True, False, False)),
                        ("pickups on other objects", _local_run(use_double, 1, True, True, False)),
                        ("drives on other objects", _local_run(use_double, 1, False, False, True)),
                        ("four renderers", _local_run(use_double, 4, False, False, False)),
                        ("everything at once, four renderers", _local_run(use_double, 4, True, True, True))):
        assert np.array_equal(alone, other), what


# ---- 3. against the restatement ----
REST_MODES, REST_T60, REST_BLOCKS, FRAMES = [32, 130, 256], 2.0, 3, 512


def _rest_specs(slots):
    specs = []
    for o, slot in enumerate(slots):
        specs += [ph.spec(slot, (o + a) % ph.POINTS, direction=(0.25, -1.0, 0.5), coupling=2.0, advance=a) for a in (0, 1, 2)]
        specs.append(ph.spec(slot, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.5, -0.25), 1.5, o % 3))
    return specs


def _rest_rows(kind, slots, b, frames=FRAMES, blocks=REST_BLOCKS):
    """One drive on every object in every block: the tuned set is rendered, nothing is culled."""
    return [(slot,) + dh.row_direction(o) + (_signal(kind, o, blocks * frames)[b * frames:(b + 1) * frames],) for o, slot in enumerate(slots)]


def _against_restatement(use_double, renderers, kind):
    """Returns (device figure, yardstick): the largest deviation of a pickup row of a block from the longdouble restatement's, relative to
    that row's peak -- of the device, and of the working-precision restatement."""
    sc, slots = dh.device_scene(REST_MODES, REST_T60, renderers, use_double)
    exact = ph.Restatement(sc, REST_MODES, np.longdouble, sc.dtype)
    working = ph.Restatement(sc, REST_MODES, sc.dtype, sc.dtype)
    specs = _rest_specs(slots)
    device, yardstick = 0.0, 0.0
    for b in range(REST_BLOCKS):
        rows = _rest_rows(kind, slots, b)
        reads, flags = sc.render_read(np.zeros(FRAMES, sc.dtype), [(o, p) + tuple(float(v) for v in d) for (o, p, d, f) in rows], np.array([f for (_, _, _, f) in rows], np.float32),
                                      ph.records(specs))
        assert (flags == 1).all()
        tuned, live, ring = sc.object_state()
        assert (ring == 1).all() and np.array_equal(tuned, live)  # nothing culled: the restatement renders every mode
        _, want = exact.render(rows, specs, FRAMES)
        _, plain = working.render(rows, specs, FRAMES)
        device, yardstick = max(device, ph.row_figure(reads, want)), max(yardstick, ph.row_figure(plain, want))
    sc.close()
    return device, yardstick


@PRECISIONS
@RENDERERS
def test_pickup_rows_match_a_longdouble_restatement(use_double, renderers):
    """Objects of 32, 130 and 256 modes (longest T60 2 s), one drive on each in every block (noise; swept sines), 3 blocks of 512 frames;
    per object pickups with advance 0, 1, 2 at single points and one blend.  The figure is the largest deviation of a row of a block from
    the longdouble restatement's row, divided by that row's peak, over every pickup row of every block.  Bound: 4 x the same figure of the
    working-precision restatement (the same recurrence and gains in numpy float32 / float64, modes added in order, no contraction) in the
    same run: the device's states follow the same uncontracted arithmetic, so only the order and the contraction of a <= 256-term read
    sum differ, which moves the error by a small factor either way.

    Measured on an MI355X (this test prints them; device / yardstick, the same for 1 and 4 renderers): fp32 noise 1.641e-06 / 1.987e-06
    (0.83 x), swept sines 3.637e-06 / 3.526e-06 (1.03 x); fp64 noise 3.331e-15 / 3.683e-15 (0.90 x), swept sines 7.191e-15 / 6.951e-15
    (1.03 x)."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    for kind in ("noise", "sweep"):
        device, yardstick = _against_restatement(use_double, renderers, kind)
        print("%s, %s, %d renderers: device %.3e, working-precision restatement %.3e (%.2f x)" % ("fp64" if use_double else "fp32", kind, renderers, device, yardstick, device / yardstick))
        assert 0 < yardstick < 1e5 * eps  # a yardstick outside this range would mean the restatements are wrong, not the bank
        assert device <= BOUND * yardstick, (kind, device, yardstick)


# ---- 4. advance ----
@PRECISIONS
@pytest.mark.parametrize("driven", [True, False], ids=["driven", "free"])
def test_advance_is_a_free_advance_of_the_read(use_double, driven):
    """Three pickups with one record but advance 0, 1, 2 on an object of 130 modes, excited in the first two blocks (noise drive) and
    compared in the third -- which carries a drive (`driven`) or nothing.  Frame s of advance 1 is frame s + 1 of advance 0, drive or
    not: a force enters Re z only.  Frame s of advance 2 is frame s + 2 of advance 0 in a block without excitation; with a drive the two
    differ by the force of frame s + 1 seen through one rotation, sum_k read[k] * c_im[k] * e[k][s + 1] -- taken from the restatement.
    The bound is that of test 3 (4 x the working-precision restatement's deviation, same scene, same run); the last comparison is
    between two differences of two rows each, every row within the bound of its restatement row: twice the bound.

    Measured on an MI355X (of the row's peak): advance 1 against 0, fp32 4.4e-07 driven / 3.8e-07 free (yardstick 1.2e-06 / 1.1e-06), fp64
    9.4e-16 / 9.5e-16 (1.7e-15 / 2.0e-15); advance 2 against 0 in the free block 4.8e-07 (fp32), 7.2e-16 (fp64); with the drive the two
    differ by 3.5e-02 of the peak, as the restatement says."""
    modes, frames = [130], FRAMES
    sc, slots = dh.device_scene(modes, REST_T60, 1, use_double)
    exact, working = ph.Restatement(sc, modes, np.longdouble, sc.dtype), ph.Restatement(sc, modes, sc.dtype, sc.dtype)
    specs = [ph.spec(slots[0], (3, 0, 1), (0.5, 0.25, 0.25), (0.25, -1.0, 0.5), 2.0, a) for a in (0, 1, 2)]
    noise = _signal("noise", 5, 3 * frames)
    for b in range(3):
        rows = [(slots[0],) + dh.row_direction(1) + (noise[b * frames:(b + 1) * frames],)] if (b < 2 or driven) else []
        reads, flags = sc.render_read(np.zeros(frames, sc.dtype), [(o, p) + tuple(float(v) for v in d) for (o, p, d, f) in rows],
                                      np.array([f for (_, _, _, f) in rows], np.float32).reshape(len(rows), frames), ph.records(specs))
        _, want = exact.render(rows, specs, frames)
        _, plain = working.render(rows, specs, frames)
    sc.close()
    assert (flags == 1).all()
    yardstick = ph.row_figure(plain, want)
    peak = float(np.abs(want[0]).max())
    reads = reads.astype(np.longdouble)
    one = float(np.abs(reads[1][:-1] - reads[0][1:]).max()) / peak
    two = reads[0][2:] - reads[2][:-2]
    print("%s, %s: advance 1 vs 0: %.3e of peak; advance 2 vs 0: %.3e; yardstick %.3e" % ("fp64" if use_double else "fp32", "driven" if driven else "free", one, float(np.abs(two).max()) / peak, yardstick))
    assert peak > 0 and yardstick > 0
    assert one <= BOUND * yardstick, (one, yardstick)
    if not driven:
        assert float(np.abs(two).max()) / peak <= BOUND * yardstick, (float(np.abs(two).max()) / peak, yardstick)
    else:
        # what the restatement says: the force of frame s + 1 through one rotation
        g = exact.drive_gain(0, *dh.row_direction(1))
        through = (exact.read_of(specs[0]) * exact.objects[0]["c_im"] * g).sum() * noise[2 * frames:].astype(np.longdouble)[1:-1]
        said = want[0][2:] - want[2][:-2]
        assert np.abs(said - through).max() <= 1e-12 * np.abs(through).max()  # the restatement agrees with the closed form of the difference
        assert np.abs(through).max() > 10 * BOUND * yardstick * peak  # and the difference is no rounding matter
        assert float(np.abs(two - said).max()) / peak <= 2 * BOUND * yardstick, (float(np.abs(two - said).max()) / peak, yardstick)


# ---- 5. left out, at rest, retuned ----
def _scene_with_an_empty_object(use_double, renderers=1):
    """Objects of 64, 130 and 0 modes."""
    from mesheditor_amd import bank as hipbank
    sc = hipbank.Scene(bh.SAMPLE_RATE, 0, use_double)
    sc.set_renderers(renderers)
    slots = []
    for o, n in enumerate((64, 130, 0)):
        mo = bh.make_modes(n, 0.5, freq_scale=1.0 + 0.013 * o)
        slots.append(sc.add_object(o, mo["shapes"], mo["positions"], mo["indices"]))
        sc.tune_object(slots[-1], mo["freqs"], mo["t60s"])
        sc.set_gains(slots[-1], 1.0, 1.0)
    sc.install()
    sc.render(np.zeros(bh.BLOCK, sc.dtype))
    return sc, slots


@PRECISIONS
def test_what_cannot_be_read_is_left_out(use_double):
    frames, blocks = FRAMES, 3
    good = [ph.spec(0, 1, direction=(0.25, -1.0, 0.5), advance=1), ph.spec(1, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.5, 0.0), 2.0, 2), ph.spec(0, 2, direction=(0.0, 1.0, 0.0))]
    bad = {"no such object": ph.spec(3, 0), "no such object at all": ph.spec(2 ** 32 - 1, 0), "an object without modes": ph.spec(2, 0),
           "first point beyond the shapes": ph.spec(0, (ph.POINTS, 0, 0)), "second point beyond": ph.spec(1, (0, 2 ** 31, 0)), "third point beyond": ph.spec(0, (0, 0, ph.POINTS)),
           "weight nan": ph.spec(0, 0, (1.0, np.nan, 0.0)), "weight inf": ph.spec(0, 0, (np.inf, 0.0, 0.0)), "direction nan": ph.spec(1, 0, direction=(1.0, 0.0, np.nan)),
           "direction inf": ph.spec(1, 0, direction=(-np.inf, 0.0, 0.0)), "scale nan": ph.spec(0, 0, coupling=np.nan), "scale inf": ph.spec(0, 0, coupling=np.inf),
           "advance 3": ph.spec(0, 0, advance=3), "advance huge": ph.spec(1, 0, advance=2 ** 31)}
    crowd = [ph.spec(1, i % ph.POINTS, direction=(1.0, 0.0, 0.0), advance=i % 3) for i in range(10)]  # with `good`'s one: the 8th to 10th here are beyond the cap of 8

    def run(specs):
        sc, slots = _scene_with_an_empty_object(use_double)
        assert slots == [0, 1, 2]
        out, rows, flags = np.zeros(blocks * frames, sc.dtype), [], None
        for b in range(blocks):
            drives = [(0, 1, 1.0, 0.5, 0.0), (1, 2, 0.5, 0.0, 1.0)]
            sig = np.array([_signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames] for o in (0, 1)], np.float32)
            reads, flags = sc.render_read(out[b * frames:(b + 1) * frames], drives, sig, ph.records(specs))
            rows.append(reads)
        state = sc.object_state()
        sc.close()
        return out, np.concatenate(rows, axis=1), flags, state
    ref_out, ref_rows, ref_flags, ref_state = run(good)
    assert (ref_flags == 1).all() and (np.abs(ref_rows).max(axis=1) > 0).all()
    for name, stray in bad.items():
        out, rows, flags, state = run([good[0], stray, good[1], good[2]])
        assert list(flags) == [1, 0, 1, 1], name
        assert (rows[1] == 0).all(), name
        assert np.array_equal(rows[[0, 2, 3]], ref_rows), name
        assert np.array_equal(out, ref_out) and all(np.array_equal(a, b) for a, b in zip(state, ref_state)), name
    out, rows, flags, state = run(good + crowd)
    assert list(flags) == [1, 1, 1] + [1] * 7 + [0] * 3
    assert (rows[10:] == 0).all() and (np.abs(rows[3:10]).max(axis=1) > 0).all()
    assert np.array_equal(rows[:3], ref_rows) and np.array_equal(out, ref_out)


@PRECISIONS
def test_an_object_at_rest_reads_zeros_and_counts_as_read(use_double):
    sc, slots = dh.device_scene([64, 130], 0.2, 1, use_double)
    specs = [ph.spec(slots[0], 1, direction=(0.0, 1.0, 0.0)), ph.spec(slots[1], 2, direction=(1.0, 0.0, 0.0), advance=2)]
    out = np.zeros(FRAMES, sc.dtype)
    reads, flags = sc.render_read(out, [], np.zeros((0, FRAMES), np.float32), ph.records(specs))  # nothing rings at all
    assert list(flags) == [1, 1] and (reads == 0).all() and (out == 0).all()
    reads, flags = sc.render_read(out, [(slots[1], 0, 1.0, 0.5, 0.0)], _signal("noise", 0, FRAMES)[None, :], ph.records(specs))  # object 1 driven, object 0 still at rest
    assert list(flags) == [1, 1] and (reads[0] == 0).all() and np.abs(reads[1]).max() > 0
    assert list(sc.object_state()[2]) == [0, 1]
    sc.close()


@PRECISIONS
def test_a_live_retune_reaches_the_next_blocks_pickup(use_double):
    """tune_object(..., live=True) with other frequencies and radius_scale 2 (DeflectionScale 1/8, other DeflectionGain): the next
    block's pickup follows the new columns.  Compared with the restatements rebuilt from the new columns (states kept), bound as in test 3;
    and the restatement still on the old columns is far from what the device now reads."""
    modes = [130]
    sc, slots = dh.device_scene(modes, REST_T60, 1, use_double)
    mo = bh.make_modes(modes[0], REST_T60)
    exact, working, stale = (ph.Restatement(sc, modes, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.longdouble))
    specs = [ph.spec(slots[0], 1, direction=(0.25, -1.0, 0.5), coupling=2.0, advance=a) for a in (0, 1, 2)]
    noise = _signal("noise", 3, 2 * FRAMES)
    for b in range(2):
        if b == 1:
            sc.tune_object(slots[0], mo["freqs"] * np.float32(1.0625), mo["t60s"], radius_scale=2.0, live=True)
        rows = [(slots[0],) + dh.row_direction(2) + (noise[b * FRAMES:(b + 1) * FRAMES],)]
        reads, flags = sc.render_read(np.zeros(FRAMES, sc.dtype), [(o, p) + tuple(float(v) for v in d) for (o, p, d, f) in rows], np.array([rows[0][3]], np.float32), ph.records(specs))
        if b == 1:
            exact.load_columns(sc)
            working.load_columns(sc)
            assert exact.objects[0]["defl_scale"] == 0.125
        _, want = exact.render(rows, specs, FRAMES)
        _, plain = working.render(rows, specs, FRAMES)
        _, old = stale.render(rows, specs, FRAMES)
    sc.close()
    assert (flags == 1).all()
    device, yardstick = ph.row_figure(reads, want), ph.row_figure(plain, want)
    print("%s after a live retune: device %.3e, working-precision restatement %.3e" % ("fp64" if use_double else "fp32", device, yardstick))
    assert device <= BOUND * yardstick, (device, yardstick)
    assert ph.row_figure(reads, old) > 0.1
