"""GPU tests of the pickups on junction objects (Scene.render_observed -> RenderModalObserved -> mh_bank_render_observed -> the tapped
entries of k_bank_modes_coupled / k_bank_modes_grouped and k_bank_observe_rows; contract: include/modalhip.h, "Pickups on junction
objects").

1. Without a pickup on a junction object render_observed is render_damped, bit for bit, on the mixed drive scene with a junction of each
   law and a group.
2. Pickups observe: 1 and 8 pickups (and a ninth, left out) on every junction object change nothing else.
3. Dead junctions, bit for bit: the rows are those render_read returns on a twin with zero-signal drives in the junctions' place.
4. Replay (fp32, objects without another row): the returned force rows as drives on a twin give the same pickup rows.
5. The law where it is solved: f[s] against K phi(u[s] - sum_sides read1[s]) with the advance-1 pickups of the same call, on objects that
   also carry drives, and a damped junction's carry against the last frame's u - sum read1.
6. Pickup rows against a numpy.longdouble restatement (tests/observed_harness.py).
7. Full width: a junction of 640 + 384 modes, eight waves, eight pickups on each object.
8. Independence: a row does not depend on the run, the renderer count, bystanders or the other pickups of its object.
9. render_coupled and render_damped still leave such pickups out."""
import functools

import numpy as np
import pytest

from tests import bank_harness as bh
from tests import damped_harness as dd
from tests import drive_harness as dh
from tests import group_harness as gh
from tests import observed_harness as oh
from tests import pickup_harness as ph
from tests import test_bank_drives_gpu as drives_suite
from tests import test_bank_junctions_gpu as junctions_suite
from tests import test_bank_pickups_gpu as pickups_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("renderers,frames", [(1, 512), (4, 333)])
BOUND = junctions_suite.BOUND  # 4 x the working-precision restatement's own deviation
_signal, _drive_args, _states, _same = junctions_suite._signal, junctions_suite._drive_args, junctions_suite._states, junctions_suite._same
RATE = np.float32(bh.SAMPLE_RATE)
L = np.longdouble


def _damping(lam):
    """D in s/m per junction whose per-frame l = float(D) * float(rate) is the float nearest each of `lam`; and those l."""
    d = [np.float32(v) / RATE for v in lam]
    return [float(v) for v in d], [np.float32(v * RATE) for v in d]


def _render(sc, entry, out, rows, pickups, junctions, u, lam, carry):
    """One block through render_observed, render_damped or render_coupled: (reads, flags, forces, C, statuses, carry -- None for
    render_coupled).  lam: the per-frame l aimed at, per junction (what the entry forms is _damping(lam)[1])."""
    drives, signals = _drive_args(rows, len(out)) if rows else ([], np.zeros((0, len(out)), np.float32))
    if entry == "coupled":
        return sc.render_coupled(out, drives, signals, ph.records(list(pickups)), junctions, u) + (None,)
    return getattr(sc, "render_" + entry)(out, drives, signals, ph.records(list(pickups)), junctions, u, _damping(lam)[0], carry)


def _figure(got, want):
    """The largest deviation over the row's peak, the largest over the rows."""
    return oh.row_figure(np.asarray(got), np.asarray(want))


# ---- 1, 2, 9. the mixed drive scene with a junction of each law and a group ----
MIXED_ON = [6, 8, 3, 1, 4, 9]  # the junctions' objects (64, 8, 256, 37, 300 and 129 modes); 0, 2, 5 and 7 stay in the main launch
MIXED_OFF = [0, 2, 5, 7]


def _mixed_specs(k, lone_only=False):
    """A linear two-sided junction (objects 6 and 8), a Hertz one on object 3, a damped linear one on object 1, and a group of two on
    objects 4 (three waves) and 9 (two).  lone_only: every junction as a lone spec of tests/damped_harness.py (the scout's)."""
    lone = [dd.spec(oh.side(6, 1, direction=(1.0, 0.5, 0.25)), oh.side(8, 2, direction=(-1.0, -0.5, -0.25)), k[0], False, False, False),
            dd.spec(oh.side(3, 0, direction=(0.25, -1.0, 0.5), coupling=2.0), None, k[1], False, True, False),
            dd.spec(oh.side(1, 2, direction=(0.0, 1.0, 0.0)), None, k[2], False, False, True)]
    group = [gh.spec(oh.side(4, 3, direction=(0.5, 0.5, -1.0)), oh.side(9, 1, direction=(-0.5, -0.5, 1.0)), k[3]),
             gh.spec(oh.side(9, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.0, -0.5)), None, k[4])]
    if lone_only:
        return lone + [dd.spec(s[0], s[1], s[2], False, False, False) for s in group]
    return lone, group


def _mixed_block(b, frames):
    """Block b of the drive tests' mixed scene: (impacts to enqueue as (object, ex_pos, direction, gamma), drive rows of the restatement's kind)."""
    impacts, rows, seen = [], [], set()
    for (o, p, d, gamma) in drives_suite._rows_of(b):
        if o not in seen:
            impacts.append((o, p, d, gamma))
        else:
            rows.append((o, p, d, dh.impulse_row(gamma, frames)))
        seen.add(o)
    return impacts, rows


@functools.lru_cache(maxsize=None)
def _mixed_plan(use_double, frames, blocks):
    """(u, K per junction, l per junction) of the mixed scene: the free deflection at every junction from a float64 restatement without
    contact on the bank's columns (read without a device), u = observed_harness.approach of its rms, K C = 3 (Hertz: K C sqrt(x0) = 3) with
    the restatement's C, l x0 = 1 for the damped junction."""
    cols = oh.HostColumns(drives_suite.MODES, drives_suite.T60, use_double)
    scout = oh.Damped(cols, drives_suite.MODES, np.float64, cols.dtype)
    specs = _mixed_specs([0.0] * 5, lone_only=True)
    free = []
    for b in range(blocks):
        impacts, rows = _mixed_block(b, frames)
        trace = {}
        scout.render_damped([(o, p, d, dh.impulse_row(g, frames)) for (o, p, d, g) in impacts] + rows, specs, np.zeros((5, frames), np.float32), [0.0] * 5, None, frames, trace)
        free.append(np.asarray(trace["d"], np.float64))
    u = oh.approach(np.sqrt((np.concatenate(free, axis=1) ** 2).mean(axis=1)), frames, blocks)
    x0 = u.max(axis=1)
    comp = [float(scout.compliance(s[:4])) for s in specs]
    k = [3.0 / (c * (np.sqrt(float(x)) if j == 1 else 1.0)) for j, (c, x) in enumerate(zip(comp, x0))]
    return u, k, [0.0, 0.0, 1.0 / float(x0[2]), 0.0, 0.0]


def _mixed_pickups(count):
    """`count` pickups on every junction object (advances 0, 1, 2 in turn, every third at a blend), grouped by object."""
    return [pickups_suite._some_pickup(o, i) for o in MIXED_ON for i in range(count)]


def _mixed_run(use_double, renderers, frames, entry, on_junctions, blocks=3):
    """The mixed scene through `entry` with 1 + (object % 3) pickups on the objects off the junctions and `on_junctions` (specs) on the
    others.  Returns per block (out, reads, flags, forces, C, statuses, carry, object_state) and the final states."""
    from mesheditor_amd import bank as hipbank
    u, k, lam = _mixed_plan(use_double, frames, blocks)
    lone, group = _mixed_specs(k)
    junctions = oh.junction_records(lone, group)
    sc, slots = dh.device_scene(drives_suite.MODES, drives_suite.T60, renderers, use_double)
    assert slots == list(range(len(slots)))
    off = [pickups_suite._some_pickup(o, i) for o in MIXED_OFF for i in range(1 + o % 3)]
    per_block, carry = [], None
    for b in range(blocks):
        impacts, rows = _mixed_block(b, frames)
        for (o, p, d, gamma) in impacts:
            assert sc.enqueue(dh.one_sample_impact(hipbank.Event, o, p, d, gamma))
        out = np.zeros(frames, sc.dtype)
        reads, flags, forces, comp, status, carry = _render(sc, entry, out, rows, off + list(on_junctions), junctions, u[:, b * frames:(b + 1) * frames], lam, carry)
        per_block.append((out, reads.copy(), flags.copy(), forces.copy(), comp.copy(), status.copy(), None if carry is None else carry.copy(), [a.copy() for a in sc.object_state()]))
    cols = _states(sc)
    sc.close()
    return per_block, cols, len(off)


def _same_blocks(a, b, n_off):
    """Everything but the junction objects' pickups: out, the rows and flags of the pickups off the junctions, forces, C, statuses, carry
    (NaN where it is NaN), object_state."""
    for blk, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), blk
        assert np.array_equal(x[1][:n_off], y[1][:n_off]) and np.array_equal(x[2][:n_off], y[2][:n_off]), blk
        assert np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]), blk
        assert np.array_equal(x[6], y[6], equal_nan=True), blk
        assert _same(x[7], y[7]), blk


@PRECISIONS
@SHAPES
def test_without_a_pickup_on_a_junction_object_it_is_render_damped(use_double, renderers, frames):
    ref, ref_cols, n_off = _mixed_run(use_double, renderers, frames, "damped", [])
    for blk in ref:
        assert list(blk[5]) == [1] * 5 and np.isfinite(blk[3]).all() and np.isfinite(blk[0]).all() and (blk[2] == 1).all()
    forces = np.concatenate([blk[3] for blk in ref], axis=1)
    print("mixed scene, in contact: " + " ".join("%.2f" % c for c in (forces > 0).mean(axis=1)))
    assert (forces.max(axis=1) > 0).all() and np.isfinite(ref[-1][6][2]) and np.isnan(ref[-1][6][[0, 1, 3, 4]]).all()  # every junction pushes; the damped one carries
    assert max(np.abs(blk[1]).max() for blk in ref) > 0
    got, cols, _ = _mixed_run(use_double, renderers, frames, "observed", [])
    _same_blocks(ref, got, n_off)
    assert _same(ref_cols, cols)


@PRECISIONS
@SHAPES
def test_pickups_on_junction_objects_observe(use_double, renderers, frames):
    ref, ref_cols, n_off = _mixed_run(use_double, renderers, frames, "damped", [])
    one, one_cols, _ = _mixed_run(use_double, renderers, frames, "observed", _mixed_pickups(1))
    nine, nine_cols, _ = _mixed_run(use_double, renderers, frames, "observed", _mixed_pickups(9))
    _same_blocks(ref, one, n_off)
    _same_blocks(ref, nine, n_off)
    assert _same(ref_cols, one_cols) and _same(ref_cols, nine_cols)
    ninth = n_off + 9 * np.arange(len(MIXED_ON)) + 8
    for blk, (a, b) in enumerate(zip(one, nine)):
        assert (a[2] == 1).all(), blk
        kept = np.ones(len(b[2]), bool)
        kept[ninth] = False
        assert (b[2][kept] == 1).all() and (b[2][ninth] == 0).all() and not b[1][ninth].any(), blk
        assert (np.abs(a[1][n_off:]).max(axis=1) > 0).all() and (np.abs(b[1][kept][n_off:]).max(axis=1) > 0).all(), blk  # every kept row sounds
        assert np.isfinite(b[1]).all()
        # the first pickup of every junction object: the same bits, alone on its object or with seven others
        assert np.array_equal(a[1][n_off:], b[1][n_off + 9 * np.arange(len(MIXED_ON))]), blk


@PRECISIONS
def test_the_older_entries_still_leave_such_pickups_out(use_double):
    on = _mixed_pickups(2)
    seen, _, n_off = _mixed_run(use_double, 1, 512, "observed", on, blocks=1)
    assert (seen[0][2] == 1).all() and (np.abs(seen[0][1][n_off:]).max(axis=1) > 0).all()
    for entry in ("damped", "coupled"):
        got, _, _ = _mixed_run(use_double, 1, 512, entry, on, blocks=1)
        assert (got[0][2][:n_off] == 1).all() and (got[0][2][n_off:] == 0).all() and not got[0][1][n_off:].any(), entry
    damped, _, _ = _mixed_run(use_double, 1, 512, "damped", on, blocks=1)
    _same_blocks(seen, damped, n_off)


# ---- 3. dead junctions, bit for bit ----
DEAD_LONE = [(oh.side(6, 1, direction=(1.0, 0.5, 0.25)), oh.side(8, 2, direction=(-1.0, -0.5, -0.25))),  # 14 and 4 further rows in block 0, none in block 1
             (oh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.0, -0.5)), None),  # 1
             (oh.side(1, 2, direction=(0.0, 1.0, 0.0)), None)]  # 2
DEAD_GROUP = [(oh.side(4, 3, direction=(0.5, 0.5, -1.0)), oh.side(9, 1, direction=(-0.5, -0.5, 1.0))),  # 5 and 2
              (oh.side(9, 0, direction=(0.25, -1.0, 0.5)), oh.side(2, 2, direction=(-0.25, 1.0, -0.5))),  # 2 and 3
              (oh.side(2, 1, direction=(1.0, 0.5, -0.25), coupling=2.0), None)]
DEAD_ON = [6, 8, 0, 1, 4, 9, 2]


def _dead_run(use_double, renderers, frames, variant):
    """Blocks 0 (every object excited: the junctions' objects carry 14, 4, 1, 2, 5, 2 and 3 further force rows) and 1 (none of them does)
    of the mixed drive scene with four pickups on each of the junctions' objects.  variant 'twin': render_read with a zero-signal drive in
    the place of every side; 'k0': K = 0 under a noise approach; 'open': K = 1e4 and u = -1e30; 'refused': the lone junctions with a
    negative coupling and K = 1e30 (C < 0, 1 + K C below 0) under a noise approach, the group's members at K = 0."""
    from mesheditor_amd import bank as hipbank
    sc, _ = dh.device_scene(drives_suite.MODES, drives_suite.T60, renderers, use_double)
    pickups = oh.probes_on(DEAD_ON)
    flip = (lambda sd: sd[:4] + (-sd[4],)) if variant == "refused" else (lambda sd: sd)
    stiff = {"k0": 0.0, "open": 1e4, "refused": 1e30}.get(variant, 0.0)
    lone = [dd.spec(flip(a), None if b is None else flip(b), stiff, damped=False) for a, b in DEAD_LONE]
    group = [gh.spec(a, b, 1e4 if variant == "open" else 0.0) for a, b in DEAD_GROUP]
    result = []
    for b in range(2):
        impacts, rows = _mixed_block(b, frames)
        for (o, p, d, gamma) in impacts:
            assert sc.enqueue(dh.one_sample_impact(hipbank.Event, o, p, d, gamma))
        out = np.zeros(frames, sc.dtype)
        if variant == "twin":
            rows = rows + [(sd[0], sd[1][0], sd[3], np.zeros(frames, np.float32)) for a, c in DEAD_LONE + DEAD_GROUP for sd in (a, c) if sd is not None]
            reads, flags = sc.render_read(out, *_drive_args(rows, frames), ph.records(pickups))
        else:
            u = np.full((6, frames), -1e30, np.float32) if variant == "open" else np.array([np.abs(_signal("noise", 40 + j, 2 * frames)[b * frames:(b + 1) * frames]) for j in range(6)], np.float32)
            reads, flags, forces, comp, status, _ = _render(sc, "observed", out, rows, pickups, oh.junction_records(lone, group), u, [0.0] * 6, None)
            assert list(status) == ([2, 2, 2, 1, 1, 1] if variant == "refused" else [1] * 6), (variant, b, list(status))
            assert not forces.any() and ((comp[:3] < 0).all() if variant == "refused" else (comp > 0).all()), (variant, b)
        result.append((out, reads.copy(), flags.copy(), [a.copy() for a in sc.object_state()], _states(sc)))
    sc.close()
    return result


@PRECISIONS
@SHAPES
def test_dead_and_refused_junctions_read_what_a_twin_with_zero_drives_reads(use_double, renderers, frames):
    twin = _dead_run(use_double, renderers, frames, "twin")
    assert all((blk[2] == 1).all() and (np.abs(blk[1]).max(axis=1) > 0).all() for blk in twin)
    for variant in ("k0", "open", "refused"):
        got = _dead_run(use_double, renderers, frames, variant)
        for b, (want, have) in enumerate(zip(twin, got)):
            assert (have[2] == 1).all(), (variant, b)
            bad = [q for q in range(len(want[1])) if not np.array_equal(want[1][q], have[1][q])]
            assert not bad, (variant, b, bad)
            assert np.array_equal(want[0], have[0]) and _same(want[3], have[3]) and _same(want[4], have[4]), (variant, b)


# ---- 4. replay (fp32) ----
def _kinds(kind, k, single=False, lam=None):
    """(lone specs, group specs, hertz per junction, the bystander) of a scene kind on observed_harness.MODES: 'lone' -- a two-sided linear
    junction and a one-sided Hertz one --, 'damped' -- the same two, damped --, 'group' -- observed_harness.group_specs."""
    if kind == "group":
        return [], oh.group_specs(k, single), (False, False, False), 3
    return oh.lone_specs(k, damped=(kind == "damped",) * 2, single=single), [], (False, True), 1


@functools.lru_cache(maxsize=None)
def _rung_plan(kind, frames, blocks):
    """(u, C per junction) for a scene rung up by two blocks of noise drives and then left to its junctions: the largest free deflection
    of the first block after the ring-up and the compliances, from a float64 restatement on the bank's columns (no device)."""
    cols = oh.HostColumns(oh.MODES, oh.T60, False)
    scout = oh.Damped(cols, oh.MODES, np.float64, cols.dtype)
    for b in range(2):
        scout.render_damped(oh.drive_rows(range(4), b, frames, 2), [], np.zeros((0, frames), np.float32), [], None, frames)
    lone, group, _, _ = _kinds(kind, [0.0] * 3, True)
    specs = lone + [dd.spec(s[0], s[1], 0.0, damped=False) for s in group]
    trace = {}
    scout.render_damped([], specs, np.zeros((len(specs), frames), np.float32), [0.0] * len(specs), None, frames, trace)
    return junctions_suite._approach(np.abs(trace["d"]).max(axis=1), frames, blocks, amp=1.0), [float(scout.compliance(s[:4])) for s in specs]


@SHAPES
@pytest.mark.parametrize("kc", [1.0, 30.0])
@pytest.mark.parametrize("kind", ["lone", "damped", "group"])
def test_the_force_rows_replayed_as_drives_give_the_pickup_rows(renderers, frames, kc, kind):
    """Two identical fp32 scenes rung up by noise drives for two blocks.  Then three blocks in which scene A carries the junctions (single
    points; K C = kc, Hertz: K C sqrt(x0) = kc; damped: l x0 = 1, the carry passed on), a drive on the bystander and, on every junction
    object, pickups of advance 0, 1 and 2 and an advance-1 blend; scene B carries the returned force rows as drives, through render_read
    with the same pickups.  An object with one side carries one row in B, and (z c + +0) + a f and z c + (+0 + f g) are the same bits:
    its pickup rows are array_equal block after block, and with lone junctions so are out and every state.  An object of a group with two
    members' sides (objects 1 and 2 here) adds a_i f_i one after another where B sums the drives' products first: it carries another row,
    the replay of DESIGN.md section 3e is close there, not equal, and its rows are not compared here (tests 5 and 6 hold them)."""
    blocks = 3
    u, comp = _rung_plan(kind, frames, blocks)
    x0 = u.max(axis=1)
    hertz = _kinds(kind, [0.0] * 3)[2]
    lone, group, _, bystander = _kinds(kind, [kc / (c * (np.sqrt(float(x)) if h else 1.0)) for c, x, h in zip(comp, x0, hertz)], True)
    lam = [1.0 / float(x) if kind == "damped" else 0.0 for x in x0]
    specs = lone + group
    sides = {}
    for s in specs:
        for sd in (s[0], s[1]):
            if sd is not None:
                sides[sd[0]] = sides.get(sd[0], 0) + 1
    pickups = oh.probes_on(sorted(sides))
    exact_rows = [q for q, p in enumerate(pickups) if sides[p[0]] == 1]
    assert exact_rows
    a, _ = dh.device_scene(oh.MODES, oh.T60, renderers, False)
    b, _ = dh.device_scene(oh.MODES, oh.T60, renderers, False)
    for blk in range(2):
        for sc in (a, b):
            sc.render_driven(np.zeros(frames, np.float32), *_drive_args(oh.drive_rows(range(4), blk, frames, 2), frames))
    assert _same(_states(a), _states(b))
    carry, contact = None, []
    for blk in range(blocks):
        rows = [(bystander,) + dh.row_direction(bystander) + (_signal("sweep", bystander, blocks * frames)[blk * frames:(blk + 1) * frames],)]
        ub = u[:, blk * frames:(blk + 1) * frames]
        out_a, out_b = np.zeros(frames, np.float32), np.zeros(frames, np.float32)
        reads, flags, forces, _, status, carry = _render(a, "observed", out_a, rows, pickups, oh.junction_records(lone, group), ub, lam, carry)
        assert (status == 1).all() and (flags == 1).all() and np.isfinite(forces).all()
        replay = rows + [(sd[0], sd[1][0], sd[3], forces[j]) for j, s in enumerate(specs) for sd in (s[0], s[1]) if sd is not None]
        twin_reads, twin_flags = b.render_read(out_b, *_drive_args(replay, frames), ph.records(pickups))
        assert (twin_flags == 1).all() and (np.abs(twin_reads).max(axis=1) > 0).all()
        bad = [q for q in exact_rows if not np.array_equal(reads[q], twin_reads[q])]
        assert not bad, (blk, bad)
        if kind != "group":
            assert np.array_equal(out_a, out_b) and _same(_states(a), _states(b)), blk
        contact.append((forces > 0).mean(axis=1))
    a.close()
    b.close()
    share = np.mean(contact, axis=0)
    print("replay, %s, K C = %g, %d renderers, %d frames: in contact %s" % (kind, kc, renderers, frames, " ".join("%.2f" % c for c in share)))
    assert (share > 0.02).all() and (share < 0.98).all(), share


# ---- 5. the law where it is solved ----
@functools.lru_cache(maxsize=None)
def _device_compliances(use_double, kind):
    """The C each junction of the kind returns, from a scene of its own (one block with K = 0)."""
    sc, _ = dh.device_scene(oh.MODES, oh.T60, 1, use_double)
    lone, group, _, _ = _kinds(kind, [0.0] * 3)
    n = len(lone) + len(group)
    _, _, forces, comp, status, _ = _render(sc, "observed", np.zeros(512, sc.dtype), [], [], oh.junction_records(lone, group), np.ones((n, 512), np.float32), [0.0] * n, None)
    sc.close()
    assert (status == 1).all() and (comp > 0).all() and not forces.any()
    return [float(c) for c in comp]


def _law_figures(u, reads, owners, forces, specs, lam, carries, frames):
    """(the largest deviation of f from the law at y' = u - sum_sides read1 over the row's peak; the largest deviation of a damped junction's
    carry from the block's last y' over the peak of |y'|), in longdouble on the numbers given, over the run's blocks concatenated.  A
    block's first frame takes the last y' of the block before as y_p; the run's first frame has no history."""
    n = len(specs)
    R = np.zeros((n, u.shape[1]), L)
    for j, row in zip(owners, reads):
        R[j] += np.asarray(row, L)
    y = np.asarray(u, L) - R
    law_fig = carry_fig = 0.0
    for j, s in enumerate(specs):
        damped = len(s) > 5 and bool(s[5]) and lam[j] > 0
        l = np.concatenate([[L(0)], np.full(y.shape[1] - 1, L(lam[j]) if damped else L(0))])
        yp = np.concatenate([[L(0)], y[j][:-1]])
        want = oh.law(y[j], yp, l, L(np.float32(s[2])), bool(s[4]))
        f = np.asarray(forces[j], L)
        assert np.abs(f).max() > 0
        law_fig = max(law_fig, float(np.abs(f - want).max() / np.abs(f).max()))
        if damped:
            for b, c in enumerate(carries):
                carry_fig = max(carry_fig, float(abs(L(c[j]) - y[j][(b + 1) * frames - 1]) / np.abs(y[j]).max()))
    return law_fig, carry_fig


@PRECISIONS
@SHAPES
@pytest.mark.parametrize("kind", ["lone", "damped", "group"])
def test_the_force_is_the_law_at_the_compression_the_pickups_of_the_same_call_read(use_double, renderers, frames, kind):
    """observed_harness.against_plan's scene -- a noise drive on every object, junction objects included -- with K C = 10 (Hertz:
    K C sqrt(x0) = 10; damped: l x0 = 1) and an advance-1 pickup at every side, two blocks with the carry passed on.  Figure: the largest
    deviation of f[s] from K phi(y'[s]) max(1 + l (y'[s] - y'[s-1]), 0), y' = u - sum_sides read1, over the row's peak; a damped junction's
    returned carry against the block's last y' over the peak of |y'|.  The device's figure against the same figure of the working-precision
    restatement of the same run on its own rows (tests/observed_harness.py), bound 4 x.

    Measured on an MI355X: DESIGN.md section 3g (this test prints the figures)."""
    blocks = 2
    comp = _device_compliances(use_double, kind)
    sc, _ = dh.device_scene(oh.MODES, oh.T60, renderers, use_double)
    specs, _, rows, u = oh.against_plan(sc, "group" if kind == "group" else "lone", 10.0, comp, frames, blocks)
    lam = [0.0] * len(specs)
    if kind == "damped":
        specs = oh.lone_specs([s[2] for s in specs], damped=(True, True))
        lam = [1.0 / float(x) for x in u.max(axis=1)]
    formed = _damping(lam)[1]  # what the entry makes of it: the restatement's l
    lone, group = ([], specs) if kind == "group" else (specs, [])
    sides = oh.side_pickups(specs)
    owners, pickups = [j for j, _ in sides], [p for _, p in sides]
    working = (oh.Grouped if kind == "group" else oh.Damped)(sc, oh.MODES, sc.dtype, sc.dtype)
    dev, plain = {"reads": [], "forces": [], "carry": []}, {"reads": [], "forces": [], "carry": []}
    carry = carry_w = None
    for b in range(blocks):
        ub = u[:, b * frames:(b + 1) * frames]
        reads, flags, forces, _, status, carry = _render(sc, "observed", np.zeros(frames, sc.dtype), rows[b], pickups, oh.junction_records(lone, group), ub, lam, carry)
        assert (status == 1).all() and (flags == 1).all() and np.isfinite(forces).all()
        if kind == "group":
            (_, f_w, _, _), r_w = working.observed(working.render_grouped, pickups, rows[b], specs, ub, frames)
        else:
            (_, f_w, _, _, carry_w), r_w = working.observed(working.render_damped, pickups, rows[b], specs, ub, formed, carry_w, frames)
        for store, (r, f, c) in ((dev, (reads, forces, carry)), (plain, (r_w, f_w, carry_w))):
            store["reads"].append(np.array(r)), store["forces"].append(np.array(f)), store["carry"].append(None if c is None else np.array(c))
    sc.close()
    figures = []
    for store in (dev, plain):
        figures.append(_law_figures(u, np.concatenate(store["reads"], axis=1), owners, np.concatenate(store["forces"], axis=1), specs, formed, store["carry"], frames))
    (law_dev, carry_dev), (law_plain, carry_plain) = figures
    share = (np.concatenate(dev["forces"], axis=1) > 0).mean(axis=1)
    print("the law where it is solved, %s, %s, %d renderers, %d frames: device %.3e, restatement %.3e (%.2f x); carry device %.3e, restatement %.3e; in contact %s" %
          ("fp64" if use_double else "fp32", kind, renderers, frames, law_dev, law_plain, law_dev / law_plain, carry_dev, carry_plain, " ".join("%.2f" % c for c in share)))
    eps = float(np.finfo(sc.dtype).eps)
    assert (share > 0.05).all() and (share < 0.95).all(), share
    assert 0 < law_plain < 1e6 * eps and law_dev <= BOUND * law_plain, (law_dev, law_plain)
    if kind == "damped":
        assert 0 < carry_plain < 1e6 * eps and carry_dev <= BOUND * carry_plain, (carry_dev, carry_plain)


# ---- 6. against longdouble ----
@PRECISIONS
@SHAPES
@pytest.mark.parametrize("kc", [1.0, 100.0])
@pytest.mark.parametrize("kind", ["lone", "group"])
def test_pickup_rows_match_a_longdouble_restatement(use_double, renderers, frames, kc, kind):
    """observed_harness.against_plan: objects of 37, 64, 130 and 256 modes, a noise drive on each, 'lone' -- a two-sided linear junction
    (one side at a blend) and a one-sided Hertz one -- or 'group' -- three linear members on three objects --, K from the returned C with
    K C = kc (Hertz: K C sqrt(x0)); on every junction object pickups of advance 0, 1 and 2 and an advance-1 blend; two blocks.  The
    longdouble run is in contact at every junction for between 15 % and 85 % of the frames (asserted; on the CPU by
    tests/test_bank_observed_cpu.py).  Figures: the largest deviation of a pickup row / a force row / the samples from the longdouble
    restatement's over the row's peak -- the device's, and the working-precision restatement's (sums in the contract's order).  Bound 4 x.

    Measured on an MI355X: DESIGN.md section 3g (this test prints the figures)."""
    blocks = 2
    comp = _device_compliances(use_double, kind)
    sc, _ = dh.device_scene(oh.MODES, oh.T60, renderers, use_double)
    specs, pickups, rows, u = oh.against_plan(sc, kind, kc, comp, frames, blocks)
    lone, group = ([], specs) if kind == "group" else (specs, [])
    exact, working = ((oh.Grouped if kind == "group" else oh.Damped)(sc, oh.MODES, t, sc.dtype) for t in (L, sc.dtype))
    fig = {"reads": [0.0, 0.0], "force": [0.0, 0.0], "out": [0.0, 0.0]}
    closed = []
    for b in range(blocks):
        ub = u[:, b * frames:(b + 1) * frames]
        out = np.zeros(frames, sc.dtype)
        reads, flags, forces, _, status, _ = _render(sc, "observed", out, rows[b], pickups, oh.junction_records(lone, group), ub, [0.0] * len(specs), None)
        assert (status == 1).all() and (flags == 1).all()
        want_out, want_f, want_r = oh.against_run(exact, kind, specs, pickups, rows[b], ub, frames)
        plain_out, plain_f, plain_r = oh.against_run(working, kind, specs, pickups, rows[b], ub, frames)
        closed.append((np.asarray(want_f) > 0).mean(axis=1))
        for key, got, yard, ref in (("reads", reads, plain_r, want_r), ("force", forces, plain_f, want_f), ("out", out[None, :], plain_out[None, :], want_out[None, :])):
            fig[key][0] = max(fig[key][0], _figure(got, ref))
            fig[key][1] = max(fig[key][1], _figure(yard, ref))
    sc.close()
    share = np.mean(closed, axis=0)
    print("%s, %s, K C = %g, %d renderers, %d frames: " % ("fp64" if use_double else "fp32", kind, kc, renderers, frames) +
          ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()) +
          "; in contact " + " ".join("%.2f" % c for c in share))
    assert ((share >= 0.15) & (share <= 0.85)).all(), share
    eps = float(np.finfo(sc.dtype).eps)
    for key, (device, yardstick) in fig.items():
        assert 0 < yardstick < 1e6 * eps, (key, yardstick)
        assert device <= BOUND * yardstick, (key, device, yardstick)


# ---- 7. full width ----
WIDE = [640, 384, 64]  # five waves and three: the whole workgroup; a bystander


def _wide_specs(k):
    return [dd.spec(oh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), oh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), k, damped=False)]


def _wide_pickups():
    return [pickups_suite._some_pickup(o, i) for o in (0, 1) for i in range(8)]


def test_a_junction_of_eight_waves_is_read_and_replays_in_fp32():
    """640 + 384 modes rung up by noise drives for two blocks; then one block of 512 frames with the junction (K C = 10 with the returned
    C), eight pickups on each object and a drive on the bystander alone: status solved; the rows array_equal to those of the twin that is
    driven by the returned force row; out and states array_equal to the same call without pickups."""
    frames = 512
    scenes = [dh.device_scene(WIDE, oh.T60, 1, False)[0] for _ in range(4)]
    for blk in range(2):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, 2 * frames)[blk * frames:(blk + 1) * frames],) for o in range(3)]
        for sc in scenes:
            sc.render_driven(np.zeros(frames, np.float32), *_drive_args(rows, frames))
    scout, a, bare, twin = scenes
    free = scout.render_observed(np.zeros(frames, np.float32), [], np.zeros((0, frames), np.float32), ph.records([oh.side_pickup(sd) for sd in _wide_specs(0.0)[0][:2]]),
                                 dd.records(_wide_specs(0.0)), np.zeros((1, frames), np.float32))
    assert free[4][0] == 1 and free[3][0] > 0
    x0 = float(np.abs(free[0][0] + free[0][1]).max())  # the free deflection at the junction: the sides' advance-1 reads without contact
    specs = _wide_specs(10.0 / float(free[3][0]))
    u = junctions_suite._approach([x0], frames, 1, amp=1.0)
    rows = [(2,) + dh.row_direction(2) + (_signal("sweep", 2, frames),)]
    out_a, out_bare, out_twin = (np.zeros(frames, np.float32) for _ in range(3))
    reads, flags, forces, _, status, _ = _render(a, "observed", out_a, rows, _wide_pickups(), dd.records(specs), u, [0.0], None)
    _, _, forces_bare, _, status_bare, _ = _render(bare, "observed", out_bare, rows, [], dd.records(specs), u, [0.0], None)
    assert list(status) == [1] and list(status_bare) == [1] and (flags == 1).all() and 0.05 < (forces > 0).mean() < 0.95
    assert np.array_equal(forces, forces_bare) and np.array_equal(out_a, out_bare) and _same(_states(a), _states(bare))
    replay = rows + [(sd[0], sd[1][0], sd[3], forces[0]) for sd in specs[0][:2]]
    twin_reads, twin_flags = twin.render_read(out_twin, *_drive_args(replay, frames), ph.records(_wide_pickups()))
    assert (twin_flags == 1).all() and (np.abs(twin_reads).max(axis=1) > 0).all()
    bad = [q for q in range(16) if not np.array_equal(reads[q], twin_reads[q])]
    assert not bad, bad
    assert np.array_equal(out_a, out_twin) and _same(_states(a), _states(twin))
    for sc in scenes:
        sc.close()


def test_a_junction_of_eight_waves_is_read_in_fp64():
    """640 + 384 modes under noise drives, the junction at K C = 10 with the returned C, eight pickups on each object, one block of 512
    frames: status solved, the rows within 4 x the float64 restatement's own deviation from the longdouble one, and out and states
    array_equal to the same call without pickups."""
    frames = 512
    a, _ = dh.device_scene(WIDE, oh.T60, 1, True)
    bare, _ = dh.device_scene(WIDE, oh.T60, 1, True)
    scout, _ = dh.device_scene(WIDE, oh.T60, 1, True)
    rows = [(o,) + dh.row_direction(o) + (_signal("noise", o, frames),) for o in range(3)]
    probe = oh.Damped(scout, WIDE, np.float64, np.float64)
    trace = {}
    _, _, c_probe, _, _ = probe.render_damped(rows, _wide_specs(0.0), np.zeros((1, frames), np.float32), [0.0], None, frames, trace)
    comp = scout.render_observed(np.zeros(frames, np.float64), [], np.zeros((0, frames), np.float32), [], dd.records(_wide_specs(0.0)), np.zeros((1, frames), np.float32))[3]
    scout.close()
    assert comp[0] > 0 and abs(comp[0] - c_probe[0]) < 1e-9 * comp[0]
    specs = _wide_specs(10.0 / float(comp[0]))
    u = oh.approach(np.sqrt((np.asarray(trace["d"], np.float64) ** 2).mean(axis=1)), frames, 1)
    pickups = _wide_pickups()
    out_a, out_bare = np.zeros(frames, np.float64), np.zeros(frames, np.float64)
    reads, flags, forces, _, status, _ = _render(a, "observed", out_a, rows, pickups, dd.records(specs), u, [0.0], None)
    _, _, forces_bare, _, _, _ = _render(bare, "observed", out_bare, rows, [], dd.records(specs), u, [0.0], None)
    assert list(status) == [1] and (flags == 1).all() and 0.05 < (forces > 0).mean() < 0.95
    assert np.array_equal(forces, forces_bare) and np.array_equal(out_a, out_bare) and _same(_states(a), _states(bare))
    exact, working = (oh.Damped(a, WIDE, t, np.float64) for t in (L, np.float64))
    (_, want_f, _, _, _), want = exact.observed(exact.render_damped, pickups, rows, specs, u, [0.0], None, frames)
    (_, plain_f, _, _, _), plain = working.observed(working.render_damped, pickups, rows, specs, u, [0.0], None, frames)
    a.close()
    bare.close()
    device, yardstick = _figure(reads, want), _figure(plain, want)
    print("full width, fp64: pickup rows device %.3e / restatement %.3e (%.2f x); force rows device %.3e / restatement %.3e" %
          (device, yardstick, device / yardstick, _figure(forces, want_f), _figure(plain_f, want_f)))
    assert 0 < yardstick < 1e6 * float(np.finfo(np.float64).eps) and device <= BOUND * yardstick, (device, yardstick)


# ---- 8. independence ----
def _independent_run(use_double, renderers, crowd, bystanders, blocks=2, frames=512):
    """Objects 0 (130 modes) and 1 (64) joined by a two-sided junction, object 2 (256) under a one-sided Hertz one, every object driven;
    K from fixed numbers (no scout: every run takes the same records).  The watched pickups: one per junction object (advance 1, 2 and 0).
    crowd: seven further pickups on each of those objects, ahead of nothing -- the watched ones stay first on their objects.  bystanders:
    three further objects with a junction, drives and pickups of their own, and a further group.  Returns the watched rows, block after block."""
    modes = [130, 64, 256] + ([37, 200, 129, 64, 64] if bystanders else [])
    sc, _ = dh.device_scene(modes, 0.5, renderers, use_double)
    lone = [dd.spec(oh.side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), oh.side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), 2e7, damped=False),
            dd.spec(oh.side(2, (3, 0, 1), (0.5, 0.25, 0.25), oh.NORMAL, 2.0), None, 5e9, hertz=True, damped=False)]
    group = []
    watched = [ph.spec(0, 2, direction=oh.NORMAL, advance=1), ph.spec(1, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.0, -0.5), 1.5, 2), ph.spec(2, 0, direction=(0.5, 0.5, -1.0), advance=0)]
    pickups = list(watched)
    if crowd:
        pickups += [pickups_suite._some_pickup(o, i) for o in range(3) for i in range(7)]
    if bystanders:
        lone = [dd.spec(oh.side(4, 0, direction=oh.NORMAL), oh.side(5, 1, direction=oh.NORMAL), 1e7, damped=True)] + lone
        group = [gh.spec(oh.side(6, 0, direction=oh.NORMAL), oh.side(7, 1, direction=oh.NORMAL), 1e7), gh.spec(oh.side(7, 2, direction=(1.0, 0.5, -0.25)), None, 1e7)]
        pickups = [ph.spec(3, 1, direction=oh.NORMAL, advance=1), ph.spec(4, 1, direction=oh.NORMAL, advance=2)] + pickups + [ph.spec(7, 0, direction=oh.NORMAL)]
    first, first_junction = (2, 1) if bystanders else (0, 0)
    n = len(lone) + len(group)
    periods = ([700.0] if bystanders else []) + [600.0, 500.0] + ([800.0, 900.0] if bystanders else [])  # the watched junctions' approach is the same in every run
    rows_out, carry = [], None
    for b in range(blocks):
        rows = [(o,) + dh.row_direction(o) + (_signal("noise" if o % 2 else "sweep", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))]
        u = np.array([(2e-5 * np.sin(2 * np.pi * (np.arange(frames) + b * frames) / periods[j])).astype(np.float32) for j in range(n)])
        lam = [1e4] + [0.0] * (n - 1) if bystanders else [0.0] * n
        reads, flags, forces, _, status, carry = _render(sc, "observed", np.zeros(frames, sc.dtype), rows, pickups, oh.junction_records(lone, group), u, lam, carry)
        assert (status == 1).all() and (flags == 1).all() and np.isfinite(forces).all()
        assert (forces[first_junction:first_junction + 2].max(axis=1) > 0).all()  # both watched junctions push
        rows_out.append(reads[first:first + 3].copy())
    sc.close()
    return np.concatenate(rows_out, axis=1)


@PRECISIONS
def test_a_junction_objects_pickup_row_depends_on_nothing_else(use_double):
    ref = _independent_run(use_double, 1, False, False)
    assert (np.abs(ref).max(axis=1) > 0).all() and np.isfinite(ref).all()
    for what, got in (("a second run", _independent_run(use_double, 1, False, False)), ("four renderers", _independent_run(use_double, 4, False, False)),
                      ("seven other pickups on its object", _independent_run(use_double, 1, True, False)), ("bystanders", _independent_run(use_double, 1, False, True)),
                      ("bystanders, a crowd and four renderers", _independent_run(use_double, 4, True, True))):
        assert np.array_equal(ref, got), what
