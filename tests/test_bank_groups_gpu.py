"""GPU tests of junction groups (Junction.of(shared=True) -> RenderModalCoupled -> mh_bank_render_coupled -> k_bank_modes_grouped).

Scenes: objects of 32, 130 and 256 modes (one wave with idle lanes, two waves with a nearly empty second, two full waves), T60 2 s, noise
drives.  Shapes: (a) a star -- the 130-mode hub with three junctions: to the 32-mode object, to the 256-mode object at a blend, to an
exciter; (b) a chain 32 - 130 - 256; (c) four exciter junctions on the 32-mode object; (d) two junctions between the same pair.

1. The second flagged junction on the hub is solved (status 1, a row that is not zero); without the feature it is left out.
2. The flag on lone junctions, linear and Hertz, changes no bit.
3. An unflagged junction beside a flagged one on the same object: whichever is second is left out.
4. A dead group observes: K = 0, and u = -1e30, are the run with zero-signal drives in the junctions' places, also on a silent hub.
5. Members gated apart, one in contact per block: the bits of the call with the others dead, and the restatement's row within the bound.
6. Replay: the rows as drives on a twin give the leaves' states bit for bit, and meet the law against advance-1 pickups.
7. Force rows, samples and C_ii against the numpy.longdouble restatement (tests/group_harness.py), K C = 0.1 ... 100.
8. A second run, the renderer count, bystanders, scaling by 2, and the order of the members.
9. The new left-out kinds.  10. A group that would amplify is refused."""
import numpy as np
import pytest

from tests import drive_harness as dh
from tests import group_harness as gh
from tests import pickup_harness as ph
from tests import test_bank_drives_gpu as drives_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
BOUND = 4  # x the working-precision restatement's own deviation: the project's bound for drives, pickups and junctions
FRAMES = 512
MODES, T60 = [32, 130, 256], 2.0
NORMAL = (0.25, -1.0, 0.5)
_signal = drives_suite._signal


def _push(d):
    return tuple(-v for v in d)


def _shape(name, k, single_points=False, **flags):
    """The junctions of a shape as specs, stiffnesses k (one per member)."""
    d0, d1, d2, d3 = (1.0, 0.5, -0.25), NORMAL, (0.5, 0.5, -1.0), (0.0, 1.0, 0.25)
    blend = ((1, 1, 1), (1.0, 0.0, 0.0)) if single_points else ((3, 0, 1), (0.5, 0.25, 0.25))
    if name == "star":
        sides = [(gh.side(1, 1, direction=d0, coupling=1.5), gh.side(0, 2, direction=_push(d0), coupling=1.5)),
                 (gh.side(1, 2, direction=d1, coupling=2.0), gh.side(2, blend[0], blend[1], _push(d1), 2.0)),
                 (gh.side(1, 3, direction=d2), None)]
    elif name == "chain":
        sides = [(gh.side(0, 1, direction=d0, coupling=1.5), gh.side(1, 3, direction=_push(d0), coupling=1.5)),
                 (gh.side(1, 0, direction=d1, coupling=2.0), gh.side(2, 2, direction=_push(d1), coupling=2.0))]
    elif name == "four":
        # (directions for which no C_ij is above 0.3 sqrt(C_ii C_jj): with d0 ... d3 one of them is 1.06, and K C = 100 leaves the float32
        # restatement 10 % of the peak away from the longdouble one -- no yardstick)
        sides = [(gh.side(0, p, direction=d, coupling=1.0 + 0.5 * p), None) for p, d in enumerate(((0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, -1.0, 0.0)))]
    elif name == "pair":
        sides = [(gh.side(0, 0, direction=d0, coupling=1.5), gh.side(1, 1, direction=_push(d0), coupling=1.5)),
                 (gh.side(0, 3, direction=d1, coupling=2.0), gh.side(1, 2, direction=_push(d1), coupling=2.0))]
    return [gh.spec(a, b, k[i], **flags) for i, (a, b) in enumerate(sides)]


SIZES = {"star": 3, "chain": 2, "four": 4, "pair": 2}


def _drive_args(rows, frames):
    return [(o, p) + tuple(float(v) for v in d) for (o, p, d, f) in rows], np.array([f for (_, _, _, f) in rows], np.float32).reshape(len(rows), frames)


def _states(sc):
    return [sc.column("StateRe"), sc.column("StateIm")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _noise_rows(modes, b, blocks, frames, scale=1.0):
    return [(o,) + dh.row_direction(o) + (np.float32(scale) * _signal("noise", o, blocks * frames)[b * frames:(b + 1) * frames],) for o in range(len(modes))]


_COMPLIANCES = {}


def _compliances(name, use_double, modes=MODES):
    """The C_ii each member of a shape returns, from a scene of its own (one block with K = 0); status 1 throughout."""
    key = (name, use_double, tuple(modes))
    if key not in _COMPLIANCES:
        n = SIZES[name]
        sc, _ = dh.device_scene(modes, T60, 1, use_double)
        _, _, forces, comp, status = sc.render_coupled(np.zeros(FRAMES, sc.dtype), [], np.zeros((0, FRAMES), np.float32), [], gh.records(_shape(name, [0.0] * n)), np.ones((n, FRAMES), np.float32))
        sc.close()
        assert (status == 1).all() and (comp > 0).all() and not forces.any(), (status, comp)
        _COMPLIANCES[key] = comp
    return _COMPLIANCES[key]


def _approach(free, frames, blocks, amp=3.0, period=400.0, phase=0.5):
    """The junction tests' approach -- a slow sine per member, `amp` times its free deflection `free`, raised a little -- with one period
    and a phase per member: the members close one after another and open one after another, so the empty set, the full set and the sets
    in between all occur."""
    t = np.arange(blocks * frames)
    return np.array([(amp * a * (np.sin(2 * np.pi * t / period - phase * j) + 0.1)).astype(np.float32) for j, a in enumerate(free)])


def _run(name, use_double, renderers, kc=10.0, blocks=2, frames=FRAMES, scale=1.0, modes=MODES, order=None, k_scale=None, extra=()):
    """A shape under noise drives on every object and the approach above, K_i C_ii = kc; extra: further junction specs behind the group.
    order: a permutation of the members.  Returns (forces [n + len(extra)][blocks * frames], out, states, comp, status, object_state)."""
    comp = _compliances(name, use_double)
    n = SIZES[name]
    specs = _shape(name, [(kc if k_scale is None else kc * k_scale[i]) / c for i, c in enumerate(comp)])
    u = np.float32(scale) * _approach([2e-5] * n, frames, blocks)
    if order is not None:
        specs, u = [specs[i] for i in order], u[list(order)]
    specs = specs + list(extra)
    u = np.concatenate([u, np.float32(scale) * _approach([2e-5] * len(extra), frames, blocks, phase=1.1)]) if extra else u
    sc, _ = dh.device_scene(modes, T60, renderers, use_double)
    rows_f, outs = [], []
    for b in range(blocks):
        out = np.zeros(frames, sc.dtype)
        _, _, forces, c_dev, status = sc.render_coupled(out, *_drive_args(_noise_rows(modes, b, blocks, frames, scale), frames), [], gh.records(specs), u[:, b * frames:(b + 1) * frames])
        rows_f.append(forces.copy())
        outs.append(out)
    result = np.concatenate(rows_f, axis=1), np.concatenate(outs), _states(sc), c_dev, status, sc.object_state()
    sc.close()
    return result


# ---- 1. the feature ----
@PRECISIONS
def test_the_second_junction_on_the_hub_is_solved(use_double):
    forces, out, _, comp, status, _ = _run("star", use_double, 1)
    assert list(status) == [1, 1, 1], list(status)
    assert (np.abs(forces).max(axis=1) > 0).all() and np.isfinite(forces).all() and (forces >= 0).all()
    assert (comp > 0).all() and np.array_equal(comp, _compliances("star", use_double))


# ---- 2. the flag on lone junctions ----
@PRECISIONS
@RENDERERS
def test_the_flag_on_a_lone_junction_changes_nothing(use_double, renderers):
    modes = MODES + [64]

    def run(shared):
        specs = [gh.spec(gh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.5, -0.25), 1.5), gh.side(2, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5), 3e5, shared=shared),
                 gh.spec(gh.side(1, 1, direction=NORMAL, coupling=2.0), None, 2e9, hertz=True, shared=shared),
                 gh.spec(gh.side(3, 0, direction=NORMAL), None, 1e5, True, shared=shared)]
        sc, _ = dh.device_scene(modes, T60, renderers, use_double)
        got = []
        for b in range(2):
            out = np.zeros(FRAMES, sc.dtype)
            u = _approach([2e-5] * 3, FRAMES, 2)[:, b * FRAMES:(b + 1) * FRAMES]
            _, _, forces, comp, status = sc.render_coupled(out, *_drive_args(_noise_rows(modes, b, 2, FRAMES), FRAMES), [], gh.records(specs), u)
            got += [forces.copy(), comp.copy(), status.copy(), out] + _states(sc) + list(sc.object_state())
        sc.close()
        return got

    plain, flagged = run(False), run(True)
    assert list(plain[2]) == [1, 1, 1] and all(np.abs(plain[0][j]).max() > 0 for j in range(3))
    assert _same(plain, flagged)


# ---- 3. unflagged beside flagged ----
@PRECISIONS
def test_an_unflagged_junction_shares_its_objects_with_nobody(use_double):
    def run(specs):
        sc, _ = dh.device_scene(MODES, T60, 1, use_double)
        out = np.zeros(FRAMES, sc.dtype)
        u = _approach([2e-5] * len(specs), FRAMES, 1)
        _, _, forces, comp, status = sc.render_coupled(out, *_drive_args(_noise_rows(MODES, 0, 1, FRAMES), FRAMES), [], gh.records(specs), u)
        got = (forces, comp, status, [out] + _states(sc) + list(sc.object_state()))
        sc.close()
        return got

    for first_shared in (True, False):
        first = gh.spec(gh.side(1, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), gh.side(0, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5), 3e5, shared=first_shared)
        second = gh.spec(gh.side(1, 3, direction=NORMAL), None, 2e5, shared=not first_shared)
        forces, comp, status, rest = run([first, second])
        alone = run([first])
        assert list(status) == [1, 0] and comp[1] == 0 and not forces[1].any() and np.abs(forces[0]).max() > 0, first_shared
        assert np.array_equal(forces[0], alone[0][0]) and comp[0] == alone[1][0] and _same(rest, alone[3]), first_shared


# ---- 4. a dead group observes ----
@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("frames", [512, 333])
def test_a_dead_group_is_an_observer(use_double, renderers, frames):
    """The star on objects with T60 10 ms: driven in blocks 0 and 1, left alone until the hub has gone silent, the group present in blocks
    0, 1, 3, 9 and 10.  K = 0 under a lively u, and stiff members whose exciters are far away (u = -1e30), give zero rows, status 1, and
    the bits of the run with a zero-signal drive at every side in the group's place."""
    blocks, on = 11, {0, 1, 3, 9, 10}

    def run(variant):
        sc, _ = dh.device_scene(MODES, 0.01, renderers, use_double)
        specs = _shape("star", [0.0 if variant == "k0" else 1e6] * 3)
        sig, states = np.zeros(blocks * frames, sc.dtype), []
        for b in range(blocks):
            rows = _noise_rows(MODES, b, blocks, frames) if b < 2 else []
            drives, signals = _drive_args(rows, frames)
            out = sig[b * frames:(b + 1) * frames]
            if b not in on:
                sc.render_driven(out, drives, signals)
            elif variant == "drive":
                places = [(sd[0], sd[1][0]) + tuple(sd[3]) for s in specs for sd in (s[0], s[1]) if sd is not None]
                sc.render_driven(out, drives + places, np.concatenate([signals, np.zeros((len(places), frames), np.float32)]))
            else:
                u = np.array([_signal("noise", 40 + j, blocks * frames)[b * frames:(b + 1) * frames] for j in range(3)], np.float32) if variant == "k0" else np.full((3, frames), -1e30, np.float32)
                _, _, forces, comp, status = sc.render_coupled(out, drives, signals, [], gh.records(specs), u)
                assert list(status) == [1, 1, 1] and not forces.any() and (comp > 0).all(), (variant, b)
            states.append([a.copy() for a in sc.object_state()] + _states(sc))
        sc.close()
        return sig, states

    ref, ref_states = run("drive")
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    ring = np.array([s[2] for s in ref_states])
    assert ring[1, 1] == 1 and ring[8, 1] == 0  # the hub has gone silent before the group comes back
    for variant in ("k0", "open"):
        got, states = run(variant)
        assert np.array_equal(ref, got), variant
        for b in range(blocks):
            assert _same(ref_states[b], states[b]), (variant, b)


@PRECISIONS
def test_a_dead_group_on_objects_with_three_force_rows_is_an_observer(use_double):
    """The pair on two objects of 100 and 128 modes with three force rows each -- one more than the group kernel keeps in registers, so the
    third row's gains go through the wave's scratch row -- two blocks of 40 frames (a whole tile and a partial one at either tile size).
    K = 0 under a lively u, and stiff members whose exciters are far away, give zero rows, status 1, and the bits of the run with a
    zero-signal drive at every side in the group's place."""
    modes, frames, blocks = [100, 128], 40, 2
    directions = ((1.0, 0.5, -0.25), NORMAL, (0.5, 0.5, -1.0))

    def run(variant):
        sc, _ = dh.device_scene(modes, T60, 1, use_double)
        specs = _shape("pair", [0.0 if variant == "k0" else 1e6] * 2)
        sig, states = np.zeros(blocks * frames, sc.dtype), []
        for b in range(blocks):
            rows = [(o, p, directions[p], _signal("noise", 3 * o + p, blocks * frames)[b * frames:(b + 1) * frames]) for o in range(len(modes)) for p in range(3)]
            drives, signals = _drive_args(rows, frames)
            out = sig[b * frames:(b + 1) * frames]
            if variant == "drive":
                places = [(sd[0], sd[1][0]) + tuple(sd[3]) for s in specs for sd in (s[0], s[1])]
                sc.render_driven(out, drives + places, np.concatenate([signals, np.zeros((len(places), frames), np.float32)]))
            else:
                u = np.array([_signal("noise", 40 + j, blocks * frames)[b * frames:(b + 1) * frames] for j in range(2)], np.float32) if variant == "k0" else np.full((2, frames), -1e30, np.float32)
                _, _, forces, comp, status = sc.render_coupled(out, drives, signals, [], gh.records(specs), u)
                assert list(status) == [1, 1] and not forces.any() and (comp > 0).all(), (variant, b)
            states.append([a.copy() for a in sc.object_state()] + _states(sc))
        sc.close()
        return sig, states

    ref, ref_states = run("drive")
    assert np.abs(ref).max() > 0 and np.isfinite(ref).all()
    for variant in ("k0", "open"):
        got, states = run(variant)
        assert np.array_equal(ref, got), variant
        for b in range(blocks):
            assert _same(ref_states[b], states[b]), (variant, b)


# ---- 5. members gated apart ----
_GATED = {}
GATED_BLOCKS = 6


def _gated(use_double):
    """The star, K C = 10, six blocks: in block b only member b % 3 has an exciter near the surface (the slow sine, period 200, 10 x its
    free deflection); the others' are far away (u = -1e30).  The longdouble and working-precision runs, once per precision."""
    if use_double in _GATED:
        return _GATED[use_double]
    n, frames = SIZES["star"], FRAMES
    comp = _compliances("star", use_double)
    specs = _shape("star", [10.0 / c for c in comp])
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    exact, working, scout = (gh.Restatement(sc, MODES, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    sc.close()
    all_rows = [_noise_rows(MODES, b, GATED_BLOCKS, frames) for b in range(GATED_BLOCKS)]
    trace = {}
    scout.render_grouped(all_rows[0], [gh.spec(s[0], s[1], 0.0) for s in specs], np.zeros((n, frames), np.float32), frames, trace)
    near = _approach(np.sqrt((trace["d"] ** 2).mean(axis=1)), frames, GATED_BLOCKS, amp=10.0, period=200.0, phase=0.0)
    runs = []
    for b in range(GATED_BLOCKS):
        live = b % n
        u = np.full((n, frames), -1e30, np.float32)
        u[live] = near[live, b * frames:(b + 1) * frames]
        trace = {}
        want = exact.render_grouped(all_rows[b], specs, u, frames, trace)
        runs.append((live, u, want, trace["sets"].copy(), working.render_grouped(all_rows[b], specs, u, frames)))
    _GATED[use_double] = (specs, all_rows, runs)
    return _GATED[use_double]


@PRECISIONS
@RENDERERS
def test_members_gated_apart_act_alone(use_double, renderers):
    """A group whose members share no active frame.  Asserted on the longdouble run: in block b the active set is {b % 3} or empty in every
    frame, each in at least 5 % of them.  Then (a) the device run is array_equal -- force rows, C, statuses, samples, states,
    object_state(), block after block -- to the same call with the other members dead (K = 0): both go through the group kernel and take
    the subset {i}, whose M_{i} does not depend on the other members' stiffness; and (b), since M_{i} is formed by the group's
    elimination and not as step 4's (K x) / (1 + K C) (include/modalhip.h), the live member's row and the samples are held to the longdouble
    restatement by the working-precision restatement's own deviation, bound 4 x.

    Measured on an MI355X (this test prints them): force rows 0.35 - 0.38 x, samples 0.32 - 0.57 x the restatement's deviation."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    specs, all_rows, runs = _gated(use_double)
    n = len(specs)
    a, _ = dh.device_scene(MODES, T60, renderers, use_double)
    b, _ = dh.device_scene(MODES, T60, renderers, use_double)
    fig = {"force": [0.0, 0.0], "out": [0.0, 0.0]}
    for blk, (live, u, (want_out, want, _, want_status), sets, (plain_out, plain, _, _)) in enumerate(runs):
        alone = float((sets == 1 << live).mean())
        assert set(np.unique(sets).tolist()) == {0, 1 << live} and 0.05 <= alone <= 0.95, (blk, np.unique(sets), alone)
        assert list(want_status) == [1] * n
        others_dead = [s if j == live else gh.spec(s[0], s[1], 0.0) for j, s in enumerate(specs)]
        out_a, out_b = np.zeros(FRAMES, a.dtype), np.zeros(FRAMES, b.dtype)
        _, _, forces, comp, status = a.render_coupled(out_a, *_drive_args(all_rows[blk], FRAMES), [], gh.records(specs), u)
        _, _, forces_b, comp_b, status_b = b.render_coupled(out_b, *_drive_args(all_rows[blk], FRAMES), [], gh.records(others_dead), u)
        assert list(status) == [1] * n and list(status_b) == [1] * n, blk
        assert np.abs(forces[live]).max() > 0 and not np.delete(forces, live, axis=0).any(), blk
        assert np.array_equal(forces, forces_b) and np.array_equal(comp, comp_b) and np.array_equal(out_a, out_b), blk
        assert _same(_states(a), _states(b)) and _same(a.object_state(), b.object_state()), blk
        for got, yard, key, ref in ((forces[live:live + 1], plain[live:live + 1], "force", want[live:live + 1]), (out_a[None, :], plain_out[None, :], "out", want_out[None, :])):
            fig[key][0] = max(fig[key][0], gh.row_figure(got, ref))
            fig[key][1] = max(fig[key][1], gh.row_figure(yard, ref))
    a.close()
    b.close()
    print("%s, gated star, %d renderers: " % ("fp64" if use_double else "fp32", renderers) +
          ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()))
    for key, (device, yardstick) in fig.items():
        assert 0 < yardstick < 1e6 * eps, (key, yardstick)
        assert device <= BOUND * yardstick, (key, device, yardstick)


# ---- 6. replay ----
@RENDERERS
@pytest.mark.parametrize("name", ["star", "chain"])
def test_the_rows_replayed_as_drives_move_the_leaves_alike_and_meet_the_law(renderers, name):
    """Two identical fp32 scenes rung up by noise drives for two blocks; then three blocks in which scene A carries the group (single-point
    sides) and nothing else, and scene B the returned rows as drives, side by side.  An object with one side of one member (a leaf) carries
    one row in B: (z c + +0) + a f there and (z c + (+0 + f g)) here are the same bits, so its state is array_equal block after block.  The
    hub adds its members' a_i f_i one after another where the drives' products are summed first: it is close, not equal.  With an
    advance-1 pickup at every side of B: f_i[s] against K_i max(u_i[s] - sum_sides read1[s], 0), the largest deviation over the row's peak,
    against the same figure of the float32 restatement of the same run (bound 4 x, as in the junction tests)."""
    n = SIZES[name]
    comp = _compliances(name, False)
    specs = _shape(name, [10.0 / c for c in comp], single_points=True)
    a, _ = dh.device_scene(MODES, T60, renderers, False)
    b, _ = dh.device_scene(MODES, T60, renderers, False)
    working = gh.Restatement(a, MODES, np.float32, np.float32)
    for blk in range(2):
        rows = _noise_rows(MODES, blk, 2, FRAMES)
        for sc in (a, b):
            sc.render_driven(np.zeros(FRAMES, np.float32), *_drive_args(rows, FRAMES))
        working.render_coupled(rows, [], np.zeros((0, FRAMES), np.float32), FRAMES)
    assert _same(_states(a), _states(b))
    probe = gh.Restatement(a, MODES, np.float64, np.float32)
    probe.z = [(re.astype(np.float64), im.astype(np.float64)) for re, im in working.z]
    trace = {}
    probe.render_grouped([], [gh.spec(s[0], s[1], 0.0) for s in specs], np.zeros((n, FRAMES), np.float32), FRAMES, trace)
    u = _approach(np.abs(trace["d"]).max(axis=1), FRAMES, 3, amp=1.0)
    sides = [[sd for sd in (s[0], s[1]) if sd is not None] for s in specs]
    pickups = [sd + (1,) for group in sides for sd in group]
    count = {}
    for group in sides:
        for sd in group:
            count[sd[0]] = count.get(sd[0], 0) + 1
    leaves = [o for o, c in count.items() if c == 1]
    assert leaves
    starts = np.cumsum([0] + MODES)
    device, yardstick, contact = 0.0, 0.0, []
    for blk in range(3):
        ub = u[:, blk * FRAMES:(blk + 1) * FRAMES]
        out_a, out_b = np.zeros(FRAMES, np.float32), np.zeros(FRAMES, np.float32)
        _, _, forces, _, status = a.render_coupled(out_a, [], np.zeros((0, FRAMES), np.float32), [], gh.records(specs), ub)
        assert list(status) == [1] * n
        replay = [(sd[0], sd[1][0], sd[3], forces[j]) for j, group in enumerate(sides) for sd in group]
        reads, flags = b.render_read(out_b, *_drive_args(replay, FRAMES), ph.records(pickups))
        assert (flags == 1).all()
        for o in leaves:
            for col_a, col_b in zip(_states(a), _states(b)):
                assert np.array_equal(col_a[starts[o]:starts[o + 1]], col_b[starts[o]:starts[o + 1]]), (blk, o)
        assert np.abs(out_a - out_b).max() <= 3 * FRAMES * float(np.finfo(np.float32).eps) * np.abs(out_a).max()  # (an ulp per frame on the hub, three blocks)
        trace = {}
        _, plain, _, _ = working.render_grouped([], specs, ub, FRAMES, trace)
        at = 0
        for j, group in enumerate(sides):
            read1 = sum(reads[at + i].astype(np.longdouble) for i in range(len(group)))
            at += len(group)
            k = np.longdouble(np.float32(specs[j][2]))
            law = k * np.maximum(ub[j].astype(np.longdouble) - read1, 0)
            law_plain = k * np.maximum(ub[j].astype(np.longdouble) - trace["read1"][j].astype(np.longdouble), 0)
            contact.append(float((forces[j] > 0).mean()))
            peak = np.abs(forces[j]).max()
            if peak == 0 or np.abs(plain[j]).max() == 0:
                continue
            device = max(device, float(np.abs(forces[j].astype(np.longdouble) - law).max() / peak))
            yardstick = max(yardstick, float(np.abs(plain[j].astype(np.longdouble) - law_plain).max() / np.abs(plain[j]).max()))
    a.close()
    b.close()
    print("the law on the device, %s, %d renderers: device %.3e, float32 restatement %.3e (%.2f x); in contact %s" % (name, renderers, device, yardstick, device / yardstick, ["%.2f" % c for c in contact]))
    assert 0.05 < np.mean(contact) < 0.9
    assert 0 < yardstick < 1e5 * float(np.finfo(np.float32).eps)
    assert device <= BOUND * yardstick, (device, yardstick)


# ---- 7. against longdouble ----
_RESTATED = {}
HOLD = 8  # frames a steered approach holds one active set


def _steered(n, C, K, scale, first_frame):
    """An approach signal that leads the group through its active sets, computed by the longdouble run as it goes: for HOLD frames at a
    time one subset A is aimed at -- the empty one, the full one, every other one in turn and one of two favoured ones -- by u = d + x with x chosen so that the
    exact solution is y_j = scale_j (1 + cos(0.37 s + j) / 2) on A and the residual of a member outside A is -scale_j / 2: x = y + C K y on
    A, x_j = -scale_j / 2 + (C K y)_j off it.  (A signal a caller could pass: the device and the working-precision run receive the float32
    samples the longdouble run arrived at.)"""
    full = (1 << n) - 1
    turn = []
    for m in range(1, full):  # (the first member alone and all but the first come up every time: in a group of four the others hold 2 % of the frames each)
        turn += [0, full, m, 1 if m & 1 else full - 1]
    C, K, scale = np.asarray(C, np.float64), np.asarray(K, np.float64), np.asarray(scale, np.float64)

    def u_of(t, d):
        s = first_frame + t
        mask = turn[(s // HOLD) % len(turn)]
        inside = np.array([bool(mask >> j & 1) for j in range(n)])
        y = np.where(inside, scale * (1 + 0.5 * np.cos(0.37 * s + np.arange(n))), 0.0)
        x = np.where(inside, y, -0.5 * scale) + C @ (K * y)
        return (np.asarray(d, np.float64) + x).astype(np.float32)
    return u_of


def _restated(name, use_double, kc, comp, blocks, frames):
    """The longdouble and working-precision runs of a shape, once per (shape, precision, K C): they do not depend on the renderer count."""
    key = (name, use_double, kc)
    if key in _RESTATED:
        return _RESTATED[key]
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    exact, working, scout = (gh.Restatement(sc, MODES, t, sc.dtype) for t in (np.longdouble, sc.dtype, np.float64))
    sc.close()
    n = SIZES[name]
    specs = _shape(name, [kc / c for c in comp])
    all_rows = [_noise_rows(MODES, b, blocks, frames) for b in range(blocks)]
    trace = {}
    scout.render_grouped(all_rows[0], [gh.spec(s[0], s[1], 0.0) for s in specs], np.zeros((n, frames), np.float32), frames, trace)  # the size of the free deflection
    scale = np.sqrt((trace["d"] ** 2).mean(axis=1))
    C, K = exact.compliance_matrix(specs), [np.float32(s[2]) for s in specs]
    runs, sets = [], []
    for b in range(blocks):
        trace = {}
        want = exact.render_grouped(all_rows[b], specs, _steered(n, C, K, scale, b * frames), frames, trace)
        ub = trace["u"]
        sets.append(trace["sets"].copy())
        runs.append((ub, want, working.render_grouped(all_rows[b], specs, ub, frames)))
    c_exact = np.diag(exact.compliance_matrix(specs)).astype(np.longdouble)
    c_plain = np.diag(working.compliance_matrix(specs)).astype(np.longdouble)
    _RESTATED[key] = (specs, all_rows, runs, np.concatenate(sets), c_exact, c_plain)
    return _RESTATED[key]


@PRECISIONS
@RENDERERS
@pytest.mark.parametrize("name", ["star", "chain", "four", "pair"])
def test_forces_and_samples_match_a_longdouble_restatement(use_double, renderers, name):
    """Noise drives on every object in every block, K_i chosen from the returned C_ii so that K C = 0.1, 1, 10, 100; 2 blocks of 512 frames.
    u: the junction tests' slow sine (amp 3, period 400, a phase per member) reaches the full set in under 5 % of the frames on the star
    and the chain and never on the four exciters -- a force rings the object up, and it is the object's response, not u, that decides
    which members touch (checked on the CPU, K C = 0.1 ... 100, amp 3 ... 100, periods 24 ... 800) -- so u is steered instead: _steered
    aims at one active set after another, eight frames each, from the longdouble run's own free prediction.  Conditions on the inputs,
    asserted on the longdouble run: at least three distinct active sets occur, the empty one and the full one among them, each in at
    least 5 % of the frames.  Figures: the largest deviation of a force row / of the block's samples from the longdouble restatement's
    over that row's peak, and the relative deviation of C_ii -- of the device, and of the working-precision restatement (every operation
    rounded to the bank's format, the header's tree, sums sequential) in the same run.  Bound: 4 x.

    Measured on an MI355X (this test prints them): force rows 0.15 - 2.40 x, samples 0.11 - 1.72 x, C_ii 0.14 - 0.48 x
    the working-precision restatement's deviation, over the four shapes, both precisions and 1 and 4 renderers."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    comp = _compliances(name, use_double)
    n, blocks, frames = SIZES[name], 2, FRAMES
    for kc in (0.1, 1.0, 10.0, 100.0):
        specs, all_rows, runs, sets, c_exact, c_plain = _restated(name, use_double, kc, comp, blocks, frames)
        share = {int(m): float((sets == m).mean()) for m in np.unique(sets)}
        often = [m for m, v in share.items() if v >= 0.05]
        assert len(often) >= 3 and 0 in often and (1 << n) - 1 in often, (name, kc, share)
        sc, _ = dh.device_scene(MODES, T60, renderers, use_double)
        fig = {"force": [0.0, 0.0], "out": [0.0, 0.0], "C": [0.0, 0.0]}
        for b in range(blocks):
            ub, (want_out, want, _, want_status), (plain_out, plain, _, _) = runs[b]
            out = np.zeros(frames, sc.dtype)
            _, _, forces, c_dev, status = sc.render_coupled(out, *_drive_args(all_rows[b], frames), [], gh.records(specs), ub)
            assert list(status) == [1] * n and list(want_status) == [1] * n
            for got, yard, key, ref in ((forces, plain, "force", want), (out[None, :], plain_out[None, :], "out", want_out[None, :])):
                fig[key][0] = max(fig[key][0], gh.row_figure(got, ref))
                fig[key][1] = max(fig[key][1], gh.row_figure(yard, ref))
            fig["C"][0] = max(fig["C"][0], float(np.abs((c_dev.astype(np.longdouble) - c_exact) / c_exact).max()))
            fig["C"][1] = max(fig["C"][1], float(np.abs((c_plain - c_exact) / c_exact).max()))
        sc.close()
        print("%s, %s, K C = %g, %d renderers: " % ("fp64" if use_double else "fp32", name, kc, renderers) +
              ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()) +
              "; active sets " + " ".join("%d:%.2f" % (m, v) for m, v in sorted(share.items())))
        for key, (device, yardstick) in fig.items():
            assert 0 < yardstick < 1e6 * eps, (key, yardstick)
            assert device <= BOUND * yardstick, (name, kc, key, device, yardstick)


# ---- 8. determinism and locality ----
@PRECISIONS
@pytest.mark.parametrize("name", ["star", "four"])
def test_a_group_is_deterministic_and_local(use_double, name):
    n = SIZES[name]
    forces, out, cols, comp, status, _ = _run(name, use_double, 1)
    assert list(status) == [1] * n and np.abs(forces).max(axis=1).min() > 0 and ((forces == 0).mean(axis=1) > 0.05).all()  # every member makes and breaks
    again = _run(name, use_double, 1)
    assert np.array_equal(forces, again[0]) and np.array_equal(out, again[1]) and _same(cols, again[2])
    four = _run(name, use_double, 4)
    assert np.array_equal(forces, four[0]) and _same(cols, four[2])
    assert np.abs(four[1] - out).max() <= 1e-3 * np.abs(out).max()  # (the mix of four renderers adds in another order)


@PRECISIONS
def test_objects_off_the_group_do_not_see_its_stiffness(use_double):
    """The chain on objects 0 - 2 and a lone junction on a fourth object: the fourth object's state and the lone junction's row are the
    same bits for any stiffness of the group's members."""
    modes = MODES + [64]
    lone = gh.spec(gh.side(3, 1, direction=NORMAL, coupling=2.0), None, 1e5, shared=False)
    runs = [_run("chain", use_double, 1, kc=kc, modes=modes, extra=[lone]) for kc in (0.0, 10.0, 1000.0)]
    first = sum(MODES)
    for other in runs[1:]:
        assert np.array_equal(runs[0][0][2], other[0][2]) and np.abs(other[0][2]).max() > 0
        assert np.array_equal(runs[0][2][0][first:], other[2][0][first:]) and np.array_equal(runs[0][2][1][first:], other[2][1][first:])
    assert not np.array_equal(runs[0][2][0][:first], runs[2][2][0][:first])


@PRECISIONS
@pytest.mark.parametrize("name", ["star", "four"])
def test_scaling_the_excitation_by_two_scales_everything_by_two(use_double, name):
    """u and every drive signal times 2 gives f, out and the states times 2, bit for bit: a power of two commutes with every rounding of
    the recurrence and of the solve (the inverses do not depend on the signals), and every comparison with 0 keeps its outcome."""
    f1, out1, cols1, _, _, _ = _run(name, use_double, 1, scale=1.0)
    f2, out2, cols2, _, _, _ = _run(name, use_double, 1, scale=2.0)
    assert np.abs(f1).max(axis=1).min() > 0
    assert np.array_equal(2 * f1, f2) and np.array_equal(2 * out1, out2)
    assert np.array_equal(2 * cols1[0], cols2[0]) and np.array_equal(2 * cols1[1], cols2[1])


@PRECISIONS
def test_the_order_of_the_members_changes_rounding_only(use_double):
    """The star with its members listed in another order.  What the contract lets that change: the order in which the hub adds its
    members' a_i f_i (step 5), the order of the rows' and columns' elimination and of the candidates' sums, and which of two consistent
    subsets is taken on a boundary -- roundings.  What it does not: every C_ii (the same sum over the same modes in the same order:
    array_equal), the statuses, and which row belongs to which member.  A rounding of one ulp of a state per frame, carried by a
    recurrence that does not amplify, is at most `frames` ulps after `frames` frames: the rows agree within frames * eps of their peak."""
    eps = float(np.finfo(np.float64 if use_double else np.float32).eps)
    order = (2, 0, 1)
    forces, out, _, comp, status, _ = _run("star", use_double, 1, blocks=1)
    moved = _run("star", use_double, 1, blocks=1, order=order)
    assert list(moved[4]) == [1, 1, 1] and np.array_equal(moved[3], comp[list(order)])
    for at, member in enumerate(order):
        peak = np.abs(forces[member]).max()
        assert peak > 0 and np.abs(moved[0][at] - forces[member]).max() <= FRAMES * eps * peak, member
    assert np.abs(moved[1] - out).max() <= FRAMES * eps * np.abs(out).max()


# ---- 9. left out ----
@PRECISIONS
def test_what_a_group_cannot_hold_is_left_out(use_double):
    """Each kind: status 0, a zero row, C = 0, and for everything else the bits of the call without that junction."""
    def run(modes, specs):
        sc, _ = dh.device_scene(modes, T60, 1, use_double)
        out = np.zeros(FRAMES, sc.dtype)
        u = _approach([2e-5] * len(specs), FRAMES, 1)
        _, _, forces, comp, status = sc.render_coupled(out, *_drive_args(_noise_rows(modes, 0, 1, FRAMES), FRAMES), [], gh.records(specs), u)
        got = (forces, comp, status, [out] + _states(sc) + list(sc.object_state()))
        sc.close()
        return got

    hub_a = lambda **kw: gh.spec(gh.side(1, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), gh.side(0, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5), 3e5, **kw)
    hub_b = lambda **kw: gh.spec(gh.side(1, 3, direction=NORMAL), None, 2e5, **kw)
    wide = [130, 520, 400]  # 2 + 5 waves, and 4 more
    cases = {"a fifth member": (MODES, _shape("four", [1e5] * 4), gh.spec(gh.side(0, 2, direction=(1.0, 0.0, 0.0)), None, 1e5)),
             "a ninth wave": (wide, [gh.spec(gh.side(0, 1, direction=NORMAL), gh.side(1, 2, direction=_push(NORMAL)), 1e5)], gh.spec(gh.side(0, 3, direction=(1.0, 0.5, 0.0)), gh.side(2, 0, direction=(-1.0, -0.5, 0.0)), 1e5)),
             "Hertz joining a group": (MODES, [hub_a()], gh.spec(gh.side(1, 3, direction=NORMAL), None, 2e9, hertz=True)),
             "joining a Hertz junction": (MODES, [gh.spec(gh.side(1, 3, direction=NORMAL), None, 2e9, hertz=True)], hub_a()),
             "flagged joining unflagged": (MODES, [hub_a(shared=False)], hub_b())}
    for kind, (modes, kept, stray) in cases.items():
        forces, comp, status, rest = run(modes, kept + [stray])
        want = run(modes, kept)
        at = len(kept)
        assert status[at] == 0 and comp[at] == 0 and not forces[at].any(), kind
        assert list(status[:at]) == [1] * at and np.abs(forces[:at]).max() > 0, kind
        assert np.array_equal(forces[:at], want[0]) and np.array_equal(comp[:at], want[1]) and _same(rest, want[3]), kind
    # (and the wide pair is a group when it fits: the same two junctions on the 130- and 400-mode objects, 2 + 4 waves)
    forces, comp, status, _ = run(wide, [gh.spec(gh.side(0, 1, direction=NORMAL), None, 1e5), cases["a ninth wave"][2]])
    assert list(status) == [1, 1] and (np.abs(forces).max(axis=1) > 0).all()


# ---- 10. refused ----
@PRECISIONS
def test_a_group_that_would_amplify_is_refused(use_double):
    """A negative coupling on one member of the chain makes its C_ii negative; with C_ii K_i <= -1 the pivot of the subset that holds it
    alone is not above 0: every member has status 2 and a zero row, and the run has the bits of the call with every K = 0."""
    def make(k):
        specs = _shape("chain", k)
        a, b, stiffness = specs[1][:3]
        specs[1] = gh.spec(a[:4] + (-2.0,), b[:4] + (-2.0,), stiffness)
        return specs

    def run(k):
        sc, _ = dh.device_scene(MODES, T60, 1, use_double)
        out = np.zeros(2 * FRAMES, sc.dtype)
        for b in range(2):
            _, _, forces, comp, status = sc.render_coupled(out[b * FRAMES:(b + 1) * FRAMES], *_drive_args(_noise_rows(MODES, b, 2, FRAMES), FRAMES), [], gh.records(make(k)), 1e-5 * np.ones((2, FRAMES), np.float32))
        got = (forces, comp, status, [out] + _states(sc) + list(sc.object_state()))
        sc.close()
        return got

    zero = run([0.0, 0.0])
    assert list(zero[2]) == [1, 1] and zero[1][0] > 0 and zero[1][1] < 0
    refused = run([1.0 / zero[1][0], -2.0 / zero[1][1]])
    assert list(refused[2]) == [2, 2] and not refused[0].any() and np.array_equal(refused[1], zero[1])
    assert _same(refused[3], zero[3])
    solved = run([1.0 / zero[1][0], -0.01 / zero[1][1]])
    assert list(solved[2]) == [1, 1] and np.abs(solved[0]).max() > 0
