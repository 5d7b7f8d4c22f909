"""Helpers of the tests of pickups on junction objects (tests/test_bank_observed_cpu.py, tests/test_bank_observed_gpu.py; contract:
include/modalhip.h, "Pickups on junction objects"): the restatements of tests/damped_harness.py (lone linear, Hertz and damped junctions)
and tests/group_harness.py (one group) with pickup rows taken from the CORRECTED state -- z[s] after step 5 of frame s, the state the
frame's output term is formed from -- in a number format of the caller's choice:

  numpy.longdouble               the reference: a row is the plain sum over every mode of g_im Im z[s] + g_re Re z[s];
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the gains with every operation rounded to the bank's format, and the
                                 sum in the contract's order -- per (wave of 128 modes from the object's mode 0, half of 64 modes)
                                 acc = fma(g_im[k], Im z[k], acc), then acc = fma(g_re[k], Re z[k], acc), even modes into one accumulator
                                 and odd modes into a second, k ascending from +0, the value even + odd; the partial rows added in
                                 ascending (wave, half) order from +0.  (The fused multiply-add is formed in numpy.longdouble and rounded
                                 to the format: exact in float32; in float64 the product is rounded to 64 bits first, which moves a result
                                 by one unit in the last place in about one operation in two thousand.)  Its deviation from the
                                 longdouble one is the yardstick the device's deviation is measured by.

The frame loops are the inherited ones, untouched: they assign every object's state once per frame (self.z[o] = ...), and `observed` keeps
those assignments -- the trajectory -- and forms the rows from it afterwards."""
import numpy as np

from tests import damped_harness as dd
from tests import group_harness as gh
from tests import pickup_harness as ph

POINTS = dd.POINTS
NO_OBJECT = dd.NO_OBJECT
side = dd.side
replay_drives = dd.replay_drives
row_figure = dd.row_figure
WAVE_MODES, HALF_MODES = 128, 64


def side_pickup(sd, advance=1):
    """The pickup at a junction side: same object, points, weights, direction and coupling."""
    return tuple(sd) + (int(advance),)


def side_pickups(specs, advance=1):
    """[(junction index, pickup spec)] of an advance-1 pickup at every side of every junction, in call order, side a before side b."""
    return [(j, side_pickup(sd, advance)) for j, s in enumerate(specs) for sd in (s[0], s[1]) if sd is not None]


def _fma(a, b, acc, T):
    L = np.longdouble
    return (np.asarray(a, L) * np.asarray(b, L) + np.asarray(acc, L)).astype(T)


def contract_sum(g_im, g_re, z_im, z_re, T):
    """A pickup's row in the contract's order.  g_im, g_re: [modes]; z_im, z_re: [frames][modes], all of format T."""
    frames, n = z_im.shape
    row = np.zeros(frames, T)
    for first in range(0, n, HALF_MODES):  # halves of 64 modes; (wave, half) ascending is this order
        acc = [np.zeros(frames, T), np.zeros(frames, T)]  # even modes, odd modes
        for k in range(first, min(first + HALF_MODES, n)):
            a = acc[(k - first) % 2]
            a = _fma(g_im[k], z_im[:, k], a, T)
            acc[(k - first) % 2] = _fma(g_re[k], z_re[:, k], a, T)
        row = row + (acc[0] + acc[1])
    assert row.dtype == T
    return row


class _Trajectory(list):
    """A restatement's list of states that also keeps what a frame loop assigns: states[o] = [(re, im) after frame 0, after frame 1, ...]."""

    def __init__(self, states):
        super().__init__(states)
        self.states = [[] for _ in states]

    def __setitem__(self, o, value):
        super().__setitem__(o, value)
        self.states[o].append(value)


class Observing:
    """Mixin for a restatement whose frame loop assigns self.z[o] once per object and frame."""

    def observed(self, render, pickups, *args, **kwargs):
        """Runs `render` (a bound frame loop of this restatement: render_coupled, render_damped, render_grouped) with *args and returns
        (its result, reads[len(pickups)][frames]): the pickups' rows from the states the loop left after every frame."""
        T = self.T
        log = _Trajectory(self.z)
        self.z = log
        try:
            result = render(*args, **kwargs)
        finally:
            self.z = list(log)
        self.trajectory = log.states  # (for a test that wants the states themselves)
        frames = max(len(s) for s in log.states) if log.states else 0
        reads = np.zeros((len(pickups), frames), T)
        for q, s in enumerate(pickups):
            states = log.states[s[0]]
            assert len(states) == frames
            if not frames:
                continue
            z_re, z_im = np.array([re for re, _ in states], T), np.array([im for _, im in states], T)
            g_im, g_re = self.pickup_gains(s)
            if T == np.longdouble:
                reads[q] = np.sum(g_im[None, :] * z_im + g_re[None, :] * z_re, axis=1)
            else:
                reads[q] = contract_sum(g_im, g_re, z_im, z_re, T)
        return result, reads


class Damped(Observing, dd.Restatement):
    """tests/damped_harness.Restatement (lone linear, Hertz and damped junctions) with `observed`."""


class Grouped(Observing, gh.Restatement):
    """tests/group_harness.Restatement (one group of linear junctions) with `observed`."""


def law(y, yp, l, k, hertz, bilateral=False, T=np.longdouble):
    """f = K phi(y) max(1 + l (y - y_p), 0) in format T; bilateral (linear, undamped): f = K y."""
    if bilateral:
        return (np.asarray(k, T) * np.asarray(y, T))[()]
    return dd.law(y, yp, l, k, hertz, T)


records = ph.records


# ---- the scenes the CPU and the GPU tests share ----
MODES, T60 = [37, 64, 130, 256], 2.0  # a part wave, a full half, two waves, two full waves
NORMAL = (0.25, -1.0, 0.5)
AMP = 20.0  # the approach's amplitude over the rms of the free deflection


class HostColumns:
    """The columns of dh.device_scene(mode_counts, t60, ...) read from the bank under construction, which needs no device: what a
    restatement is built from on the CPU."""

    def __init__(self, mode_counts, t60, use_double=False):
        from mesheditor_amd import bank as hipbank
        from tests import bank_harness as bh
        self.sc = hipbank.Scene(bh.SAMPLE_RATE, 0, use_double)
        self.dtype = self.sc.dtype
        for o, n in enumerate(mode_counts):
            mo = bh.make_modes(n, t60, freq_scale=1.0 + 0.013 * o)
            slot = self.sc.add_object(o, mo["shapes"], mo["positions"], mo["indices"])
            self.sc.tune_object(slot, mo["freqs"], mo["t60s"])
            self.sc.set_gains(slot, 1.0, 1.0)

    def column(self, name):
        return self.sc.column(name, live=False)


def _blend(obj, single):
    """The side that sits at a blend of three points -- or, single, at the first of them (a side a drive can replay)."""
    return (obj, 3) if single else (obj, (3, 0, 1), (0.5, 0.25, 0.25))


def lone_specs(k, hertz=(False, True), damped=(False, False), single=False):
    """A two-sided junction between objects 0 (37 modes; side a at a blend of three points) and 2 (130), and a one-sided one on object 3
    (256); object 1 is a bystander.  Specs of tests/damped_harness.py."""
    return [dd.spec(side(*_blend(0, single), direction=(1.0, 0.5, -0.25), coupling=1.5), side(2, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5), k[0], False, hertz[0], damped[0]),
            dd.spec(side(3, 1, direction=NORMAL, coupling=2.0), None, k[1], False, hertz[1], damped[1])]


def group_specs(k, single=False):
    """A group of three on objects 0 (37 modes), 1 (64) and 2 (130): 0 - 1, 1 - 2 and a one-sided member on 2 (at a blend of three
    points); object 3 is a bystander.  Specs of tests/group_harness.py."""
    return [gh.spec(side(0, 1, direction=(1.0, 0.5, -0.25), coupling=1.5), side(1, 3, direction=(-1.0, -0.5, 0.25), coupling=1.5), k[0]),
            gh.spec(side(1, 0, direction=(0.5, 1.0, 0.25)), side(2, 2, direction=(-0.5, -1.0, -0.25)), k[1]),
            gh.spec(side(*_blend(2, single), direction=NORMAL, coupling=2.0), None, k[2])]


def junction_records(lone=(), group=()):
    """One array of the binding's records: specs of tests/damped_harness.py, then specs of tests/group_harness.py."""
    from mesheditor_amd import bank as hipbank
    rows = [dd.record(s) for s in lone] + [gh.record(s) for s in group]
    return (hipbank.Junction * len(rows))(*rows) if rows else []


def probes_on(objects):
    """Per object four pickups: advance 0, 1 and 2 at single points and an advance-1 blend of three."""
    out = []
    for o in objects:
        out += [ph.spec(o, o % POINTS, direction=NORMAL, coupling=2.0, advance=0), ph.spec(o, (o + 1) % POINTS, direction=(1.0, 0.5, -0.25), coupling=1.5, advance=1),
                ph.spec(o, (o + 2) % POINTS, direction=(0.5, 0.5, -1.0), advance=2), ph.spec(o, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.0, -0.5), 1.0, 1)]
    return out


def drive_rows(objects, block, frames, blocks):
    """A noise drive on each of `objects` (restatement rows), the block's part of a signal `blocks` blocks long."""
    from tests import drive_harness as dh
    from tests.test_bank_drives_gpu import _signal
    return [(o,) + dh.row_direction(o) + (_signal("noise", o, blocks * frames)[block * frames:(block + 1) * frames],) for o in objects]


def approach(free, frames, blocks, amp=AMP, period=300.0, lift=0.5):
    """tests/test_bank_junctions_gpu.py's _approach with a shorter period and raised further: a slow sine per junction, `amp` times its free
    deflection, raised by `lift` of its amplitude.  (With that suite's 3 x, 400 frames and 0.1 a stiff contact on these ringing objects is
    closed for 9 % - 14 % of two blocks of 333 frames; AMP = 20, 300 frames and 0.5 keep every junction of against_plan between 15 % and
    85 % -- 17 % ... 70 %, held by tests/test_bank_observed_cpu.py on the longdouble restatement.)"""
    t = np.arange(blocks * frames)
    return np.array([(amp * a * (np.sin(2 * np.pi * t / (period + 90 * j)) + lift)).astype(np.float32) for j, a in enumerate(free)])


def against_plan(columns, kind, kc, comp, frames, blocks, modes=MODES, t60=T60):
    """The scene of the runs against longdouble: kind "lone" (lone_specs: the two-sided junction linear, the one-sided one Hertz) or
    "group" (group_specs), K from the compliances `comp` so that K C = kc (Hertz: K C sqrt(x0) = kc with x0 the approach's peak), a noise
    drive on every object, u a slow sine AMP times the rms of the free deflection (a float64 restatement without contact, first block).
    Returns (specs, pickups, rows block by block, u)."""
    scout = (Damped if kind == "lone" else Grouped)(columns, modes, np.float64, columns.dtype)
    rows = [drive_rows(range(len(modes)), b, frames, blocks) for b in range(blocks)]
    make = (lambda k: lone_specs(k)) if kind == "lone" else group_specs
    n = 2 if kind == "lone" else 3
    trace = {}
    if kind == "lone":
        scout.render_damped(rows[0], make([0.0] * n), np.zeros((n, frames), np.float32), [0.0] * n, None, frames, trace)
    else:
        scout.render_grouped(rows[0], make([0.0] * n), np.zeros((n, frames), np.float32), frames, trace)
    u = approach(np.sqrt((np.asarray(trace["d"], np.float64) ** 2).mean(axis=1)), frames, blocks)
    x0 = u.max(axis=1)
    hertz = (False, True) if kind == "lone" else (False, False, False)
    specs = make([kc / (float(c) * (np.sqrt(float(x)) if h else 1.0)) for c, x, h in zip(comp, x0, hertz)])
    objects = sorted({sd[0] for s in specs for sd in (s[0], s[1]) if sd is not None})
    return specs, probes_on(objects), rows, u


def against_run(rest, kind, specs, pickups, rows, u, frames):
    """One block of the plan on a restatement (Damped or Grouped): (out, forces, reads)."""
    if kind == "lone":
        (out, forces, _, status, _), reads = rest.observed(rest.render_damped, pickups, rows, specs, u, [0.0] * len(specs), None, frames)
    else:
        (out, forces, _, status), reads = rest.observed(rest.render_grouped, pickups, rows, specs, u, frames)
    assert (np.asarray(status) == 1).all(), status
    return out, forces, reads
