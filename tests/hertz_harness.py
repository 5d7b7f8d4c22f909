"""Helpers of the Hertz junction tests (tests/test_bank_hertz_cpu.py, tests/test_bank_hertz_gpu.py): junction records with a law field, the
scalar solve of step 4h of the junction contract (include/modalhip.h, MH_JUNCTION_HERTZ), and tests/junction_harness.Restatement with
that step, in a number format of the caller's choice:

  numpy.longdouble               the reference: Newton's iteration run to a fixed point (EXACT_STEPS steps), not four;
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the header's expression tree with every operation rounded to the
                                 bank's format -- numpy.cbrt, four Newton steps, nothing contracted.  Its deviation from the longdouble
                                 one is the yardstick the device's deviation is measured by."""
import numpy as np

from tests import junction_harness as jh

POINTS = jh.POINTS
NO_OBJECT = jh.NO_OBJECT
side = jh.side
replay_drives = jh.replay_drives
row_figure = jh.row_figure
STEPS, EXACT_STEPS = 4, 200


def spec(a, b=None, stiffness=0.0, bilateral=False, hertz=True):
    """A junction as plain data: (side a, side b or None, K as the float the record holds, bilateral, hertz)."""
    return (a, b, float(np.float32(stiffness)), bool(bilateral), bool(hertz))


def record(s):
    """The binding's Junction record of a spec."""
    from mesheditor_amd import bank as hipbank
    a, b, k, bilateral, hertz = s
    return hipbank.Junction.of(a, b, k, bilateral, hertz)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Junction * len(specs))(*[record(s) for s in specs]) if specs else []


def hertz_root(x, c, T, steps=None, start_factor=1.0):
    """The root y of y + c y sqrt(y) = x for x > 0, c >= 0, by the header's tree in format T: the smaller of the upper bounds x and
    (x / c)^(2/3), then `steps` Newton steps (default: four in a working precision, EXACT_STEPS in longdouble).  start_factor scales
    the cube root (what a device cbrt that is not correctly rounded would do).  Scalars or arrays, element by element."""
    x, c = np.asarray(x, T), np.asarray(c, T)
    if steps is None:
        steps = EXACT_STEPS if T == np.longdouble else STEPS
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        g = np.cbrt(x / np.where(c > 0, c, T(1))) * T(start_factor)
        g = g * g
        y = np.where((c > 0) & (g < x), g, x)
        c15 = T(1.5) * c
        for _ in range(steps):
            r = np.sqrt(y)
            y = y - ((y + (c * y) * r) - x) / (T(1) + c15 * r)
    assert y.dtype == T
    return y[()]


def hertz_force(x, c, k, T, steps=None, start_factor=1.0):
    """f of step 4h: 0 unless x > 0 (a NaN included), else (K y) sqrt(y) at the root y.  Scalars or arrays."""
    x, k = np.asarray(x, T), np.asarray(k, T)
    closed = x > 0
    y = np.asarray(hertz_root(np.where(closed, x, T(1)), c, T, steps, start_factor), T)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        f = np.where(closed, (k * y) * np.sqrt(y), T(0))
    assert f.dtype == T
    return f[()]


class Restatement(jh.Restatement):
    """tests/junction_harness.Restatement whose render_coupled takes specs with a law field (this module's spec) and restates step 4 for a
    Hertz junction; side gains, compliance and the frame loop's other steps are the inherited ones."""

    steps = None  # Newton steps of a Hertz junction (None: the format's default)

    def render_coupled(self, rows, junctions, approach, frames, trace=None):
        """As jh.Restatement.render_coupled; junctions are 5-tuples (a 4-tuple is a linear junction).  Statuses: 0 for Hertz + bilateral
        (left out: a zero row, C = 0), 2 for a Hertz junction with C < 0, or C or K C not finite."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else jh._sequential
        junctions = [tuple(s) + (False,) * (5 - len(s)) for s in junctions]
        out, forces = np.zeros(frames, T), np.zeros((len(junctions), frames), T)
        u = np.asarray(approach, np.float32).reshape(len(junctions), frames)
        u = np.where(np.isfinite(u), u, np.float32(0)).astype(T)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains = [[(sd[0],) + self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None] for s in junctions]
        comp = [self.compliance(s[:4]) for s in junctions]
        stiff = [T(np.float32(s[2])) for s in junctions]
        status = []
        with np.errstate(over="ignore", invalid="ignore"):
            kc = [k * c for k, c in zip(stiff, comp)]
            denom = [T(1) + v for v in kc]
        for j, s in enumerate(junctions):
            if s[4] and s[3]:
                status.append(0)
                comp[j] = T(0)
            elif s[4]:
                status.append(1 if (np.isfinite(comp[j]) and comp[j] >= 0 and np.isfinite(kc[j]) and kc[j] >= 0) else 2)
            else:
                status.append(1 if (np.isfinite(denom[j]) and denom[j] > 0) else 2)
        free, after = np.zeros((len(junctions), frames), T), np.zeros((len(junctions), frames), T)
        for t in range(frames):
            stepped = []
            for o, ob in enumerate(self.objects):
                (z_re, z_im), c_re, c_im = self.z[o], ob["c_re"], ob["c_im"]
                e = np.zeros(len(z_re), T)
                for g, f in mine[o]:
                    e = e + f[t] * g
                stepped.append([z_re * c_re - z_im * c_im + e, z_re * c_im + z_im * c_re])
            for j, s in enumerate(junctions):
                d = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
                free[j, t] = d
                if status[j] != 1:
                    continue
                x = u[j, t] - d
                if s[4]:
                    f = hertz_force(x, kc[j], stiff[j], T, self.steps)
                else:
                    reach = x if s[3] else (x if x > 0 else T(0))
                    f = (stiff[j] * reach) / denom[j]
                forces[j, t] = f
                for (o, a, _, _) in gains[j]:
                    stepped[o][0] = stepped[o][0] + a * f
            for j in range(len(junctions)):  # what an advance-1 pickup on every side reads after the frame: the next frame's deflection
                after[j, t] = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
            for o, ob in enumerate(self.objects):
                z_re, z_im = stepped[o]
                self.z[o] = (z_re, z_im)
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
        if trace is not None:
            trace["d"], trace["read1"] = free, after
        return out, forces, np.array([float(c) for c in comp]), np.array(status, np.uint8)
