"""Helpers of the junction tests (tests/test_bank_junctions_cpu.py, tests/test_bank_junctions_gpu.py): junction records, and the
restatement of tests/pickup_harness.py extended by the five steps of the junction contract (include/modalhip.h, mh_junction), in a number
format of the caller's choice:

  numpy.longdouble               the reference the device is compared with;
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the same steps with every operation rounded to the bank's format, no
                                 contraction, the sums of d and C sequential in mode order (side a's modes, then side b's).  Its
                                 deviation from the longdouble one is the yardstick the device's deviation is measured by."""
import numpy as np

from tests import pickup_harness as ph

POINTS = ph.POINTS
NO_OBJECT = 0xffffffff


def side(obj, points, weights=(1.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), coupling=1.0):
    """A junction side as plain data: (object, three points, three weights, direction, coupling).  One point p = (p, p, p)."""
    return ph.spec(obj, points, weights, direction, coupling)[:5]


def spec(a, b=None, stiffness=0.0, bilateral=False):
    """A junction as plain data: (side a, side b or None, K as the float the record holds, bilateral)."""
    return (a, b, float(np.float32(stiffness)), bool(bilateral))


def record(s):
    """The binding's Junction record of a spec."""
    from mesheditor_amd import bank as hipbank
    a, b, k, bilateral = s
    return hipbank.Junction.of(a, b, k, bilateral)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Junction * len(specs))(*[record(s) for s in specs]) if specs else []


def replay_drives(s):
    """The drives that apply a junction's force row as an open-loop excitation: one per side, at the side's first point along the side's
    direction (a junction side with weights (1, 0, 0) has a drive's gain bit for bit)."""
    out = []
    for sd in (s[0], s[1]):
        if sd is not None:
            assert sd[2] == (1.0, 0.0, 0.0), "only a single-point side is a drive"
            out.append((sd[0], sd[1][0]) + tuple(sd[3]))
    return out


def _sequential(terms):
    return np.cumsum(terms)[-1] if len(terms) else terms.dtype.type(0)


class Restatement(ph.Restatement):
    """tests/pickup_harness.Restatement with junctions: render_coupled steps every object frame by frame and closes each junction's loop
    per frame as the contract says."""

    def side_gains(self, sd):
        """(a, g_im, g_re) per mode of a side: the drive gain at the blend along the direction, and the advance-1 read row."""
        obj, pts, w, d, coupling = sd
        ob, T = self.objects[obj], self.T
        w0, w1, w2 = (T(np.float32(v)) for v in w)
        nx, ny, nz = (T(np.float32(v)) for v in d)
        sx, sy, sz = (w0 * s[pts[0]] + w1 * s[pts[1]] + w2 * s[pts[2]] for s in ob["shapes"])
        a = ob["rad"] * (sx * nx + sy * ny + sz * nz)
        read = self.read_of((obj, pts, w, d, coupling, 1))
        return a, read * ob["c_re"], read * ob["c_im"]

    def compliance(self, s):
        T = self.T
        terms = np.concatenate([g_re * a for (a, _, g_re) in (self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None)])
        return np.sum(terms) if T == np.longdouble else _sequential(terms)

    def render_coupled(self, rows, junctions, approach, frames, trace=None):
        """rows: (object, ex_pos, direction, float32 signal[frames]); junctions: specs; approach: float32 [len(junctions)][frames].
        Returns (out[frames], forces[len(junctions)][frames], compliances, statuses).  trace (a dict, optional) receives "d": the free
        predictions, and "read1": the deflection of the next frame as the state after the frame predicts it, both [junction][frame]."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else _sequential
        out, forces = np.zeros(frames, T), np.zeros((len(junctions), frames), T)
        u = np.asarray(approach, np.float32).reshape(len(junctions), frames)
        u = np.where(np.isfinite(u), u, np.float32(0)).astype(T)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains = [[(sd[0],) + self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None] for s in junctions]
        comp = [self.compliance(s) for s in junctions]
        stiff = [T(np.float32(s[2])) for s in junctions]
        denom = [T(1) + k * c for k, c in zip(stiff, comp)]
        status = [1 if (np.isfinite(dn) and dn > 0) else 2 for dn in denom]
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


row_figure = ph.row_figure
