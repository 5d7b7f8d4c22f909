"""Helpers of the pickup tests (tests/test_bank_pickups_cpu.py, tests/test_bank_pickups_gpu.py): pickup records, and a restatement of
the resonator recurrence WITH pickup rows from the bank's own columns (Scene.column), written from the contract in include/modalhip.h --
the idea of tests/drive_harness.Restatement, in a number format of the caller's choice:

  numpy.longdouble               the reference the device is compared with (plain sums over every mode);
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement -- the same recurrence and gains with every operation rounded to the
                                 bank's format, no contraction, a pickup's modes added sequentially in mode order.  Its deviation from
                                 the longdouble one is the yardstick the device's deviation is measured by."""
import numpy as np

from tests import bank_harness as bh

POINTS = bh.SAMPLE_POINTS


def spec(obj, points, weights=(1.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), coupling=1.0, advance=0):
    """A pickup as plain data: (object, three points, three weights, direction, coupling, advance).  One point p = (p, p, p)."""
    pts = (points,) * 3 if np.isscalar(points) else tuple(points)
    return (int(obj), tuple(int(p) for p in pts), tuple(float(np.float32(w)) for w in weights), tuple(float(np.float32(v)) for v in direction), float(np.float32(coupling)),
            int(advance))


def record(s):
    """The binding's Pickup record of a spec."""
    from mesheditor_amd import bank as hipbank
    obj, pts, w, d, coupling, advance = s
    return hipbank.Pickup.of(obj, pts, w, d, coupling, advance)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Pickup * len(specs))(*[record(s) for s in specs]) if specs else []


def _ordered_sum(terms):
    """Sum of a vector in index order, every partial sum rounded to the vector's format (numpy's cumsum adds sequentially)."""
    return np.cumsum(terms)[-1] if len(terms) else terms.dtype.type(0)


class Restatement:
    """z <- z*c + sum_rows f_row[t]*gain_row;  out[t] = OutGain*ListenerGain * sum_k (OutPhaseIm*Im z + OutPhaseRe*Re z);
    pickup[t] = sum_k (g_im*Im z + g_re*Re z) of the state after frame t's step.  Every mode of every object, no chunks, no culling.
    `dtype`: the format every operation is rounded to; `bank_dtype`: the device bank's format (a pickup's coupling is multiplied by
    DeflectionScale in it and narrowed to float, as RenderBlock does)."""

    def __init__(self, scene, mode_counts, dtype=np.longdouble, bank_dtype=np.float64):
        self.T, self.bank_dtype, self.mode_counts = dtype, bank_dtype, list(mode_counts)
        self.z = [(np.zeros(n, dtype), np.zeros(n, dtype)) for n in mode_counts]  # (re, im)
        self.load_columns(scene)

    def load_columns(self, scene):
        """(Re)reads the bank's columns; the resonator states are kept."""
        T = self.T
        names = ("CoeffRe", "CoeffIm", "RadiationGain", "DeflectionGain", "OutPhaseRe", "OutPhaseIm", "ShapeX", "ShapeY", "ShapeZ", "OutGain", "ListenerGain", "DeflectionScale")
        col = {n: scene.column(n).astype(T) for n in names}
        self.objects = []
        k0 = s0 = 0
        for o, n in enumerate(self.mode_counts):
            sl = slice(k0, k0 + n)
            shapes = [col[a][s0:s0 + POINTS * n].reshape(POINTS, n) for a in ("ShapeX", "ShapeY", "ShapeZ")]
            self.objects.append({"c_re": col["CoeffRe"][sl], "c_im": col["CoeffIm"][sl], "rad": col["RadiationGain"][sl], "defl": col["DeflectionGain"][sl], "p_re": col["OutPhaseRe"][sl],
                                 "p_im": col["OutPhaseIm"][sl], "shapes": shapes, "mix": T(col["OutGain"][o] * col["ListenerGain"][o]), "defl_scale": col["DeflectionScale"][o]})
            k0 += n
            s0 += POINTS * n

    def drive_gain(self, obj, ex_pos, direction):
        ob, T = self.objects[obj], self.T
        jx, jy, jz = (T(np.float32(v)) for v in direction)
        sx, sy, sz = (s[ex_pos] for s in ob["shapes"])
        return ob["rad"] * (sx * jx + sy * jy + sz * jz)

    def read_of(self, s):
        """`read` of the contract, per mode."""
        obj, pts, w, d, coupling, _ = s
        ob, T, B = self.objects[obj], self.T, self.bank_dtype
        scale = T(np.float32(B(np.float32(coupling)) * B(ob["defl_scale"])))
        w0, w1, w2 = (T(np.float32(v)) for v in w)
        nx, ny, nz = (T(np.float32(v)) for v in d)
        sx, sy, sz = (w0 * a[pts[0]] + w1 * a[pts[1]] + w2 * a[pts[2]] for a in ob["shapes"])
        return scale * (sx * nx + sy * ny + sz * nz) * ob["defl"]

    def pickup_gains(self, s):
        """(g_im, g_re) per mode: the rows of ModeReadGains::Fill for the pickup's advance."""
        ob, T, read, advance = self.objects[s[0]], self.T, self.read_of(s), s[5]
        cr, ci = ob["c_re"], ob["c_im"]
        if advance == 0:
            return read, np.zeros_like(read)
        if advance == 1:
            return read * cr, read * ci
        return read * (cr * cr - ci * ci), read * (T(2) * cr * ci)

    def render(self, rows, pickups, frames):
        """rows: (object, ex_pos, direction, float32 signal[frames]); pickups: specs.  Returns (out[frames], reads[len(pickups)][frames])."""
        T = self.T
        exact = T == np.longdouble
        out, reads = np.zeros(frames, T), np.zeros((len(pickups), frames), T)
        for o, ob in enumerate(self.objects):
            mine = [(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o]
            probes = [(q,) + self.pickup_gains(s) for q, s in enumerate(pickups) if s[0] == o]
            (z_re, z_im), c_re, c_im = self.z[o], ob["c_re"], ob["c_im"]
            for t in range(frames):
                e = np.zeros(len(z_re), T)
                for g, f in mine:
                    e = e + f[t] * g
                re = z_re * c_re - z_im * c_im + e
                z_im = z_re * c_im + z_im * c_re
                z_re = re
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
                for q, g_im, g_re in probes:
                    terms = g_im * z_im + g_re * z_re
                    reads[q, t] = np.sum(terms) if exact else _ordered_sum(terms)
            self.z[o] = (z_re, z_im)
        return out, reads


def row_figure(got, want):
    """The largest deviation of a row from the restatement's, divided by that row's peak (rows: [n][frames])."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    peak = np.abs(want).max(axis=-1)
    assert (peak > 0).all(), "a pickup row of the restatement is silent"
    return float((np.abs(got - want).max(axis=-1) / peak).max())
