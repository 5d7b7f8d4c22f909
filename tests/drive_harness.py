"""Helpers of the drive tests (tests/test_bank_drives_cpu.py, tests/test_bank_drives_gpu.py): the one-sample impact that a
drive can be compared with bit for bit, scenes of objects of unequal size, and an independent numpy.longdouble restatement
of the resonator recurrence from the bank's own columns."""
import numpy as np

from tests import bank_harness as bh

POINTS = bh.SAMPLE_POINTS


def forces_restatement(dtype, gamma, pulse_step, frames):
    """k_bank_forces' force curve (ModalAudio.cpp:504-524) for a fresh impact, in `dtype`, operation for operation: a phasor that
    starts at (1, 0) and turns by (rot_re, rot_im) per sample for ceil(1 / step) samples, force = gamma * 0.5 * (1 - phase_re).
    Returns (samples, (rot_re, rot_im), samples_left_after)."""
    T = dtype
    step = T(np.float32(pulse_step))
    turn = T(2) * T(np.pi) * step
    rot_re, rot_im = T(np.cos(turn)), T(np.sin(turn))
    left = int(np.ceil(T(1) / step))
    phase_re, phase_im, g = T(1), T(0), T(np.float32(gamma))
    out = np.zeros(frames, dtype)
    for s in range(frames):
        cur = T(0)
        if left > 0:
            re = T(T(phase_re * rot_re) - T(phase_im * rot_im))
            phase_im = T(T(phase_re * rot_im) + T(phase_im * rot_re))
            phase_re = re
            cur = T(T(g * T(0.5)) * T(T(1) - phase_re))
            left -= 1
        out[s] = cur
    return out, (rot_re, rot_im), left


def one_sample_impact(event_type, obj, ex_pos, direction, gamma):
    """An impact whose force curve is exactly [gamma, 0, 0, ...] and whose click is exactly zero: pulse_step 0.5 (two samples, the
    second at phase 1 -> force 0), accel_amp 0, click coefficients 0.  It retires in the block it starts in."""
    jx, jy, jz = direction
    return event_type(0, obj, ex_pos, jx, jy, jz, 0.5, gamma, 0.0, 0.0, 0.0, 0.0)


def impulse_row(gamma, frames):
    """The drive signal of one_sample_impact."""
    f = np.zeros(frames, np.float32)
    f[0] = gamma
    return f


def device_scene(mode_counts, longest_t60, renderers, use_double=False):
    """One object per entry of mode_counts (tests/bank_harness.py's synthetic body at that size, pitch spread per object), installed,
    first block rendered.  Returns (Scene, slots)."""
    from mesheditor_amd import bank as hipbank
    sc = hipbank.Scene(bh.SAMPLE_RATE, 0, use_double)
    sc.set_renderers(renderers)
    slots = []
    for o, n in enumerate(mode_counts):
        mo = bh.make_modes(n, longest_t60, freq_scale=1.0 + 0.013 * o)
        slot = sc.add_object(o, mo["shapes"], mo["positions"], mo["indices"])
        sc.tune_object(slot, mo["freqs"], mo["t60s"])
        sc.set_gains(slot, 1.0, 1.0)
        slots.append(slot)
    sc.install()
    sc.render(np.zeros(bh.BLOCK, sc.dtype))
    return sc, slots


def row_direction(i):
    """A direction and excitation position that differ from row to row (float32-exact components)."""
    return (i * 7 + 3) % POINTS, (np.float32(1.0 - 0.125 * (i % 5)), np.float32(0.5 - 0.25 * (i % 3)), np.float32(0.125 * (i % 4) - 0.25))


class Restatement:
    """The resonator recurrence in numpy.longdouble, from what Scene.column() returns -- written from the contract
    (z <- z*c + sum_rows f_row[t] * gain_row,  out[t] = OutGain * ListenerGain * sum_k (OutPhaseIm*Im z + OutPhaseRe*Re z)), not from
    the kernel: every mode of every object, all modes summed at once, no chunks, no culling."""

    def __init__(self, scene, mode_counts):
        L = np.longdouble
        col = {n: scene.column(n).astype(L) for n in ("CoeffRe", "CoeffIm", "RadiationGain", "OutPhaseRe", "OutPhaseIm", "ShapeX", "ShapeY", "ShapeZ", "OutGain", "ListenerGain")}
        self.objects = []
        k0 = s0 = 0
        for o, n in enumerate(mode_counts):
            sl = slice(k0, k0 + n)
            shapes = [col[a][s0:s0 + POINTS * n].reshape(POINTS, n) for a in ("ShapeX", "ShapeY", "ShapeZ")]
            self.objects.append({"c": col["CoeffRe"][sl] + 1j * col["CoeffIm"][sl], "rad": col["RadiationGain"][sl], "p_re": col["OutPhaseRe"][sl], "p_im": col["OutPhaseIm"][sl],
                                 "shapes": shapes, "mix": col["OutGain"][o] * col["ListenerGain"][o], "z": np.zeros(n, np.clongdouble)})
            k0 += n
            s0 += POINTS * n

    def gain(self, obj, ex_pos, direction):
        ob = self.objects[obj]
        jx, jy, jz = (np.longdouble(np.float32(v)) for v in direction)
        sx, sy, sz = (s[ex_pos] for s in ob["shapes"])
        return ob["rad"] * (sx * jx + sy * jy + sz * jz)

    def render(self, rows, frames):
        """rows: list of (object, ex_pos, direction, float32 signal[frames]).  Returns the block's samples (longdouble)."""
        out = np.zeros(frames, np.longdouble)
        for o, ob in enumerate(self.objects):
            mine = [(self.gain(o, p, d), np.asarray(f, np.float32).astype(np.longdouble)) for (obj, p, d, f) in rows if obj == o]
            z, c = ob["z"], ob["c"]
            for t in range(frames):
                e = np.zeros(len(z), np.longdouble)
                for g, f in mine:
                    e = e + f[t] * g
                z = z * c + e
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z.imag + ob["p_re"] * z.real)
            ob["z"] = z
        return out
