"""Helpers of the friction tests (tests/test_bank_friction_cpu.py, tests/test_bank_friction_gpu.py): junction and friction records, the
scalar step 4t of the junction contract (include/modalhip.h, MH_JUNCTION_FRICTION), and tests/hertz_harness.Restatement extended by
steps 2, 3, 4t and 5 of a frictional junction, in a number format of the caller's choice:

  numpy.longdouble               the reference (a Hertz candidate's Newton iteration run to a fixed point);
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the header's expression trees with every operation rounded to the
                                 bank's format, nothing contracted, the sums of d_n, d_t and of the four compliances sequential in mode
                                 order (side a's modes, then side b's).  Its deviation from the longdouble one is the yardstick the
                                 device's deviation is measured by."""
import numpy as np

from tests import group_harness as gh
from tests import hertz_harness as hh
from tests import junction_harness as jh

L = np.longdouble
POINTS = jh.POINTS
side = jh.side
O, S, P, M = 0, 1, 2, 3  # the branch a frame takes: open, stick, slip +, slip -
BRANCHES = "OSPM"


def spec(a, b=None, stiffness=0.0, hertz=False, ta=(0.0, 0.0, 0.0), tb=(0.0, 0.0, 0.0), mu=0.0, kt=0.0, friction=True):
    """A junction as plain data: tests/hertz_harness.spec (unilateral) plus its friction -- (ta, tb, mu, kt) as the floats the record holds,
    or None for a junction without the flag."""
    f32 = lambda v: float(np.float32(v))
    fr = (tuple(f32(v) for v in ta), tuple(f32(v) for v in tb), f32(mu), f32(kt)) if friction else None
    return hh.spec(a, b, stiffness, False, hertz) + (fr,)


def records(specs):
    """The binding's Junction records and Friction records of specs (5-tuples of tests/hertz_harness count as unflagged)."""
    from mesheditor_amd import bank as hipbank
    specs = [tuple(s) + (None,) * (6 - len(s)) for s in specs]
    junctions = [hipbank.Junction.of(s[0], s[1], s[2], s[3], s[4], friction=s[5] is not None) for s in specs]
    slides = [hipbank.Friction.of(*s[5]) if s[5] is not None else hipbank.Friction.of() for s in specs]
    n = max(len(specs), 1)
    return (hipbank.Junction * n)(*junctions), (hipbank.Friction * n)(*slides)


def left_out(s):
    """Whether the render leaves a junction out for its friction: the flag on a bilateral junction, a tangent component, mu or kt that is
    not finite, mu < 0 or kt < 0.  (With the damped or the shared flag as well -- a spec of this module holds neither.)"""
    fr = s[5] if len(s) > 5 else None
    if fr is None:
        return False
    numbers = list(fr[0]) + list(fr[1]) + [fr[2], fr[3]]
    return bool(s[3]) or not all(np.isfinite(v) for v in numbers) or fr[2] < 0 or fr[3] < 0


def tangent_side(sd, t):
    """A side with the tangent t in the place of its direction: what a_t and read_t are the normal channel's gains of."""
    return (sd[0], sd[1], sd[2], tuple(float(np.float32(v)) for v in t), sd[4])


def replay_drives(s):
    """The drives that apply a frictional junction's rows as open-loop excitations: per side one along n (signal f_n), then one along t
    (signal f_t).  Returns [(object, ex_pos, direction, which)] with which = 0 for f_n and 1 for f_t."""
    out = []
    for sd, t in ((s[0], s[5][0]), (s[1], s[5][1])):
        if sd is not None:
            assert sd[2] == (1.0, 0.0, 0.0), "only a single-point side is a drive"
            out += [(sd[0], sd[1][0], tuple(sd[3]), 0), (sd[0], sd[1][0], tuple(t), 1)]
    return out


# ---- step 3's constants and step 4t, element by element ----
def normal_force(x, c_b, k, T, hertz, steps=None):
    """N(x, C_b): the scalar solve of the junction's normal law -- linear: step 4's expression; Hertz: step 4h's tree with c = K C_b."""
    x, c_b, k = np.asarray(x, T), np.asarray(c_b, T), np.asarray(k, T)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        if hertz:
            return np.asarray(hh.hertz_force(x, k * c_b, k, T, steps), T)
        return (k * np.where(x > 0, x, T(0))) / (T(1) + k * c_b)


def constants(c_nn, c_nt, c_tn, c_tt, k, mu, kt, T, hertz):
    """What a block forms once, nothing contracted: den, beta, C_S, C_P, C_M, and whether the junction is solved (the header's status)."""
    c_nn, c_nt, c_tn, c_tt, k, mu, kt = (np.asarray(v, T) for v in (c_nn, c_nt, c_tn, c_tt, k, mu, kt))
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        den = T(1) + kt * c_tt
        beta = (kt * c_tn) / den
        c_s, c_p, c_m = c_nn - c_nt * beta, c_nn + mu * c_nt, c_nn - mu * c_nt
        finite, from_zero = np.isfinite, lambda v: np.isfinite(v) & (v >= 0)
        law = (from_zero(c_nn) & from_zero(k * c_nn)) if hertz else (finite(T(1) + k * c_nn) & (T(1) + k * c_nn > 0))
        solved = law & finite(c_tt) & finite(c_nt) & finite(c_tn) & (c_tt >= 0) & finite(den) & (den > 0) & from_zero(c_p) & from_zero(c_m) & \
            finite(k * c_s) & finite(k * c_p) & finite(k * c_m)
    return {"c_nn": c_nn, "c_nt": c_nt, "c_tn": c_tn, "c_tt": c_tt, "k": k, "mu": mu, "kt": kt, "den": den, "beta": beta, "c_s": c_s, "c_p": c_p, "c_m": c_m, "solved": solved,
            "hertz": bool(hertz)}


def step(x_n, x_t, q, c, T, steps=None):
    """Step 4t on scalars or arrays, element by element, by the header's tree in format T.  c: constants().  Returns a dict: f_n, f_t, q
    (the new anchor), branch (O, S, P, M), consistent (how many of S, P, M were consistent; 0 on an open frame), none (no candidate was
    consistent: the least miss was taken), and per candidate its (f_n, f_t, q', ok, miss) under "S", "P", "M"."""
    x_n, x_t, q = np.asarray(x_n, T), np.asarray(x_t, T), np.asarray(q, T)
    k, mu, kt, hertz = c["k"], c["mu"], c["kt"], c["hertz"]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        q = np.where(np.isfinite(q), q, x_t)
        closed = x_n > 0
        alpha = (kt * (x_t - q)) / c["den"]
        fn_s = normal_force(x_n - c["c_nt"] * alpha, c["c_s"], k, T, hertz, steps)
        ft_s = alpha - c["beta"] * fn_s
        ok_s, miss_s = np.abs(ft_s) <= mu * fn_s, np.abs(ft_s) - mu * fn_s
        fn_p = normal_force(x_n, c["c_p"], k, T, hertz, steps)
        ft_p = mu * fn_p
        q_p = ((x_t - c["c_tn"] * fn_p) - c["c_tt"] * ft_p) - ft_p / kt
        ok_p, miss_p = q_p >= q, kt * (q - q_p)
        fn_m = normal_force(x_n, c["c_m"], k, T, hertz, steps)
        ft_m = -(mu * fn_m)
        q_m = ((x_t - c["c_tn"] * fn_m) - c["c_tt"] * ft_m) - ft_m / kt
        ok_m, miss_m = q_m <= q, kt * (q_m - q)
        least = np.where(miss_p < miss_s, 1, 0)
        least = np.where(miss_m < np.where(least == 1, miss_p, miss_s), 2, least)
        none = closed & ~(ok_s | ok_p | ok_m)
        taken = np.where(ok_s, 0, np.where(ok_p, 1, np.where(ok_m, 2, least)))
        pick = lambda a, b, m: np.where(taken == 0, a, np.where(taken == 1, b, m))
        zero = np.zeros_like(x_n)
        f_n, f_t = np.where(closed, pick(fn_s, fn_p, fn_m), zero), np.where(closed, pick(ft_s, ft_p, ft_m), zero)
        q_new = np.where(closed, pick(q, q_p, q_m), x_t)
    assert f_n.dtype == T and f_t.dtype == T and q_new.dtype == T
    return {"f_n": f_n, "f_t": f_t, "q": q_new, "branch": np.where(closed, taken + 1, O), "none": none,
            "consistent": np.where(closed, ok_s.astype(int) + ok_p.astype(int) + ok_m.astype(int), 0),
            "S": (fn_s, ft_s, q, ok_s, miss_s), "P": (fn_p, ft_p, q_p, ok_p, miss_p), "M": (fn_m, ft_m, q_m, ok_m, miss_m)}


def gram(rng, count, modes=6):
    """Random compliances of `count` junctions as the bank forms them: C_ab = sum_k w_k g_a[k] g_b[k] with positive weights -- a positive
    diagonal times a Gram matrix; symmetric here.  Returns (C_nn, C_nt, C_tt) in longdouble."""
    g_n, g_t, w = rng.standard_normal((count, modes)), rng.standard_normal((count, modes)), rng.uniform(0.1, 1.0, (count, modes))
    mix = rng.uniform(-1, 1, (count, 1))  # (the tangent's gains lean on the normal's: every size of C_nt / sqrt(C_nn C_tt))
    g_t = mix * g_n + (1 - np.abs(mix)) * g_t
    as_l = lambda v: np.asarray(v, L)
    return as_l((w * g_n * g_n).sum(axis=1)), as_l((w * g_n * g_t).sum(axis=1)), as_l((w * g_t * g_t).sum(axis=1))


def cases(count, seed, hertz, inside=True):
    """Random cases of step 4t in longdouble: mu from 0.01 to 2, K C_nn and kt C_tt from 0.01 to 100 (Hertz: K C_nn sqrt(x_n)), open and
    closed, both signs of x_t - q, sized so that every branch occurs.  inside: the cone condition mu |C_nt| < C_nn holds (mu is drawn below
    C_nn / |C_nt| where that is needed); otherwise it fails.  Returns (x_n, x_t, q, constants)."""
    rng = np.random.default_rng(seed)
    c_nn, c_nt, c_tt = gram(rng, count)
    log = lambda lo, hi: np.asarray(10.0 ** rng.uniform(np.log10(lo), np.log10(hi), count), L)
    mu = log(0.01, 2.0)
    limit = c_nn / np.abs(c_nt)
    if inside:
        mu = np.where(mu < limit, mu, limit * np.asarray(rng.uniform(0.05, 0.95, count), L))
    else:
        mu = np.where(mu > limit, mu, limit * log(1.05, 5.0))
    x0 = log(1e-6, 1e-3)
    x_n = np.where(rng.uniform(size=count) < 0.15, -x0, x0)
    k = log(0.01, 100.0) / (c_nn * (np.sqrt(x0) if hertz else 1))
    kt = log(0.01, 100.0) / c_tt
    c = constants(c_nn, c_nt, c_nt, c_tt, k, mu, kt, L, hertz)
    # the spring's stretch against the cone's edge: |kt r| from a hundredth of mu f_n to a hundred times it
    f0 = normal_force(x0, c_nn, k, L, hertz)
    r = np.asarray(rng.choice([-1.0, 1.0], count), L) * log(0.01, 100.0) * mu * f0 / kt
    q = np.asarray(rng.standard_normal(count), L) * x0
    return x_n, q + r, q, c


def rounded(x_n, x_t, q, c, T):
    """The cases' numbers rounded to T and taken as exact: the same problem in T and, widened again, in longdouble."""
    r = lambda v: np.asarray(v, L).astype(T)
    cs = [constants(r(c["c_nn"]).astype(F), r(c["c_nt"]).astype(F), r(c["c_tn"]).astype(F), r(c["c_tt"]).astype(F), r(c["k"]).astype(F), r(c["mu"]).astype(F), r(c["kt"]).astype(F), F, c["hertz"])
          for F in (T, L)]
    return [(r(x_n).astype(F), r(x_t).astype(F), r(q).astype(F), cc) for F, cc in zip((T, L), cs)]


def figure(got, ref, kt):
    """Per case: the largest of |f_n - f_n*|, |f_t - f_t*| and |q - q*| kt, over max(f_n*, |f_t*|); 0 where the reference has no force."""
    a = lambda v: np.asarray(v, L)
    top = np.maximum(a(ref["f_n"]), np.abs(a(ref["f_t"])))
    err = np.maximum(np.maximum(np.abs(a(got["f_n"]) - a(ref["f_n"])), np.abs(a(got["f_t"]) - a(ref["f_t"]))), np.abs(a(got["q"]) - a(ref["q"])) * a(kt))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(top > 0, err / np.where(top > 0, top, 1), 0).astype(float)


def linearised(x_n, x_t, q, c, ref, T):
    """The project's yardstick: the bank's linear solve in format T on each case's linearisation at its solution, |f - f_exact| over
    max |f_exact| of that linear problem (0 on an open case).  The normal law is linearised to the stiffness 1.5 K sqrt(y*) (Hertz; K for
    the linear law) at the compression y* = x_n - C_nn f_n* - C_nt f_t*.  A slipping case is step 4's scalar solve, (K x) / (1 + K C_b) on
    C_P or C_M, followed by f_t = +- mu f_n and the anchor q' = ((x_t - C_tn f_n) - C_tt f_t) - f_t / kt of that force: the same quantity --
    forces and anchor -- of the linear problem (the anchor is a position, and what its rounding costs in force is a property of the
    problem's numbers, not of the solve).  A sticking case is two linear springs (K, kt) on the compliance matrix [[C_nn, C_nt], [C_tn, C_tt]] with x = (x_n, x_t - q):
    section 3e's linear solve of two members in contact (tests/group_harness.inverse and candidate), which is what mh.linearised uses."""
    out = np.zeros(len(x_n))
    a = lambda v, i: L(np.asarray(v, L).reshape(-1)[i] if np.asarray(v).size > 1 else np.asarray(v, L).reshape(-1)[0])
    for i in range(len(x_n)):
        br = int(ref["branch"][i])
        if br == O:
            continue
        fn, ft = a(ref["f_n"], i), a(ref["f_t"], i)
        c_nn, c_nt, c_tn, c_tt, k, mu, kt = (a(c[n], i) for n in ("c_nn", "c_nt", "c_tn", "c_tt", "k", "mu", "kt"))
        y = a(x_n, i) - c_nn * fn - c_nt * ft
        k_lin = L(1.5) * k * np.sqrt(max(y, L(0))) if c["hertz"] else k
        if br == S:
            C2, K2 = np.array([[c_nn, c_nt], [c_tn, c_tt]], L), np.array([k_lin, kt], L)
            f_lin = np.array([k_lin * y, ft], L)
            x_lin = np.array([y, ft / kt if kt > 0 else L(0)], L) + C2 @ f_lin
            Ct, Kt, xt = C2.astype(T), K2.astype(T), x_lin.astype(T)
            B = np.eye(2, dtype=L) + Ct.astype(L) * Kt.astype(L)[None, :]
            exact = Kt.astype(L) * gh._solve_pivoted(B, xt.astype(L))
            Minv, _ = gh.inverse(Ct, Kt, 3, T)
            _, f, _ = gh.candidate(xt, Ct, Kt, 3, Minv, T)
        else:
            c_b = c_nn + mu * c_nt if br == P else c_nn - mu * c_nt
            x_lin = y + c_b * (k_lin * y)
            kT, cT, xT = T(k_lin), T(c_b), T(x_lin)
            sign = 1 if br == P else -1
            def slipping(F):
                fn_ = (F(kT) * F(xT)) / (F(1) + F(kT) * F(cT))
                ft_ = F(sign) * (F(T(mu)) * fn_)
                q_ = ((F(T(a(x_t, i))) - F(T(c_tn)) * fn_) - F(T(c_tt)) * ft_) - ft_ / F(T(kt))
                return np.array([fn_, ft_, q_ * F(T(kt))], F)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                exact, f = slipping(L), slipping(T)
            top = np.abs(exact[:2]).max()
            out[i] = float(np.abs(f.astype(L) - exact).max() / top) if top > 0 else 0.0
            continue
        top = np.abs(exact).max()
        out[i] = float(np.abs(f.astype(L) - exact).max() / top) if top > 0 else 0.0
    return out


# ---- the render ----
class Restatement(hh.Restatement):
    """tests/hertz_harness.Restatement with render_friction: every junction a spec of this module; a frictional one takes steps 2, 3, 4t
    and 5 of the header's "Friction", every other one render_coupled's steps."""

    def four_compliances(self, s):
        """(C_nn, C_nt, C_tn, C_tt) of a frictional junction, each with step 3's summation order."""
        total = np.sum if self.T == L else jh._sequential
        sides = [(sd, tangent_side(sd, t)) for sd, t in ((s[0], s[5][0]), (s[1], s[5][1])) if sd is not None]
        g = [(self.side_gains(n), self.side_gains(t)) for n, t in sides]
        return tuple(total(np.concatenate([(read[2] * push[0]) for read, push in pairs]))
                     for pairs in ([(n, n) for n, t in g], [(n, t) for n, t in g], [(t, n) for n, t in g], [(t, t) for n, t in g]))

    def render_friction(self, rows, junctions, approach, travel, frames, anchor=None, trace=None):
        """rows: (object, ex_pos, direction, float32 signal[frames]); junctions: specs (friction None: render_coupled's junction);
        approach, travel: float32 [len(junctions)][frames]; anchor: one value per junction (None or not finite: no history).
        Returns (out, f_n rows, f_t rows, C_nn, statuses, anchors, counts[len(junctions)][3]).  trace (a dict, optional) receives
        "branch": [junction][frame]; "read1_n", "read1_t": what advance-1 pickups along n and along t on every side read after the frame;
        "compliances": the four per junction."""
        T = self.T
        total = np.sum if T == L else jh._sequential
        nj = len(junctions)
        junctions = [tuple(s) + (None,) * (6 - len(s)) for s in junctions]
        out, forces, tangents = np.zeros(frames, T), np.zeros((nj, frames), T), np.zeros((nj, frames), T)
        clean = lambda v: (lambda a: np.where(np.isfinite(a), a, np.float32(0)).astype(T))(np.asarray(v, np.float32).reshape(nj, frames))
        u, w = clean(approach), clean(travel)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains, gains_t, consts, status, comp, four = [], [], [], [], [], []
        for s in junctions:
            sides = [(sd, t) for sd, t in ((s[0], s[5][0] if s[5] else None), (s[1], s[5][1] if s[5] else None)) if sd is not None]
            gains.append([(sd[0],) + self.side_gains(sd) for sd, _ in sides])
            gains_t.append([(sd[0],) + self.side_gains(tangent_side(sd, t)) for sd, t in sides] if s[5] else None)
            k = T(np.float32(s[2]))
            if left_out(s):
                consts.append(None), four.append(None), comp.append(T(0)), status.append(0)
                gains_t[-1] = None
                continue
            if s[5]:
                cs = self.four_compliances(s)
                c = constants(*cs, k, T(np.float32(s[5][2])), T(np.float32(s[5][3])), T, s[4])
                four.append(cs)
                comp.append(cs[0])
                status.append(1 if bool(c["solved"]) else 2)
            else:
                c_nn = self.compliance(s[:4])
                with np.errstate(over="ignore", invalid="ignore"):
                    kc = k * c_nn
                    ok = (np.isfinite(c_nn) and c_nn >= 0 and np.isfinite(kc) and kc >= 0) if s[4] else (np.isfinite(T(1) + kc) and T(1) + kc > 0)
                c = {"k": k, "kc": kc, "denom": T(1) + kc}
                four.append(None)
                comp.append(c_nn)
                status.append(1 if ok else 2)
            consts.append(c)
        q = [T(np.nan) if anchor is None else T(anchor[j]) for j in range(nj)]
        counts, branch = np.zeros((nj, 3), np.uint32), np.zeros((nj, frames), np.int8)
        after_n, after_t = np.zeros((nj, frames), T), np.zeros((nj, frames), T)
        read = lambda g, stepped: total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in g]))
        for t in range(frames):
            stepped = []
            for o, ob in enumerate(self.objects):
                (z_re, z_im), c_re, c_im = self.z[o], ob["c_re"], ob["c_im"]
                e = np.zeros(len(z_re), T)
                for g, f in mine[o]:
                    e = e + f[t] * g
                stepped.append([z_re * c_re - z_im * c_im + e, z_re * c_im + z_im * c_re])
            for j, s in enumerate(junctions):
                if status[j] != 1:
                    continue
                x_n = u[j, t] - read(gains[j], stepped)
                if s[5]:
                    x_t = w[j, t] - read(gains_t[j], stepped)
                    got = step(x_n, x_t, q[j], consts[j], T, self.steps)
                    f_n, f_t, q[j], br = T(got["f_n"]), T(got["f_t"]), T(got["q"]), int(got["branch"])
                    forces[j, t], tangents[j, t], branch[j, t] = f_n, f_t, br
                    counts[j] += np.array([br == S, br in (P, M), bool(got["none"])], np.uint32)
                    for (o, a, _, _), (_, a_t, _, _) in zip(gains[j], gains_t[j]):
                        stepped[o][0] = stepped[o][0] + (a * f_n + a_t * f_t)
                else:
                    c = consts[j]
                    f_n = hh.hertz_force(x_n, c["kc"], c["k"], T, self.steps) if s[4] else (c["k"] * (x_n if x_n > 0 else T(0))) / c["denom"]
                    forces[j, t] = f_n
                    for (o, a, _, _) in gains[j]:
                        stepped[o][0] = stepped[o][0] + a * f_n
            for j in range(nj):
                after_n[j, t] = read(gains[j], stepped)
                if gains_t[j]:
                    after_t[j, t] = read(gains_t[j], stepped)
            for o, ob in enumerate(self.objects):
                z_re, z_im = stepped[o]
                self.z[o] = (z_re, z_im)
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
        anchors = np.array([q[j] if (junctions[j][5] and status[j] == 1) else T(np.nan) for j in range(nj)], T)
        for j in range(nj):
            if not (junctions[j][5] and status[j] == 1):
                counts[j] = 0
        if trace is not None:
            trace["branch"], trace["read1_n"], trace["read1_t"], trace["compliances"] = branch, after_n, after_t, four
        return out, forces, tangents, np.array([float(c) for c in comp]), np.array(status, np.uint8), anchors, counts
