"""Helpers of the damped-group tests (tests/test_bank_damped_groups_cpu.py, tests/test_bank_damped_groups_gpu.py): step 4 of a junction
group with a damped member (include/modalhip.h, mh_bank_render_damped_groups, step 4g), restated in numpy for MANY CASES AT ONCE as
tests/mixed_harness does -- the cases along the first axis, each numpy operation one operation of the header's tree:

  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: `solve`, the header's tree operation for operation;
  numpy.longdouble               the reference: `reference`, a damped Newton iteration run to a fixed point, with a residual check.

and tests/mixed_harness.Restatement extended by step 4g and the carry (`Restatement.render_damped_groups`).  `linearised` is the
yardstick of the accuracy checks: section 3e's linear group solve on the linearisation of a case at its solution."""
import numpy as np

from tests import damped_harness as dd
from tests import group_harness as gh
from tests import mixed_harness as mh

L = np.longdouble
GROUP = gh.GROUP
SWEEPS, STEPS, REFINED = 1, 8, 2  # the header's counts for step 4g
RESIDUAL_TERMS = 32  # the residual test's multiple of u * (the magnitudes summed), derived in the header
KINDS = mh.KINDS


def spec(a, b=None, stiffness=0.0, bilateral=False, hertz=False, damped=False):
    """A flagged junction: tests/group_harness.spec plus the damped flag as a sixth field."""
    return gh.spec(a, b, stiffness, bilateral, hertz, True) + (bool(damped),)


def record(s):
    from mesheditor_amd import bank as hipbank
    a, b, k, bilateral, hertz, shared = s[:6]
    return hipbank.Junction.of(a, b, k, bilateral, hertz, shared=shared, damped=bool(s[6]) if len(s) > 6 else False)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Junction * len(specs))(*[record(s) for s in specs]) if specs else []


# ---- the laws ----
def forces(y, K, hertz, bilateral, damped, lam, yp, T):
    """Per member f_j, kd_j = df_j / dy_j and the magnitude g_j of the residual test.  With (phi, phi') of step 4m, kp = K phi and
    kq = K phi': a member that is not damped has f = kp, kd = kq, g = |kp|; a damped one m = 1 + l (y - y_p) and, for m > 0, f = kp m,
    kd = kq m + kp l, else f = +0, kd = 0; its g = kp (1 + l (|y| + |y_p|))."""
    phi, dphi = mh.laws(y, hertz, bilateral, T)
    kp, kq = K * phi, K * dphi
    m = T(1) + lam * (y - yp)
    closed = m > 0
    f = np.where(damped, np.where(closed, kp * m, T(0)), kp)
    kd = np.where(damped, np.where(closed, kq * m + kp * lam, T(0)), kq)
    g = np.where(damped, kp * (T(1) + lam * (np.abs(y) + np.abs(yp))), np.abs(kp))
    return f.astype(T), kd.astype(T), g.astype(T)


def alone(x, c, K, hertz, bilateral, damped, lam, yp, T):
    """A member alone: the root y of y + c psi(y) = x.  A damped member by step 4d's trees (tests/damped_harness.damped_solve, cl = c l,
    six Newton steps in every format: the longdouble reference takes it as a start only), every other one by step 4m's
    (tests/mixed_harness.one_dimensional)."""
    plain = mh.one_dimensional(x, c, hertz, bilateral, T)
    with np.errstate(all="ignore"):
        _, y_lin = dd.damped_solve(x, c, lam, yp, K, T, False)
        _, y_hz = dd.damped_solve(x, c, lam, yp, K, T, True, steps=dd.STEPS)
    return np.where(damped, np.where(hertz, y_hz, y_lin), plain).astype(T)


def _row(C, f, i, skip=None):
    return mh._row(C, f, i, skip)


def force_residual(y, C, K, x, hertz, bilateral, damped, lam, yp, T, twice):
    """tests/mixed_harness.force_residual with step 4g's forces: F, f, kd, g."""
    f, kd, g = forces(y, K, hertz, bilateral, damped, lam, yp, T)
    n = y.shape[1]
    F = np.empty_like(y)
    for i in range(n):
        if not twice:
            F[:, i] = (y[:, i] + _row(C, f, i)) - x[:, i]
            continue
        s, c = y[:, i].copy(), np.zeros_like(y[:, i])
        for j in range(n):
            p, e = mh.two_product(C[:, i, j], f[:, j], T)
            s, r = mh.two_sum(s, p)
            c = c + (r + e)
        s, r = mh.two_sum(s, -x[:, i])
        c = c + r
        F[:, i] = s + c
    return F, f, kd, g


def _padded(arrays, n, T):
    x, C, K, hertz, bilateral, damped, lam, yp = arrays
    N, m = len(x), GROUP - n
    z, zb = np.zeros((N, m), T), np.zeros((N, m), bool)
    Cp = np.zeros((N, GROUP, GROUP), T)
    Cp[:, :n, :n] = C
    cat = lambda a, b: np.concatenate([a, b], 1)
    return cat(x, z), Cp, cat(K, z), cat(hertz, zb), cat(bilateral, zb), cat(damped, zb), cat(lam, z), cat(yp, z)


def solve(x, C, K, hertz, bilateral, damped, lam, yp, T, sweeps=SWEEPS, steps=STEPS, refine=REFINED, pad=False, history=None, report=None):
    """Step 4g in format T for cases x [N][n], C [N][n][n], and K, hertz, bilateral, damped, lam, yp [N][n] (lam and yp as the frame takes
    them: 0 on a member without history): the start y_j = the member alone at x_j; `sweeps` Gauss-Seidel sweeps in ascending j; `steps`
    Newton steps with J = I + C diag(kd), the last `refine` from a residual summed in twice the working precision and plain, every earlier
    one followed by the step back through a member's own tree (below); the forces of the last y.  pad: the kernel's layout, every group
    padded to GROUP members with K = 0, C = 0, x = 0.  Returns (f, y, unconverged: the header's residual test, one bool per case);
    report (a dict) receives "residual": the largest |F_i| / (u times the magnitudes summed) per case."""
    x, C, K, lam, yp = (np.asarray(v, T) for v in (x, C, K, lam, yp))
    hertz, bilateral, damped = (np.asarray(v, bool) for v in (hertz, bilateral, damped))
    N, n = x.shape
    if pad and n < GROUP:
        x, C, K, hertz, bilateral, damped, lam, yp = _padded((x, C, K, hertz, bilateral, damped, lam, yp), n, T)
    width = x.shape[1]
    with np.errstate(all="ignore"):
        cjj = np.stack([C[:, j, j] * K[:, j] for j in range(width)], 1)
        cdiag = np.stack([C[:, j, j] for j in range(width)], 1)
        y = alone(x, cjj, K, hertz, bilateral, damped, lam, yp, T)
        for _ in range(sweeps):
            for j in range(width):
                f, _, _ = forces(y, K, hertz, bilateral, damped, lam, yp, T)
                s = slice(j, j + 1)
                y[:, j] = alone((x[:, j] - _row(C, f, j, skip=j))[:, None], cjj[:, s], K[:, s], hertz[:, s], bilateral[:, s], damped[:, s], lam[:, s], yp[:, s], T)[:, 0]
        F, f, kd, g = force_residual(y, C, K, x, hertz, bilateral, damped, lam, yp, T, steps <= refine)
        for step in range(steps):
            moved = y - mh.newton_direction(C, kd, F, T)
            if step < steps - refine:
                # a unilateral member that was open or clamped (kd = 0), or whose step more than doubles y, takes its own tree at its
                # row's linearised right-hand side, x_j - sum_{i != j} C_ji (f_i + kd_i dy_i) = moved_j + C_jj (f_j + kd_j dy_j)
                own = moved + cdiag * (f + kd * (moved - y))
                far = (kd == 0) | (moved > T(2) * y)
                y = np.where(far & ~bilateral, alone(own, cjj, K, hertz, bilateral, damped, lam, yp, T), moved)
            else:
                y = moved
            F, f, kd, g = force_residual(y, C, K, x, hertz, bilateral, damped, lam, yp, T, step + 1 >= steps - refine)
            if history is not None:
                history.append(f[:, :n])
        u = T(np.finfo(T).eps) * T(0.5)
        bad, worst = np.zeros(N, bool), np.zeros(N)
        for i in range(width):
            mag = np.abs(y[:, i]) + _row(np.abs(C), g, i) + np.abs(x[:, i])
            bad |= ~(np.abs(F[:, i]) <= (T(RESIDUAL_TERMS) * u) * mag)
            worst = np.maximum(worst, np.where(mag > 0, np.abs(F[:, i]).astype(float) / np.where(mag > 0, float(u) * mag.astype(float), 1.0), 0.0))
        if report is not None:
            report["residual"] = worst
    assert f.dtype == T and y.dtype == T
    return f[:, :n], y[:, :n], bad


def _exact_residual(y, ck, x, hertz, bilateral, damped, lam, yp):
    """F = y + ck psi(y) - x in longdouble, with psi = phi max(m, 0) on a damped member, and psi'."""
    phi, dphi = mh.laws(y, hertz, bilateral, L)
    m = L(1) + lam * (y - yp)
    closed = m > 0
    psi = np.where(damped, np.where(closed, phi * m, L(0)), phi)
    dpsi = np.where(damped, np.where(closed, dphi * m + phi * lam, L(0)), dphi)
    F = np.stack([(y[:, i] + _row(ck, psi, i)) - x[:, i] for i in range(y.shape[1])], 1)
    return F, psi, dpsi


def reference(x, C, K, hertz, bilateral, damped, lam, yp):
    """The longdouble reference, tests/mixed_harness.reference's iteration on step 4g's law: Newton steps, each halved while it does not
    lower the largest residual, until the iterate no longer moves.  Returns (f, y, the largest |F_i| over the magnitudes the residual test sums, per case)."""
    x, C, K, lam, yp = (np.asarray(v, L) for v in (x, C, K, lam, yp))
    hertz, bilateral, damped = (np.asarray(v, bool) for v in (hertz, bilateral, damped))
    N, n = x.shape
    res = lambda v: _exact_residual(v, ck, x, hertz, bilateral, damped, lam, yp)
    with np.errstate(all="ignore"):
        ck = C * K[:, None, :]
        cjj = np.stack([ck[:, j, j] for j in range(n)], 1)
        y = alone(x, cjj, K, hertz, bilateral, damped, lam, yp, L)
        F, psi, dpsi = res(y)
        for it in range(300):
            d = mh.newton_direction(ck, dpsi, F, L)
            yn = y - d
            Fn, pn, dn = res(yn)
            if it < 250:
                worse = ~(np.abs(Fn).max(1) <= np.abs(F).max(1))
                t = L(1)
                for _ in range(8):
                    if not worse.any():
                        break
                    t = t / 2
                    yt = y - t * d
                    Ft, pt, dt = res(yt)
                    take = worse & ~(np.abs(Ft).max(1) >= np.abs(Fn).max(1))
                    yn, Fn, pn, dn = (np.where(take[:, None], a, b) for a, b in ((yt, yn), (Ft, Fn), (pt, pn), (dt, dn)))
                    worse = worse & ~(np.abs(Fn).max(1) <= np.abs(F).max(1))
            moved = np.abs(yn - y).max()
            y, F, psi, dpsi = yn, Fn, pn, dn
            if it >= 8 and moved == 0:
                break
        best_y, best_F, best_psi = y, F, psi
        for _ in range(6):
            y = y - mh.newton_direction(ck, dpsi, F, L)
            F, psi, dpsi = res(y)
            better = np.abs(F).max(1) < np.abs(best_F).max(1)
            best_y, best_F, best_psi = (np.where(better[:, None], p, q) for p, q in ((y, best_y), (F, best_F), (psi, best_psi)))
        y, F, psi = best_y, best_F, best_psi
        _, _, g = forces(y, K, hertz, bilateral, damped, lam, yp, L)
        mag = np.stack([np.abs(y[:, i]) + _row(np.abs(C), g, i) + np.abs(x[:, i]) for i in range(n)], 1)
    return K * psi, y, (np.abs(F) / np.where(mag > 0, mag, 1)).max(1)


def measure(y, K, hertz, bilateral, damped, lam, yp):
    """The accuracy measure's denominator per case, in longdouble: max_j K_j phi_j(y_j) (1 + l_j (|y_j| + |y_p,j|)) (|K phi| on a member
    that is not damped)."""
    _, _, g = forces(np.asarray(y, L), np.asarray(K, L), hertz, bilateral, damped, np.asarray(lam, L), np.asarray(yp, L), L)
    return np.abs(g).max(1)


def status(C, K, hertz, damped, lam, T):
    """A group's status by the header's rule: tests/mixed_harness.status's conditions with a damped member counted as a Hertz one where
    the law decides (C_ii and C_ii K_i not below 0), plus, on a damped member, C_ii K_i l_i a finite number not below 0 and every
    |C_ij K_j l_j| within the square root of the format's largest number."""
    C, K, lam = np.asarray(C, T), np.asarray(K, T), np.asarray(lam, T)
    damped = np.asarray(damped, bool)
    with np.errstate(all="ignore"):
        base = mh.status(C, K, np.asarray(hertz, bool) | damped, T) == 1
        ck = C * K[:, None, :]
        ckl = ck * lam[:, None, :]
        ckii = np.einsum("nii->ni", ck)
        cl = ckii * lam
        ok = np.where(damped, (cl >= 0) & np.isfinite(cl), True).all(axis=1)
        ok &= np.where(damped[:, None, :], np.abs(ckl) <= np.sqrt(T(np.finfo(T).max)), True).all(axis=(1, 2))
    return np.where(base & ok, 1, 2)


def sequence(xs, C, K, hertz, bilateral, damped, lam, carry, T, exact=False):
    """A block of frames of one group: xs [frames][n]; carry [n], not finite: no history for that member.  Frame by frame step 4g with
    y_p the compression the previous frame's solve left (`reference` when exact).  Returns (f [frames][n], carry out: the last frame's y
    on a damped member, a quiet NaN on every other; the carry that came in when there is no frame)."""
    F = L if exact else T
    damped = np.asarray(damped, bool)
    came = np.asarray(carry, F)
    known = damped & np.isfinite(came)
    yp = np.where(known, came, F(0)).astype(F)
    out = np.zeros((len(xs), len(damped)), F)
    one = lambda v: np.asarray(v)[None]
    for t, x in enumerate(xs):
        l_now = np.where(known, np.asarray(lam, F), F(0)).astype(F)
        if exact:
            f, y, res = reference(one(x), one(C), one(K), one(hertz), one(bilateral), one(damped), one(l_now), one(yp))
            assert float(res[0]) <= 1e-18
        else:
            f, y, bad = solve(one(x), one(C), one(K), one(hertz), one(bilateral), one(damped), one(l_now), one(yp), T, pad=True)
            assert not bad[0]
        out[t] = f[0]
        yp, known = np.where(damped, y[0], F(0)).astype(F), damped.copy()
    if not len(xs):
        return out, came
    return out, np.where(damped, yp, F(np.nan)).astype(F)


# ---- the case sets ----
def cases(kind, n, count, mixed, seed):
    """tests/mixed_harness.cases plus, per member: damped -- about half of the unilateral members --, l with l |x| = 0 (one case in eight)
    or 1e-3 .. 1e3 log-uniform, and y_p = x times a uniform number in [-3, 3].  Returns (x, C, K, hertz, bilateral, damped, lam, yp)."""
    x, C, K, hertz, bilateral = mh.cases(kind, n, count, mixed, seed)
    rng = np.random.default_rng(seed + 7919)
    damped = ~bilateral & (rng.random((count, n)) < 0.5)
    strength = np.where(rng.random((count, n)) < 0.125, 0.0, 10.0 ** rng.uniform(-3, 3, (count, n)))
    lam = np.where(damped, strength / np.abs(x), 0.0)
    yp = np.where(damped, x * rng.uniform(-3, 3, (count, n)), 0.0)
    return x, C, K, hertz, bilateral, damped, lam, yp


def linearised(x, C, K, hertz, bilateral, damped, lam, yp, y_star, T):
    """Section 3e's linear solve in format T, by tests/group_harness's own functions, on each case's linearisation at its solution: stiffness
    K (phi' m + phi l) on a damped member (1.5 K sqrt(y*) on a Hertz one, K on a linear one), the same C, the active set of the solution,
    and the x at which that linear problem has the solution y*.  Returns per case |f - f_exact| of that linear problem."""
    out = np.zeros(len(x), L)
    _, kd_all, _ = forces(np.asarray(y_star, L), np.asarray(K, L), hertz, bilateral, damped, np.asarray(lam, L), np.asarray(yp, L), L)
    for c in range(len(x)):
        n = x.shape[1]
        ys, Cl, Kl = np.asarray(y_star[c], L), np.asarray(C[c], L), kd_all[c]
        mask = sum(1 << i for i in range(n) if bilateral[c][i] or (ys[i] > 0 and Kl[i] > 0))
        A = gh.members(mask, n)
        if not A:
            continue
        f_lin = np.zeros(n, L)
        f_lin[A] = Kl[A] * ys[A]
        x_lin = ys + Cl @ f_lin
        Ct, Kt, xt = Cl.astype(T), Kl.astype(T), x_lin.astype(T)
        exact = np.zeros(n, L)
        B = np.eye(len(A), dtype=L) + Ct.astype(L)[np.ix_(A, A)] * Kt.astype(L)[A][None, :]
        exact[A] = Kt.astype(L)[A] * gh._solve_pivoted(B, xt.astype(L)[A])
        M, _ = gh.inverse(Ct, Kt, mask, T)
        _, f, _ = gh.candidate(xt, Ct, Kt, mask, M, T)
        top = np.abs(exact).max()
        out[c] = np.abs(f.astype(L) - exact).max() / top if top > 0 else 0
    return out


# ---- the render ----
class Steer:
    """tests/mixed_harness.steered for step 4g's law: for `hold` frames at a time one subset A is aimed at -- the empty one, the full one,
    every other one in turn and one of two favoured ones -- by u = d + x with x chosen so that the exact solution is
    y_j = scale_j (1 + cos(w s + j) / 2) on A and x_j - (C f)_j = -scale_j / 2 off it: x = y + C f(y), f the member's own law at the
    y_p this object keeps from frame to frame (the aimed-at y of the frame before; none ahead of the first).  w = 0.37 / max(1, l d): a
    member that stays in A changes y by less than a fifth of 1 / l per frame, so its factor m stays above 0 and the set aimed at is the
    set that pushes."""

    def __init__(self, n, C, K, hertz, damped, lam, scale, hold, lam_x):
        full = (1 << n) - 1
        self.turn = []
        for m in range(1, full):
            self.turn += [0, full, m, 1 if m & 1 else full - 1]
        self.n, self.hold = n, hold
        self.C, self.K, self.scale, self.lam = (np.asarray(v, np.float64) for v in (C, K, scale, lam))
        self.hertz, self.damped = np.asarray(hertz, bool), np.asarray(damped, bool)
        self.yp, self.first, self.speed = None, 0, 0.37 / max(1.0, lam_x)

    def __call__(self, t, d):
        s = self.first + t
        mask = self.turn[(s // self.hold) % len(self.turn)]
        inside = np.array([bool(mask >> j & 1) for j in range(self.n)])
        y = np.where(inside, self.scale * (1 + 0.5 * np.cos(self.speed * s + np.arange(self.n))), -0.5 * self.scale)
        pos = np.maximum(y, 0.0)
        m = np.ones(self.n) if self.yp is None else np.where(self.damped, np.maximum(1.0 + self.lam * (y - self.yp), 0.0), 1.0)
        f = np.where(inside, self.K * np.where(self.hertz, pos * np.sqrt(pos), pos) * m, 0.0)
        self.yp = y
        return (np.asarray(d, np.float64) + y + self.C @ f).astype(np.float32)


class Restatement(mh.Restatement):
    """tests/mixed_harness.Restatement whose render_damped_groups closes one group's loop per frame with step 4g and keeps the carry."""

    def render_damped_groups(self, rows, junctions, approach, damping, carry, frames, trace=None):
        """render_mixed's arguments plus damping (l per member and frame, float32, as mh_bank_render_damped_groups takes it) and carry (one
        value per member, not finite: no history).  A junction's damped flag is spec[6].  Returns (out, forces, C_ii, statuses,
        unconverged frames, carry); trace also receives "y", the compressions the solve left."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else gh.jh._sequential
        n = len(junctions)
        assert 2 <= n <= GROUP
        out, forces_out = np.zeros(frames, T), np.zeros((n, frames), T)
        steer = approach if callable(approach) else None
        u = np.zeros((n, frames), np.float32) if steer else np.asarray(approach, np.float32).reshape(n, frames)
        u = np.where(np.isfinite(u), u, np.float32(0)).astype(T)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains = [[(sd[0],) + self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None] for s in junctions]
        C = self.compliance_matrix(junctions)
        K = np.array([T(np.float32(s[2])) for s in junctions], T)
        bilateral, hertz = np.array([bool(s[3]) for s in junctions]), np.array([bool(s[4]) for s in junctions])
        damped = np.array([len(s) > 6 and bool(s[6]) for s in junctions])
        lam_all = np.where(damped, np.asarray(damping, np.float32).astype(T), T(0)).astype(T)
        came = np.asarray(carry, T)
        known = damped & np.isfinite(came)
        yp = np.where(known, came, T(0)).astype(T)
        free, after, xs, ys = (np.zeros((n, frames), T) for _ in range(4))
        active = np.zeros(frames, np.int32)
        unconverged = 0
        for t in range(frames):
            stepped = []
            for o, ob in enumerate(self.objects):
                (z_re, z_im), c_re, c_im = self.z[o], ob["c_re"], ob["c_im"]
                e = np.zeros(len(z_re), T)
                for g, f in mine[o]:
                    e = e + f[t] * g
                stepped.append([z_re * c_re - z_im * c_im + e, z_re * c_im + z_im * c_re])
            for j in range(n):
                free[j, t] = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
            if steer:
                u[:, t] = np.asarray(steer(t, free[:, t]), np.float32).astype(T)
            x = u[:, t] - free[:, t]
            xs[:, t] = x
            lam = np.where(known, lam_all, T(0)).astype(T)
            args = (x[None], C[None], K[None], hertz[None], bilateral[None], damped[None], lam[None], yp[None])
            if exact:
                f, y, res = reference(*args)
                assert float(res[0]) <= 1e-18, float(res[0])
            else:
                f, y, bad = solve(*args, T, pad=True)
                unconverged += int(bad[0])
            f, y = f[0], y[0]
            yp, known = np.where(damped, y, T(0)).astype(T), damped.copy()
            forces_out[:, t], ys[:, t] = f, y
            active[t] = sum(1 << j for j in range(n) if f[j] > 0)
            for j in range(n):
                for (o, a, _, _) in gains[j]:
                    stepped[o][0] = stepped[o][0] + a * f[j]
            for j in range(n):
                after[j, t] = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
            for o, ob in enumerate(self.objects):
                z_re, z_im = stepped[o]
                self.z[o] = (z_re, z_im)
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
        if trace is not None:
            trace["d"], trace["read1"], trace["x"], trace["y"], trace["u"], trace["sets"] = free, after, xs, ys, u.astype(np.float32), active
        carry_out = np.where(damped, yp if frames else came, T(np.nan)).astype(T)
        return out, forces_out, np.array([float(C[i, i]) for i in range(n)]), np.array([1] * n, np.uint8), unconverged, carry_out
