"""Helpers of the mixed-group tests (tests/test_bank_mixed_cpu.py, tests/test_bank_mixed_gpu.py): step 4 of a junction group with a Hertz
member (include/modalhip.h, mh_bank_render_mixed, step 4m), restated in numpy for MANY CASES AT ONCE -- every array has the cases along
its first axis, so each numpy operation is one operation of the header's tree, rounded to the array's format, nothing contracted:

  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: `solve`, the header's tree operation for operation;
  numpy.longdouble               the reference: `reference`, a damped Newton iteration run to a fixed point, with a residual check.

and tests/group_harness.Restatement extended by the mixed step 4 (`Restatement.render_mixed`).  `linearised` is the yardstick of the
accuracy checks: section 3e's linear group solve, by its own functions, on the linearisation of a case at its solution."""
import numpy as np

from tests import group_harness as gh

L = np.longdouble
GROUP = gh.GROUP
SWEEPS, STEPS, REFINED = 1, 10, 1  # the header's counts: Gauss-Seidel sweeps, Newton steps, and those of them that start from a residual in twice the precision
RESIDUAL_TERMS = 16  # the residual test's multiple of u * (the magnitudes summed), derived in the header


# ---- the laws ----
def laws(y, hertz, bilateral, T):
    """phi(y) and phi'(y) per member: Hertz max(y, 0) sqrt(max(y, 0)) and 1.5 sqrt(max(y, 0)); bilateral y and 1; else max(y, 0) and [y > 0]."""
    pos = np.where(y > 0, y, T(0))
    r = np.sqrt(pos)
    phi = np.where(hertz, pos * r, np.where(bilateral, y, pos))
    dphi = np.where(hertz, T(1.5) * r, np.where(bilateral | (y > 0), T(1), T(0)))
    return phi, dphi


def _row(ck, phi, i, skip=None):
    """sum_j ck_ij phi_j in ascending j from +0 (without j = skip)."""
    acc = np.zeros_like(phi[:, 0])
    for j in range(phi.shape[1]):
        if j != skip:
            acc = acc + ck[:, i, j] * phi[:, j]
    return acc


def residual(y, ck, x, hertz, bilateral, T):
    """F_i = (y_i + sum_j ck_ij phi_j) - x_i, with phi and phi'."""
    phi, dphi = laws(y, hertz, bilateral, T)
    F = np.stack([(y[:, i] + _row(ck, phi, i)) - x[:, i] for i in range(y.shape[1])], 1)
    return F, phi, dphi


def one_dimensional(x, c, hertz, bilateral, T, offset=None):
    """A member alone: the root y of y + c phi(y) = x.  Hertz: step 4h's tree (the smaller of the bounds x and (x / c)^(2/3), four Newton
    steps); linear: x / (1 + c), taken for x > 0 only unless bilateral.  offset (a relative error, tests only) perturbs the cube root."""
    with np.errstate(all="ignore"):
        g = np.cbrt(np.where(x > 0, x, T(1)) / c)
        if offset is not None:
            g = g * T(1 + offset)
        g = g * g
        yh = np.where((c > 0) & (g < x), g, x)
        for _ in range(4):
            r = np.sqrt(np.where(x > 0, yh, T(0)))
            yh = yh - ((yh + (c * yh) * r) - x) / (T(1) + (T(1.5) * c) * r)
        yl = x / (T(1) + c)
    return np.where(hertz, np.where(x > 0, yh, x), np.where(bilateral | (x > 0), yl, x)).astype(T)


def newton_direction(ck, dphi, F, T):
    """d with J d = F, J = I + ck diag(phi'): elimination without pivoting in ascending order (row p times 1 / J_pp, then every later row
    minus J_ip times row p), back substitution in descending order."""
    n = F.shape[1]
    J = ck * dphi[:, None, :]
    for i in range(n):
        J[:, i, i] = T(1) + J[:, i, i]
    r = F.copy()
    for p in range(n):
        inv = T(1) / J[:, p, p]
        for j in range(p + 1, n):
            J[:, p, j] = J[:, p, j] * inv
        r[:, p] = r[:, p] * inv
        for i in range(p + 1, n):
            t = J[:, i, p].copy()
            for j in range(p + 1, n):
                J[:, i, j] = J[:, i, j] - t * J[:, p, j]
            r[:, i] = r[:, i] - t * r[:, p]
    d = np.empty_like(F)
    for p in range(n - 1, -1, -1):
        acc = r[:, p]
        for j in range(p + 1, n):
            acc = acc - J[:, p, j] * d[:, j]
        d[:, p] = acc
    return d


def two_sum(a, b):
    """a + b as (the rounded sum, its rounding error): six operations, exact."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_product(a, b, T):
    """a b as (the rounded product, its rounding error).  The device forms the error with one fused multiply-add, fma(a, b, -p); numpy has
    none, so it is formed here by Veltkamp's splitting -- the same number, since both are exact (barring overflow of the split)."""
    split = T(134217729.0) if T == np.float64 else (T(4097.0) if T == np.float32 else T(4294967297.0))
    p = a * b
    t = split * a
    ah = t - (t - a)
    al = a - ah
    t = split * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def forces(y, K, hertz, bilateral, T):
    """f_j = K_j phi_j(y_j) and K_j phi'_j(y_j)."""
    phi, dphi = laws(y, hertz, bilateral, T)
    return K * phi, K * dphi


def force_residual(y, C, K, x, hertz, bilateral, T, twice):
    """F_i = (y_i + sum_j C_ij f_j, ascending from +0) - x_i in the forces the solve returns; twice: the same sum carried in twice the
    working precision -- s = y_i, c = +0; per j: (p, e) = two_product(C_ij, f_j), (s, r) = two_sum(s, p), c = c + (r + e); then
    (s, r) = two_sum(s, -x_i), c = c + r; F_i = s + c."""
    f, kd = forces(y, K, hertz, bilateral, T)
    n = y.shape[1]
    F = np.empty_like(y)
    for i in range(n):
        if not twice:
            F[:, i] = (y[:, i] + _row(C, f, i)) - x[:, i]
            continue
        s, c = y[:, i].copy(), np.zeros_like(y[:, i])
        for j in range(n):
            p, e = two_product(C[:, i, j], f[:, j], T)
            s, r = two_sum(s, p)
            c = c + (r + e)
        s, r = two_sum(s, -x[:, i])
        c = c + r
        F[:, i] = s + c
    return F, f, kd


def solve(x, C, K, hertz, bilateral, T, sweeps=SWEEPS, steps=STEPS, offset=None, pad=False, history=None, refine=REFINED):
    """Step 4m in format T for cases x [N][n], C [N][n][n], K, hertz, bilateral [N][n]: the start y_j = the member alone at x_j (with
    ck_jj = C_jj K_j); `sweeps` Gauss-Seidel sweeps in ascending j (member j alone at x_j - sum_{i != j} C_ji f_i); `steps` Newton steps
    y -= d with J = I + C diag(K phi'), of which the last `refine` start from a residual summed in twice the working precision, as is the
    residual of the final y; f = K phi(y).  pad: the kernel's layout, every group padded to GROUP members with K = 0, C = 0, x = 0.
    Returns (f, y, unconverged: the residual test of the header, one bool per case)."""
    x, C, K = np.asarray(x, T), np.asarray(C, T), np.asarray(K, T)
    hertz, bilateral = np.asarray(hertz, bool), np.asarray(bilateral, bool)
    N, n = x.shape
    if pad and n < GROUP:
        m = GROUP - n
        x, K = np.concatenate([x, np.zeros((N, m), T)], 1), np.concatenate([K, np.zeros((N, m), T)], 1)
        hertz, bilateral = np.concatenate([hertz, np.zeros((N, m), bool)], 1), np.concatenate([bilateral, np.zeros((N, m), bool)], 1)
        Cp = np.zeros((N, GROUP, GROUP), T)
        Cp[:, :n, :n] = C
        C = Cp
    width = x.shape[1]
    with np.errstate(all="ignore"):
        cjj = np.stack([C[:, j, j] * K[:, j] for j in range(width)], 1)
        y = one_dimensional(x, cjj, hertz, bilateral, T, offset)
        for _ in range(sweeps):
            for j in range(width):
                f, _ = forces(y, K, hertz, bilateral, T)
                y[:, j] = one_dimensional((x[:, j] - _row(C, f, j, skip=j))[:, None], cjj[:, j:j + 1], hertz[:, j:j + 1], bilateral[:, j:j + 1], T, offset)[:, 0]
        F, f, kd = force_residual(y, C, K, x, hertz, bilateral, T, steps <= refine)
        for step in range(steps):
            y = y - newton_direction(C, kd, F, T)
            F, f, kd = force_residual(y, C, K, x, hertz, bilateral, T, step + 1 >= steps - refine)
            if history is not None:
                history.append(f[:, :n])
        # the residual test: |F_i| against RESIDUAL_TERMS u (|y_i| + sum_j |C_ij f_j| + |x_i|)
        u = T(np.finfo(T).eps) * T(0.5)
        bad = np.zeros(N, bool)
        for i in range(width):
            mag = np.abs(y[:, i]) + _row(np.abs(C), np.abs(f), i) + np.abs(x[:, i])
            bad |= ~(np.abs(F[:, i]) <= (T(RESIDUAL_TERMS) * u) * mag)
    assert f.dtype == T and y.dtype == T
    return f[:, :n], y[:, :n], bad


def reference(x, C, K, hertz, bilateral):
    """The longdouble reference: Newton steps, each halved while it does not lower the largest residual and taken at the last halving
    otherwise, until the iterate no longer moves.  Returns (f, y, largest residual / max |x| per case)."""
    x, C, K = np.asarray(x, L), np.asarray(C, L), np.asarray(K, L)
    hertz, bilateral = np.asarray(hertz, bool), np.asarray(bilateral, bool)
    N, n = x.shape
    with np.errstate(all="ignore"):
        ck = C * K[:, None, :]
        cjj = np.stack([ck[:, j, j] for j in range(n)], 1)
        y = one_dimensional(x, cjj, hertz, bilateral, L)
        F, phi, dphi = residual(y, ck, x, hertz, bilateral, L)
        for it in range(200):
            d = newton_direction(ck, dphi, F, L)
            yn = y - d
            Fn, pn, dn = residual(yn, ck, x, hertz, bilateral, L)
            if it < 150:  # damped while far; the last rounds are plain Newton
                worse = np.abs(Fn).max(1) > np.abs(F).max(1)
                t = L(1)
                for _ in range(6):
                    if not worse.any():
                        break
                    t = t / 2
                    yt = y - t * d
                    Ft, pt, dt = residual(yt, ck, x, hertz, bilateral, L)
                    take = worse & (np.abs(Ft).max(1) < np.abs(Fn).max(1))
                    yn, Fn, pn, dn = (np.where(take[:, None], a, b) for a, b in ((yt, yn), (Ft, Fn), (pt, pn), (dt, dn)))
                    worse = worse & (np.abs(Fn).max(1) > np.abs(F).max(1))
            moved = np.abs(yn - y).max()
            y, F, phi, dphi = yn, Fn, pn, dn
            if it >= 8 and moved == 0:
                break
        # at the fixed point the iterate moves within the rounding of F: of a few more steps the one of least residual is kept
        best_y, best_F, best_phi = y, F, phi
        for _ in range(6):
            y = y - newton_direction(ck, dphi, F, L)
            F, phi, dphi = residual(y, ck, x, hertz, bilateral, L)
            better = np.abs(F).max(1) < np.abs(best_F).max(1)
            best_y, best_F, best_phi = (np.where(better[:, None], p, q) for p, q in ((y, best_y), (F, best_F), (phi, best_phi)))
        y, F, phi = best_y, best_F, best_phi
    return K * phi, y, np.abs(F).max(1) / np.abs(x).max(1)


def status(C, K, hertz, T):
    """A group's status by the header's rule, per case: 2 (refused) when a C_ij or C_ij K_j is not finite, a |C_ij K_j| is above the square
    root of the format's largest number, C_ii or C_ii K_i is below 0 on a Hertz member, or 1 + C_ii K_i is not a finite number above 0 on
    a linear one; else 1."""
    C, K = np.asarray(C, T), np.asarray(K, T)
    with np.errstate(all="ignore"):
        ck = C * K[:, None, :]
        ok = np.isfinite(C).all(axis=(1, 2)) & np.isfinite(ck).all(axis=(1, 2)) & (np.abs(ck) <= np.sqrt(T(np.finfo(T).max))).all(axis=(1, 2))
        cii, ckii = np.einsum("nii->ni", C), np.einsum("nii->ni", ck)
        ok &= np.where(hertz, (cii >= 0) & (ckii >= 0), (T(1) + ckii > 0) & np.isfinite(T(1) + ckii)).all(axis=1)
    return np.where(ok, 1, 2)


# ---- the case sets ----
KINDS = ("gram", "rank-one", "opposite")


def cases(kind, n, count, mixed, seed):
    """`count` groups of n: C = D G with D a positive diagonal (0.32 .. 3.2) and G the Gram matrix of n vectors in six dimensions -- random;
    nearly rank one (+-(0.5 .. 2) times one direction, plus 1e-3 of a random one); two nearly opposite rows (row 1 = -row 0 plus 1e-3 of a random one) --,
    x = +-(1e-6 .. 1), and K with K C_ii sqrt|x_i| (Hertz) or K C_ii (linear) = 1e-3 .. 1e3, all log-uniform.  mixed: each member Hertz
    with probability 1/2 and a fifth of the linear ones bilateral.  Returns (x, C, K, hertz, bilateral) as float64 and bool arrays."""
    rng = np.random.default_rng(seed)
    dims = 6
    A = rng.standard_normal((count, n, dims))
    if kind == "rank-one":
        along = rng.uniform(0.5, 2.0, (count, n, 1)) * rng.choice([-1.0, 1.0], (count, n, 1))
        A = along * rng.standard_normal((count, 1, dims)) + 1e-3 * A
    elif kind == "opposite":
        A[:, 1] = -A[:, 0] + 1e-3 * rng.standard_normal((count, dims))
    else:
        assert kind == "gram"
    G = A @ A.transpose(0, 2, 1)
    C = 10.0 ** rng.uniform(-0.5, 0.5, (count, n))[:, :, None] * G
    x = 10.0 ** rng.uniform(-6, 0, (count, n)) * rng.choice([-1.0, 1.0], (count, n))
    hertz = rng.random((count, n)) < 0.5 if mixed else np.ones((count, n), bool)
    bilateral = ~hertz & (rng.random((count, n)) < 0.2)
    strength = 10.0 ** rng.uniform(-3, 3, (count, n))
    cii = np.einsum("nii->ni", C)
    K = np.where(hertz, strength / (cii * np.sqrt(np.abs(x))), strength / cii)
    return x, C, K, hertz, bilateral


def linearised(x, C, K, hertz, bilateral, y_star, f_star, T):
    """Section 3e's linear solve in format T, by tests/group_harness's own functions, on each case's linearisation at its solution:
    stiffness 1.5 K sqrt(y*) on a Hertz member, the same C, the active set of the solution, and the x at which that linear problem has
    the solution y*.  Returns per case |f - f_exact| / max |f_exact| of that linear problem (0 where it has no force)."""
    out = np.zeros(len(x))
    for c in range(len(x)):
        n = x.shape[1]
        ys, Cl = np.asarray(y_star[c], L), np.asarray(C[c], L)
        Kl = np.where(hertz[c], L(1.5) * np.asarray(K[c], L) * np.sqrt(np.where(ys > 0, ys, 0)), np.asarray(K[c], L))
        mask = sum(1 << i for i in range(n) if bilateral[c][i] or (ys[i] > 0 and Kl[i] > 0))
        A = gh.members(mask, n)
        if not A:
            continue
        f_lin = np.zeros(n, L)
        f_lin[A] = Kl[A] * ys[A]
        x_lin = ys + Cl @ f_lin  # the linear problem's x: y* solves it on A
        Ct, Kt, xt = Cl.astype(T), Kl.astype(T), x_lin.astype(T)
        # the exact solution of the problem the working precision is given (its rounded inputs)
        exact = np.zeros(n, L)
        B = np.eye(len(A), dtype=L) + Ct.astype(L)[np.ix_(A, A)] * Kt.astype(L)[A][None, :]
        exact[A] = Kt.astype(L)[A] * gh._solve_pivoted(B, xt.astype(L)[A])
        M, _ = gh.inverse(Ct, Kt, mask, T)
        _, f, _ = gh.candidate(xt, Ct, Kt, mask, M, T)
        top = np.abs(exact).max()
        out[c] = float(np.abs(f.astype(L) - exact).max() / top) if top > 0 else 0.0
    return out


# ---- the render ----
def spec(a, b=None, stiffness=0.0, bilateral=False, hertz=False):
    """A flagged junction as tests/group_harness.spec gives it."""
    return gh.spec(a, b, stiffness, bilateral, hertz, True)


def steered(n, C, K, hertz, scale, first_frame, hold=8):
    """tests/test_bank_groups_gpu._steered for every member's own law: for `hold` frames at a time one subset A is aimed at -- the empty
    one, the full one, every other one in turn and one of two favoured ones -- by u = d + x with x chosen so that the exact solution is
    y_j = scale_j (1 + cos(0.37 s + j) / 2) on A and x_j - (C f)_j = -scale_j / 2 off it: x = y + C (K phi(y)) on A."""
    full = (1 << n) - 1
    turn = []
    for m in range(1, full):
        turn += [0, full, m, 1 if m & 1 else full - 1]
    C, K, scale, hertz = np.asarray(C, np.float64), np.asarray(K, np.float64), np.asarray(scale, np.float64), np.asarray(hertz, bool)

    def u_of(t, d):
        s = first_frame + t
        mask = turn[(s // hold) % len(turn)]
        inside = np.array([bool(mask >> j & 1) for j in range(n)])
        y = np.where(inside, scale * (1 + 0.5 * np.cos(0.37 * s + np.arange(n))), 0.0)
        x = np.where(inside, y, -0.5 * scale) + C @ (K * np.where(hertz, y * np.sqrt(y), y))
        return (np.asarray(d, np.float64) + x).astype(np.float32)
    return u_of


class Restatement(gh.Restatement):
    """tests/group_harness.Restatement whose render_mixed closes one group's loop per frame with step 4m: steps 1, 2, 3 and 5 are
    render_grouped's, operation for operation; step 4 is `solve` in the working precision and `reference` in numpy.longdouble."""

    def render_mixed(self, rows, junctions, approach, frames, trace=None):
        """render_grouped's arguments; a junction's hertz flag (spec[4]) is read as well.  Returns (out, forces, C_ii, statuses, unconverged
        frames); trace receives "d", "read1", "x", "u", "touching": the number of members with a force above 0, per frame, and "sets": the
        active set per frame as a bit mask over the members, bit j set when f_j > 0."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else gh.jh._sequential
        n = len(junctions)
        assert 2 <= n <= GROUP
        out, forces = np.zeros(frames, T), np.zeros((n, frames), T)
        steer = approach if callable(approach) else None
        u = np.zeros((n, frames), np.float32) if steer else np.asarray(approach, np.float32).reshape(n, frames)
        u = np.where(np.isfinite(u), u, np.float32(0)).astype(T)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains = [[(sd[0],) + self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None] for s in junctions]
        C = self.compliance_matrix(junctions)
        K = np.array([T(np.float32(s[2])) for s in junctions], T)
        bilateral, hertz = np.array([bool(s[3]) for s in junctions]), np.array([bool(s[4]) for s in junctions])
        free, after, xs, touching = np.zeros((n, frames), T), np.zeros((n, frames), T), np.zeros((n, frames), T), np.zeros(frames, np.int32)
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
            if exact:
                f, _, res = reference(x[None], C[None], K[None], hertz[None], bilateral[None])
                assert float(res[0]) <= 1e-15 or not np.abs(x).max() > 0, float(res[0])
            else:
                f, _, bad = solve(x[None], C[None], K[None], hertz[None], bilateral[None], T, pad=True)
                unconverged += int(bad[0])
            f = f[0]
            forces[:, t] = f
            touching[t] = int((f > 0).sum())
            active[t] = sum(1 << j for j in range(n) if f[j] > 0)
            for j in range(n):  # on each object its junctions in ascending call order
                for (o, a, _, _) in gains[j]:
                    stepped[o][0] = stepped[o][0] + a * f[j]
            for j in range(n):
                after[j, t] = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
            for o, ob in enumerate(self.objects):
                z_re, z_im = stepped[o]
                self.z[o] = (z_re, z_im)
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
        if trace is not None:
            trace["d"], trace["read1"], trace["x"], trace["touching"], trace["u"] = free, after, xs, touching, u.astype(np.float32)
            trace["sets"] = active
        return out, forces, np.array([float(C[i, i]) for i in range(n)]), np.array([1] * n, np.uint8), unconverged
