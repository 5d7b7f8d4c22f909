"""Helpers of the junction-group tests (tests/test_bank_groups_cpu.py, tests/test_bank_groups_gpu.py): junction records with the shared
flag, the scalar solve of a group's step 4 (include/modalhip.h, MH_JUNCTION_SHARED), and tests/junction_harness.Restatement extended by
the group steps, in a number format of the caller's choice:

  numpy.longdouble               the reference: the complementarity problem solved by exact enumeration -- every admissible subset's
                                 linear system solved with partial pivoting, the consistent one taken;
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the header's tree operation for operation, every operation rounded to
                                 the bank's format, nothing contracted -- the elimination of [B | I] over the subset without pivoting in
                                 ascending order, the candidates' rows summed in ascending order from +0, the consistent subset of lowest
                                 mask, the subset that fails by least, clamped, when rounding leaves none.  The sums of d and C are sequential in mode order
                                 (side a's modes, then side b's).  Its deviation from the longdouble one is the yardstick the device's
                                 deviation is measured by."""
import numpy as np

from tests import junction_harness as jh

POINTS = jh.POINTS
NO_OBJECT = jh.NO_OBJECT
GROUP = 4  # MH_JUNCTION_GROUP
side = jh.side
replay_drives = jh.replay_drives
row_figure = jh.row_figure


def spec(a, b=None, stiffness=0.0, bilateral=False, hertz=False, shared=True):
    """A junction as plain data: (side a, side b or None, K as the float the record holds, bilateral, hertz, shared)."""
    return (a, b, float(np.float32(stiffness)), bool(bilateral), bool(hertz), bool(shared))


def record(s):
    """The binding's Junction record of a spec (a 4- or 5-tuple of the other harnesses is an unflagged junction)."""
    from mesheditor_amd import bank as hipbank
    a, b, k, bilateral, hertz, shared = tuple(s) + (False,) * (6 - len(s))
    return hipbank.Junction.of(a, b, k, bilateral, hertz, shared)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Junction * len(specs))(*[record(s) for s in specs]) if specs else []


# ---- the scalar solve ----
def admissible(n, bilateral):
    """The subsets of a group of n, as bit masks in ascending order, that contain every bilateral member (bilateral: a list of bools)."""
    must = sum(1 << i for i in range(n) if bilateral[i])
    return [m for m in range(1 << n) if m & must == must]


def members(mask, n):
    return [i for i in range(n) if mask >> i & 1]


def inverse(C, K, mask, T):
    """M_A = (I + C_AA diag(K_A))^-1 by the header's tree in format T: the elimination of [B | I] over the members of A, without pivoting,
    in ascending order -- pivot p: r = 1 / B_pp; row p of both halves times r; every other row i: t = B_ip, row i minus t times row p.
    Returns (M as an n x n array whose rows and columns outside A are zero, pivots_ok)."""
    n = len(K)
    A = members(mask, n)
    C, K = np.asarray(C, T), np.asarray(K, T)
    B, M = np.zeros((n, n), T), np.zeros((n, n), T)
    ok = True
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in A:
            for j in A:
                kc = C[i, j] * K[j]
                B[i, j] = T(1) + kc if i == j else kc
            M[i, i] = T(1)
        for p in A:
            pivot = B[p, p]
            ok = ok and bool(np.isfinite(pivot) and pivot > 0)
            r = T(1) / pivot
            for j in A:
                B[p, j], M[p, j] = B[p, j] * r, M[p, j] * r
            for i in A:
                if i == p:
                    continue
                t = B[i, p]
                for j in A:
                    B[i, j], M[i, j] = B[i, j] - t * B[p, j], M[i, j] - t * M[p, j]
    assert M.dtype == T
    return M, ok


def prepare(C, K, bilateral, T):
    """What a block forms once: [(mask, M_A)] of the admissible subsets, and the group's status -- 2 (refused) when a C_ij or C_ij K_j is
    not finite or a pivot of an M_A is not a finite number above 0, else 1."""
    n = len(K)
    C, K = np.asarray(C, T), np.asarray(K, T)
    with np.errstate(over="ignore", invalid="ignore"):
        finite = bool(np.isfinite(C).all() and np.isfinite(C * K[None, :]).all())
    sets, ok = [], finite
    for mask in admissible(n, bilateral):
        M, good = inverse(C, K, mask, T)
        sets.append((mask, M))
        ok = ok and good
    return sets, (1 if ok else 2)


def candidate(x, C, K, mask, M, T):
    """Subset A's candidate by the header's tree: y_i = sum_{j in A} M_ij x_j (ascending j from +0), f_i = K_i y_i on A and +0 off it;
    outside A the residual x_j - sum_{i in A} C_ji f_i (ascending i from +0).  Returns (y, f, residual)."""
    n = len(K)
    A = members(mask, n)
    y, f, res = np.zeros(n, T), np.zeros(n, T), np.zeros(n, T)
    for i in A:
        acc = T(0)
        for j in A:
            acc = acc + M[i, j] * x[j]
        y[i] = acc
        f[i] = K[i] * acc
    for j in range(n):
        if j in A:
            continue
        push = T(0)
        for i in A:
            push = push + C[j, i] * f[i]
        res[j] = x[j] - push
    return y, f, res


def consistent(y, res, mask, bilateral):
    n = len(y)
    return all((bilateral[j] or y[j] > 0) if mask >> j & 1 else not (res[j] > 0) for j in range(n))


def solve(x, C, K, bilateral, T, sets=None):
    """Step 4 of a group in the working precision T: the consistent subset of lowest mask; when rounding leaves none (on a boundary
    between two subsets), the subset that fails by least -- the largest -y_j of a unilateral member or residual of a member outside it,
    lowest mask among equals -- with f_j = K_j max(y_j, 0) on its unilateral members.  Returns (f, mask taken, negated - 1 for that last
    resort: -1 - mask)."""
    x, C, K = np.asarray(x, T), np.asarray(C, T), np.asarray(K, T)
    n = len(K)
    if sets is None:
        sets, _ = prepare(C, K, bilateral, T)
    best = None
    for mask, M in sets:
        y, f, res = candidate(x, C, K, mask, M, T)
        if consistent(y, res, mask, bilateral):
            return f, mask
        miss = T(0)
        for j in range(n):
            over = (T(0) if bilateral[j] else T(0) - y[j]) if mask >> j & 1 else res[j]
            miss = over if over > miss else miss
        if best is None or miss < best[0]:
            best = (miss, mask, y, f)
    _, mask, y, f = best
    f = np.array([(f[j] if bilateral[j] else K[j] * (y[j] if y[j] > 0 else T(0))) if mask >> j & 1 else T(0) for j in range(n)], T)
    return f, -1 - mask


def lane_solve(x, C, K, bilateral, T):
    """Step 4 the way k_bank_modes_grouped lays it out (mh_bank.hip), restated lane by lane in format T: the group padded to GROUP members
    (K = 0, C = 0, x = 0 beyond n); lane m = the subset with mask m keeps ONE matrix W -- row i of M_A for a member of A, row i of C for
    one outside it -- eliminated in place over A; per frame y_i = sum_{j in A} W_ij x_j for EVERY i (off the subset that is a product with
    a row of C, not a displacement), f_i = K_i y_i on A and +0 off it, the residuals from the rows of C in W, `miss`; then the ballot: the
    lowest consistent admissible lane, else the lowest lane whose miss is the least, clamped.  Returns (f[:n], mask taken, or -1 - mask)."""
    n = len(K)
    xs, Ks, Cs = np.zeros(GROUP, T), np.zeros(GROUP, T), np.zeros((GROUP, GROUP), T)
    xs[:n], Ks[:n], Cs[:n, :n] = np.asarray(x, T), np.asarray(K, T), np.asarray(C, T)
    bil = sum(1 << i for i in range(n) if bilateral[i])
    full, most, zero = (1 << n) - 1, np.finfo(T).max, T(0)
    lanes = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for mask in range(1 << GROUP):
            inside = [bool(mask >> i & 1) for i in range(GROUP)]
            admissible_lane = mask <= full and mask & bil == bil
            W = np.zeros((GROUP, GROUP), T)
            for j in range(GROUP):
                for i in range(GROUP):
                    kc = Cs[i, j] * Ks[j]
                    W[i, j] = ((T(1) + kc if i == j else kc) if inside[j] else zero) if inside[i] else Cs[i, j]
            for p in range(GROUP):
                if not inside[p]:
                    continue
                r = T(1) / W[p, p]
                W[p, p] = T(1)
                for j in range(GROUP):
                    W[p, j] = W[p, j] * r
                for i in range(GROUP):
                    if i == p or not inside[i]:
                        continue
                    t = W[i, p]
                    W[i, p] = zero
                    for j in range(GROUP):
                        W[i, j] = W[i, j] - t * W[p, j]
            y, f = np.zeros(GROUP, T), np.zeros(GROUP, T)
            for i in range(GROUP):
                acc = zero
                for j in range(GROUP):
                    if inside[j]:
                        acc = acc + W[i, j] * xs[j]
                y[i] = acc
                f[i] = Ks[i] * acc if inside[i] else zero
            ok, miss = admissible_lane, zero
            for j in range(GROUP):
                push = zero
                for i in range(GROUP):
                    if inside[i]:
                        push = push + W[j, i] * f[i]
                two_way = bool(bil >> j & 1)
                over = (zero if two_way else zero - y[j]) if inside[j] else xs[j] - push
                fits = (two_way or y[j] > 0) if inside[j] else not (over > 0)
                ok = ok and fits
                miss = over if over > miss else miss
            clamped = np.array([((f[i] if bil >> i & 1 else Ks[i] * (y[i] if y[i] > 0 else zero)) if inside[i] else zero) for i in range(GROUP)], T)
            lanes.append((admissible_lane, ok, miss, f, clamped))
    found = [m for m, lane in enumerate(lanes) if lane[1]]
    if found:
        return lanes[found[0]][3][:n].copy(), found[0]
    least = min((lane[2] if lane[0] else most) for lane in lanes)
    taken = [m for m, lane in enumerate(lanes) if lane[0] and lane[2] == least][0]
    return lanes[taken][4][:n].copy(), -1 - taken


def _solve_pivoted(B, rhs):
    """B y = rhs in numpy.longdouble by elimination with partial pivoting (numpy.linalg has no longdouble)."""
    B, rhs = np.array(B, np.longdouble), np.array(rhs, np.longdouble)
    m = len(rhs)
    for p in range(m):
        q = p + int(np.argmax(np.abs(B[p:, p])))
        if q != p:
            B[[p, q]], rhs[[p, q]] = B[[q, p]], rhs[[q, p]]
        for i in range(p + 1, m):
            t = B[i, p] / B[p, p]
            B[i, p:] -= t * B[p, p:]
            rhs[i] -= t * rhs[p]
    y = np.zeros(m, np.longdouble)
    for p in range(m - 1, -1, -1):
        y[p] = (rhs[p] - np.dot(B[p, p + 1:], y[p + 1:])) / B[p, p]
    return y


def solve_exact(x, C, K, bilateral, every=True, first=None):
    """Step 4 in numpy.longdouble by exact enumeration.  Returns (f of the consistent subset of lowest mask, the consistent masks -- one,
    for a P-matrix and an x in general position; every = False stops at the first, and then `first`, a mask, is tried before the others:
    the consistent subset being the only one, the order of the search does not change what is found)."""
    L = np.longdouble
    x, C, K = np.asarray(x, L), np.asarray(C, L), np.asarray(K, L)
    n = len(K)
    found = []
    order = admissible(n, bilateral)
    if first is not None and not every and first in order:
        order = [first] + [m for m in order if m != first]
    for mask in order:
        A = members(mask, n)
        y, f = np.zeros(n, L), np.zeros(n, L)
        if A:
            B = np.eye(len(A), dtype=L) + C[np.ix_(A, A)] * K[A][None, :]
            y[A] = _solve_pivoted(B, x[A])
            f[A] = K[A] * y[A]
        res = x - C @ f
        if consistent(y, res, mask, bilateral):
            found.append((mask, f))
            if not every:
                break
    assert found, "no consistent subset in longdouble"
    return found[0][1], [m for m, _ in found]


# ---- the render ----
class Restatement(jh.Restatement):
    """tests/junction_harness.Restatement whose render_grouped closes ONE GROUP's loop per frame: every junction passed is a member, in
    call order."""

    def compliance_matrix(self, junctions):
        """C_ij = sum over the objects on a side of both i and j -- side a of i, then side b of i -- of sum_k g_re_i[k] a_j[k]."""
        T = self.T
        n = len(junctions)
        gains = [{sd[0]: self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None} for s in junctions]
        C = np.zeros((n, n), T)
        for i, s in enumerate(junctions):
            for j in range(n):
                terms = [gains[i][sd[0]][2] * gains[j][sd[0]][0] for sd in (s[0], s[1]) if sd is not None and sd[0] in gains[j]]
                if terms:
                    terms = np.concatenate(terms)
                    C[i, j] = np.sum(terms) if T == np.longdouble else jh._sequential(terms)
        return C

    def render_grouped(self, rows, junctions, approach, frames, trace=None):
        """rows: (object, ex_pos, direction, float32 signal[frames]); junctions: the group's members (specs; only sides, K and bilateral are
        read); approach: float32 [len(junctions)][frames], or a function (frame, d of that frame) -> the frame's n samples, for a signal
        that is steered by the run itself (trace["u"] then holds what it gave, as float32).  Returns (out[frames], forces[n][frames], C_ii, statuses).  trace (a dict,
        optional) receives "d", "read1" as jh.Restatement.render_coupled's, "x" [n][frames], and "sets": the mask taken per frame (exact:
        the consistent one of lowest mask; working: -1 - mask for the clamped last resort)."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else jh._sequential
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
        bilateral = [bool(s[3]) for s in junctions]
        if exact:
            sets, status = None, 1
            for mask in admissible(n, bilateral):
                A = members(mask, n)
                if A and not (np.linalg.det(np.eye(len(A)) + np.asarray(C, np.float64)[np.ix_(A, A)] * np.asarray(K, np.float64)[A][None, :]) > 0):
                    status = 2
        else:
            sets, status = prepare(C, K, bilateral, T)
        free, after, xs, taken = np.zeros((n, frames), T), np.zeros((n, frames), T), np.zeros((n, frames), T), np.zeros(frames, np.int32)
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
            if status == 1:
                if exact:
                    f, masks = solve_exact(x, C, K, bilateral, every=False, first=int(taken[t - 1]) if t else None)
                    taken[t] = masks[0]
                else:
                    f, taken[t] = solve(x, C, K, bilateral, T, sets)
                forces[:, t] = f
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
            trace["d"], trace["read1"], trace["x"], trace["sets"], trace["u"] = free, after, xs, taken, u.astype(np.float32)
        return out, forces, np.array([float(C[i, i]) for i in range(n)]), np.array([status] * n, np.uint8)
