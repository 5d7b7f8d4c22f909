"""CPU-side checks of the Coulomb friction of the contact junctions (include/modalhip.h, "Friction"): every layer declares the flag, the
record and the entries; step 4t's enumeration is well posed inside the cone condition and not outside it; the step in float32 and float64
is within the project's margin of the longdouble step, across the boundaries between its branches as well; and the restatement the GPU
tests trust (tests/friction_harness.py) agrees with closed forms on one mode, with the dead kinds and with the refused ones."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import friction_harness as fh
from tests.test_bank_pickups_cpu import _OneMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
L = np.longdouble
FORMATS = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["fp32", "fp64"])
LAWS = pytest.mark.parametrize("hertz", [False, True], ids=["linear", "hertz"])


# ---- 1. the layers ----
def _parameters(path, name):
    """The number of parameters of the one `int name(...)` in a C or C++ source, comments stripped (tests/test_bank_entries_cpu.py)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, path)).read(), flags=re.S)
    found = re.findall(r"\bint\s+%s\s*\(([^()]*)\)" % re.escape(name), text)
    assert len(found) == 1, (path, name, len(found))
    return len([p for p in found[0].split(",") if p.strip()])


def test_every_layer_carries_the_flag_the_record_and_the_entries():
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    assert re.search(r"#define\s+MH_JUNCTION_FRICTION\s+16u", header)
    from mesheditor_amd import _lib, bank
    assert bank.JUNCTION_FRICTION == 16 and _lib.JUNCTION_FRICTION == 16
    a = (3, 2, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0)
    assert bank.Junction.of(a, None, 5.0).flags == 0 and bank.Junction.of(a, None, 5.0, friction=True).flags == 16
    assert bank.Junction.of(a, None, 5.0, hertz=True, friction=True).flags == 18
    assert C.sizeof(bank.Junction) == C.sizeof(_lib.Junction) == _lib.lib().mh_junction_struct_size()  # no struct changes
    order = ["ta", "tb", "mu", "stiffness"]
    for image in (_lib.Friction, bank.Friction):
        assert C.sizeof(image) == 32 and [n for n, _ in image._fields_] == order and [getattr(image, n).offset for n in order] == [0, 12, 24, 28]
    assert _lib.lib().mh_friction_struct_size() == 32
    mirror = open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "bank.hpp")).read()
    assert re.search(r"ModalJunctionFriction\{16\}", mirror) and "struct ModalFriction" in mirror and "RenderModalFriction" in mirror
    assert "TangentialStiffness" in open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "contact.hpp")).read()
    assert hasattr(bank.Scene, "render_friction")


def test_the_entries_have_the_parameters_their_bindings_pass_and_refuse_a_null_bank():
    from mesheditor_amd import _lib, bank
    fn, parent = _lib.lib().mh_bank_render_friction, _lib.lib().mh_bank_render_damped_groups
    assert "mh_bank_render_friction" in _lib.lib()._declared and "mh_friction_struct_size" in _lib.lib()._declared
    assert _parameters("include/modalhip.h", "mh_bank_render_friction") == len(fn.argtypes) == len(parent.argtypes) + 5
    assert _parameters("mesheditor_amd/csrc/mh_bank.hip", "mh_bank_render_friction") == len(fn.argtypes)
    assert list(fn.argtypes[:len(parent.argtypes)]) == list(parent.argtypes)  # mh_bank_render_damped_groups' parameters in its order, then five
    assert fn(*([None] + [0] * (len(fn.argtypes) - 1))) == _lib.MH_EINVAL
    scene, scene_parent = bank.lib().mhx_render_friction, bank.lib().mhx_render_damped_groups
    assert _parameters("mesheditor_amd/cpp/src/capi.cpp", "mhx_render_friction") == len(scene.argtypes) == len(scene_parent.argtypes) + 5


def test_the_mirror_s_friction_test_compiles_and_its_host_cases_pass():
    """tests/cpp/modal_friction_test.cpp holds the static_asserts on the flag and the record; built the way tests/test_cpp_junction_mirror.py
    builds its own, and its cases that need no GPU run."""
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "mesheditor_amd", "libmodalhost.so")):
        ge.build()
    subprocess.run(["make", "-s", "-C", CPP, "bin/modal_friction_test"], check=True)
    p = subprocess.run([os.path.join(CPP, "bin", "modal_friction_test"), "--host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ---- 2. well-posedness ----
@LAWS
def test_inside_the_cone_condition_exactly_one_candidate_is_consistent(hertz):
    """50 000 random cases per law (tests/friction_harness.cases: mu 0.01 ... 2, K C and kt C_tt 0.01 ... 100, open and closed, both signs of
    x_t - q, random Gram C) with mu |C_nt| < C_nn, in longdouble: every closed case has exactly one consistent candidate, every junction is
    solved, and each of O, S, P, M holds at least 5 % of the cases."""
    x_n, x_t, q, c = fh.cases(50000, 20260 + int(hertz), hertz, inside=True)
    assert (c["mu"] * np.abs(c["c_nt"]) < c["c_nn"]).all() and c["solved"].all()
    got = fh.step(x_n, x_t, q, c, L)
    closed = x_n > 0
    assert (got["consistent"][closed] == 1).all(), np.bincount(got["consistent"][closed])
    assert not got["none"].any() and (got["branch"][~closed] == fh.O).all()
    shares = [float((got["branch"] == b).mean()) for b in (fh.O, fh.S, fh.P, fh.M)]
    print("%s: shares of O, S, P, M: %s" % ("hertz" if hertz else "linear", ["%.3f" % s for s in shares]))
    assert min(shares) >= 0.05, shares


@LAWS
def test_outside_the_cone_condition_two_candidates_can_be_consistent(hertz):
    """20 000 cases per law with mu |C_nt| > C_nn: the junction is refused, and cases with two consistent candidates exist."""
    x_n, x_t, q, c = fh.cases(20000, 20270 + int(hertz), hertz, inside=False)
    assert (c["mu"] * np.abs(c["c_nt"]) > c["c_nn"]).all() and not c["solved"].any()
    got = fh.step(x_n, x_t, q, c, L)
    two = int((got["consistent"] >= 2).sum())
    print("%s: %d of %d cases outside the cone condition have two consistent candidates" % ("hertz" if hertz else "linear", two, len(x_n)))
    assert two > 0


# ---- 3. the step against longdouble ----
MARGIN = 4  # x the error of the bank's linear solve on the linearisation at the solution: the project's margin
# twice the ratio measured on each of the four sets below (the test prints them): 0.87, 1.25, 1.88, 1.01
ASSERTED = {(np.float32, False): 1.74, (np.float32, True): 2.5, (np.float64, False): 3.76, (np.float64, True): 2.02}
COUNT = 4000
_CACHE = {}


def _set(T, hertz):
    """The set's cases rounded to T, the step in T and in longdouble on those numbers, the figure per case and the yardstick per case."""
    key = (T, hertz)
    if key not in _CACHE:
        x_n, x_t, q, c = fh.cases(COUNT, 20280 + int(hertz), hertz, inside=True)
        (wx_n, wx_t, wq, wc), (ex_n, ex_t, eq, ec) = fh.rounded(x_n, x_t, q, c, T)
        keep = np.asarray(ec["solved"] & wc["solved"] & (ec["mu"] * np.abs(ec["c_nt"]) < ec["c_nn"]))  # (rounding may move a case out of the cone)
        got, ref = fh.step(wx_n, wx_t, wq, wc, T), fh.step(ex_n, ex_t, eq, ec, L)
        fig = np.where(keep, fh.figure(got, ref, ec["kt"]), 0.0)
        yard = np.where(keep, fh.linearised(ex_n, ex_t, eq, ec, ref, T), 0.0)
        _CACHE[key] = {"inputs": (wx_n, wx_t, wq, wc, ex_n, ex_t, eq, ec), "got": got, "ref": ref, "figure": fig, "yard": yard, "keep": keep}
    return _CACHE[key]


@FORMATS
@LAWS
def test_the_step_is_within_the_margin_of_the_linear_solve(T, hertz):
    """|f_n - f_n*|, |f_t - f_t*| and |q - q*| kt over max(f_n*, |f_t*|), the largest over the set, against the largest error of the bank's
    linear solve in the same format on the linearisations at the solutions (tests/friction_harness.linearised: step 4's scalar solve on a
    slipping case, section 3e's two-member solve on a sticking one).  A case whose two precisions choose different candidates stays in the
    figure: the law is continuous across every boundary.  4 x is allowed; asserted is twice the largest ratio measured.

    Measured (this test prints them): see DESIGN.md section 3j."""
    s = _set(T, hertz)
    differ = int((s["got"]["branch"] != s["ref"]["branch"])[s["keep"]].sum())
    err, yard = float(s["figure"].max()), float(s["yard"].max())
    eps = float(np.finfo(T).eps)
    print("%s %s: step %.3e (%.1f eps), linear solve %.3e (%.1f eps), ratio %.2f; %d of %d cases choose another candidate; %d frames without a consistent one" %
          (T.__name__, "hertz" if hertz else "linear", err, err / eps, yard, yard / eps, err / yard, differ, int(s["keep"].sum()), int(s["got"]["none"].sum())))
    assert yard > 0 and ASSERTED[(T, hertz)] <= MARGIN
    assert err <= ASSERTED[(T, hertz)] * yard, (err, yard, err / yard)


@FORMATS
@LAWS
def test_the_law_does_not_jump_across_a_boundary(T, hertz):
    """Lines in (x_n, x_t) across each boundary -- O | closed along x_n; S | P and S | M along x_t and along x_n -- located by bisection
    in longdouble on 40 cases each; at the 16 numbers of format T nearest to the boundary on either side the step in T is compared with the
    longdouble step at the same point, whichever candidates the two choose.  The deviations of the test above -- |f_n - f_n*|, |f_t - f_t*|,
    |q - q*| kt -- over the case's own max(f_n*, |f_t*|), the forces at the line's start, within the same bound.  (Not over the forces at the
    boundary point: along a line on which x_n shrinks to 0 they vanish while the anchor stays the position it is, and what its last place
    is worth in force, kt eps |q|, does not shrink with them.  A jump would be a step in the force itself.)"""
    s = _set(T, hertz)
    wx_n, wx_t, wq, wc, ex_n, ex_t, eq, ec = s["inputs"]
    bound = ASSERTED[(T, hertz)] * float(s["yard"].max())
    ref_branch = s["ref"]["branch"]
    pick = lambda v, i: np.asarray(v).reshape(-1)[i] if np.asarray(v).size > 1 else np.asarray(v).reshape(-1)[0]
    worst, walked = 0.0, 0
    for br in (fh.S, fh.P, fh.M):
        for i in [int(i) for i in np.flatnonzero((ref_branch == br) & s["keep"])[:40]]:
            names = ("c_nn", "c_nt", "c_tn", "c_tt", "k", "mu", "kt")
            c_t = fh.constants(*[pick(wc[n], i) for n in names], T, hertz)
            c_l = fh.constants(*[L(pick(wc[n], i)) for n in names], L, hertz)
            xn, xt, q = L(wx_n[i]), L(wx_t[i]), L(wq[i])
            scale = max(L(s["ref"]["f_n"][i]), abs(L(s["ref"]["f_t"][i])))
            assert scale > 0
            branch_at = lambda a, b: int(fh.step(L(T(a)), L(T(b)), q, c_l, L)["branch"])
            lines = [(lambda t: (xn * t, xt), 1.0, 0.0)]  # x_n shrinks through the cone's edge (a sticking case) and through 0
            if br == fh.S:
                lines.append((lambda t: (xn, q + (xt - q) * t), 1.0, 1e6))  # the spring stretches until it slips
            else:
                lines.append((lambda t: (xn, q + (xt - q) * t), 1.0, 0.0))  # it relaxes until it sticks
            for line, inside, outside in lines:
                lo, hi = L(inside), L(outside)
                if branch_at(*line(lo)) == branch_at(*line(hi)):
                    continue
                here = branch_at(*line(lo))
                for _ in range(90):
                    mid = (lo + hi) / 2
                    lo, hi = (mid, hi) if branch_at(*line(mid)) == here else (lo, mid)
                a, b = line(lo)
                moving = 0 if line(L(0.5))[0] != xn else 1
                centre = T(a if moving == 0 else b)
                points = [centre]
                for direction in (-np.inf, np.inf):
                    v = centre
                    for _ in range(16):
                        v = np.nextafter(v, T(direction))
                        points.append(v)
                for v in points:
                    pn, pt = (v, T(b)) if moving == 0 else (T(a), v)
                    got, ref = fh.step(pn, pt, T(q), c_t, T), fh.step(L(pn), L(pt), q, c_l, L)
                    off = max(abs(L(got["f_n"]) - ref["f_n"]), abs(L(got["f_t"]) - ref["f_t"]), abs(L(got["q"]) - ref["q"]) * c_l["kt"])
                    worst = max(worst, float(off / scale))
                walked += 1
    print("%s %s: %d boundary crossings walked, largest figure %.3e, bound %.3e" % (T.__name__, "hertz" if hertz else "linear", walked, worst, bound))
    assert walked >= 100
    assert worst <= bound, (worst, bound)


# ---- 4. one mode ----
NORMAL, TANGENT, COUPLING, POINT = (0.25, -1.0, 0.5), (0.25, 1.0, 0.5), 3.0, 2  # (the mode moves as far along t as along n: mu |C_nt| <= C_nn up to mu = 1)
MODE_FORMATS = pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])


def _one_mode_gains(s, direction):
    """(a, read) of the one mode at POINT along a direction, in double."""
    along = s.shape_x[POINT] * direction[0] + s.shape_y[POINT] * direction[1] + s.shape_z[POINT] * direction[2]
    return s.rad * along, COUPLING * s.defl_scale * along * s.defl


def _static(s):
    """The one-mode static compliances G_ab = read_a a_b c_im / |1 - c|^2: a constant force pair holds the mode at z = (a f_n + a_t f_t) / (1 - c)."""
    (a, read), (a_t, read_t) = _one_mode_gains(s, NORMAL), _one_mode_gains(s, TANGENT)
    g = s.c.imag / abs(1 - s.c) ** 2
    return read * a * g, read * a_t * g, read_t * a * g, read_t * a_t * g


def _junction(stiffness, mu, kt, hertz=False, friction=True, tangent=TANGENT):
    return fh.spec(fh.side(0, POINT, direction=NORMAL, coupling=COUPLING), None, stiffness, hertz, tangent, (0.0, 0.0, 0.0), mu, kt, friction)


@MODE_FORMATS
def test_a_stuck_contact_is_the_stick_spring_in_series_with_the_compliances(dtype):
    """One mode, constant u, the anchor at 0 and a small slow oscillation of w (period 6 000 frames against the mode's 14-frame decay):
    every frame sticks, the compliances are the closed forms, and f_t follows the static solution of
    y = u - G_nn f_n - G_nt f_t,  e = w - G_tn f_n - G_tt f_t,  f_n = K y,  f_t = kt e -- two springs in series with the static compliances --
    to 2 % of its swing (the lag of a 14-frame decay on a 6 000-frame period is 2 pi 14 / 6000 = 1.5 %)."""
    s, frames, K, kt, mu = _OneMode(), 6000, 40.0, 25.0, 0.8
    r = fh.Restatement(s, [1], dtype)
    t = np.arange(frames)
    u = np.full((1, frames), 0.375, np.float32)
    w = (0.01 * np.sin(2 * np.pi * t / 6000.0)).astype(np.float32)[None, :]
    trace = {}
    _, f_n, f_t, comp, status, anchor, counts = r.render_friction([], [_junction(K, mu, kt)], u, w, frames, [0.0], trace)
    (a, read), (a_t, read_t) = _one_mode_gains(s, NORMAL), _one_mode_gains(s, TANGENT)
    want = [read * s.c.imag * a, read * s.c.imag * a_t, read_t * s.c.imag * a, read_t * s.c.imag * a_t]
    assert status[0] == 1 and all(abs(float(g) - v) <= 8 * float(np.finfo(dtype).eps) * abs(v) + 1e-18 for g, v in zip(trace["compliances"][0], want))
    assert list(counts[0]) == [frames, 0, 0] and anchor[0] == 0
    g_nn, g_nt, g_tn, g_tt = _static(s)
    A = np.array([[1 + K * g_nn, kt * g_nt], [K * g_tn, 1 + kt * g_tt]])  # unknowns: y and the stretch e - q
    sol = np.linalg.solve(A, np.stack([u[0].astype(float), w[0].astype(float)]))
    law_t = kt * sol[1]
    settled = slice(200, frames)
    swing = float(np.abs(law_t[settled]).max() - law_t[settled].min()) / 2
    assert swing > 0 and float(np.abs(np.asarray(f_t[0], float) - law_t)[settled].max()) <= 0.02 * 2 * swing
    assert float(np.abs(np.asarray(f_n[0], float) - K * sol[0])[settled].max()) <= 0.02 * float(K * sol[0].max())


@MODE_FORMATS
@pytest.mark.parametrize("rate", [2e-3, -2e-3])
def test_a_dragged_contact_slides_at_the_edge_of_the_cone(dtype, rate):
    """One mode, constant u, w a ramp: once the contact has settled and the stick spring has stretched, the contact slides -- every later
    frame on P (on M for a ramp the other way), f_t = +- mu f_n to the bit, the anchor follows w, and |f_t| <= mu f_n throughout.  (While
    the normal force sets in, the coupling C_tn shears the contact as well: the first frames may take any branch.)"""
    s, frames, K, kt, mu = _OneMode(), 600, 40.0, 25.0, 0.3
    r = fh.Restatement(s, [1], dtype)
    u = np.full((1, frames), 0.375, np.float32)
    w = (rate * np.arange(frames)).astype(np.float32)[None, :]
    trace = {}
    _, f_n, f_t, _, status, anchor, counts = r.render_friction([], [_junction(K, mu, kt)], u, w, frames, None, trace)
    f_n, f_t, br = np.asarray(f_n[0]), np.asarray(f_t[0]), trace["branch"][0]
    T = f_n.dtype.type
    assert status[0] == 1 and counts[0][2] == 0 and (f_n > 0).all()
    sliding = fh.P if rate > 0 else fh.M
    first = int(np.flatnonzero(br != sliding)[-1]) + 1
    assert 0 < first < frames // 2 and (br[:first] == fh.S).any()
    cone = T(np.float32(mu)) * f_n
    assert (np.abs(f_t) <= cone).all() and (f_t[first:] == (cone[first:] if rate > 0 else -cone[first:])).all()
    assert counts[0][0] == int((br == fh.S).sum()) and counts[0][1] == frames - counts[0][0]
    assert np.sign(float(anchor[0])) == np.sign(rate) and abs(float(anchor[0])) > 0.5 * abs(rate) * frames  # the slider was dragged along


@MODE_FORMATS
@LAWS
def test_the_slider_never_gives_work_back(dtype, hertz):
    """One mode rung by a drive, u a slow sine that makes and breaks the contact, w a sine: in every closed frame the slider moves in the
    direction of the force, f_t (q[s] - q[s-1]) >= 0, and over the run the friction dissipates; every branch occurs."""
    s, frames = _OneMode(), 2400
    r = fh.Restatement(s, [1], dtype)
    t = np.arange(frames)
    u = (0.05 * (np.sin(2 * np.pi * t / 300.0) + 0.5)).astype(np.float32)[None, :]
    w = (0.02 * np.sin(2 * np.pi * t / 170.0)).astype(np.float32)[None, :]
    drive = (0.05 * np.sin(0.9 * t)).astype(np.float32)
    q, work, seen = None, 0.0, set()
    for blk in range(frames // 100):  # the anchor frame by frame: blocks of one frame would do; 100-frame blocks with a trace of the branch
        sl = slice(100 * blk, 100 * blk + 100)
        trace = {}
        _, f_n, f_t, _, status, anchor, _ = r.render_friction([(0, 1, (1.0, 0.5, 0.0), drive[sl])], [_junction(25.0, 0.4, 60.0, hertz)], u[:, sl], w[:, sl], 100, q, trace)
        assert status[0] == 1
        seen |= set(int(b) for b in trace["branch"][0])
        q = [anchor[0]]
    assert seen == {fh.O, fh.S, fh.P, fh.M}
    # the same run frame by frame, the anchor read after every frame
    r = fh.Restatement(s, [1], dtype)
    q, before = None, None
    for f in range(frames):
        _, f_n, f_t, _, _, anchor, counts = r.render_friction([(0, 1, (1.0, 0.5, 0.0), drive[f:f + 1])], [_junction(25.0, 0.4, 60.0, hertz)], u[:, f:f + 1], w[:, f:f + 1], 1, q)
        if before is not None and f_n[0, 0] > 0:
            moved = float(anchor[0]) - before
            if counts[0][0]:
                assert moved == 0  # a sticking frame leaves the slider
            else:
                assert float(f_t[0, 0]) * moved >= 0, (f, float(f_t[0, 0]), moved)
                work += float(f_t[0, 0]) * moved
        q, before = [anchor[0]], float(anchor[0])
    assert work > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@LAWS
def test_dead_friction_is_the_unflagged_junction(dtype, hertz):
    """kt = 0, mu = 0 and zero tangents in the working precisions: f_n, `out` and the state are the bits of the same junction without the
    flag.  f_t is 0 for kt = 0 and for mu = 0; with zero tangents it is 0 under a travel of 0 (under a lively one it is the rigid slider's
    force, which moves nothing: a_t = 0)."""
    s, frames = _OneMode(), 400
    t = np.arange(frames)
    u = (0.05 * (np.sin(2 * np.pi * t / 150.0) + 0.3)).astype(np.float32)[None, :]
    w = (0.02 * np.sin(2 * np.pi * t / 170.0) + 1e-4 * t).astype(np.float32)[None, :]
    rows = [(0, 1, (1.0, 0.5, 0.0), (0.3 * np.sin(0.9 * t)).astype(np.float32))]
    plain = fh.Restatement(s, [1], dtype)
    out0, f0, ft0, c0, st0, an0, _ = plain.render_friction(rows, [_junction(25.0, 0.4, 60.0, hertz, friction=False)], u, w, frames)
    assert st0[0] == 1 and (f0 > 0).any() and (f0 == 0).any() and (ft0 == 0).all() and np.isnan(an0[0])
    for name, junction, travel in (("kt = 0", _junction(25.0, 0.4, 0.0, hertz), w), ("mu = 0", _junction(25.0, 0.0, 60.0, hertz), w),
                                   ("zero tangents", _junction(25.0, 0.4, 60.0, hertz, tangent=(0.0, 0.0, 0.0)), w),
                                   ("zero tangents, no travel", _junction(25.0, 0.4, 60.0, hertz, tangent=(0.0, 0.0, 0.0)), np.zeros_like(w))):
        r = fh.Restatement(s, [1], dtype)
        out, f_n, f_t, c, st, an, _ = r.render_friction(rows, [junction], u, travel, frames)
        assert st[0] == 1 and c[0] == c0[0] and np.isfinite(an[0]), name
        assert np.array_equal(f_n, f0) and np.array_equal(out, out0), name
        assert np.array_equal(r.z[0][0], plain.z[0][0]) and np.array_equal(r.z[0][1], plain.z[0][1]), name
        if name != "zero tangents":
            assert (f_t == 0).all(), name
        else:
            assert (np.abs(f_t) <= dtype(np.float32(0.4)) * f_n).all() and (f_t != 0).any(), name


# ---- 5. left out and refused ----
def test_every_refused_kind():
    """constants() is the header's status: beyond the normal law's own conditions, a C_tt, C_nt or C_tn that is not finite, C_tt < 0, a den
    that is not a finite number above 0, C_P or C_M below 0 (mu |C_nt| > C_nn) or not finite, a K C_b that is not finite."""
    T = np.float32
    ok = dict(c_nn=2.0, c_nt=0.5, c_tn=0.5, c_tt=1.0, k=3.0, mu=0.5, kt=4.0)
    solved = lambda hertz=False, **kw: bool(fh.constants(T=T, hertz=hertz, **{**ok, **kw})["solved"])
    assert solved() and solved(True) and solved(mu=4.0) and solved(c_nt=-0.5, c_tn=-0.5)  # (mu |C_nt| = C_nn is inside)
    for bad in (np.inf, -np.inf, np.nan):
        for name in ("c_tt", "c_nt", "c_tn"):
            assert not solved(**{name: bad}) and not solved(True, **{name: bad}), (name, bad)
    assert not solved(c_tt=-1e-3)
    assert not solved(c_tt=3e38, kt=3e38) and not solved(kt=np.inf)  # den overflows
    assert not solved(mu=4.01) and not solved(mu=4.01, c_nt=-0.5) and not solved(True, mu=4.01)  # the cone condition, either sign of C_nt
    assert not solved(k=3e38) and not solved(True, k=3e38)  # K C_b overflows
    assert not solved(c_nn=-2.0, c_nt=0.0, c_tn=0.0, k=1.0) and not solved(True, c_nn=-1e-3, c_nt=0.0, c_tn=0.0)  # the normal law's own: 1 + K C <= 0; Hertz: C < 0
    assert not solved(c_nn=np.nan) and not solved(True, c_nn=np.inf)


def test_every_left_out_kind_of_the_restatement():
    """What the render leaves out (status 0, zero rows, a NaN anchor, zero counts): a tangent component, mu or kt that is not finite, mu < 0,
    kt < 0, and the flag on a bilateral junction.  (The device entries' decisions, with the damped and the shared flag, are held against
    this by tests/test_bank_friction_gpu.py.)"""
    s, frames = _OneMode(), 8
    u, w = np.full((1, frames), 0.375, np.float32), np.full((1, frames), 0.01, np.float32)
    good = _junction(25.0, 0.4, 60.0)
    assert fh.left_out(good) is False
    kinds = [_junction(25.0, bad, 60.0) for bad in (-0.1, np.inf, np.nan)] + [_junction(25.0, 0.4, bad) for bad in (-0.1, np.inf, np.nan)] + \
            [_junction(25.0, 0.4, 60.0, tangent=(1.0, bad, 0.0)) for bad in (np.inf, np.nan)] + [good[:3] + (True,) + good[4:]]
    for junction in kinds:
        assert fh.left_out(junction)
        out, f_n, f_t, c, st, an, counts = fh.Restatement(s, [1], np.float64).render_friction([], [junction], u, w, frames, [0.0])
        assert st[0] == 0 and c[0] == 0 and (f_n == 0).all() and (f_t == 0).all() and np.isnan(an[0]) and (counts == 0).all() and (out == 0).all()
