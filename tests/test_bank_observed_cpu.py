"""CPU-side checks of the pickups on junction objects (include/modalhip.h, "Pickups on junction objects"): every layer declares and exports
the entry; and in the restatement the GPU tests trust (tests/observed_harness.py), with advance-1 pickups at a junction's own sides,

    sum_sides read1[s] = d[s] + C f[s]                         (a group: d_i[s] + sum_j C_ij f_j[s]),
    f[s] = K phi(u[s] - sum_sides read1[s]) x damping factor   for the linear, the Hertz and the damped laws and for a group of three,
    a damped junction's carry = u - sum_sides read1 of the last frame,

each in numpy.longdouble, float64 and float32, to a bound that is derived below from the mode count and the format's eps.  The scenes are
those of the GPU tests' runs against longdouble (observed_harness.against_plan), built from the columns of the bank under construction,
which needs no device; the share of frames in contact that the GPU test asserts is held here on the longdouble restatement alone.

The bound.  Let n be the modes of the junction's sides, u = eps / 2 the unit roundoff, and
    S[s] = sum_sides sum_k |g_im[k] Im z[s][k]| + |g_re[k] Re z[s][k]|  +  2 sum_j sum_k |g_re[k] a_j[k] f_j[s]|
(an upper bound of the absolute terms on either side: |Re z~| <= |Re z| + |a f|).  In exact arithmetic on the rounded gains and states the
first identity holds term by term, Re z = Re z~ + sum_j a_j f_j.  What separates the two sides is rounding:
    read1:  the contract's order is 2 n fused multiply-adds in 2 x (n / 64) chains plus the adds of the partial rows: at most
            gamma(2 n + 8) S, gamma(m) = m u / (1 - m u)  (Higham, Accuracy and Stability, section 3.1: any order of summation);
    Re z:   one product and one add per member on the object, weighted by |g_re|: at most 2 GROUP u S;
    d:      three roundings per term and n sequential adds: gamma(n + 3) S;
    C f:    n products and adds, then the product with f: gamma(n + 2) S.
Together (4 n + 13 + 2 GROUP) u S (1 + O(n u)); asserted with eps = 2 u in place of u -- E[s] = (4 n + 13 + 2 GROUP) eps S[s] -- which
leaves a factor 2 for the second-order terms and for the near-fused multiply-add of the float64 restatement.
The law: with y' = u - sum read1 formed exactly from the rounded numbers, the solve's own y is y' up to E[s] + 2 eps (|u| + |d|) (the
rounding of x = u - d and of d), and the law K phi(y) m(y, y_p), m = max(1 + l (y - y_p), 0), is Lipschitz in y with
Lip = K (phi'(y) (1 + l (|y| + |y_p|)) + 2 l phi(y)) and in y_p with K l phi(y) <= Lip; the solves themselves leave
SOLVE eps K phi(y) (1 + l (|y| + |y_p|)) (tests/test_bank_damped_cpu.py: 7 for the closed form, 6 for Newton; 16 is asserted), a group's
elimination SOLVE eps (1 + sum_j K |C_ij|) max_j |f_j| (its backward error; tests/test_bank_groups_cpu.py measures 13 eps of max |f|):
    |f[s] - law(y'[s], y'[s-1])| <= Lip[s] (E[s] + E[s-1] + 2 eps (|u| + |d|)) + the solve's term + 2 eps |f[s]|.
The carry: the root y the solve left against y' of the last frame: E + 2 eps (|u| + |d|) + SOLVE eps (|x| + C |f|)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import damped_harness as dd
from tests import group_harness as gh
from tests import observed_harness as oh
from tests.test_abi_cpu import _exported_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble
SOLVE = 16.0
FORMATS = pytest.mark.parametrize("T", [np.longdouble, np.float64, np.float32], ids=["longdouble", "float64", "float32"])


def test_every_layer_declares_and_exports_the_observed_entry():
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    assert re.search(r"int\s+mh_bank_render_observed\s*\(", header)
    assert 0 < header.index("Contact damping, flags & MH_JUNCTION_DAMPED") < header.index("Pickups on junction objects, mh_bank_render_observed")
    assert "pickups on junction objects" in header  # the older entries' "Not in this version" item stays, and points here
    from mesheditor_amd import _lib, bank
    _lib.build()
    core = _lib.lib()
    assert "mh_bank_render_observed" in _exported_functions(_lib.SO_PATH, "mh_") and "mh_bank_render_observed" in core._declared
    assert core.mh_bank_render_observed.argtypes == core.mh_bank_render_damped.argtypes and core.mh_bank_render_observed.restype == core.mh_bank_render_damped.restype
    assert "mhx_render_observed" in _exported_functions(bank.SO_PATH, "mhx_")
    assert bank.lib().mhx_render_observed.argtypes == bank.lib().mhx_render_damped.argtypes
    assert hasattr(bank.Scene, "render_observed")
    # the records the entry takes are the ones the older entries take
    assert core.mh_pickup_struct_size() == C.sizeof(_lib.Pickup) == C.sizeof(bank.Pickup) == 48
    assert core.mh_junction_struct_size() == C.sizeof(_lib.Junction) == C.sizeof(bank.Junction) == 96
    mirror = open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "bank.hpp")).read()
    assert len(re.findall(r"void RenderModalObserved\(ModalAudio(?:64)? &", mirror)) == 2
    assert "is left out in this version" in mirror  # still true of the older entries
    assert '#include "../modal/bank.hpp"' in open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "audio", "ModalAudio.h")).read()


def test_the_contract_order_is_the_plain_sum_and_cuts_at_64_modes():
    """contract_sum on numbers whose sums are exact in float32 (small integers) is the plain sum; and the order is visible where it is not:
    one large term in the first half is added to the second half's sum last, not first."""
    rng = np.random.default_rng(7)
    n, frames = 130, 5
    g_im, g_re = (rng.integers(-8, 9, n).astype(np.float32) for _ in range(2))
    z_im, z_re = (rng.integers(-8, 9, (frames, n)).astype(np.float32) for _ in range(2))
    assert np.array_equal(oh.contract_sum(g_im, g_re, z_im, z_re, np.float32), (g_im * z_im + g_re * z_re).sum(axis=1))
    g, z = np.ones(128, np.float32), np.full((1, 128), np.float32(2.0 ** -24))
    z[0, 0] = 1.0  # mode 0: the even accumulator of the first half starts at 1 and absorbs none of its 31 further tiny terms
    got = oh.contract_sum(g, np.zeros_like(g), z, np.zeros_like(z), np.float32)[0]
    odd, second = np.float32(32 * 2.0 ** -24), np.float32(64 * 2.0 ** -24)
    assert got == (np.float32(1.0) + odd) + second and got != np.float32(1.0)


@pytest.fixture(scope="module")
def columns():
    return {False: oh.HostColumns(oh.MODES, oh.T60, False), True: oh.HostColumns(oh.MODES, oh.T60, True)}


def _compliances(cols, kind):
    scout = (oh.Damped if kind == "lone" else oh.Grouped)(cols, oh.MODES, np.float64, cols.dtype)
    specs = oh.lone_specs([0.0, 0.0]) if kind == "lone" else oh.group_specs([0.0] * 3)
    return [float(scout.compliance(s[:4])) for s in specs]


def _run(cols, T, kind, damped, frames, kc=10.0, lx0=1.0):
    """One block of against_plan's scene in format T with advance-1 pickups at every side.  Returns a dict of longdouble arrays:
    u, d, f [junction][frames], R = sum_sides read1, Cm (the compliance matrix; diagonal for lone junctions), E (the bound of the first
    identity), K, l, hertz per junction, and the returned carry."""
    comp = _compliances(cols, kind)
    specs, _, rows, u = oh.against_plan(cols, kind, kc, comp, frames, 1)
    n = len(specs)
    lam = [0.0] * n
    if damped:
        specs = oh.lone_specs([s[2] for s in specs], damped=(True, True))
        lam = [np.float32(lx0 / float(x)) for x in u.max(axis=1)]
    rest = (oh.Damped if kind == "lone" else oh.Grouped)(cols, oh.MODES, T, cols.dtype)
    sides = oh.side_pickups(specs)
    pickups = [p for _, p in sides]
    trace, carry = {}, None
    if kind == "lone":
        (_, forces, _, status, carry), reads = rest.observed(rest.render_damped, pickups, rows[0], specs, u, lam, None, frames, trace)
        Cm = np.diag([L(rest.compliance(s[:4])) for s in specs])
    else:
        (_, forces, _, status), reads = rest.observed(rest.render_grouped, pickups, rows[0], specs, u, frames, trace)
        Cm = np.asarray(rest.compliance_matrix(specs), L)
    assert (np.asarray(status) == 1).all() and reads.dtype == T and forces.dtype == T
    f, d = np.asarray(forces, L), np.asarray(trace["d"], L)
    R = np.zeros((n, frames), L)
    for (j, _), row in zip(sides, reads):
        R[j] += np.asarray(row, L)
    # S and E of the module's derivation
    eps = L(np.finfo(T).eps)
    gains = [{sd[0]: rest.side_gains(sd) for sd in (s[0], s[1]) if sd is not None} for s in specs]
    E = np.zeros((n, frames), L)
    for j in range(n):
        S, modes = np.zeros(frames, L), 0
        for o, (_, g_im, g_re) in gains[j].items():
            z_re, z_im = (np.array([st[c] for st in rest.trajectory[o]], L) for c in (0, 1))
            S += (np.abs(np.asarray(g_im, L))[None, :] * np.abs(z_im) + np.abs(np.asarray(g_re, L))[None, :] * np.abs(z_re)).sum(axis=1)
            for i in range(n):
                if o in gains[i]:
                    S += 2 * np.abs(np.asarray(g_re, L) * np.asarray(gains[i][o][0], L)).sum() * np.abs(f[i])
            modes += len(g_im)
        E[j] = (4 * modes + 13 + 2 * gh.GROUP) * eps * S
    return {"u": np.asarray(u, L), "d": d, "f": f, "R": R, "Cm": Cm, "E": E, "eps": eps, "K": [L(np.float32(s[2])) for s in specs], "l": [L(v) for v in lam],
            "hertz": [bool(s[4]) for s in specs], "carry": carry, "kind": kind, "damped": damped}


SCENES = pytest.mark.parametrize("kind,damped", [("lone", False), ("lone", True), ("group", False)], ids=["linear-and-hertz", "damped", "group-of-three"])
FRAMES = 333  # two and a half tiles of the kernels; every scene makes and breaks within it


@FORMATS
@SCENES
def test_the_sides_advance_1_reads_are_the_prediction_moved_by_the_force(columns, T, kind, damped):
    r = _run(columns[T == np.float64], T, kind, damped, FRAMES)
    moved = r["d"] + r["Cm"] @ r["f"]
    miss = np.abs(r["R"] - moved)
    assert (np.abs(r["f"]).max(axis=1) > 0).all() and ((r["f"] == 0).mean(axis=1) > 0.05).all()  # every junction makes and breaks
    assert (np.abs(r["Cm"] @ r["f"]).max(axis=1) > 100 * r["E"].max(axis=1)).all()  # and the force's part is far above the bound: the identity says something
    print("sum read1 against d + C f, %s, %s%s: largest miss / bound %.3f" % (T.__name__, kind, ", damped" if damped else "", float((miss / r["E"]).max())))
    assert (miss <= r["E"]).all(), float((miss / r["E"]).max())


def _law_bound(r, j, y, yp, l):
    """The bound of |f - law(y', y_p')| of junction j frame by frame (module docstring)."""
    K, eps, hertz = r["K"][j], r["eps"], r["hertz"][j]
    E = r["E"][j]
    before = np.concatenate([[L(0)], E[:-1]]) if r["damped"] else np.zeros_like(E)
    reach = np.maximum(y, 0) + E
    phi, slope = (reach * np.sqrt(reach), L(1.5) * np.sqrt(reach)) if hertz else (reach, np.ones_like(reach))
    factor = 1 + l * (np.abs(y) + np.abs(yp))
    lip = K * (slope * factor + 2 * l * phi)
    rounding = 2 * eps * (np.abs(r["u"][j]) + np.abs(r["d"][j]))
    if r["kind"] == "group":
        solve = SOLVE * eps * (1 + (np.array(r["K"], L)[j] * np.abs(r["Cm"][j])).sum()) * np.abs(r["f"]).max(axis=0)
    else:
        solve = SOLVE * eps * K * phi * factor
    return lip * (E + before + rounding) + solve + 2 * eps * np.abs(r["f"][j])


@FORMATS
@SCENES
def test_the_force_is_the_law_at_the_compression_the_sides_read(columns, T, kind, damped):
    r = _run(columns[T == np.float64], T, kind, damped, FRAMES)
    y = r["u"] - r["R"]
    worst = peak = 0.0
    for j in range(len(r["K"])):
        yp = np.concatenate([[L(0)], y[j][:-1]])
        l = np.concatenate([[L(0)], np.full(FRAMES - 1, r["l"][j])])  # the block's first frame has no history
        want = oh.law(y[j], yp, l, r["K"][j], r["hertz"][j])
        bound = _law_bound(r, j, y[j], yp, l)
        miss = np.abs(r["f"][j] - want)
        # the bound is below the force it speaks about: by 10 x at the least (float32, K C = 10: y' is the difference of numbers S / (C f), about
        # 15, times its size, over some 170 modes, and K C multiplies what is left), by 1e9 x in float64
        assert np.abs(want).max() > 10 * bound.max(), j
        worst = max(worst, float((miss / bound).max()))
        peak = max(peak, float(miss.max() / np.abs(want).max()))
        assert (miss <= bound).all(), (j, float((miss / bound).max()))
    print("f against the law at u - sum read1, %s, %s%s: largest miss / bound %.3f, largest miss / the row's peak %.2e" %
          (T.__name__, kind, ", damped" if damped else "", worst, peak))


@FORMATS
def test_a_damped_junctions_carry_is_the_last_frames_compression(columns, T):
    r = _run(columns[T == np.float64], T, "lone", True, FRAMES)
    y = r["u"] - r["R"]
    for j in range(2):
        x = r["u"][j][-1] - r["d"][j][-1]
        bound = r["E"][j][-1] + 2 * r["eps"] * (abs(r["u"][j][-1]) + abs(r["d"][j][-1])) + SOLVE * r["eps"] * (abs(x) + r["Cm"][j, j] * abs(r["f"][j][-1]))
        miss = abs(L(r["carry"][j]) - y[j][-1])
        assert np.isfinite(r["carry"][j]) and abs(y[j][-1]) > 1e3 * bound
        assert miss <= bound, (j, float(miss / bound))


@pytest.mark.parametrize("frames", [512, 333])
def test_the_runs_against_longdouble_are_in_contact_for_15_to_85_percent(columns, frames):
    """The scenes of tests/test_bank_observed_gpu.py's test 6 (K C = 1 and 100, two blocks) on the longdouble restatement alone, K from
    the float64 restatement's C (the GPU test takes the device's): every junction is in contact -- f > 0 -- for between 15 % and 85 % of
    the frames, and every pickup row sounds."""
    cols = columns[False]
    for kind in ("lone", "group"):
        comp = _compliances(cols, kind)
        for kc in (1.0, 100.0):
            specs, pickups, rows, u = oh.against_plan(cols, kind, kc, comp, frames, 2)
            exact = (oh.Damped if kind == "lone" else oh.Grouped)(cols, oh.MODES, L, cols.dtype)
            closed = []
            for b in range(2):
                _, forces, reads = oh.against_run(exact, kind, specs, pickups, rows[b], u[:, b * frames:(b + 1) * frames], frames)
                closed.append((np.asarray(forces) > 0).mean(axis=1))
                assert (np.abs(reads).max(axis=1) > 0).all()
            share = np.mean(closed, axis=0)
            print("%s, K C = %g, %d frames: in contact %s" % (kind, kc, frames, " ".join("%.2f" % c for c in share)))
            assert ((share >= 0.15) & (share <= 0.85)).all(), (kind, kc, share)
