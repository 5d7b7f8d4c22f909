"""The single-precision smoothers' stores that no later kernel reads (Precond<float>::cheb): after a zero start r is the
right-hand side and x is d, so the start pass stores neither and the first fused step reads b and d; the last step of a sequence that
hands nothing on stores neither r nor d'; the restriction writes its float copy itself.  No arithmetic changed, so no bit of any result
may change.  MH_TEST=smoother_stores brings every one of those stores, and the conversion launch, back.

MH_TEST and MH_CYCLE are read once per process, so every arm of every cycle shape is one child process; the arms of a test run side by
side.  Three things are compared for equality: the cycle alone, with and without the stores (1); the cycle alone with fresh arrays
started as NaN (MH_TEST=poison) and without -- a dropped store that something still read would show as a NaN or a changed bit (2);
whole solves, cold and warm, with and without the stores (3)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mesheditor_amd import meshes
from tests import test_copy_passes_gpu as cp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAT = meshes.MATERIALS["Ceramic"]


def _flat_uv_sphere():
    """A 32 x 16 UV sphere's fill with 60 interior points moved to 1e-6 of a face (tests/test_preconditioner_gpu.py, restated): flat cells,
    hence clusters on both smoothed levels -- the path this change leaves alone."""
    from mesheditor_amd import tets as fe
    v, f = meshes.uv_sphere_surface(0.15, 32, 16)
    p, t, left = fe.tetrahedralize(v, f)
    assert left == 0
    fp, made = meshes.with_flat_cells(p, t, len(v), count=60, eps=1e-6, seed=32)
    assert made == 60
    return fp, t


# name -> (mesh, has patches or clusters)
CYCLE_MESHES = {
    "cube4": (lambda: meshes.kuhn_box(4, 4, 4, 0.1, 0.1, 0.1), False),
    "plate2": (lambda: meshes.kuhn_box(6, 6, 2, 0.15, 0.15, 0.05), False),  # two cells thick: the surface-dominated bodies' shape
    "flat60": (_flat_uv_sphere, True),
}
WIDTHS = (1, 3, 4, 5, 80)  # pad columns of the 4-float pitch: 3, 1, 0, 3, 0
# MH_CYCLE = P2 degree, P1 degree, P1 cycles.  Per sequence of degree d: 1 = no step at all (the start pass keeps storing x), 2 = the
# first step is also the last, 3 and 12 = a first step that is not the last and a last that is not the first; three P1 cycles: the
# second P1 sequence of each cycle, and the first of cycles two and three, do not start from zero.
CYCLES = tuple("%d,%d,%d" % (d2, d1, g) for d2 in (1, 2, 3) for d1 in (1, 2, 12) for g in (1, 3))


def _panel(n, w):
    return np.asfortranarray(np.random.default_rng(1000 + w).standard_normal((n, w)))


def cycle_outputs(inputs):
    """Child side: B X in single precision for every mesh and width, "<mesh>.<w>" -> panel, and "<mesh>.patches" -> has any."""
    from mesheditor_amd import api
    from tools import lab
    ctx = api.Context(0)
    out = {}
    for name in CYCLE_MESHES:
        mesh = api.Mesh(ctx, inputs[name + ".pts"], inputs[name + ".tets"])
        s = api.System(ctx, mesh, api.material(*MAT))
        h = lab.hierarchy(s, lab.SIGMA, width=64)
        out[name + ".patches"] = np.asarray([len(h["patches%d" % lv]["nodes"]) + len(h["patches%d" % lv]["clusters"]) for lv in (2, 1)])
        for w in WIDTHS:
            out["%s.%d" % (name, w)] = lab.precondition(s, _panel(s.n, w), 0)
    ctx.close()
    return out


def solve_outputs(inputs):
    """Child side: the whole-solve cases, "<case>.<solve>.<field>" -> array (restarts = iterations among the fields)."""
    from mesheditor_amd import api
    ctx = api.Context(0)
    out = {}
    for name, (cfg, kind) in SOLVES.items():
        for k, v in cp._run_case(api, ctx, inputs[name + ".pts"], inputs[name + ".tets"], cfg, kind).items():
            out[name + "." + k] = v
    ctx.close()
    return out


_CFG = dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6)
SOLVE_MESHES = {"cube_small": cp._cube, "sliver_plate": cp._sliver_plate, "flat_sphere": cp._flat_sphere}
# case -> (solver configuration, "cold" = one cold solve, "warm" = a cold solve, then two materials seeded with its basis)
SOLVES = {"cube_small": (_CFG, "warm"), "sliver_plate": (_CFG, "warm"), "flat_sphere": (_CFG, "warm")}

_CHILD = """
import sys
import numpy as np
from tests import test_smoother_stores_gpu as t
np.savez(sys.argv[3], **getattr(t, sys.argv[1])(np.load(sys.argv[2])))
"""


def _run_arms(what, given, out_dir, arms, cycle=None):
    """One child per arm (name -> MH_TEST value or None), all at once; name -> the arrays it saved."""
    procs = {}
    for arm, mh_test in arms.items():
        env = {k: v for k, v in os.environ.items() if k not in ("MH_TEST", "MH_CYCLE", "MH_PRECOND_FP64")}
        env["PYTHONPATH"] = ROOT
        if mh_test:
            env["MH_TEST"] = mh_test
        if cycle:
            env["MH_CYCLE"] = cycle
        path = os.path.join(out_dir, "%s_%s_%s.npz" % (what, arm, (cycle or "own").replace(",", "_")))
        procs[arm] = (subprocess.Popen([sys.executable, "-c", _CHILD, what, given, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=ROOT), path)
    got = {}
    for arm, (p, path) in procs.items():
        try:
            text, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q, _ in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, (arm, text[-2000:])
        got[arm] = dict(np.load(path))
    return got


@pytest.fixture(scope="module")
def cycle_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("smoother_stores_cycle")
    given = str(d / "inputs.npz")
    np.savez(given, **{name + "." + k: v for name, (make, _) in CYCLE_MESHES.items() for k, v in zip(("pts", "tets"), make())})
    return given, str(d)


@pytest.fixture(scope="module")
def cycle_arms(cycle_inputs):
    """cycle -> {"lean": default, "stores": MH_TEST=smoother_stores, "poison": MH_TEST=poison}, each run once for both cycle tests."""
    cache = {}

    def get(cycle):
        if cycle not in cache:
            cache[cycle] = _run_arms("cycle_outputs", cycle_inputs[0], cycle_inputs[1], {"lean": None, "stores": "smoother_stores", "poison": "poison"}, cycle)
        return cache[cycle]
    return get


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k, v in a.items():
        assert b[k].shape == v.shape and b[k].dtype == v.dtype and v.tobytes() == b[k].tobytes(), (what, k)  # (the bytes: -0.0 is not 0.0 here)


def _check_cycle_arm(rec):
    for name, (_, patched) in CYCLE_MESHES.items():
        assert bool(rec[name + ".patches"].sum()) == patched, (name, rec[name + ".patches"])  # (the mesh still is what it was chosen for)
        for w in WIDTHS:
            y = rec["%s.%d" % (name, w)]
            assert y.shape[1] == w and np.isfinite(y).all() and np.abs(y).max() > 0, (name, w)


@pytest.mark.parametrize("cycle", CYCLES)
def test_the_cycle_is_the_same_bit_for_bit_with_and_without_the_stores(cycle_arms, cycle):
    arms = cycle_arms(cycle)
    _check_cycle_arm(arms["lean"])
    _same(arms["lean"], arms["stores"], cycle)


@pytest.mark.parametrize("cycle", CYCLES)
def test_nothing_reads_a_store_that_was_dropped(cycle_arms, cycle):
    """With every fresh array started as NaN the default arm gives the same finite panels: no kernel reads a panel nobody wrote."""
    arms = cycle_arms(cycle)
    _check_cycle_arm(arms["poison"])
    _same(arms["lean"], arms["poison"], cycle)


def test_whole_solves_are_the_same_bit_for_bit_with_and_without_the_stores(tmp_path):
    given = str(tmp_path / "inputs.npz")
    np.savez(given, **{name + "." + k: v for name, make in SOLVE_MESHES.items() for k, v in zip(("pts", "tets"), make())})
    arms = _run_arms("solve_outputs", given, str(tmp_path), {"lean": None, "stores": "smoother_stores"})
    lean = arms["lean"]
    for name in SOLVES:
        for i in range(3):
            assert len(lean["%s.%d.freqs" % (name, i)]) > 0 and len(lean["%s.%d.eigenvalues" % (name, i)]) > 0, (name, i)  # (solved, not two empty results)
    assert lean["cube_small.1.restarts"] < lean["cube_small.0.restarts"]  # (the seeded solve did start from its basis)
    _same(lean, arms["stores"], "solves")  # every field, the iteration counts (restarts) among them
