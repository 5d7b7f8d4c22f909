"""The block iteration's tall copy passes: the scatter of the new Ritz vectors into the basis, the gather of the residuals in front of the
preconditioner, the start block's panel copy, image transform and full random fill, the conversion of the shifted operator's values.  None
of them computed anything, so taking them out may change no bit of any result.  MH_TEST=copy_passes runs every one of them again: each
case below is solved in both arms -- here, and by one child process with the hook set -- and every field is compared for equality.  The
basis update's two-destination form is also called directly and compared with the one-destination form."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mesheditor_amd import meshes
from tools import lab

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.RESULT_FIELDS, restated: api.ModalResult minus profile (timings) and basis
RESULT_FIELDS = ("eigenvalues", "freqs", "t60s", "shapes", "positions", "summary_shapes", "original_fundamental", "mass", "center_of_mass",
                 "inertia_diagonal", "inertia_orientation_wxyz", "sample_point_of_excitation")
MAT_A, MAT_B = meshes.MATERIALS["Ceramic"], meshes.MATERIALS["Glass"]


def _sliver_plate():
    """A Kuhn box of three layers whose middle layer is a hundredth of a cell thick (tests/test_mesh_structure_gpu.py, restated): its 96
    tetrahedra have a shape measure of about 0.011, under the 0.02 of the smoothers' patch selection."""
    pts, tets = meshes.kuhn_box(4, 4, 3, 0.1, 0.1, 0.075)
    z = np.array([0.0, 0.025, 0.02525, 0.05025])
    pts[:, 2] = z[np.rint(pts[:, 2] / 0.025).astype(int)]
    return pts, tets


def _flat_sphere():
    """A small UV sphere's fill with ten interior points moved almost into a face of one of their tetrahedra (as
    test_a_callers_mesh_with_flat_cells_still_comes_back builds its spheres): the solve starts with double-precision smoothers."""
    from mesheditor_amd import tets as front_end
    P, F = meshes.uv_sphere_surface(0.15, 24, 12)
    good_p, good_t, left = front_end.tetrahedralize(P, F)
    assert left == 0
    flat_p, made = meshes.with_flat_cells(good_p, good_t, len(P), count=10, eps=1e-6, seed=24)
    assert made == 10
    return flat_p, good_t


def _cube():
    return meshes.workload("cube_small")[:2]


# name -> (mesh, solver configuration, what is solved: "cold" = one cold solve; "warm" = a cold solve, then MAT_A and MAT_B seeded with its basis)
CASES = {
    "cube_small_30": (_cube, dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6), "cold"),
    "cube_small_29": (_cube, dict(num_modes=20, num_fem_modes=29, max_mode_freq=1e6), "cold"),
    "cube_small_27": (_cube, dict(num_modes=20, num_fem_modes=27, max_mode_freq=1e6), "cold"),
    "bar_thin": (lambda: meshes.workload("bar_thin")[:2], dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6), "cold"),
    "cube_small_warm": (_cube, dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6), "warm"),
    "sliver_plate": (_sliver_plate, dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6), "cold"),
    "flat_sphere": (_flat_sphere, dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6), "cold"),
    "cube_small_wide": (_cube, dict(num_modes=120, num_fem_modes=135, max_mode_freq=1e6), "cold"),
}


def _record(r):
    out = {k: np.asarray(getattr(r, k)) for k in RESULT_FIELDS}
    out["restarts"] = np.asarray(r.profile["restarts"])
    return out


def _run_case(api, ctx, pts, tets, cfg, kind):
    """The case's solves as one flat dict "<solve>.<field>" -> array."""
    ex = pts[::13].astype(np.float32)
    config = api.default_config(**cfg)
    cold = api.mesh2modes(ctx, pts, tets, api.material(*MAT_A), ex, config=config, keep_basis=kind == "warm")
    solves = [cold]
    if kind == "warm":
        solves += [api.mesh2modes(ctx, pts, tets, api.material(*m), ex, config=config, seed_basis=cold.basis) for m in (MAT_A, MAT_B)]
    return {"%d.%s" % (i, k): v for i, r in enumerate(solves) for k, v in _record(r).items()}


_HOOK_CHILD = """
import sys
import numpy as np
from mesheditor_amd import api
from tests import test_copy_passes_gpu as t
inputs = np.load(sys.argv[1])
ctx = api.Context(0)
out = {}
for name, (_, cfg, kind) in t.CASES.items():
    for k, v in t._run_case(api, ctx, inputs[name + ".pts"], inputs[name + ".tets"], cfg, kind).items():
        out[name + "." + k] = v
np.savez(sys.argv[2], **out)
ctx.close()
"""


@pytest.fixture(scope="module")
def api():
    from mesheditor_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs():
    return {name: make() for name, (make, _, _) in CASES.items()}


@pytest.fixture(scope="module")
def hook_arm(inputs, tmp_path_factory):
    """Every case solved by one child process under MH_TEST=copy_passes, on the very arrays this process solves."""
    d = tmp_path_factory.mktemp("copy_passes")
    given, path = str(d / "inputs.npz"), str(d / "hook.npz")
    np.savez(given, **{name + "." + k: v for name, (pts, tets) in inputs.items() for k, v in (("pts", pts), ("tets", tets))})
    env = dict(os.environ, PYTHONPATH=ROOT, MH_TEST="copy_passes")
    p = subprocess.run([sys.executable, "-c", _HOOK_CHILD, given, path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_are_the_same_bit_for_bit_with_and_without_the_copy_passes(api, ctx, inputs, hook_arm, name):
    _, cfg, kind = CASES[name]
    pts, tets = inputs[name]
    rec = _run_case(api, ctx, pts, tets, cfg, kind)
    for i in range(3 if kind == "warm" else 1):
        assert len(rec["%d.freqs" % i]) > 0 and len(rec["%d.eigenvalues" % i]) > 0, (name, i)  # (solved, not two empty results)
    if kind == "warm":
        assert rec["1.restarts"] < rec["0.restarts"]  # (the seeded solve did start from its basis)
    assert sorted(k for k in hook_arm.files if k.startswith(name + ".")) == sorted(name + "." + k for k in rec)
    for k, v in rec.items():
        got = hook_arm[name + "." + k]
        assert got.shape == v.shape and np.array_equal(got, v), (name, k)


@pytest.mark.parametrize("n, wa, gaps", [(200, 5, True), (200, 5, False), (200, 16, True), (200, 16, False), (64 * 4096 + 8, 16, True)])
def test_both_destinations_of_the_basis_update_equal_the_single_store_scattered(ctx, n, wa, gaps):
    """n = 200 rows (four row tiles, the last of 8 rows), a basis of up to 3 x 16 columns (37 columns: a K tail; 48: whole chunks), the
    active columns of X through a map with gaps or through the identity; and once 262 152 rows, where the update's persistent workgroups
    (at most 8 per compute unit) take two or three row tiles each -- X is written in the launch that reads it, and a tile's stores must
    not reach rows another tile still has to read.  The lab library's check (kinds 2 and 3 of its dense bench entry) runs the update in
    both forms on the same inputs and counts, on the host, the entries that differ from what the one-destination form's compact panel,
    scattered into X, requires: X after the two-destination form (columns outside the map keep their values), that form's compact panel
    and second output -- and the one-destination form against the product formed on the host."""
    assert lab.mapped_update_mismatches(ctx, n, wa, 16, gaps) == 0
