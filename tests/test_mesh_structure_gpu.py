"""The mesh structure: what mh_assemble derives from the points and tets alone is built on the first assembly on a resident mesh and
kept with it; later assemblies form K and M on it.  Reuse must be invisible in every result -- equality here is bit equality -- and
visible only in the counter (api.Mesh.structure_stats).  MH_TEST=fresh_structure rebuilds the structure on every assembly (and takes
the start block's bounding box from the device again), which is what every assembly did before the structure was kept."""
import gc
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
CFG = dict(num_modes=20, num_fem_modes=30, max_mode_freq=1e6)


@pytest.fixture(scope="module")
def api():
    from mesheditor_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


def _cube_with_degenerate_tets():
    """cube_small with flat tets (four coplanar grid points each) put between its own: the kept tets' indices are not the given ones."""
    pts, tets, _, _ = meshes.workload("cube_small")
    flat = np.array([[0, 5, 25, 30], [1, 6, 26, 31], [2, 7, 27, 32]], np.uint32)  # points of the plane k = const: vid = (i * 5 + j) * 5 + k
    return pts, np.ascontiguousarray(np.vstack([tets[:5], flat[:1], tets[5:200], flat[1:], tets[200:], flat[:2]]), dtype=np.uint32)


def _two_boxes():
    p1, t1 = meshes.kuhn_box(3, 3, 3, 0.1, 0.08, 0.09)
    p2, t2 = meshes.kuhn_box(2, 3, 2, 0.05, 0.07, 0.06, origin=(0.5, 0.1, -0.2))
    return np.vstack([p1, p2]), np.ascontiguousarray(np.vstack([t1, t2 + len(p1)]), dtype=np.uint32)


def _far_cube():
    pts, tets, _, _ = meshes.workload("cube_small")
    return pts + np.array([1000.0, 0.0, 0.0]), tets  # 1 km from the origin: node coordinates relative to the bounding box's corner


def _sliver_plate():
    """A Kuhn box of three layers whose middle layer is a hundredth of a cell thick: its 96 tetrahedra have a shape measure of about
    0.011, under the 0.02 of the smoothers' patch selection."""
    pts, tets = meshes.kuhn_box(4, 4, 3, 0.1, 0.1, 0.075)
    z = np.array([0.0, 0.025, 0.02525, 0.05025])
    pts[:, 2] = z[np.rint(pts[:, 2] / 0.025).astype(int)]
    return pts, tets


MESHES = {
    "cube_small": lambda: meshes.workload("cube_small")[:2],
    "cube_with_degenerate_tets": _cube_with_degenerate_tets,
    "two_boxes": _two_boxes,
    "cube_1km_away": _far_cube,
}


def _record(r):
    out = {k: np.asarray(getattr(r, k)) for k in RESULT_FIELDS}
    out["restarts"] = np.asarray(r.profile["restarts"])
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _solve(api, ctx, pts, tets, m, mesh=None, **kw):
    ex = pts[::13].astype(np.float32)
    return api.mesh2modes(ctx, pts, tets, api.material(*m), ex, config=api.default_config(**CFG), mesh=mesh, **kw)


def _reused_and_fresh(api, ctx, pts, tets):
    """Records of A, B, A on one resident mesh and of A, B on fresh meshes; the shared mesh's build count."""
    mesh = api.Mesh(ctx, pts, tets)
    reused = [_record(_solve(api, ctx, pts, tets, m, mesh=mesh)) for m in (MAT_A, MAT_B, MAT_A)]
    builds, nbytes = mesh.structure_stats()
    mesh.close()
    fresh = [_record(_solve(api, ctx, pts, tets, m)) for m in (MAT_A, MAT_B)]
    return reused, fresh, builds, nbytes


@pytest.mark.parametrize("name", ["cube_small", "bar_thin"])
def test_reused_structure_gives_the_same_blocks(api, ctx, name):
    pts, tets, _, _ = meshes.workload(name)
    shared = api.Mesh(ctx, pts, tets)
    assert shared.structure_stats() == (0, 0)
    for m in (MAT_A, MAT_B, MAT_A):
        reused = api.System(ctx, shared, api.material(*m))
        fresh_mesh = api.Mesh(ctx, pts, tets)
        fresh = api.System(ctx, fresh_mesh, api.material(*m))
        for a, b in zip(reused.export_blocks(), fresh.export_blocks()):
            assert np.array_equal(a, b)
        assert np.array_equal(reused.element_nodes(), fresh.element_nodes())
        assert fresh_mesh.structure_stats()[0] == 1
        for h in (reused, fresh, fresh_mesh):
            h.close()
    builds, nbytes = shared.structure_stats()
    assert builds == 1 and nbytes > 0
    shared.close()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_reused_structure_gives_the_same_results(api, ctx, name):
    pts, tets = MESHES[name]()
    reused, fresh, builds, _ = _reused_and_fresh(api, ctx, pts, tets)
    assert builds == 1
    assert len(fresh[0]["freqs"]) > 0 and len(fresh[1]["freqs"]) > 0  # (solved, not two empty results)
    _same(reused[0], fresh[0])
    _same(reused[1], fresh[1])
    _same(reused[2], fresh[0])
    if name == "two_boxes":  # two free bodies: twelve rigid-body modes
        assert (np.abs(fresh[0]["eigenvalues"][:12]) < 1e-6 * fresh[0]["eigenvalues"][12]).all()


def test_reused_structure_gives_the_same_results_with_sliver_patches(api, ctx):
    pts, tets = _sliver_plate()
    probe = _solve(api, ctx, pts, tets, MAT_A, keep_system=True)
    h = lab.hierarchy(probe.system)
    probe.system.close()
    assert len(h["patches2"]["nodes"]) + len(h["patches2"]["clusters"]) > 0 and h["patches2"]["n_bad_elements"] > 0  # the precondition: the smoothers have patches
    reused, fresh, builds, _ = _reused_and_fresh(api, ctx, pts, tets)
    assert builds == 1
    assert len(fresh[0]["freqs"]) > 0 and len(fresh[1]["freqs"]) > 0
    _same(reused[0], fresh[0])
    _same(reused[1], fresh[1])
    _same(reused[2], fresh[0])


def test_a_kept_system_outlives_its_mesh_and_nothing_leaks(api, ctx):
    pts, tets, _, _ = meshes.workload("cube_small")
    nodes = np.arange(0, len(pts), 7, dtype=np.uint32)

    def live_bytes():
        gc.collect()
        reserved, idle, _ = lab.pool_stats(ctx)
        return reserved - idle

    _solve(api, ctx, pts, tets, MAT_A)  # (whatever the context allocates once, on its first solve, is there before the baseline is read)
    before = live_bytes()
    orphan = _solve(api, ctx, pts, tets, MAT_A, keep_system=True)  # no mesh passed: mesh2modes closes its own before it returns
    mesh = api.Mesh(ctx, pts, tets)
    living = _solve(api, ctx, pts, tets, MAT_A, mesh=mesh, keep_system=True)
    assert orphan.system is not None and living.system is not None
    assert np.array_equal(orphan.system.gather_shapes(nodes, 30), living.system.gather_shapes(nodes, 30))
    assert np.array_equal(orphan.system.basis(30), living.system.basis(30))
    assert live_bytes() > before
    mesh.close()  # the mesh first: its structure lives on with the system
    assert np.array_equal(orphan.system.basis(30), living.system.basis(30))
    living.system.close()
    orphan.system.close()
    assert live_bytes() == before


def test_failed_structure_builds_cache_nothing(api, ctx):
    pts, tets = meshes.kuhn_box(3, 2, 2, 0.3, 0.2, 0.2)
    extra = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]) + 5.0  # a flat tet on its own points
    pts2 = np.vstack([pts, extra])
    flat = np.array([[len(pts), len(pts) + 1, len(pts) + 2, len(pts) + 3]], dtype=np.uint32)
    mat = api.material(*MAT_B)
    for mesh, code in ((api.Mesh(ctx, pts2, flat), 6), (api.Mesh(ctx, np.zeros((0, 3)), np.zeros((0, 4), np.uint32)), 6)):  # every tet degenerate; empty mesh
        for _ in range(2):
            with pytest.raises(api.ModalHipError) as e:
                api.System(ctx, mesh, mat)
            assert e.value.code == code
            assert mesh.structure_stats() == (0, 0)
        mesh.close()
    for _ in range(2):  # out-of-range tet index: no mesh comes to be
        with pytest.raises(api.ModalHipError) as e:
            api.Mesh(ctx, pts, np.array([[0, 1, 2, 10 ** 6]], np.uint32))
        assert e.value.code == 1


_HOOK_CHILD = """
import sys
import numpy as np
from mesheditor_amd import api
from tests import test_mesh_structure_gpu as t
ctx = api.Context(0)
out = {}
for name in ("cube_small", "cube_1km_away"):
    pts, tets = t.MESHES[name]()
    mesh = api.Mesh(ctx, pts, tets)
    for i, m in enumerate((t.MAT_A, t.MAT_B, t.MAT_A)):
        for k, v in t._record(t._solve(api, ctx, pts, tets, m, mesh=mesh)).items():
            out["%s.%d.%s" % (name, i, k)] = v
    out[name + ".builds"] = np.asarray(mesh.structure_stats()[0])
    mesh.close()
np.savez(sys.argv[1], **out)
ctx.close()
"""


def test_fresh_structure_hook_rebuilds_every_time_with_the_same_results(api, ctx, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, MH_TEST="fresh_structure")
    path = str(tmp_path / "hook.npz")
    p = subprocess.run([sys.executable, "-c", _HOOK_CHILD, path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    hook = np.load(path)
    for name in ("cube_small", "cube_1km_away"):
        pts, tets = MESHES[name]()
        mesh = api.Mesh(ctx, pts, tets)
        for i, m in enumerate((MAT_A, MAT_B, MAT_A)):
            rec = _record(_solve(api, ctx, pts, tets, m, mesh=mesh))
            assert len(rec["freqs"]) > 0
            for k, v in rec.items():
                got = hook["%s.%d.%s" % (name, i, k)]
                assert got.shape == v.shape and np.array_equal(got, v), (name, i, k)
        assert mesh.structure_stats()[0] == 1 and int(hook[name + ".builds"]) == 3  # one assembly per solve
        mesh.close()
