"""CPU-side checks of the contact junctions: every layer declares and exports them, the bindings' mh_junction images have the library's
size, field order and offsets, and the restatement the GPU tests trust (tests/junction_harness.py) agrees with closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import junction_harness as jh
from tests.test_abi_cpu import _exported_functions
from tests.test_bank_pickups_cpu import _OneMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mh_bank_render_coupled", "mh_junction_struct_size"}


@pytest.fixture(scope="module")
def core():
    from mesheditor_amd import _lib
    _lib.build()
    return _lib


def test_header_declares_and_library_exports_the_junction_entries(core):
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert NEW | {"mh_bank_render_read", "mh_bank_render_driven", "mh_bank_render"} <= declared
    assert re.search(r"}\s*mh_junction_side\s*;", header) and re.search(r"}\s*mh_junction\s*;", header)
    assert re.search(r"#define\s+MH_NO_OBJECT\s+0xffffffffu", header) and re.search(r"#define\s+MH_JUNCTION_BILATERAL\s+1u", header)
    modes = re.search(r"#define\s+MH_JUNCTION_MODES\s+(\d+)", header)
    assert modes and int(modes.group(1)) == core.JUNCTION_MODES and int(modes.group(1)) % 128 == 0
    assert NEW <= _exported_functions(core.SO_PATH, "mh_")
    assert NEW <= set(core.lib()._declared)


def test_host_library_exports_the_coupled_render():
    from mesheditor_amd import bank
    assert os.path.exists(bank.SO_PATH), "run __graft_entry__.build()"
    assert "mhx_render_coupled" in _exported_functions(bank.SO_PATH, "mhx_")
    assert hasattr(bank.Scene, "render_coupled") and hasattr(bank, "Junction") and hasattr(bank.Junction, "of")


def test_the_bindings_junction_images_match_the_library(core):
    from mesheditor_amd import bank
    size = core.lib().mh_junction_struct_size()
    assert size == C.sizeof(core.Junction) == C.sizeof(bank.Junction) == 96, size
    side_order = ["object", "points", "weights", "nx", "ny", "nz", "scale"]
    for image in (core.JunctionSide, bank.JunctionSide):
        assert [n for n, _ in image._fields_] == side_order and C.sizeof(image) == 44
        assert [getattr(image, n).offset for n in side_order] == [0, 4, 16, 28, 32, 36, 40]
    order = ["a", "b", "stiffness", "flags"]
    for image in (core.Junction, bank.Junction):
        assert [n for n, _ in image._fields_] == order
        assert [getattr(image, n).offset for n in order] == [0, 44, 88, 92]
    j = bank.Junction.of((3, 2, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0), None, 5.0, True)
    assert (j.a.object, j.a.points[0], j.a.ny, j.a.scale, j.b.object, j.stiffness, j.flags) == (3, 2, 1.0, 2.0, core.NO_OBJECT, 5.0, core.JUNCTION_BILATERAL)
    sizes = (C.c_uint32 * 4)()
    core.lib().mh_abi_struct_sizes(sizes)  # still the four entries it always had
    assert list(sizes) == [C.sizeof(core.Profile), C.sizeof(core.SolverConfig), C.sizeof(core.Material), C.sizeof(core.MassProps)]
    assert core.lib().mh_drive_struct_size() == C.sizeof(core.Drive) == 20
    assert core.lib().mh_pickup_struct_size() == C.sizeof(core.Pickup) == 48


NORMAL, COUPLING, POINT = (0.25, -1.0, 0.5), 3.0, 2


def _one_mode_gains(s):
    """(a, read) of the one mode at POINT along NORMAL, in double."""
    along = s.shape_x[POINT] * NORMAL[0] + s.shape_y[POINT] * NORMAL[1] + s.shape_z[POINT] * NORMAL[2]
    return s.rad * along, COUPLING * s.defl_scale * along * s.defl


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])
@pytest.mark.parametrize("stiffness", [0.5, 40.0, 3000.0])
def test_a_bilateral_junction_on_one_mode_meets_the_spring_law_and_its_static_limit(dtype, stiffness):
    """One mode, bilateral, constant u, no other excitation.  The force of frame s is the spring law at the displacement of frame s + 1,
    f[s] = K (u - read Im z[s+1]), to 64 eps of the row's peak (the law is met by construction: what is left is the rounding of the solve's
    few operations); and f converges to the static limit of one mode, K u / (1 + K read a c_im / |1 - c|^2): a constant force f holds the
    mode at z = a f / (1 - c), whose imaginary part is a f c_im / |1 - c|^2.  The limit is compared to 64 eps x (1 + K C): the loop's
    denominator is what a rounding of d is divided by."""
    s, frames = _OneMode(), 1200
    r = jh.Restatement(s, [1], dtype)
    u = np.full((1, frames), 0.375, np.float32)
    junction = jh.spec(jh.side(0, POINT, direction=NORMAL, coupling=COUPLING), None, stiffness, True)
    im_after = []
    forces = np.zeros(frames)
    for t in range(frames):  # frame by frame, to see the state between frames
        _, f, comp, status = r.render_coupled([], [junction], u[:, t:t + 1], 1)
        forces[t] = float(f[0, 0])
        im_after.append(float(r.z[0][1][0]))
    a, read = _one_mode_gains(s)
    assert status[0] == 1 and abs(comp[0] - read * s.c.imag * a) <= 4 * float(np.finfo(dtype).eps) * abs(comp[0]) + 1e-18
    eps = max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps))
    # Im z[s+1] of the free advance of the state after frame s: the recorded Im z of the next frame (no other excitation enters it)
    law = stiffness * (0.375 - read * np.array(im_after[1:]))
    peak = np.abs(forces).max()
    assert peak > 0
    assert np.abs(forces[:-1] - law).max() <= 64 * eps * peak, (np.abs(forces[:-1] - law).max(), peak)
    limit = stiffness * 0.375 / (1 + stiffness * read * a * s.c.imag / abs(1 - s.c) ** 2)
    assert abs(forces[-1] - limit) <= 64 * eps * (1 + stiffness * abs(comp[0])) * abs(limit), (forces[-1], limit)
    assert np.isfinite(forces).all()


@pytest.mark.parametrize("dtype", [np.longdouble, np.float32])
def test_a_unilateral_junction_never_pulls(dtype):
    """A contact that makes and breaks: u a slow sine around zero over a mode rung by a drive.  f >= 0 throughout, f = 0 exactly where
    u[s] <= d (the free prediction), and f > 0 elsewhere."""
    s, frames = _OneMode(), 600
    r = jh.Restatement(s, [1], dtype)
    t = np.arange(frames)
    u = (0.05 * np.sin(2 * np.pi * t / 150.0)).astype(np.float32)[None, :]
    drive = (0.3 * np.sin(0.9 * t)).astype(np.float32)
    trace = {}
    _, f, _, status = r.render_coupled([(0, 1, (1.0, 0.5, 0.0), drive)], [jh.spec(jh.side(0, POINT, direction=NORMAL, coupling=COUPLING), None, 25.0)], u, frames, trace)
    f, d = np.asarray(f[0]), np.asarray(trace["d"][0])
    open_ = u[0].astype(dtype) <= d
    assert status[0] == 1 and (f >= 0).all()
    assert 0.1 * frames < open_.sum() < 0.9 * frames  # it does make and break
    assert (f[open_] == 0).all() and (f[~open_] > 0).all()


def test_a_refused_junction_gives_no_force():
    """A negative coupling makes C negative; with K >= -1 / C the denominator 1 + K C is not above 0: status 2, a zero row, and the
    objects move as with K = 0."""
    s, frames = _OneMode(), 64
    drive = (0.3 * np.sin(0.9 * np.arange(frames))).astype(np.float32)
    rows = [(0, 1, (1.0, 0.5, 0.0), drive)]
    u = np.full((1, frames), 0.25, np.float32)
    r = jh.Restatement(s, [1], np.float64)
    comp = r.compliance(jh.spec(jh.side(0, POINT, direction=NORMAL, coupling=-COUPLING), None, 1.0))
    assert comp < 0
    out, f, _, status = r.render_coupled(rows, [jh.spec(jh.side(0, POINT, direction=NORMAL, coupling=-COUPLING), None, -2.0 / comp)], u, frames)
    free, f0, _, status0 = jh.Restatement(s, [1], np.float64).render_coupled(rows, [jh.spec(jh.side(0, POINT, direction=NORMAL, coupling=-COUPLING), None, 0.0)], u, frames)
    assert status[0] == 2 and status0[0] == 1 and (f == 0).all() and (f0 == 0).all() and np.array_equal(out, free)
