"""CPU-side checks of the deflection pickups: every layer declares and exports them, the binding's mh_pickup images have the library's
size and field order, and the restatement the GPU tests trust (tests/pickup_harness.py) agrees with a closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import drive_harness as dh
from tests import pickup_harness as ph
from tests.test_abi_cpu import _exported_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mh_bank_render_read", "mh_bank_set_deflection_gain", "mh_pickup_struct_size"}


@pytest.fixture(scope="module")
def core():
    from mesheditor_amd import _lib
    _lib.build()
    return _lib


def test_header_declares_and_library_exports_the_pickup_entries(core):
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert NEW | {"mh_bank_render_driven", "mh_bank_render", "mh_bank_set_coefficients"} <= declared
    assert re.search(r"}\s*mh_pickup\s*;", header)
    cap = re.search(r"#define\s+MH_PICKUPS_PER_OBJECT\s+(\d+)", header)
    assert cap and int(cap.group(1)) >= 8
    assert NEW <= _exported_functions(core.SO_PATH, "mh_")
    assert NEW <= set(core.lib()._declared)


def test_host_library_exports_the_read_render():
    from mesheditor_amd import bank
    assert os.path.exists(bank.SO_PATH), "run __graft_entry__.build()"
    assert "mhx_render_read" in _exported_functions(bank.SO_PATH, "mhx_")
    assert hasattr(bank.Scene, "render_read") and hasattr(bank, "Pickup")


def test_the_bindings_pickup_images_match_the_library(core):
    from mesheditor_amd import bank
    size = core.lib().mh_pickup_struct_size()
    assert size == C.sizeof(core.Pickup) == C.sizeof(bank.Pickup) == 48, size
    order = ["object", "points", "weights", "nx", "ny", "nz", "scale", "advance"]
    assert [n for n, _ in core.Pickup._fields_] == [n for n, _ in bank.Pickup._fields_] == order
    for image in (core.Pickup, bank.Pickup):
        assert [getattr(image, n).offset for n in order] == [0, 4, 16, 28, 32, 36, 40, 44]
    sizes = (C.c_uint32 * 4)()
    core.lib().mh_abi_struct_sizes(sizes)  # still the four entries it always had
    assert list(sizes) == [C.sizeof(core.Profile), C.sizeof(core.SolverConfig), C.sizeof(core.Material), C.sizeof(core.MassProps)]
    assert core.lib().mh_drive_struct_size() == C.sizeof(core.Drive) == 20


class _OneMode:
    """One object, one mode, four points: the columns a Scene would return."""
    c, rad, defl, defl_scale = 0.875 + 0.3125j, 2.0, 0.25, 0.5  # (binary fractions: the same numbers in every format)
    shape_x, shape_y, shape_z = [0.125, 0.25, 0.5, 0.75], [0.375, -0.125, 0.0625, 0.25], [0.0, 0.5, -0.25, 0.125]

    def column(self, name):
        table = {"CoeffRe": [self.c.real], "CoeffIm": [self.c.imag], "RadiationGain": [self.rad], "DeflectionGain": [self.defl], "OutPhaseRe": [0.0], "OutPhaseIm": [1.0],
                 "ShapeX": self.shape_x, "ShapeY": self.shape_y, "ShapeZ": self.shape_z, "OutGain": [1.0], "ListenerGain": [1.0], "DeflectionScale": [self.defl_scale]}
        return np.asarray(table[name], float)


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])
def test_a_pickup_of_one_struck_mode_is_the_closed_form(dtype):
    """One mode, a one-sample impulse of gain g: the state after frame t is g c^t, so frame t of an advance-a pickup is
    read * Im(g c^(t + a))."""
    s, frames = _OneMode(), 24
    r = ph.Restatement(s, [1], dtype)
    direction, normal, coupling = (1.0, 0.5, 0.0), (0.25, -1.0, 0.5), 3.0
    pickups = [ph.spec(0, 2, direction=normal, coupling=coupling, advance=a) for a in (0, 1, 2)]
    out, reads = r.render([(0, 1, direction, dh.impulse_row(0.75, frames))], pickups, frames)
    g = 0.75 * s.rad * (s.shape_x[1] * direction[0] + s.shape_y[1] * direction[1] + s.shape_z[1] * direction[2])
    read = coupling * s.defl_scale * (s.shape_x[2] * normal[0] + s.shape_y[2] * normal[1] + s.shape_z[2] * normal[2]) * s.defl
    tol = 64 * max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps))  # (the closed form itself is evaluated in double)
    for a in (0, 1, 2):
        want = np.array([read * (g * s.c ** (t + a)).imag for t in range(frames)])
        assert np.abs(want).max() > 0
        assert np.abs(np.asarray(reads[a], float) - want).max() <= tol * np.abs(want).max(), a
    assert np.abs(np.asarray(out, float) - np.array([(g * s.c ** t).imag for t in range(frames)])).max() <= tol * abs(g)


@pytest.mark.parametrize("dtype", [np.longdouble, np.float32])
def test_a_blend_is_the_weighted_sum_of_its_points(dtype):
    s, frames = _OneMode(), 16
    weights, normal = (0.5, 0.25, 0.25), (0.25, -1.0, 0.5)
    pickups = [ph.spec(0, (3, 0, 1), weights, normal, 2.0, 1)] + [ph.spec(0, p, direction=normal, coupling=2.0, advance=1) for p in (3, 0, 1)]
    _, reads = ph.Restatement(s, [1], dtype).render([(0, 0, (1.0, 0.0, 0.0), dh.impulse_row(1.0, frames))], pickups, frames)
    reads = np.asarray(reads, float)
    mixed = weights[0] * reads[1] + weights[1] * reads[2] + weights[2] * reads[3]
    assert np.abs(reads[0]).max() > 0
    assert np.abs(reads[0] - mixed).max() <= 16 * max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps)) * np.abs(reads[1:]).max()

