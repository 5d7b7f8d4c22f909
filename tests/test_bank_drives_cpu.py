"""CPU-side checks of the sustained-drive feature: the boundary declares and exports it at every layer, the binding's mh_drive image
has the library's size, and the one-sample impact the GPU tests compare drives with has the force curve they assume (a restatement of
k_bank_forces' recurrence in both precisions -- no GPU, and no dependence on what the C library's cos/sin return at pi)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import drive_harness as dh
from tests.test_abi_cpu import _exported_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core():
    from mesheditor_amd import _lib
    _lib.build()
    return _lib


def test_header_declares_and_library_exports_the_driven_render(core):
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert {"mh_bank_render_driven", "mh_drive_struct_size", "mh_bank_render"} <= declared
    assert re.search(r"}\s*mh_drive\s*;", header)
    exported = _exported_functions(core.SO_PATH, "mh_")
    assert {"mh_bank_render_driven", "mh_drive_struct_size", "mh_bank_render"} <= exported
    assert "mh_bank_render_driven" in core.lib()._declared


def test_host_library_exports_the_driven_render():
    from mesheditor_amd import bank
    assert os.path.exists(bank.SO_PATH), "run __graft_entry__.build()"
    assert "mhx_render_driven" in _exported_functions(bank.SO_PATH, "mhx_")
    assert hasattr(bank.Scene, "render_driven")


def test_the_bindings_drive_image_matches_the_library(core):
    from mesheditor_amd import bank
    size = core.lib().mh_drive_struct_size()
    assert size == C.sizeof(core.Drive) == C.sizeof(bank.Drive) == 20, size
    assert [n for n, _ in core.Drive._fields_] == [n for n, _ in bank.Drive._fields_] == ["object", "ex_pos", "jx", "jy", "jz"]
    sizes = (C.c_uint32 * 4)()
    core.lib().mh_abi_struct_sizes(sizes)  # still the four entries it always had
    assert list(sizes) == [C.sizeof(core.Profile), C.sizeof(core.SolverConfig), C.sizeof(core.Material), C.sizeof(core.MassProps)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_half_turn_pulse_is_one_sample_of_gamma(dtype):
    """pulse_step = 0.5: the phasor turns by (cos pi, sin pi) = (-1, ~1e-7 in float, ~1e-16 in double).  First sample gamma * 0.5 * 2,
    second gamma * 0.5 * (1 - 1): the square of the sine's rounding error is far below half an ulp of 1, so the second phase is exactly
    1 whatever sin(pi) rounds to; then the pulse is spent.  The click input is accel_amp * force = 0, so the click is exactly zero."""
    f, (rot_re, rot_im), left = dh.forces_restatement(dtype, 0.75, 0.5, 16)
    assert rot_re == dtype(-1) and abs(rot_im) < 2 * np.finfo(dtype).eps
    assert left == 0
    assert np.array_equal(f, dh.impulse_row(0.75, 16).astype(dtype))
    for bad_sine in (dtype(3) * np.finfo(dtype).eps, -dtype(3) * np.finfo(dtype).eps, dtype(0)):  # any sine a C library could return for pi gives the same curve
        phase_re = dtype(dtype(-1) * dtype(-1)) - dtype(bad_sine * bad_sine)
        assert dtype(phase_re) == dtype(1)
    for gamma in (20.0, 0.125, 3.5):
        assert np.array_equal(dh.forces_restatement(dtype, gamma, 0.5, 4)[0], dh.impulse_row(gamma, 4).astype(dtype))


def test_the_longdouble_restatement_rings_and_superposes():
    """The restatement the GPU test trusts, checked against a closed form: one mode driven by an impulse rings as g * c^t."""
    L = np.longdouble

    class FakeScene:
        def column(self, name):
            n = 3
            table = {"CoeffRe": [0.9, 0.5, 0.0], "CoeffIm": [0.1, -0.3, 0.0], "RadiationGain": [2.0, 1.0, 1.0], "OutPhaseRe": [0.0, 1.0, 0.0], "OutPhaseIm": [1.0, 0.0, 1.0],
                     "ShapeX": np.arange(dh.POINTS * n) * 0.1 + 0.1, "ShapeY": np.zeros(dh.POINTS * n), "ShapeZ": np.zeros(dh.POINTS * n), "OutGain": [0.5], "ListenerGain": [2.0]}
            return np.asarray(table[name], float)
    r = dh.Restatement(FakeScene(), [3])
    f = dh.impulse_row(1.0, 8)
    out = r.render([(0, 1, (1.0, 0.0, 0.0), f)], 8)
    g = np.array([2.0 * 0.4, 1.0 * 0.5, 1.0 * 0.6], L)
    c = np.array([0.9 + 0.1j, 0.5 - 0.3j, 0.0], np.clongdouble)
    want = [float((g[0] * c[0] ** t).imag + (g[1] * c[1] ** t).real + (g[2] * c[2] ** t).imag) for t in range(8)]
    assert np.allclose(np.asarray(out, float), want, rtol=1e-14, atol=1e-16)
