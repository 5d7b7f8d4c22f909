"""The bank's render entries, layer against layer (no GPU): the parameters include/modalhip.h declares for each mh_bank_render* are as
many as the binding's argtypes (mesheditor_amd/_lib.py), a call without a bank is MH_EINVAL before the device is touched, and the
parameters mesheditor_amd/cpp/src/capi.cpp defines for each mhx_render_* junction entry are as many as mesheditor_amd/bank.py binds.
(A null scene is not a defined call of the mhx_ entries: counts only there.)"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANK_ENTRIES = ["mh_bank_render", "mh_bank_render_driven", "mh_bank_render_read", "mh_bank_render_coupled", "mh_bank_render_damped", "mh_bank_render_observed",
                "mh_bank_render_mixed", "mh_bank_render_damped_groups"]
SCENE_ENTRIES = ["mhx_render_coupled", "mhx_render_damped", "mhx_render_observed", "mhx_render_mixed", "mhx_render_damped_groups"]


def _parameters(path, name):
    """The number of parameters of the one `int name(...)` in a C or C++ source, comments stripped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, path)).read(), flags=re.S)
    found = re.findall(r"\bint\s+%s\s*\(([^()]*)\)" % re.escape(name), text)
    assert len(found) == 1, (path, name, len(found))
    return len([p for p in found[0].split(",") if p.strip()])


@pytest.mark.parametrize("name", BANK_ENTRIES)
def test_a_bank_entry_has_the_header_s_parameters_and_refuses_a_null_bank(name):
    from mesheditor_amd import _lib
    fn = getattr(_lib.lib(), name)
    assert _parameters("include/modalhip.h", name) == len(fn.argtypes), name
    assert fn(*([None] + [0] * (len(fn.argtypes) - 1))) == _lib.MH_EINVAL, name


@pytest.mark.parametrize("name", SCENE_ENTRIES)
def test_a_scene_entry_has_the_parameters_the_binding_passes(name):
    from mesheditor_amd import bank
    assert _parameters("mesheditor_amd/cpp/src/capi.cpp", name) == len(getattr(bank.lib(), name).argtypes), name
