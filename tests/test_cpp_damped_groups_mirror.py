"""tests/cpp/modal_damped_groups_test.cpp, built and run the way tests/test_cpp_mixed_mirror.py builds and runs the mixed test: on the CPU
it compiles and links against libmodalhost.so through the reference-style include path (<audio/ModalAudio.h>), so RenderModalDampedGroups
is part of the mirrored surface (the test names both overloads by their full types), and its host case runs: the argument check.  On
the GPU every case runs: a damped member of a group is solved by RenderModalDampedGroups and left out by RenderModalMixed, and without
such a member the entry is RenderModalMixed bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NAME = "modal_damped_groups_test"


def _build():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "mesheditor_amd", "libmodalhost.so")):
        ge.build()
    subprocess.run(["make", "-s", "-C", CPP, "bin/" + NAME], check=True)  # the Makefile's pattern rule: any <name>.cpp beside it


def test_damped_groups_test_compiles_against_the_mirror_and_its_host_case_passes():
    _build()
    p = subprocess.run([os.path.join(CPP, "bin", NAME), "--host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "1 case(s), 0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.gpu
def test_damped_groups_properties_through_the_mirror():
    _build()
    p = subprocess.run([os.path.join(CPP, "bin", NAME)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "3 case(s), 0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
