"""tests/cpp/modal_friction_test.cpp, built and run the way tests/test_cpp_junction_mirror.py builds and runs the junction test: on the CPU
it compiles and links against libmodalhost.so through the reference-style include path (<audio/ModalAudio.h>), so ModalFriction /
RenderModalFriction are part of the mirrored surface (tests/test_bank_friction_cpu.py runs its host cases); on the GPU its cases run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NAME = "modal_friction_test"


def _build():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "mesheditor_amd", "libmodalhost.so")):
        ge.build()
    subprocess.run(["make", "-s", "-C", CPP, "bin/" + NAME], check=True)  # the Makefile's pattern rule: any <name>.cpp beside it


def test_friction_test_compiles_against_the_mirror():
    _build()
    assert os.path.exists(os.path.join(CPP, "bin", NAME))


@pytest.mark.gpu
def test_friction_properties_through_the_mirror():
    _build()
    p = subprocess.run([os.path.join(CPP, "bin", NAME)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
