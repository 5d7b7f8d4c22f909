"""tests/cpp/modal_damped_test.cpp, built and run the way tests/test_cpp_hertz_mirror.py builds and runs the Hertz test: on the CPU it
compiles and links against libmodalhost.so through the reference-style include path (<audio/ModalAudio.h>, <audio/ContactModel.h>), so
ModalJunctionDamped, RenderModalDamped and ContactDamping are part of the mirrored surface (the test holds
static_assert(ModalJunctionDamped == 8)), and its host cases run: the grouping decision of include/modalhip_groups.hpp for damped
junctions, and the damping helper.  On the GPU every case runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NAME = "modal_damped_test"


def _build():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "mesheditor_amd", "libmodalhost.so")):
        ge.build()
    subprocess.run(["make", "-s", "-C", CPP, "bin/" + NAME], check=True)  # the Makefile's pattern rule: any <name>.cpp beside it


def test_damped_test_compiles_against_the_mirror_and_its_host_cases_pass():
    _build()
    p = subprocess.run([os.path.join(CPP, "bin", NAME), "--host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "2 case(s), 0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.gpu
def test_damped_properties_through_the_mirror():
    _build()
    p = subprocess.run([os.path.join(CPP, "bin", NAME)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "4 case(s), 0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
