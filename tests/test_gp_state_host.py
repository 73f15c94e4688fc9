"""The transitions of an emulator's cached state (csrc/gp_state.h: alpha, L^-1 and K^-1 belong to the factor) through a sanitised host
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gp_state_transitions(tmp_path):
    """tests/c/gp_state_check.cpp sweeps every sequence of up to six transitions itself and exits non-zero at the first property that
    fails; built with the address and undefined-behaviour sanitisers"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gp_state_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "gp_state_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
