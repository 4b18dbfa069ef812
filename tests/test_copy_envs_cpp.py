"""BatchEnvironment::CopyGames / CopyGamesDevice (include/pom_bboard.hpp) from a C++ program: builds everywhere, runs on the GPU."""
import os
import subprocess

import pytest

from tests.host_build import POM_BATCH, program


@pytest.fixture(scope="module")
def copy_games_exe(hip_lib):
    return program("tests/cpp/copy_games.cpp", extra=["-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"], link=POM_BATCH)


def test_copy_games_program_builds(copy_games_exe):
    assert os.path.exists(copy_games_exe)


@pytest.mark.gpu
def test_copy_games_from_cpp(copy_games_exe):
    out = subprocess.run([copy_games_exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "copy games ok" in out.stdout, f"rc={out.returncode}\n{out.stdout}\n{out.stderr}"
