"""BatchEnvironment::CopyGames / CopyGamesDevice (include/pom_bboard.hpp) from a C++ program: builds everywhere, runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")
LINK = ["-L" + os.path.join(ROOT, "pomcpp_amd"), "-lpom_batch", "-Wl,-rpath," + os.path.join(ROOT, "pomcpp_amd"),
        "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-pthread"]


@pytest.fixture(scope="module")
def copy_games_exe(hip_lib):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "copy_games")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "copy_games.cpp"), "-o", exe] + LINK, check=True)
    return exe


def test_copy_games_program_builds(copy_games_exe):
    assert os.path.exists(copy_games_exe)


@pytest.mark.gpu
def test_copy_games_from_cpp(copy_games_exe):
    out = subprocess.run([copy_games_exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "copy games ok" in out.stdout, f"rc={out.returncode}\n{out.stdout}\n{out.stderr}"
