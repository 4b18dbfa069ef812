"""Every header under pomcpp_amd/csrc includes what it uses: a unit that holds nothing but `#include "<header>"` compiles for gfx950
(syntax only — no code is generated, no GPU needed).  So any of them can stand first in a translation unit, and the order of includes
is a matter of what the unit wants emitted in which order, never of what happens to be declared already."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pomcpp_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))


def test_there_are_headers():
    assert len(HEADERS) >= 30 and "pom_step_body.h" in HEADERS and "pom_host.h" in HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone(header, tmp_path):
    import __graft_entry__ as ge
    unit = tmp_path / "unit.hip"
    unit.write_text(f'#include "{header}"\n')
    cmd = ge.hip_compile_cmd("pom_batch", flags=("-fsyntax-only",))[:-1] + [str(unit)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
