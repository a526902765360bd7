"""The edge-function arithmetic of the rasterisers (stillleben_amd/csrc/slhip_raster_walk.h) on the host: the 32-bit form against
the 64-bit one, texel by texel, with every 32-bit intermediate re-evaluated in 64 bits and checked for the int32 range.  The
program is tests/raster_walk_check.cpp: plain C++, no GPU, no sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "raster_walk_check.cpp")
INC = os.path.join(ROOT, "stillleben_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("raster_walk") / "raster_walk_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + INC, SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return r


def _counts(out):
    rows = {}
    for m in re.finditer(r"^(\w+): triangles (\d+) narrow (\d+) wide (\d+) culled (\d+)$", out, re.M):
        rows[m.group(1)] = tuple(int(x) for x in m.group(2, 3, 4, 5))
    return rows


def test_narrow_walk_equals_the_wide_one_and_stays_in_range(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    m = re.search(r"^texels (\d+) covered (\d+) out_of_range (\d+) failures (\d+)$", report.stdout, re.M)
    assert m, report.stdout[-2000:]
    texels, covered, out_of_range, failures = (int(x) for x in m.groups())
    assert failures == 0 and out_of_range == 0
    assert texels > 100000 and 0 < covered < texels


def test_every_input_family_was_exercised(report):
    rows = _counts(report.stdout)
    assert set(rows) == {"random", "bound", "sliver", "zero", "far", "border"}, report.stdout[-2000:]
    assert rows["random"][1] > 1000                                 # random triangles walked in the narrow form (both windings)
    assert rows["bound"][1] > 0 and rows["bound"][2] > 0            # at / below the bound: narrow; just above: wide
    assert rows["sliver"][1] > 0 and rows["sliver"][2] > 0          # the extent limit on its own, from both sides
    assert rows["zero"][3] == rows["zero"][0] > 0                   # zero area: rejected by the set-up
    assert rows["far"][1] == 0 and rows["far"][2] > 0               # far vertices, small clamped box: never narrow
    assert rows["border"][1] > 0 and rows["border"][2] == 0         # boxes at the borders of the target: all narrow
