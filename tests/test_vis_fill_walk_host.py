"""The strided edge walk of k_vis_fill (stillleben_amd/csrc/slhip_raster_walk.h, Walk::rows_down) on the host: whole targets
walked in the order of the fill pass -- strips of 64 columns, four waves on alternate rows, eight rows per start, the skip of a
wave outside the triangle's pixel box -- against cover<long long>, pixel by pixel.  The program is tests/vis_fill_walk_check.cpp:
plain C++, no GPU, no sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "vis_fill_walk_check.cpp")
INC = os.path.join(ROOT, "stillleben_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("vis_fill_walk") / "vis_fill_walk_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + INC, SRC, "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_stepped_values_are_those_of_cover_and_every_pixel_has_one_owner(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    m = re.search(r"^pixels (\d+) covered (\d+) waves_walked (\d+) waves_skipped (\d+) failures (\d+)$", report.stdout, re.M)
    assert m, report.stdout[-2000:]
    pixels, covered, walked, skipped, failures = (int(x) for x in m.groups())
    assert failures == 0
    assert pixels > 1000000 and 0 < covered < pixels
    assert walked > 0 and skipped > 0                      # both sides of the pixel-box test of a wave


def test_every_input_family_was_exercised(report):
    rows = {}
    for m in re.finditer(r"^(\w+): triangles (\d+) walked (\d+) flipped (\d+) culled (\d+)$", report.stdout, re.M):
        rows[m.group(1)] = tuple(int(x) for x in m.group(2, 3, 4, 5))
    assert set(rows) == {"random", "sliver", "border", "far", "corner", "plane"}, report.stdout[-2000:]
    for name in ("random", "sliver", "border", "far", "corner"):
        tris, walked, flipped, culled = rows[name]
        assert walked > 0 and 0 < flipped < walked, name   # both windings of every family reach the walk
        assert walked + culled == tris
    assert rows["plane"][1] == 2
