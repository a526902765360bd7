"""The large-triangle queue of the rasterisers (stillleben_amd/csrc/slhip_tile_queue.h) on the host: queues filled by the producer's
arithmetic or laid out by hand, consumed range by range as the kernels consume them.  Every tile of every queued box is visited
exactly once over all ranges, nothing outside a box is visited, and a triangle the producer walks in place is never visited.  The
program is tests/tile_queue_check.cpp: plain C++, no GPU, no sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tile_queue_check.cpp")
INC = os.path.join(ROOT, "stillleben_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("tile_queue") / "tile_queue_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + INC, SRC, "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def _line(out, name, keys):
    m = re.search(r"^%s%s$" % (name, " ".join(k + r" (\d+)" for k in keys)), out, re.M)
    assert m, out[-2000:]
    return dict(zip(keys, (int(x) for x in m.groups())))


def test_every_tile_once_and_nothing_else(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    t = _line(report.stdout, "", ("lists", "walks", "tiles", "visited", "in_place", "failures"))
    assert t["failures"] == 0
    assert t["walks"] == 6 * t["lists"]                       # 1, 2, 3, 7, 64 and 8 192 ranges over every list
    assert 0 < t["visited"] < t["tiles"] and t["in_place"] > 0    # boxes consumed from the queue and boxes left to their producers
    assert t["visited"] > 6 * (256 * 256 + 80 * 60)           # the large boxes were among them


def test_every_kind_of_queue_and_split_was_exercised(report):
    s = _line(report.stdout, "starts ", ("boundary", "midrow", "gap"))
    assert s["boundary"] > 64 and s["midrow"] > 1000 and s["gap"] > 10, s
    k = _line(report.stdout, "kinds ", ("carried", "clipped", "empty"))
    assert k["carried"] >= 4 and k["clipped"] >= 6 and k["empty"] >= 4, k
