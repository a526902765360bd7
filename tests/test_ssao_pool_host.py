"""The pooled end-of-band drain of the SSAO tap kernel (stillleben_amd/csrc/slhip_ssao_pool.h) on the host: the four waves of a
block drain their 4 x 5 level remainders as ONE list, level 5 of waves 0..3 first, in runs of 64.  The header's position -> (level,
queue word) arithmetic is checked against a plain enumeration of that list, for count vectors laid out by hand (nothing queued, an
empty level, a level whose four remainders exceed 64, totals that are multiples of 64) and at random; every entry is in exactly one
run, and a run's list is at least the level of each of its entries.  The program is tests/ssao_pool_check.cpp: plain C++, no GPU,
no sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ssao_pool_check.cpp")
INC = os.path.join(ROOT, "stillleben_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("ssao_pool") / "ssao_pool_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + INC, SRC, "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def _line(out, name, keys):
    m = re.search(r"^%s%s$" % (name, " ".join(k + r" (\d+)" for k in keys)), out, re.M)
    assert m, out[-2000:]
    return dict(zip(keys, (int(x) for x in m.groups())))


def test_every_position_is_the_enumerated_entry(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    t = _line(report.stdout, "", ("vectors", "positions", "runs", "mixed", "failures"))
    assert t["failures"] == 0
    assert t["vectors"] > 3000 and t["positions"] > 130 * t["vectors"]      # every vector: its whole list and 130 positions behind it
    assert 0 < t["mixed"] < t["runs"]                                        # runs that straddle a level edge, and runs of one level


def test_every_kind_of_count_vector_was_exercised(report):
    k = _line(report.stdout, "kinds ", ("empty_level", "level_over_64", "multiple_of_64", "zero"))
    assert k["empty_level"] > 100 and k["level_over_64"] > 100 and k["multiple_of_64"] > 100 and k["zero"] >= 1, k
