"""Per-object visibility statistics (slhip_render_object_stats, sl.ObjectStats) without a device: the C-ABI entries resolve,
the pool sizing, the record layout, the argument checks, and BOP's scene_gt_info form of hand-made statistics."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stillleben_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_resolve():
    L = _abi.lib()
    assert hasattr(L, "slhip_render_object_stats")
    assert hasattr(L, "slhip_render_object_stats_bytes")
    assert L.slhip_abi_version() == 5


@pytest.mark.parametrize("B,S,W,H,words", [
    (1, 2, 8, 8, 1),                        # one object slot, one tile
    (3, 21, 640, 480, 3 * 20 * 80 * 60),
    (2, 4, 100, 50, 2 * 3 * 13 * 7),         # W, H not multiples of 8: partial tiles count
    (5, 1, 640, 480, 0),                    # slot 0 only: nothing to raster
])
def test_worst_case_words(B, S, W, H, words):
    out = C.c_uint64(123)
    assert _abi.lib().slhip_render_object_stats_bytes(B, S, W, H, C.byref(out)) == 0
    assert out.value == words


def test_bytes_rejects_null():
    L = _abi.lib()
    assert L.slhip_render_object_stats_bytes(1, 2, 8, 8, None) != 0
    assert b"null" in L.slhip_last_error()


def test_record_dtype_matches_header():
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    m = re.search(r"typedef struct \{\s*uint32_t px_visib, px_all;\s*int32_t\s+bbox_visib\[4\];\s*int32_t\s+bbox_obj\[4\];\s*\}"
                  r" slhip_object_stats;", hdr)
    assert m, "slhip_object_stats changed in include/slhip.h"
    assert "40 bytes" in hdr[max(0, m.start() - 400):m.start()]
    assert _abi.OBJECT_STATS_DTYPE.itemsize == 40
    assert _abi.OBJECT_STATS_DTYPE.names == ("px_visib", "px_all", "bbox_visib", "bbox_obj")
    assert "#define SLHIP_OBJECT_STATS_CAPACITY %d " % _abi.OBJECT_STATS_CAPACITY in hdr


@pytest.mark.parametrize("missing", ["words", "out"])
def test_null_pool_or_output_is_an_error(missing):
    """The argument checks run before anything touches a device: fake (never dereferenced) addresses for the rest."""
    L = _abi.lib()
    pool = _abi.MeshPool()
    scratch = _abi.RenderScratch()
    fake = C.c_void_p(0x1000)
    need = C.c_uint64(0)
    words = None if missing == "words" else fake
    out = None if missing == "out" else fake
    st = L.slhip_render_object_stats(C.byref(pool), fake, fake, fake, 1, 1, 1, 64, 64, C.byref(scratch), 2, words, 16, out,
                                     C.byref(need), None)
    assert st != 0 and st != _abi.OBJECT_STATS_CAPACITY
    assert b"slhip_render_object_stats" in L.slhip_last_error()


def test_object_stats_is_exported():
    import stillleben as sl
    import stillleben_amd

    assert sl.ObjectStats is stillleben_amd.ObjectStats
    import stillleben.lib.libstillleben_python as m

    assert not hasattr(m, "ObjectStats")      # the reference's module keeps the reference's names


def _stats(visib, all_, bv, bo):
    from stillleben_amd.object_stats import ObjectStats

    t = lambda a: torch.tensor(a, dtype=torch.int32)   # noqa: E731
    return ObjectStats(t(visib), t(all_), t(bv), t(bo))


def test_to_bop():
    # two scenes, slots 0..3; scene 1: object 1 partly hidden, object 2 fully hidden, object 3 not drawn
    st = _stats(
        [[0, 10, 0, 0], [0, 25, 0, 0]],
        [[0, 10, 4, 0], [0, 100, 7, 0]],
        [[[-1] * 4, [3, 4, 5, 2], [-1] * 4, [-1] * 4], [[-1] * 4, [0, 0, 5, 5], [-1] * 4, [-1] * 4]],
        [[[-1] * 4, [3, 4, 5, 2], [7, 7, 2, 2], [-1] * 4], [[-1] * 4, [0, 0, 10, 10], [20, 1, 7, 1], [-1] * 4]],
    )
    assert st.visib_fract.dtype == torch.float32
    assert torch.equal(st.visib_fract, torch.tensor([[0.0, 1.0, 0.0, 0.0], [0.0, 0.25, 0.0, 0.0]]))
    bop = st.to_bop(1)
    assert bop == [
        {"bbox_obj": [0, 0, 10, 10], "bbox_visib": [0, 0, 5, 5], "px_count_all": 100, "px_count_visib": 25, "visib_fract": 0.25},
        {"bbox_obj": [20, 1, 7, 1], "bbox_visib": [-1, -1, -1, -1], "px_count_all": 7, "px_count_visib": 0, "visib_fract": 0.0},
        {"bbox_obj": [-1, -1, -1, -1], "bbox_visib": [-1, -1, -1, -1], "px_count_all": 0, "px_count_visib": 0,
         "visib_fract": 0.0},
    ]
    assert st[0].to_bop() == st.to_bop(0)
    assert st.to_bop(0)[0]["visib_fract"] == 1.0
    with pytest.raises(ValueError):
        st.to_bop()


def test_from_records_layout():
    from stillleben_amd.object_stats import ObjectStats

    rec = np.zeros((1, 3), _abi.OBJECT_STATS_DTYPE)
    rec[0, 2] = (3, 12, (1, 2, 3, 1), (0, 0, 4, 4))
    rec[0, 0]["bbox_visib"] = rec[0, 0]["bbox_obj"] = -1
    rec[0, 1]["bbox_visib"] = rec[0, 1]["bbox_obj"] = -1
    st = ObjectStats.from_records(torch.from_numpy(rec.view(np.int32).reshape(1, 3, 10).copy()))
    assert st.n_slots == 3
    assert st.to_bop(0)[1] == {"bbox_obj": [0, 0, 4, 4], "bbox_visib": [1, 2, 3, 1], "px_count_all": 12, "px_count_visib": 3,
                               "visib_fract": 0.25}
