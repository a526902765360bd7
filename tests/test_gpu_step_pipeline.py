"""bench.Pipeline -- the overlapped step the headline figure is measured on -- against one stream.  The pipeline keeps a ring of
SceneBatch record sets, stages / settles / places step k + 1 on a settle stream while the chunks of step k render on two render
streams (each with a scratch set of its own), re-renders its target slots after TARGET_RING chunks and guards every record set
with a `free` event.  Here it runs five steps of 28 scenes (chunks of 8, 8, 8, 4 on two target slots; every record set used at
least twice) without a synchronisation in between, and everything it computed is compared, byte for byte, with a fresh SceneBatch
that does the same steps on the default stream, every call synchronised, every step on cold scratch.

The pipeline is observed without touching its ordering: `place` and `render` of its record sets are wrapped, and the wrapper
enqueues clone()s of the records / the render targets on whatever stream is current -- no synchronise, no event, no stream switch.

The test proves equality, not that the device overlapped anything: the timeline it prints (from the pipeline's own events) tells.

Also here: the first two renders of a fresh process on two streams (tests/first_render_two_streams.py)."""
import os
import subprocess
import sys

import pytest
import torch

from stillleben_amd import _abi
from test_gpu_scratch_state import keep_is_clean

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SCENES, N_OBJECTS, RES, CHUNK, STEPS, SEED = 28, 6, (320, 240), 8, 5, 20260929
INTRINSICS = (533.389, 533.7435, 156.49345, 120.65545)
RECORDS = ("d_bodies", "d_scenes", "d_srec", "d_drec", "d_crec")
TARGETS = ("rgb", "coord", "cls", "instance", "normals")        # the five tensors of OUT_GT6
FRAMES = None               # settle frames of both runs (None: the batch's default, 400)


@pytest.fixture(scope="module")
def table(sl):
    from stillleben_amd import synthetic

    return sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))


@pytest.fixture(scope="module")
def lockstep():
    """SLHIP_SETTLE_PERSISTENT=0 for the module: the form the benchmark's batches take, 2 400 short launches per settle."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SLHIP_SETTLE_PERSISTENT", "0")
        yield


def cold(eng, se):
    torch.cuda.synchronize()
    eng._scratch.clear()
    eng.__dict__.setdefault("_clips", {}).clear()
    se._scratch.clear()


@pytest.fixture(scope="module")
def reference(sl, table, lockstep):
    """Per step: the five record arrays after place() and the five targets of every chunk, on the device."""
    b = sl.SceneBatch(table, N_SCENES, N_OBJECTS, resolution=RES, seed=SEED, render_chunk=CHUNK, shadows=True, pair_contact_budget=0)
    b.set_camera_intrinsics(*INTRINSICS)
    if FRAMES is not None:
        b.settle_params["frames"] = FRAMES
    steps = []
    for k in range(STEPS):
        cold(b.eng, b.se)
        b.stage(scene_id_base=k * N_SCENES)
        torch.cuda.synchronize()
        b.settle()
        torch.cuda.synchronize()
        b.check_settled()
        b.place()
        torch.cuda.synchronize()
        step = {"records": [getattr(b, name).clone() for name in RECORDS], "chunks": []}
        for c in range(b.n_render_chunks()):
            bufs = b.render(c, _abi.OUT_GT6, ssao=True)
            torch.cuda.synchronize()
            step["chunks"].append([getattr(bufs, name) for name in TARGETS])
        steps.append(step)
    assert [t[0].shape[0] for t in steps[0]["chunks"]] == [8, 8, 8, 4]
    assert int((steps[0]["chunks"][3][3] != 0).sum()) > 0          # objects are in the pictures
    assert not same(steps[0]["records"][0], steps[1]["records"][0])    # ... and every step has other scenes
    return steps


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def tap(batch, log, cur):
    """Wraps place / render of one record set: the original, then clones on the current stream."""
    place, render = batch.place, batch.render

    def tapped_place(*a, **kw):
        r = place(*a, **kw)
        log.append((cur["k"], "records", None, [getattr(batch, name).clone() for name in RECORDS]))
        return r

    def tapped_render(chunk=0, *a, **kw):
        bufs = render(chunk, *a, **kw)
        log.append((cur["k"], "chunk", chunk, [getattr(bufs, name).clone() for name in TARGETS]))
        return bufs

    batch.place, batch.render = tapped_place, tapped_render


def timeline(recs):
    """From the pipeline's events: per step the settle's length, and from the end of its last render to the next step's settle
    start (negative: that settle began while the step still rendered)."""
    lines, overlapped = [], False
    for k, rec in enumerate(recs):
        settle = rec["ev0"].elapsed_time(rec["ev1"])
        render = [e0.elapsed_time(e1) for e0, e1 in rec["render_events"]]
        line = "step %d: settle %.2f ms, render chunks %s ms" % (k, settle, " ".join("%.2f" % r for r in render))
        if k + 1 < len(recs):
            gap = min(e1.elapsed_time(recs[k + 1]["ev0"]) for _, e1 in rec["render_events"])
            overlapped |= gap < 0
            line += "; last render end -> settle start of step %d: %+.2f ms" % (k + 1, gap)
        lines.append(line)
    lines.append("a settle began before the previous step's last render ended: %s" % ("yes" if overlapped else "no"))
    return lines


@pytest.mark.parametrize("settle_streams", [1, 2])
def test_overlapped_steps_equal_one_stream(sl, table, lockstep, reference, monkeypatch, settle_streams):
    import bench

    monkeypatch.setattr(bench, "N_OBJECTS", N_OBJECTS)
    monkeypatch.setattr(bench, "RESOLUTION", RES)
    monkeypatch.setattr(bench, "INTRINSICS", INTRINSICS)
    monkeypatch.setattr(bench, "TARGET_RING", 2)
    monkeypatch.delenv("SLHIP_BENCH_RING", raising=False)
    cold(table.eng, table.se)
    pipe = bench.Pipeline(sl, table, batch=N_SCENES, render_chunk=CHUNK, ssao=True, settle_streams=settle_streams, seed=SEED, rank=0,
                          render_streams=2)
    assert len(pipe.sets) == settle_streams + 1 and len(pipe.s_render_all) == 2
    log, cur = [], {"k": None}
    for b in pipe.sets:
        if FRAMES is not None:
            b.settle_params["frames"] = FRAMES
        tap(b, log, cur)
    recs = []
    for k in range(STEPS):                                      # no synchronisation in between
        cur["k"] = k
        recs.append(pipe.launch_step(k, k * N_SCENES))
    pipe.drain()

    print()
    for line in timeline(recs):
        print("settle_streams=%d  %s" % (settle_streams, line))

    assert [(k, what, c) for k, what, c, _ in log] == [(k, what, c) for k in range(STEPS)
                                                       for what, c in [("records", None)] + [("chunk", c) for c in range(4)]]
    wrong = []
    for k, what, c, got in log:
        want = reference[k]["records"] if what == "records" else reference[k]["chunks"][c]
        names = RECORDS if what == "records" else TARGETS
        for name, g, w in zip(names, got, want):
            if not same(g, w):
                n = int((g.contiguous().view(torch.uint8) != w.contiguous().view(torch.uint8)).sum()) if g.shape == w.shape else -1
                wrong.append("step %d %s %s: %d bytes differ" % (k, what if c is None else "chunk %d" % c, name, n))
    assert not wrong, "%d of %d snapshots differ from the one-stream run: %s" % (len(wrong), 5 * len(log), "; ".join(wrong[:12]))
    assert len(log) * 5 == STEPS * (5 + 4 * 5)
    # the ragged last chunk got buffers of its own each step, the others share the two slots
    assert len(pipe.buffers) == 2 and all(r["last_chunk"].B == 4 for r in recs)
    for b in pipe.sets:
        b.check_settled()
    streams = {s.cuda_stream for s in pipe.s_render_all}
    sets = [(key, keep) for key, keep in table.eng._scratch.items() if key[6] in streams]
    assert sorted(key[0] for key, _ in sets) == [4, 8, 8]
    for key, keep in sets:
        why = keep_is_clean(keep, key[0])
        assert why is None, "scratch of %d scenes on stream %#x: %s" % (key[0], key[6], why)
    cold(table.eng, table.se)


def test_first_renders_of_a_process_on_two_streams():
    """One fresh child process whose first two renders (SSAO on) go to two streams back to back: the one-time upload of the SSAO
    tables is complete before the first slhip_render returns, so all three pictures are the same bytes."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "first_render_two_streams.py")], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pictures equal: True" in r.stdout, r.stdout + r.stderr
