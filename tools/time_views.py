#!/usr/bin/env python3
"""Developer tool (GPU box): what several views per settled scene buy a SceneBatch on the C2 shape (20 objects, 640x480,
6-channel GT, shadows + SSAO), and what the view entry costs the place step.

    views   stage + settle once, then V x (place(view=v) + render of all chunks) for V = 1, 2, 4, 8: pictures/s and the
            settle's share of the time
    place   place() against place(view=1) and place(view=1, object_to_camera=True) of the same process
    parent  place() with the library SLHIP_PARENT_LIB names (the parent commit's build): the plain path across commits

All timed with HIP events on the stream, the variants taken in turn with a rotating start, median / min / max over the
repetitions.  Every step runs in a child process of its own under a time limit; a step that fails ends the run.  Prints one JSON line.

    python tools/time_views.py [scenes=2048] [chunk=512] [repeats=10]
    SLHIP_PARENT_LIB=/path/to/parent/libslhip.so python tools/time_views.py"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = {"views": 420, "place": 180, "parent": 180}
VIEW_COUNTS = (1, 2, 4, 8)


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def step(name, N, CHUNK, REP):
    import torch

    import bench
    import stillleben_amd as sl
    from stillleben_amd import _abi, synthetic

    sl.init_cuda(0)
    table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=1024))
    batch = sl.SceneBatch(table, N, 20, resolution=bench.RESOLUTION, seed=20261017, render_chunk=CHUNK)
    batch.set_camera_intrinsics(*bench.INTRINSICS)

    def timed(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e)

    def settle():
        batch.stage()
        batch.settle()

    settle()
    batch.check_settled()
    out = {"library": _abi.lib_path() if name == "parent" else "lib/libslhip.so"}
    if name == "views":
        bufs = [None]

        def pictures(V):
            for v in range(V):
                batch.place(view=v)
                for c in range(batch.n_render_chunks()):
                    bufs[0] = batch.render(c, _abi.OUT_GT6, ssao=True, buffers=bufs[0])

        pictures(2)                  # warm-up: code objects, scratch
        torch.cuda.synchronize()
        t_settle, t_views = [], {V: [] for V in VIEW_COUNTS}
        for r in range(REP):
            t_settle.append(timed(settle))
            k = r % len(VIEW_COUNTS)
            for V in VIEW_COUNTS[k:] + VIEW_COUNTS[:k]:
                t_views[V].append(timed(lambda: pictures(V)))
        batch.check_settled()
        ms = statistics.median(t_settle)
        out["settle"] = summary(t_settle)
        out["views"] = {}
        for V in VIEW_COUNTS:
            mv = statistics.median(t_views[V])
            # the spread of pictures/s: the slowest and the fastest repetition of both parts
            out["views"][str(V)] = dict(summary(t_views[V]), pictures_per_s=round(N * V / (ms + mv) * 1e3, 1),
                                        pictures_per_s_min=round(N * V / (max(t_settle) + max(t_views[V])) * 1e3, 1),
                                        pictures_per_s_max=round(N * V / (min(t_settle) + min(t_views[V])) * 1e3, 1),
                                        settle_share=round(ms / (ms + mv), 4))
    else:
        variants = {"place()": lambda: batch.place()}
        if name == "place":
            variants["place(view=1)"] = lambda: batch.place(view=1)
            variants["place(view=1, object_to_camera=True)"] = lambda: batch.place(view=1, object_to_camera=True)
        names = list(variants)
        for n in names * 2:
            variants[n]()
        torch.cuda.synchronize()
        t = {n: [] for n in names}
        for r in range(REP):
            k = r % len(names)
            for n in names[k:] + names[:k]:
                t[n].append(timed(variants[n]))
        out["place"] = {n: summary(t[n]) for n in names}
    print("TIME_VIEWS_STEP " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(sys.argv[2], *(int(v) for v in sys.argv[3:6]))
        return
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    CHUNK = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    REP = max(5, int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    parent = os.environ.get("SLHIP_PARENT_LIB")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    result = {"metric": "views per settled scene, C2 shape: %d scenes, %d-scene render chunks, HIP events, %d repetitions per "
                        "variant taken in turn" % (N, CHUNK, REP), "commit": commit}
    for name in ("views", "place") + (("parent",) if parent else ()):
        env = dict(os.environ)
        env.pop("SLHIP_LIB", None)
        if name == "parent":
            env["SLHIP_LIB"] = parent
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, str(N), str(CHUNK), str(REP)]
        try:
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=STEP_TIMEOUT_S[name])
        except subprocess.TimeoutExpired:
            result[name] = {"error": "no result within %d s" % STEP_TIMEOUT_S[name]}
            break
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("TIME_VIEWS_STEP ")]
        if done.returncode != 0 or not lines:                  # nothing more is started on the device after a failure
            result[name] = {"error": "exit status %d" % done.returncode, "stderr": done.stderr[-2000:]}
            break
        result[name] = json.loads(lines[-1][len("TIME_VIEWS_STEP "):])
    if "place" in result and "parent" in result and "place" in result["place"] and "place" in result["parent"]:
        a, b = result["place"]["place"]["place()"], result["parent"]["place"]["place()"]
        result["place_vs_parent"] = {"median_ratio": round(a["median_ms"] / b["median_ms"], 4),
                                     "spread_this": round(a["max_ms"] / a["min_ms"], 4), "spread_parent": round(b["max_ms"] / b["min_ms"], 4)}
    print(json.dumps(result))
    if any("error" in v for v in result.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
