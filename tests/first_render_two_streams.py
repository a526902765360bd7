"""Run as a fresh process by tests/test_gpu_step_pipeline.py (not collected by pytest): the FIRST two renders of a process, with
SSAO, back to back on two torch streams and with no synchronisation in between, then a third after a full synchronise.  The three
SSAO constant tables are uploaded once per process and device by the first slhip_render; the render on the second stream must not
run its SSAO kernels on tables that have not landed.  Prints `pictures equal: True` and exits 0 when the three pictures are the
same bytes."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402


def main():
    import scenes as SC
    import stillleben_amd as sl
    from stillleben_amd import _abi
    from stillleben_amd._batch import build_batch
    from stillleben_amd._context import engine

    sl.init_cuda(0)
    eng = engine()
    scene = SC.clutter_scene(sl, 7, n_objects=4, size=(160, 128))      # a multiple of 32 x 16: the tiled SSAO pass and its level table
    scene.manual_exposure = 1.0
    srec, drec, crec = build_batch([scene], eng.pool, None, with_shadows=True)
    eng.pool_abi()                                                      # the mesh pool is in HBM: the renders below upload records only
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=eng.device) for _ in range(2)]
    bufs = []
    for st in streams:                                                  # the process's first two slhip_render calls
        with torch.cuda.stream(st):
            bufs.append(eng.render_records(srec, drec, crec, 160, 128, _abi.OUT_ALL, ssao=True, shadows=True))
    torch.cuda.synchronize()
    bufs.append(eng.render_records(srec, drec, crec, 160, 128, _abi.OUT_ALL, ssao=True, shadows=True))
    torch.cuda.synchronize()
    pics = [b.rgb.cpu().numpy() for b in bufs]
    lit = int((pics[2][..., :3].astype(int).sum(axis=-1) > 0).sum())
    diff = [int((pics[i] != pics[2]).sum()) for i in range(2)]
    equal = diff == [0, 0] and lit > 0
    print("lit pixels: %d; bytes that differ from the third picture: %s" % (lit, diff))
    print("pictures equal: %s" % equal)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
