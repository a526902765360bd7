"""The scaffold of the tools/time_*.py that read a module's step timers: repeated calls under the HIP events of
slhip_<entry>_timing_enable, read out with slhip_<entry>_timings after every call.  `entry` is the stem of the two names, such
as "object_crops" or "pose_icp"."""
import ctypes as C
import statistics

from stillleben_amd import _abi


def timed(entry, steps, fn, rep, warm=2):
    """fn() warm + rep times with the step timers of `entry` on (the warm-up calls: code objects, allocator).  Returns
    (the last result, the `steps` milliseconds of each of the last `rep` calls as tuples; -1.0 or an error for a step that fn
    does not run, as the module's read-out has it)."""
    L = _abi.lib()
    enable, read = "slhip_%s_timing_enable" % entry, "slhip_%s_timings" % entry
    _abi.check(getattr(L, enable)(1), enable)
    out, times = None, []
    for r in range(warm + rep):
        out = fn()
        ms = (C.c_float * steps)()
        _abi.check(getattr(L, read)(C.byref(ms)), read)
        if r >= warm:
            times.append(tuple(ms))
    _abi.check(getattr(L, enable)(0), enable)
    return out, times


def timed_step(entry, steps, which, fn, rep, warm=2):
    """timed() for step `which` alone: (the last result, its median ms, its ms of every call)"""
    out, times = timed(entry, steps, fn, rep, warm)
    ms = [t[which] for t in times]
    return out, statistics.median(ms), ms
