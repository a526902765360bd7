"""The scaffold of tools/time_object_{crops,points,keypoints,regions}.py: repeated calls under the HIP events of
slhip_object_<what>_timing_enable, read out with slhip_object_<what>_timings after every call."""
import ctypes as C

from stillleben_amd import _abi


def timed(what, steps, fn, rep, warm=2):
    """fn() warm + rep times with the step timers of object_<what> on (the warm-up calls: code objects, allocator).  Returns
    (the last result, the `steps` milliseconds of each of the last `rep` calls as tuples; -1.0 or an error for a step that fn
    does not run, as the module's read-out has it)."""
    L = _abi.lib()
    enable, read = "slhip_object_%s_timing_enable" % what, "slhip_object_%s_timings" % what
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
