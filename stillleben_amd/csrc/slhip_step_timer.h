// slhip_step_timer.h -- the optional HIP-event timing of the per-object outputs (slhip_object_*_timing_enable / _timings): one
// pair of events round the last timed call of each of a module's N steps.  Host code; every method returns the library's status
// (0, or what SLHIP_CHECK returns).  The checks of an entry come before begin(): a refused call records no event.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "slhip_common.h"

namespace slhip {

template <int N>
struct StepTimer {
    bool on = false;
    hipEvent_t ev[2 * N] = {};      // (start, end) of step i at 2 i, 2 i + 1; created by the first enable(1), kept for the process
    bool timed[N] = {};

    int enable(int want)
    {
        if (want && !ev[0])
            for (hipEvent_t& e : ev) SLHIP_CHECK(hipEventCreate(&e));
        on = want != 0;
        for (bool& t : timed) t = false;
        return 0;
    }
    int begin(int step, hipStream_t stream)
    {
        if (on) SLHIP_CHECK(hipEventRecord(ev[2 * step], stream));
        return 0;
    }
    int end(int step, hipStream_t stream)
    {
        if (on) {
            SLHIP_CHECK(hipEventRecord(ev[2 * step + 1], stream));
            timed[step] = true;
        }
        return 0;
    }
    bool all_timed() const
    {
        for (bool t : timed)
            if (!t) return false;
        return true;
    }
    // ms_out[i]: the milliseconds of step i, -1.0 for a step that was not timed.  Returns how many were timed (or a status < 0).
    int read(float ms_out[N])
    {
        int n = 0;
        for (int i = 0; i < N; ++i) {
            ms_out[i] = -1.0f;
            if (!timed[i]) continue;
            SLHIP_CHECK(hipEventSynchronize(ev[2 * i + 1]));
            SLHIP_CHECK(hipEventElapsedTime(&ms_out[i], ev[2 * i], ev[2 * i + 1]));
            ++n;
        }
        return n;
    }
    // the body of an entry slhip_<module>_timings(ms_out): 0, or a status < 0
    int read_for(const char* entry, float ms_out[N])
    {
        if (!ms_out) {
            set_error("%s: null argument", entry);
            return -1;
        }
        return std::min(read(ms_out), 0);
    }
};

}  // namespace slhip
