// slhip_select.h -- the select pass of the per-object outputs (slhip_object_crops_select, slhip_object_points_select): the
// eligible (scene, slot) pairs of a batch as a compact record array in ascending (scene, slot) order.
//   k_select_count   one wave per scene: the eligible slots, ballot + popcount over the slots in strides of 64
//   k_scan_counts    (slhip_scan.h) one block: exclusive scan of the per-scene counts, the total behind them
//   k_select_emit    the walk of k_select_count again; every eligible lane writes its record at the scene's offset + its rank
// A Rule is a small aggregate {Params p; const In0* in0; ...}: the params record and the input arrays it reads.  The kernels
// take its members as their own arguments and put it together again, so that the record stays in the kernel-argument segment
// and every pointer keeps its __restrict__ (as members of one by-value argument they lose it, and the code comes out larger):
//   typedef ... Params, Record;
//   __device__ Row row(uint32_t scene, uint32_t n_slots) const;                    the scene's row of the [n_scenes, n_slots] inputs
//   __device__ bool eligible(Row row, uint32_t slot) const;                        slot in [1, n_slots)
//   __device__ Record make(Row row, uint32_t scene, uint32_t slot) const;          the record of an eligible slot
// Row is the rule's own (a pointer, an index): a wave takes it once, before its walk over the slots.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slhip_common.h"
#include "slhip_scan.h"
#include "slhip_step_timer.h"

namespace slhip {

// blocks of four waves, one scene per wave; the loop bounds are the same in every lane of a wave, so every ballot sees all 64
template <class Rule, class... In>
__global__ __launch_bounds__(256) void k_select_count(typename Rule::Params p, const In* __restrict__... in, uint32_t n_scenes,
                                                      uint32_t n_slots, unsigned long long* __restrict__ counts)
{
    const Rule rule = {p, in...};
    const uint32_t scene = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (scene >= n_scenes) return;
    const auto row = rule.row(scene, n_slots);
    unsigned long long n = 0ull;
    for (uint32_t base = 1u; base < n_slots; base += 64u) {
        const uint32_t slot = base + lane;
        const bool ok = slot < n_slots && rule.eligible(row, slot);
        n += (unsigned long long)__popcll(__ballot(ok));
    }
    if (lane == 0u) counts[scene] = n;
}

template <class Rule, class... In>
__global__ __launch_bounds__(256) void k_select_emit(typename Rule::Params p, const In* __restrict__... in, uint32_t n_scenes,
                                                     uint32_t n_slots, const unsigned long long* __restrict__ offsets,
                                                     typename Rule::Record* __restrict__ records, unsigned long long capacity)
{
    const Rule rule = {p, in...};
    const uint32_t scene = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (scene >= n_scenes) return;
    const auto row = rule.row(scene, n_slots);
    unsigned long long at = offsets[scene];
    for (uint32_t base = 1u; base < n_slots; base += 64u) {
        const uint32_t slot = base + lane;
        const bool ok = slot < n_slots && rule.eligible(row, slot);
        const unsigned long long votes = __ballot(ok);
        const unsigned long long mine = at + (unsigned long long)__popcll(votes & ((1ull << lane) - 1ull));
        if (ok && mine < capacity) records[mine] = rule.make(row, scene, slot);
        at += (unsigned long long)__popcll(votes);
    }
}

// the scratch of select(): per-scene counts / offsets, then the total
inline uint64_t select_scratch_bytes(uint32_t n_scenes) { return ((uint64_t)n_scenes + 1u) * 8u; }

// Count, scan, emit, the total copied back, one synchronisation.  *n_out is the needed total even when it exceeds `capacity`
// (then the status is `capacity_status` and nothing is written at or behind `capacity`); n_scenes == 0 launches nothing.  The
// entry has checked its arguments; `array` names the record array in the capacity text.  Step `step` of `timer` takes the
// kernels; `in`: the rule's input arrays in the order of its members.
template <class Rule, int N, class... In>
int select(const typename Rule::Params& p, uint32_t n_scenes, uint32_t n_slots, typename Rule::Record* d_records, uint64_t capacity,
           void* d_scratch, uint64_t* n_out, hipStream_t stream, int capacity_status, const char* who, const char* array,
           StepTimer<N>& timer, int step, const In*... in)
{
    *n_out = 0;
    if (n_scenes == 0u) return 0;
    unsigned long long* counts = (unsigned long long*)d_scratch;
    const uint32_t blocks = (n_scenes + 3u) / 4u;
    if (const int st = timer.begin(step, stream)) return st;
    k_select_count<Rule, In...><<<blocks, 256, 0, stream>>>(p, in..., n_scenes, n_slots, counts);
    k_scan_counts<1024><<<1, 1024, 0, stream>>>(counts, n_scenes);
    k_select_emit<Rule, In...><<<blocks, 256, 0, stream>>>(p, in..., n_scenes, n_slots, counts, d_records, capacity);
    SLHIP_LAUNCH_CHECK();
    if (const int st = timer.end(step, stream)) return st;
    unsigned long long total = 0;
    SLHIP_CHECK(hipMemcpyAsync(&total, counts + n_scenes, 8, hipMemcpyDeviceToHost, stream));
    SLHIP_CHECK(hipStreamSynchronize(stream));
    *n_out = total;
    if (total > capacity) {
        set_error("%s: %s holds %llu records, this batch needs %llu", who, array, (unsigned long long)capacity, total);
        return capacity_status;
    }
    return 0;
}

}  // namespace slhip
