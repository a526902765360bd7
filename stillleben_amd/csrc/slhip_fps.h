// slhip_fps.h -- farthest point sampling per mesh class (slhip_fps.hip) for any count in [1, limit]: the body of
// slhip_object_keypoints_fps / _fps_host and, with their own limit, of slhip_object_regions_centres / _centres_host.
// `what` names the count in the error text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slhip.h"

namespace slhip {

// the scratch of fps_device(): dmin, one row of max_verts floats per class
inline uint64_t fps_scratch_bytes(uint32_t n_assets, uint64_t max_verts) { return (uint64_t)n_assets * max_verts * 4u; }

// n_assets in [1, SLHIP_SYNTH_MAX_ASSETS] and n_fps in [1, limit]: what an entry checks before it records a timing event
int check_fps(const char* who, const char* what, uint32_t limit, uint32_t n_assets, uint32_t n_fps);

// checks, then the launch of k_fps
int fps_device(const char* who, const char* what, uint32_t limit, const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets,
               uint32_t n_assets, const slhip_draw* d_templates, uint32_t n_templates, uint32_t n_fps, uint64_t max_verts,
               void* d_scratch, float* d_keypoints, int32_t* d_vertex, hipStream_t stream);
int fps_host(const char* who, const char* what, uint32_t limit, const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets,
             uint32_t n_assets, const slhip_draw* h_templates, uint32_t n_templates, uint32_t n_fps, float* h_keypoints,
             int32_t* h_vertex);

}  // namespace slhip
