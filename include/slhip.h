/*
 * slhip.h -- C ABI of libslhip.so, the MI355X (gfx950) scene-synthesis hot path.
 *
 * This is the drop-in boundary for the path stillleben implements with
 *   - PhysX  : Scene::simulateTableTopScene / Scene::simulate / Scene::checkCollisions /
 *              ManipulationSim::step       (reference src/scene.cpp:612-759, :903-925,
 *                                           src/manipulation_sim.cpp:83-93)
 *   - OpenGL : RenderPass::render           (reference src/render_pass.cpp:303-796 and
 *                                           src/shaders/render_shader.{vert,geom,frag})
 *   - CUDA   : generateSobelValidMask / dilateObjectMask (reference python/src/diff.cu,
 *              python/src/bridge_diff.cpp:13-157) and the pose backward of
 *              python/stillleben/diff.py:355-523
 *
 * Conventions
 *   - plain C, no exceptions, no torch types.  Every function returns 0 on success and a
 *     negative code on failure; slhip_last_error() returns a thread-local message.
 *   - every pointer named d_* is a DEVICE pointer into caller-owned memory (the Python host
 *     allocates it with torch); h_* are host pointers.  Nothing is allocated behind the
 *     caller's back except the opaque handles created by *_create.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All launches are
 *     asynchronous on that stream; nothing synchronises unless documented.
 *   - matrices are ROW-major float[16] (m[4*r+c]); the reference's Magnum matrices are
 *     column-major and its Python boundary transposes them (python/src/py_magnum.h:55-69),
 *     so row-major here == the tensors the reference's Python API hands out.
 *   - all structs are PODs with explicit sizes; arrays of structs are tightly packed.
 */
#ifndef SLHIP_H
#define SLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLHIP_ABI_VERSION 5   /* 2: slhip_render_scratch.d_shadow_tiles, slhip_render_scratch_bytes fills 7 sizes
                                 3: slhip_render_scratch.d_vattr is REQUIRED (the post-transform vertex cache) and `_pad` became
                                    shadow_lights; d_clip holds 9 float4 planes per vertex; slhip_settle_params grew to 116 bytes
                                    (list capacities instead of caps, pair_contact_budget, resume: the contact state of a settle
                                    outlives the call); slhip_settle_caps fills counts[8]
                                 4: slhip_settle_params.max_body_pairs_per_scene (120 bytes); slhip_settle_caps fills ten counts
                                 5: slhip_settle_params.stabilization_threshold (128 bytes); slhip_body.stab (304 bytes) carries the
                                    stabilisation state of a body, SLHIP_BODY_FROZEN; slhip_settle_solver_wave_lds, slhip_host_convex_hull,
                                    slhip_host_fill_holes
                                 5, additive (no struct or signature changed; detect with dlsym): slhip_object_stats,
                                    slhip_render_object_stats, slhip_render_object_stats_bytes; slhip_object_mask,
                                    slhip_render_object_masks, slhip_render_object_masks_bytes, slhip_object_masks_expand;
                                    slhip_object_crops_check_params, _scratch_bytes, _select, _gather, _timing_enable, _timings;
                                    slhip_object_points_check_params, _scratch_bytes, _select, _gather, _host_pixels,
                                    _timing_enable, _timings;
                                    slhip_object_keypoints_check_params, _fps_bytes, _fps, _fps_host, _project, _field,
                                    _timing_enable, _timings;
                                    slhip_object_regions_check_params, _centres_bytes, _centres, _centres_host, _vertices,
                                    _vertices_host, _label, _label_host, _timing_enable, _timings;
                                    slhip_pose_error_check_params, _diameter, _diameter_host, slhip_pose_error,
                                    slhip_pose_error_host, _timing_enable, _timings;
                                    slhip_render_flow_check_params, slhip_render_flow, _host, _motion, _motion_host */
#define SLHIP_NUM_LIGHTS 3 /* reference include/stillleben/common.h:17 */

/* ---------------------------------------------------------------------------------------------
 * Render half
 * ------------------------------------------------------------------------------------------- */

/* Image-based lighting ('next' row f1 of SURVEY.md 8f): the textures LightMap::load builds
 * (reference src/light_map.cpp:360-606).  All cube maps are RGBA f32; faces in the OpenGL order
 * +X -X +Y -Y +Z -Z; level l of a cube holds 6 faces of (size >> l)^2 texels and starts
 * 4 * 6 * sum_{k<l} (size >> k)^2 floats into the buffer; rows of a face run along t.
 * Sampling rules (OpenGL leaves them to the implementation; these are ours, shared by the oracle):
 * bilinear within a level, texels beyond a face edge are taken from the face their direction points
 * into (seamless), explicit-LOD fetches blend the two nearest levels linearly, `texture()` without an
 * explicit LOD reads level 0.                                                                     */
typedef struct {
    float* d_env;            /* environment cube, env_levels levels (light_map.cpp:379-430)          */
    float* d_irradiance;     /* diffuse irradiance cube, 1 level      (:455-515)                     */
    float* d_prefilter;      /* GGX-prefiltered cube, pre_levels levels, roughness = l / (levels-1) (:517-573) */
    float* d_brdf_lut;       /* f32 [lut_size][lut_size][2]: scale, bias of F0 (:575-603)             */
    uint32_t env_size, env_levels;   /* reference: 512, 10 */
    uint32_t irr_size;               /* 32  */
    uint32_t pre_size, pre_levels;   /* 128, 5 */
    uint32_t lut_size;               /* 512 */
} slhip_light_map;

/* Mesh pool: structure-of-arrays vertex storage shared by every scene of a batch.
 * Replaces the 68-byte interleaved GL vertex buffer of consolidateMesh
 * (reference src/mesh_tools/consolidate.cpp:53-61).  The 1-based `vertexIndex` attribute of
 * the reference (consolidate.cpp:335) is implicit: vertexIndex = (vertex - vtx_base) + 1.   */
typedef struct {
    const float* d_pos;   /* float4[V]  x y z 1                                   */
    const float* d_nrm;   /* float4[V]  nx ny nz 0                                */
    const float* d_uv;    /* float2[V]                                            */
    const float* d_col;   /* float4[V]  vertex colour (default 1,1,1,1)            */
    const float* d_tan;   /* float4[V]  tangent xyz, bitangent sign (consolidate.cpp:275-279 writes w = 1;
                             missing tangents are computed, compute_tangents.cpp); may be NULL when no
                             draw has a normal texture                                          */
    const uint32_t* d_idx;/* u32[3T]    indices relative to the draw's vtx_base   */
    const uint8_t* d_tex; /* RGBA8 texel pool (all base-colour textures, mip 0)   */
    uint64_t n_vertices;
    uint64_t n_indices;
    uint64_t n_tex_bytes;
    const slhip_light_map* d_light_maps;  /* DEVICE array; may be NULL when no scene uses one */
    uint64_t n_light_maps;
} slhip_mesh_pool;

/* draw flags */
#define SLHIP_DRAW_HAS_BASE_TEX   1u  /* base colour texture bound (render_shader.cpp:430-433)   */
#define SLHIP_DRAW_VERTEX_COLORS  2u  /* mesh carries vertex colours; informational: the reference's
                                         fragment shader never reads the varying (render_shader.vert:86) */
#define SLHIP_DRAW_CASTS_SHADOW   4u  /* Object::castsShadows (render_pass.cpp:437)              */
#define SLHIP_DRAW_ALPHA_TEST     8u  /* texture has an alpha channel: cut-off in the z pass     */
#define SLHIP_DRAW_NO_VERTEX_ID  16u  /* mesh without the vertexIndex attribute (the background
                                         plane): vertex ids read 0 (render_pass.cpp:573-581)     */
/* further material textures of RenderShader::setMaterial (render_shader.cpp:395-415), all RGBA8 in the
 * texel pool with their mip chains, sampled through the sampler of the asset file (see below)          */
#define SLHIP_DRAW_HAS_NORMAL_TEX    32u  /* tangent-space normal map (render_shader.frag:262-266)      */
#define SLHIP_DRAW_HAS_MR_TEX        64u  /* roughness in G, metallic in B (frag:284-288)               */
#define SLHIP_DRAW_HAS_OCCLUSION_TEX 128u /* R scales the image-based lighting term (frag:292-294,393)  */
#define SLHIP_DRAW_HAS_EMISSIVE_TEX  256u /* sRGB, multiplies the emissive factor (frag:296-298)        */
#define SLHIP_DRAW_HAS_STICKER       512u /* projected decal (frag:248-256, object.cpp:494-513)         */

/* Texture sampler state (one byte per texture of a draw).  Every 2D texture is stored with its full mip
 * chain: level l has max(1, w >> l) x max(1, h >> l) texels and follows level l-1 directly; a level is the
 * 2x2 box filter of the previous one, rounded to nearest (glGenerateMipmap leaves the filter to the
 * implementation).  Level of detail per OpenGL 4.5 section 8.14: rho = max(|d(u,v)/dx|, |d(u,v)/dy|) in
 * texels with forward differences of the perspective-correct coordinates to the pixel's +x / +y
 * neighbours, lambda = log2(rho); lambda <= 0 uses the magnification filter on level 0.               */
#define SLHIP_SAMPLER_WRAP_S(m)   ((m) & 3u)          /* 0 repeat, 1 clamp to edge, 2 mirrored repeat */
#define SLHIP_SAMPLER_WRAP_T(m)   (((m) >> 2) & 3u)
#define SLHIP_SAMPLER_MAG_LINEAR  0x10u               /* else nearest */
#define SLHIP_SAMPLER_MIN_LINEAR  0x20u               /* else nearest */
#define SLHIP_SAMPLER_MIP(m)      (((m) >> 6) & 3u)   /* 0 base level only, 1 nearest level, 2 linear between levels */
#define SLHIP_SAMPLER_DEFAULT     (SLHIP_SAMPLER_MAG_LINEAR | SLHIP_SAMPLER_MIN_LINEAR | (2u << 6))   /* repeat, trilinear */

/* One drawable (sub-mesh of an object, or the background plane) of one scene.
 * Carries what RenderShader::setTransformations / setMaterial / setClassIndex /
 * setInstanceIndex upload as uniforms (reference src/shaders/render_shader.cpp:233-265,
 * :326-417) -- normal matrices and camera position are derived on the host exactly there.   */
typedef struct {
    float mesh_to_object[16];
    float object_to_world[16];
    float normal_to_world[12];   /* 3x3 row-major, rows padded to 4 floats */
    float base_color[4];
    float emissive[4];
    float alpha_cutoff, metallic, roughness;
    uint32_t scene;              /* index of the owning scene in the batch            */
    uint32_t class_index, instance_index, flags;
    uint32_t n_verts;            /* vertices of the mesh this draw indexes into       */
    uint32_t vtx_base;           /* first vertex in the pool                          */
    uint32_t idx_base;           /* first index in the pool                           */
    uint32_t n_tris;
    uint32_t prim_base;          /* id of triangle 0 in the scene's draw order        */
    uint32_t tex_offset;         /* byte offset of the RGBA8 base-colour texture      */
    uint32_t tex_w, tex_h;
    uint32_t clip_base;          /* first entry of this draw in the clip-position scratch */
    uint32_t normal_tex_offset, normal_tex_w, normal_tex_h;
    uint32_t mr_tex_offset, mr_tex_w, mr_tex_h;
    uint32_t occlusion_tex_offset, occlusion_tex_w, occlusion_tex_h;
    uint32_t emissive_tex_offset, emissive_tex_w, emissive_tex_h;
    uint32_t sticker_tex_offset, sticker_tex_w, sticker_tex_h;   /* rectangle texture, clamp to edge, row 0 = top of the image */
    uint8_t  tex_sampler[8];     /* SLHIP_SAMPLER_* of the base, normal, metallic-roughness, occlusion, emissive
                                    texture (mesh.cpp:656-663: the file's filters and wrapping, mipmaps generated) */
    uint32_t _pad[3];
    float sticker_projection[16];  /* Object::stickerViewProjection, row-major (object.cpp:494-513)       */
    float sticker_range[4];        /* min.x, min.y, max(1e-6, size.x), max(1e-6, size.y) (render_shader.cpp:426-437) */
} slhip_draw;                    /* 432 bytes */

/* Per-scene camera + lights (reference Scene::setCameraIntrinsics src/scene.cpp:222-253,
 * RenderShader::setManualLighting render_shader.cpp:298-316).                               */
typedef struct {
    float proj[16];
    float world_to_cam[16];
    float cam_position[4];
    float light_dir[SLHIP_NUM_LIGHTS][4];    /* world frame; zero = inactive          */
    float light_color[SLHIP_NUM_LIGHTS][4];
    float shadow_mat[SLHIP_NUM_LIGHTS][16];  /* world -> light clip (render_pass.cpp:131-211) */
    float ambient[4];
    float manual_exposure;                   /* <0: auto exposure (tone_map_shader.frag:110) */
    uint32_t draw_begin, draw_end;           /* range in the draw array               */
    uint32_t n_prims;                        /* total triangles of the scene          */
    uint32_t light_map;                      /* 1 + index into pool->d_light_maps, 0 = none: IBL term
                                                (render_shader.frag:375-394) + sky background
                                                (render_pass.cpp:647-661)                          */
    uint32_t bg_tex[3];                      /* background image (Scene::setBackgroundImage, render_pass.cpp:637-646):
                                                byte offset in the texel pool, width, height; width 0 = none.
                                                A rectangle texture: one level, row 0 = top of the image     */
} slhip_scene;                               /* 480 bytes */

/* A unit of raster work: `count` consecutive triangles of one draw (<= SLHIP_CHUNK_TRIS).
 * Built on the host when the draw list is assembled so that every workgroup has a
 * wave-uniform scene and draw (matrices live in SGPRs).                                    */
#define SLHIP_CHUNK_TRIS 256
typedef struct {
    uint32_t scene, draw, first_tri, count;
} slhip_chunk;

/* output selection mask for slhip_render */
#define SLHIP_OUT_RGB        0x01u
#define SLHIP_OUT_COORD      0x02u   /* objectCoordinates xyz + camera z in w               */
#define SLHIP_OUT_CLASS      0x04u
#define SLHIP_OUT_INSTANCE   0x08u
#define SLHIP_OUT_NORMALS    0x10u
#define SLHIP_OUT_VERTEX_IDX 0x20u
#define SLHIP_OUT_BARY       0x40u
#define SLHIP_OUT_CAM_COORD  0x80u
#define SLHIP_OUT_ALL        0xFFu
#define SLHIP_OUT_GT6        0x1Fu   /* BASELINE "6-channel GT": rgb, coord+depth, class, instance, normals */

#define SLHIP_RENDER_SSAO     0x100u /* RenderPass::ssaoEnabled (render_pass.h:150)          */
#define SLHIP_RENDER_SHADOWS  0x200u /* shadow pass + PCF (render_pass.cpp:408-460)          */
#define SLHIP_RENDER_SHADOW_RESET 0x400u /* d_shadow / d_shadow_tiles hold garbage (first use of the buffers, or a
                                            previous call failed half way): clear all of it first.  Without the flag
                                            the call RELIES on the invariant it maintains: on entry and on exit every
                                            shadow texel is 1.0 and every tile bit 0 -- a render marks the 64x64-texel
                                            tiles its casters may touch and resets exactly those after shading, instead
                                            of clearing 16.8 MB per scene and light on every call                     */
#define SLHIP_RENDER_KEEP_HDR 0x800u /* with SLHIP_RENDER_SSAO: also store the float image the tone map consumes (AO applied) in the
                                        second half of scratch d_hdr -- the fused apply + tone-map pass otherwise never writes it */

/* Result buffers, batch-major [B][H][W][C] -- the 8 colour attachments of
 * RenderPass::Result (reference include/stillleben/render_pass.h:48-78, formats
 * src/render_pass.cpp:347-365).  A NULL pointer == output not wanted.                       */
typedef struct {
    uint8_t*  d_rgb;          /* u8  [B,H,W,4]   tone-mapped, linear (tone_map_shader.frag:129-130) */
    float*    d_coord;        /* f32 [B,H,W,4]   object xyz, camera z                        */
    uint16_t* d_class;        /* u16 [B,H,W]                                                 */
    uint16_t* d_instance;     /* u16 [B,H,W]                                                 */
    float*    d_normals;      /* f32 [B,H,W,4]   camera-frame normal, w = n.v                */
    uint32_t* d_vertex_idx;   /* u32 [B,H,W,4]   1-based ids, 4th = 0                        */
    float*    d_bary;         /* f32 [B,H,W,4]   4th = 0                                     */
    float*    d_cam_coord;    /* f32 [B,H,W,4]   camera xyz, 1                               */
} slhip_render_out;

/* Scratch the caller provides (sizes from slhip_render_scratch_bytes).                      */
typedef struct {
    uint64_t* d_vis;          /* u64 [B,H,W] visibility keys (depth24<<32 | prim id)         */
    float*    d_hdr;          /* f32 [B,H,W,4] HDR colour (ssaoRGBInput / postprocessInput)  */
    float*    d_ao;           /* f32 [B,H,W] occlusion + f32 [B,H+2,W+2] camera-z plane + per 8 x 8 tile a
                                 float2 record and a skip byte (SSAO; slhip_render_scratch_bytes sizes it) */
    float*    d_shadow;       /* f32 [B,NUM_LIGHTS,S,S] shadow depth (only active lights)    */
    uint32_t* d_queue;        /* large-triangle work queue, 16-byte aligned: a 16-byte header ([0] entries, [1] the
                                 8 x 8 tiles of their pixel boxes), then one 32-byte entry per queued triangle   */
    float*    d_lum;          /* f32 [B,4] HDR sums for auto exposure                        */
    float*    d_clip;         /* f32 [1 + NUM_LIGHTS][n_clip_verts][4]: clip positions written by the
                                 MFMA vertex-transform kernel (plane 0: camera, 1..3: lights)  */
    uint32_t* d_shadow_tiles; /* u32 [B][NUM_LIGHTS][ceil(ceil(S/64)^2 / 32)]: touched-tile bits (see
                                 SLHIP_RENDER_SHADOW_RESET)                                     */
    uint32_t  queue_capacity; /* 16-byte units of d_queue behind its header (an entry takes two); triangles
                                 beyond it are rasterised by one thread each: the same picture, slowly          */
    uint32_t  shadow_res;     /* S (reference: 2048, render_pass.cpp:271)                    */
    uint32_t  n_clip_verts;   /* sum of n_verts over the draws of the batch                  */
    uint32_t  shadow_lights;  /* light maps per scene in d_shadow: 0 = SLHIP_NUM_LIGHTS; 1 or 2 = d_shadow is
                                 [B, shadow_lights, S, S] (lights beyond the count cast no shadow)  */
    float*    d_vattr;        /* n_clip_verts x 80 B, 64-byte aligned: the rest of the vertex stage
                                 (render_shader.vert:57-95) once per vertex -- [n_clip_verts] records of 64 B: (object xyz,
                                 camera z), (world xyz, camera x), (world normal, camera y), window coordinates (x, y in
                                 1/256 px as i32, depth, 1/w; x = INT_MIN behind the near plane) -- followed by the window
                                 coordinates once more as a dense [n_clip_verts] x 16 B plane.  (The light planes of d_clip
                                 end up holding window coordinates of the shadow map instead of clip positions.)        */
} slhip_render_scratch;

/* Renders a batch of scenes.  Replaces RenderPass::render (src/render_pass.cpp:303-796):
 * shadow pass, main G-buffer pass, SSAO, tone map.  d_depth_peel (f32 [B,H,W,4], the
 * previous result's objectCoordinates; NULL = none) implements `depthBufferResult`.         */
int slhip_render(const slhip_mesh_pool* pool,
                 const slhip_scene* d_scenes, const slhip_draw* d_draws,
                 const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_draws, uint32_t n_chunks,
                 uint32_t width, uint32_t height, uint32_t flags,
                 const float* d_depth_peel,
                 const slhip_render_out* out, const slhip_render_scratch* scratch,
                 void* stream);

/* Optional per-phase timing of slhip_render with HIP events recorded on the render stream
 * (used by bench.py for the roofline figures).  Phases: 0 shadow raster, 1 shadow large
 * triangles, 2 visibility raster, 3 large triangles, 4 deferred shade, 5 SSAO, 6 SSAO apply,
 * 7 tone map.  slhip_render_timings synchronises on the last render and fills ms_out[8].    */
int slhip_timing_enable(int on);
int slhip_render_timings(float* ms_out);
/* The SSAO pass runs its 64 taps only where something can occlude: on the open background plane (every texel a tap can reach
 * belongs to the plane or to the cleared background, no tap leaves the image) the occlusion is 1 exactly, and whole 8 x 8 tiles are
 * written without the loop (viewports that are multiples of 32 x 16; slhip_render.hip k_ssao_mask).  This read-out of the last
 * slhip_render on `scratch` (same n_scenes, width, height) returns counts[0] = tiles, counts[1] = tiles skipped; synchronises.  */
int slhip_render_ssao_skipped(const slhip_render_scratch* scratch, uint32_t n_scenes, uint32_t width, uint32_t height,
                              uint64_t counts[2], void* stream);
/* ... and sample by sample: a plane tile near an object still leaves out the taps whose sample vectors are too short to reach it.
 * A tile has a LEVEL: 0 = no taps (the tiles counted as skipped above, which are clear at the full radius, and some more),
 * j = only the samples with 1.001 |s_k| > rho_j run (compacted lists in ascending k, nested, so the occlusion sum keeps its
 * bits), 5 = all 64.  slhip_render_ssao_level_tables returns the thresholds rho[5], the list lengths
 * counts[6] and the lists taps[6 * 64] (list j at taps + 64 j), no GPU needed.  slhip_render_ssao_levels reads the last slhip_render
 * on `scratch` (same n_scenes, width, height): counts[0..5] = tiles per level, counts[6] = the end-of-band runs of the tap
 * kernel, counts[7] = those of them that held pixels of more than one level; synchronises.  Environment, read at every
 * slhip_render: SLHIP_SSAO_DEBUG=2 runs every tile at the full list, =3 keeps the levels and counts the end-of-band runs (they
 * are zero otherwise); SLHIP_SSAO_BAND_ROWS = rows per band of the tap kernel (a multiple of 16, default 16; placement only);
 * SLHIP_SSAO_POOL=0: every wave of the tap kernel drains its own queues at the end of a band, instead of the four waves of a block
 * draining theirs as one list (the same bits).  slhip_render_ssao_run_slots, also counted under SLHIP_SSAO_DEBUG=3 only: slots[0] = full runs of the tap
 * kernel, slots[1] = the tap lane-slots they issued (taps of the list x 64), slots[2] = the tap lane-slots the end-of-band runs
 * issued, slots[3] = those their pixels needed (each running lane's own list); synchronises.  */
int slhip_render_ssao_level_tables(float rho[5], uint32_t counts[6], uint8_t taps[384]);
int slhip_render_ssao_levels(const slhip_render_scratch* scratch, uint32_t n_scenes, uint32_t width, uint32_t height,
                             uint64_t counts[8], void* stream);
int slhip_render_ssao_run_slots(const slhip_render_scratch* scratch, uint32_t n_scenes, uint32_t width, uint32_t height,
                                uint64_t slots[4], void* stream);

/* Bytes of each scratch buffer for a batch (host helper, no GPU needed).  `hdr` is sized for TWO float4 planes per scene: plane 0
 * = the fragment shader's linear colour (always written when rgb is asked for), plane 1 = the same after ambient occlusion, the
 * image the tone map consumes -- written ONLY under SLHIP_RENDER_KEEP_HDR (the fused blur + tone-map pass does not materialise it
 * otherwise; a caller that does not keep it may pass half the size).  Colour parity bar of the path (tests/test_gpu_render.py): the
 * float image within 1e-3 relative of the CPU restatement; the 8-bit rgb within 1 LSB on all but 1e-4 of the values, never more
 * than 2 (the tone map's divisions and the blur's exponentials go through the hardware's rcp / exp2).                          */
int slhip_render_scratch_bytes(uint32_t n_scenes, uint32_t width, uint32_t height,
                               uint32_t shadow_res, uint32_t queue_capacity,
                               uint64_t bytes_out[7]);   /* vis, hdr, ao, shadow, queue, lum, shadow_tiles */

/* Per-object visibility statistics of a render: for every scene and slot, the numbers of the BOP toolkit's scene_gt_info.
 * Slot i is instance index i (instance_index & 0xFFFF, what the instance output shows; draws that share an index share a slot);
 * slot 0 -- the background plane and other unindexed draws -- is always empty, as is a slot without draws.
 *   px_visib, bbox_visib: the pixels whose instance output is i, and their box;
 *   px_all, bbox_obj:     the pixels the visibility pass covers with slot i's draws drawn alone (no other draw, no plane; same
 *                         viewport, camera, fill rule, near clipping, depth-range rules and alpha test), and their box.
 * Boxes are (x, y, w, h) with (x, y) the top-left pixel; an empty box is (-1, -1, -1, -1).  All values are integers computed with
 * integer atomics: bit-exact and the same from run to run.  visib_fract = px_visib / px_all (0 when px_all == 0) is left to
 * the caller.  40 bytes. */
typedef struct {
    uint32_t px_visib, px_all;
    int32_t  bbox_visib[4];
    int32_t  bbox_obj[4];
} slhip_object_stats;

#define SLHIP_OBJECT_STATS_CAPACITY 1   /* status of slhip_render_object_stats: the word pool is too small (see below) */

/* Worst-case size of the word pool of slhip_render_object_stats: one u64 word per 8 x 8-pixel tile of the viewport for every
 * scene and slot 1..n_slots-1, n_scenes * (n_slots - 1) * ceil(W / 8) * ceil(H / 8).  A call needs one word per tile of each
 * slot's screen box only (the box of its vertices; the whole viewport for a slot with a vertex behind the near plane), usually
 * far less.  Host only.                                                                                                        */
int slhip_render_object_stats_bytes(uint32_t n_scenes, uint32_t n_slots, uint32_t width, uint32_t height,
                                    uint64_t* worst_case_words);

/* Statistics of the slhip_render that preceded this call on the same stream.  pool, d_scenes, d_draws, d_chunks, n_scenes,
 * n_draws, n_chunks, width and height are the arguments that render consumed, and `scratch` its scratch: the visibility keys
 * (d_vis), the vertex caches (d_clip, d_vattr) are read, the queue (d_queue, queue_capacity) is reused.  PRECONDITION: nothing
 * touches that scratch between the two calls.  A render with a depth-peel input has no single "whole silhouette": its
 * statistics describe the unpeeled draws, and callers should not ask for them.
 *   n_slots   slots per scene (the largest instance index of the batch + 1; draws with a larger index are not counted)
 *   d_words   u64 working pool of capacity_words words (device)
 *   d_out     slhip_object_stats [n_scenes][n_slots] (device); also the working space of the call
 *   words_needed  (host, may be NULL) the words this batch needs
 * Returns 0, SLHIP_OBJECT_STATS_CAPACITY when capacity_words < *words_needed (no statistics are written; d_out holds working
 * values; grow the pool and call again -- the render's outputs stay valid), or a negative error (slhip_last_error).
 * Synchronises `stream` once (the pool size is known after the first pass).                                                    */
int slhip_render_object_stats(const slhip_mesh_pool* pool,
                              const slhip_scene* d_scenes, const slhip_draw* d_draws,
                              const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_draws, uint32_t n_chunks,
                              uint32_t width, uint32_t height, const slhip_render_scratch* scratch,
                              uint32_t n_slots, uint64_t* d_words, uint64_t capacity_words,
                              slhip_object_stats* d_out, uint64_t* words_needed, void* stream);

/* Per-object masks of a render (slhip_render_object_masks): of every (scene, slot) the whole silhouette (kind 0: the pixels
 * px_all counts, BOP's mask/) and the visible part (kind 1: the pixels px_visib counts, BOP's mask_visib/), in two forms --
 *   bit tiles: one u64 word per 8 x 8-pixel tile of the slot's tile box (the box of slhip_render_object_stats' working pool),
 *              for slhip_object_masks_expand or a kernel of the caller's;
 *   run lengths: the uncompressed RLE of COCO / the BOP toolkit's scene_gt_coco.json, {"counts": [...], "size": [H, W]}:
 *              the mask read column by column (pixel (x, y) at position x * H + y), lengths of zeros and ones in turn, zeros
 *              first (a first length of 0 when pixel (0, 0) is set), summing to W * H; an empty mask is the single length W * H.
 * Record per (scene, slot), device, [n_scenes][n_slots].  56 bytes.  A slot whose whole silhouette is empty (unused, outside
 * the picture, behind the camera) has no tiles. */
typedef struct {
    int32_t  tile_box[4];     /* tx0, ty0, tx1, ty1 in 8x8 tiles; tx0 > tx1: the slot has no tiles            */
    uint64_t word_offset[2];  /* first u64 word of kind 0 (whole silhouette) and 1 (visible) in d_words;
                                 row-major over the tile box, bit (y & 7) * 8 + (x & 7) = pixel (x, y)         */
    uint64_t rle_offset[2];   /* first u32 run length of each kind in d_runs                                   */
    uint32_t rle_count[2];    /* number of run lengths of each kind                                           */
} slhip_object_mask;

#define SLHIP_OBJECT_MASKS_CAPACITY 2   /* status of slhip_render_object_masks: the word pool or the run pool is too small */

/* Worst-case sizes of the two pools of slhip_render_object_masks.  Words: both kinds of every slot 1..n_slots-1 over the whole
 * viewport, twice slhip_render_object_stats_bytes.  Run lengths: W * H + 1 per mask of a slot 1..n_slots-1 (a mask that
 * changes at every pixel) and 1 per mask of slot 0.  Real use is FAR below both: words follow the objects' screen boxes, and
 * a mask of a convex shape has about two run lengths per image column it covers -- start from a modest size and let the
 * capacity status grow the pools rather than allocating these.  Host only.                                                  */
int slhip_render_object_masks_bytes(uint32_t n_scenes, uint32_t n_slots, uint32_t width, uint32_t height,
                                    uint64_t* worst_words, uint64_t* worst_runs);

/* slhip_render_object_stats plus the masks: the same arguments, precondition and statistics (d_out is filled bit for bit as
 * by that call), and
 *   d_words   holds both kinds, so it needs twice the words the statistics call reports; the words stay valid after the call
 *   d_masks   slhip_object_mask [n_scenes][n_slots] (device)
 *   d_runs    u32 pool of capacity_runs run lengths (device)
 *   words_needed, runs_needed  (host, may be NULL) what this batch needs, as far as the call got to know it
 * Returns 0, SLHIP_OBJECT_MASKS_CAPACITY when either pool is too small (no partial result is promised; grow the pools and call
 * again -- the render's outputs stay valid), or a negative error (slhip_last_error).  width * height must be below 2^31.
 * Synchronises `stream` twice: after the tile scan and after the run count.                                                 */
int slhip_render_object_masks(const slhip_mesh_pool* pool,
                              const slhip_scene* d_scenes, const slhip_draw* d_draws,
                              const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_draws, uint32_t n_chunks,
                              uint32_t width, uint32_t height, const slhip_render_scratch* scratch,
                              uint32_t n_slots, uint64_t* d_words, uint64_t capacity_words,
                              slhip_object_stats* d_out, uint64_t* words_needed,
                              slhip_object_mask* d_masks, uint32_t* d_runs, uint64_t capacity_runs, uint64_t* runs_needed,
                              void* stream);

/* Bit tiles to dense masks.  d_select holds n_select pairs (scene, slot) as u32 (device); d_dense is uint8
 * [n_select][height][width] with values 0 / 1 (device).  Every byte is written: pixels outside the slot's tile box, of an empty
 * slot or of a pair outside [n_scenes][n_slots] are 0.  kind: 0 the whole silhouette, 1 the visible part.  Returns 0 or a
 * negative error (null pointers, zero sizes and kind > 1 are rejected before anything touches the device).                  */
int slhip_object_masks_expand(const slhip_object_mask* d_masks, const uint64_t* d_words, uint32_t n_scenes, uint32_t n_slots,
                              uint32_t width, uint32_t height, uint32_t kind, const uint32_t* d_select, uint64_t n_select,
                              uint8_t* d_dense, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Settle half (replaces PhysX as driven by Scene::simulateTableTopScene, scene.cpp:612-759)
 * ------------------------------------------------------------------------------------------- */

/* Convex collision shape: a vertex cloud in the OBJECT frame (mesh pretransform incl. scale
 * already applied -- the counterpart of PxConvexMeshGeometry + PxMeshScale + shape local pose,
 * reference src/object.cpp:173-204).  <= 64 vertices (VHACD.h:235).                          */
#define SLHIP_MAX_HULL_VERTS 64
typedef struct {
    uint32_t vtx_begin;      /* first vertex in the hull vertex pool (float4 each)            */
    uint32_t vtx_count;
    uint32_t _pad[2];
    float sphere[4];         /* bounding sphere: centre (object frame), radius                */
    float aabb_center[4];    /* object-frame AABB (broadphase: |R| * half is its world box)   */
    float aabb_half[4];
} slhip_hull;                /* 64 bytes */

#define SLHIP_BODY_STATIC   1u   /* Object::isStatic -> eKINEMATIC (object.cpp:515-520)       */
#define SLHIP_BODY_ASLEEP   2u
#define SLHIP_BODY_FROZEN   4u   /* out: held in place by the stabilisation this step (PxSceneFlag::eENABLE_STABILIZATION) */

/* Rigid body state.  `pose` is the object pose exactly as sl.Object.pose() returns it.       */
typedef struct {
    float pose[16];
    float lin_vel[4];        /* velocity of the centre of mass, world frame                   */
    float ang_vel[4];
    float com[4];            /* centre of mass, object frame                                  */
    float inv_inertia[12];   /* inverse inertia about the COM in object axes, 3 rows padded   */
    float inv_mass;          /* 0 for static bodies                                           */
    float mu_s, mu_d, restitution;    /* material (context.cpp:250-252 / object.cpp:565-605)  */
    float bsphere[4];        /* bounding sphere of all hulls (object frame centre, radius)    */
    float bbox_center[4];    /* mesh bbox centre (object frame); w = bbox diagonal / 2        */
    float max_lin_vel;       /* Object::setLinearVelocityLimit (object.cpp:259-264)           */
    float separation;        /* out: min contact separation of the last step (scene.cpp:73-116) */
    float wake_counter;
    uint32_t flags;
    uint32_t hull_begin, hull_end;
    int32_t stuck_counter;
    uint32_t drive_flags;    /* bit 0: linear spring drive enabled; bits 1..3: rotation about the
                                joint x/y/z axis locked (ManipulationSim, manipulation_sim.cpp:28-93) */
    float drive_target[4];   /* world position the object origin is driven to                 */
    float drive_frame[4];    /* joint frame orientation (quaternion x y z w) = initial pose   */
    float drive_params[4];   /* stiffness, damping, force limit (manipulation_sim.cpp:52-55), unused */
    float stab[4];           /* state of the stabilisation (slhip_settle_params.stabilization_threshold), 0 in a fresh record:
                                [0] seconds the body has spent below its threshold (PhysX: PXD_FREEZE_INTERVAL - PxsRigidBody::freezeCount [ext]),
                                [1] 1 - the share of gravity the body feels (PhysX: 1 - accelScale [ext]), [2], [3] unused      */
} slhip_body;                /* 304 bytes */

/* One scene of the settle batch: bodies [body_begin, body_end).                              */
typedef struct {
    uint32_t body_begin, body_end;
    uint32_t has_plane;      /* 1: static table box, top face at z = plane_z (scene.cpp:629-663) */
    float plane_z;
} slhip_settle_scene;

/* Constants of the step (defaults == the reference's call sites).   */
typedef struct {
    float dt;                    /* 0.01  = 1/25/4  (scene.cpp:681-684)                      */
    uint32_t substeps;           /* 4                                                         */
    uint32_t frames;             /* 100   (scene.cpp:720)                                     */
    uint32_t pos_iters, vel_iters; /* 4, 4 (object.cpp:209)                                  */
    float gravity[3];            /* 0,0,-9.81 (scene.cpp:157,665)                             */
    float contact_offset;        /* 0.004 = 0.02 * tolerance length 0.2 [ext]                 */
    float rest_offset;           /* 0.0015 (object.cpp:201); the plane box has 0              */
    float bounce_threshold;      /* 2.0   = 0.2 * tolerance speed 10 [ext]                    */
    float sleep_threshold;       /* 5e-3  = 5e-5 * speed^2 [ext]                              */
    float wake_time;             /* 0.4 s [ext]                                               */
    float angular_damping;       /* 0.05 [ext]                                                */
    float max_angular_velocity;  /* 100 rad/s [ext]                                           */
    float plane_mu_s, plane_mu_d, plane_restitution; /* 0.5, 0.5, 0 (scene.cpp:645)          */
    float redrop_z;              /* -0.5 (scene.cpp:746)                                      */
    float stuck_separation;      /* -0.01 (scene.cpp:748)                                     */
    int32_t stuck_frames;        /* 10 = 0.4 s * 25 FPS (scene.cpp:750)                       */
    uint32_t tabletop;           /* 1: run the redrop logic of simulateTableTopScene          */
    /* LDS sizing hints for the kernel (0 = worst case / hull vertices stay in global memory):
       maxima over the scenes of the batch.  A scene that exceeds a non-zero hint (or has more
       than 1024 hulls in one body) is left untouched by the launch -- the kernel never writes
       outside the layout the hints sized.                                                     */
    uint32_t max_bodies_per_scene;
    uint32_t max_hull_verts_per_scene;   /* sum over a scene's bodies of their hull vertices  */
    uint32_t max_hulls_per_scene;
    /* Capacities of a scene's per-step lists in the scratch (PhysX allocates as it goes, scene.cpp:738-739; here the caller sizes
       the scratch): candidate hull pairs the broadphase may file, contacts the solver may take.  0 = SLHIP_DEFAULT_HULL_PAIRS /
       SLHIP_DEFAULT_CONTACTS (on the 20-object YCB-like workload: p99.99 of the pairs 1 000, most ever seen 1 551; contacts 477).
       What a step offers beyond a capacity is dropped in list order AND COUNTED (slhip_settle_caps): a caller that finds a
       non-zero count settles again with larger capacities -- nothing is ever dropped silently.                                */
    uint32_t max_hull_pairs_per_scene;
    uint32_t max_contacts_per_scene;
    /* Compound manifold reduction (NOT in the reference: PhysX hands every convex pair's manifold to the solver).  0: the solver takes
       every point.  B >= 16: a body pair that touches through more than B hull pairs -- nested concave shapes: a mug in a bowl offers
       several hundred one-point manifolds, one Gauss-Seidel chain of that length -- keeps the B hull pairs with the deepest points
       (ties: list order); the others stay filed as manifolds (no impulse) and return when they are among the deepest.  Counted per
       (scene, step) by slhip_settle_caps.  On the 20-object workload a budget of 32 or 64 leaves the share of bodies at rest, the redrops
       and the deepest penetrations where they are without it.  Every host path of this repository passes 0.   */
    uint32_t pair_contact_budget;
    /* 0: the call starts from a cold contact state (it initialises the scratch).  N > 0: the call CONTINUES the N steps that earlier
       calls ran on the same d_scratch with the same scenes, bodies (same order, same hulls) and sizing hints -- the state PhysX
       keeps for the life of a PxScene (pair cache, persistent manifolds and their impulses, table contacts; scene.cpp:720-739,
       903-912, manipulation_sim.cpp:83-93) is taken from the scratch as the last call left it, d_bodies carries poses, velocities,
       wake counters and sleep flags.  k calls of one step give bit for bit what one call of k steps gives.                      */
    uint32_t resume;
    /* Capacity of a scene's list of touching BODY pairs (one solver group each, beside one group per body against the table).
       0: min(all body pairs, max_hull_pairs_per_scene, 12 x bodies + 64) -- enough for piles, where a body has a handful of
       neighbours.  A body pair beyond the capacity is dropped with its hull pairs AND COUNTED (slhip_settle_caps counts[8]):
       the caller settles again with a larger value, like for the other two lists.                                          */
    uint32_t max_body_pairs_per_scene;
    /* PxSceneFlag::eENABLE_STABILIZATION (scene.cpp:163).  The per-body stabilisation threshold, PhysX default 1e-5 * tolerance speed^2
       = 1e-3 with context.cpp:236-238's speed of 10 [ext].  A body in an island that rests on something static, whose frame energy
       (mass-normalised, from the velocities that moved it this step) is below min(10, touching body pairs) x threshold: both velocities
       are scaled by 1 - SLHIP_STAB_DAMPING dt, the share of gravity it feels goes to SLHIP_STAB_GRAVITY by a quarter of the
       distance per step (and back up by dt per step); after SLHIP_STAB_FREEZE_INTERVAL s of that, below
       SLHIP_STAB_FREEZE_TOLERANCE x threshold, it is frozen: the step's pose change is taken back (SLHIP_BODY_FROZEN).  0: off. */
    float stabilization_threshold;
    uint32_t _pad_params;
} slhip_settle_params;           /* 128 bytes */
#define SLHIP_STAB_DAMPING          0.5f   /* PXD_SLEEP_DAMPING [ext]   */
#define SLHIP_STAB_GRAVITY          0.9f   /* PXD_FREEZE_SCALE [ext]    */
#define SLHIP_STAB_FREEZE_INTERVAL  1.5f   /* PXD_FREEZE_INTERVAL [ext] */
#define SLHIP_STAB_FREEZE_TOLERANCE 0.25f  /* PXD_FREEZE_TOLERANCE [ext] */
#define SLHIP_STAB_MAX_INTERACTIONS 10

/* per-scene scratch (device), sized by slhip_settle_scratch_bytes */
#define SLHIP_MAX_BODIES     400  /* bodies per scene (the kernels keep a scene's working bodies in LDS: 152 B each -- and its body-
                                     pair groups: above ~300 bodies set max_body_pairs_per_scene so that both fit the 160 KB)       */
#define SLHIP_DEFAULT_HULL_PAIRS 2048 /* slhip_settle_params.max_hull_pairs_per_scene = 0 (at most 65535)                  */
#define SLHIP_DEFAULT_CONTACTS   1024 /* slhip_settle_params.max_contacts_per_scene = 0 (at most 65535)                    */
#define SLHIP_PAIR_CACHE_DENSE_HULLS 256 /* up to this many convex hulls per scene the pair cache (cached simplex + the way to the
                                          pair's persistent manifold) is a dense [hulls]^2 table, beyond it an open-addressing hash
                                          table keyed by the hull pair -- same contents, same results                         */

/* Steps every scene of the batch `frames * substeps` times without a host round trip -- a short sequence of kernel launches per
 * step over the whole batch (broadphase; GJK / portal refinement per hull pair; the face manifold of NEW contact pairs and of those that lost a point; persistent
 * manifolds, contact list and colouring; the warm-started 4 + 4 Gauss-Seidel sweeps, integration, sleeping), including the redrop
 * heuristic when params->tabletop.  Batches of up to 2048 scenes take ONE launch instead, in which a wave carries a scene through
 * all its steps (the same per-scene and per-pair functions: the results are the same bits; environment SLHIP_SETTLE_PERSISTENT=0/1
 * forces a form; the per-kernel timings below exist for the lockstep form only).  State that PhysX keeps from step to step lives in the scratch: the cached simplex, the
 * persistent contact manifold and its impulses per hull pair, the table contacts per body -- and stays valid after the call:
 * a later call with params->resume = (steps run so far) continues from it (Scene::simulate, ManipulationSim::step and the
 * frames of simulateTableTopScene with a visualisation callback step ONE long-lived PxScene in the reference).
 * d_bodies is updated in place (pose, velocities, separation).  Replaces the hot loop of
 * Scene::simulateTableTopScene (scene.cpp:720-756) and, with frames=substeps=1 and
 * tabletop=0, Scene::simulate(dt) (scene.cpp:903-912).                                       */
int slhip_settle(const slhip_settle_scene* d_scenes, uint32_t n_scenes,
                 slhip_body* d_bodies, const slhip_hull* d_hulls, const float* d_hull_verts,
                 const slhip_settle_params* params, void* d_scratch, uint64_t scratch_bytes,
                 void* stream);
/* Per-scene outcome of the last slhip_settle that used `d_scratch` (synchronises `stream`): h_status[i]
 * (may be NULL) = 0 when scene i was stepped, SLHIP_SETTLE_REFUSED_* when the kernel left it untouched
 * because it exceeds the sizing hints; *h_n_refused counts those.  Returns -2 (and sets the error
 * message) when any scene was refused -- a wrong hint must never pass silently.                       */
#define SLHIP_SETTLE_REFUSED_BODIES 1u   /* more bodies than max_bodies_per_scene (or than SLHIP_MAX_BODIES) */
#define SLHIP_SETTLE_REFUSED_HULLS  2u   /* more hulls than max_hulls_per_scene, or > 1024 in one body */
/* (below) What the capacities cost since the last cold start on `d_scratch` (synchronises `stream`; same `params` as those calls).
 * counts[0] (scene, step) pairs whose contacts went beyond what the scene's solver wave holds in LDS (swept from global
 * memory, nothing lost), [1] (scene, step) pairs in which contacts beyond max_contacts_per_scene were DROPPED, [2] (scene, step)
 * pairs in which hull pairs beyond max_hull_pairs_per_scene were DROPPED, [3] scenes with a non-zero [1] or [2], [4] scenes whose
 * contacts ever went beyond the LDS-resident part, [5] the most contacts and [6] the most hull pairs a step of any scene offered,
 * [7] (scene, step) pairs in which pair_contact_budget reduced some body pair's points, [8] (scene, step) pairs in which body
 * pairs beyond max_body_pairs_per_scene were DROPPED (such scenes count in [3] too), [9] the contacts the solver took, summed over
 * all (scene, step) pairs (bench.py's byte model: contacts per scene-step).
 * The reference has no caps (scene.cpp:738-739): [1] = [2] = [8] = 0 is the contract, a caller that sees otherwise re-sizes.     */
int slhip_settle_caps(const void* d_scratch, uint32_t n_scenes, const slhip_settle_params* params,
                      uint64_t counts[10], void* stream);
int slhip_settle_status(const void* d_scratch, uint32_t n_scenes, uint32_t* h_status, uint32_t* h_n_refused,
                        void* stream);
/* Optional live timing of the phases of a lockstep step (bench.py's roofline leg): HIP events on the launch's stream
 * around every phase of every 8th step.  slhip_settle_timings synchronises the recorded events and returns, since the last
 * call, the average duration [ms] and the number of timed launches of 0 k_w_begin (integrate, table contacts, broadphase),
 * 1 k_w_gjk_first + k_w_gjk_rest (the two passes of the main GJK), 2 k_w_manifold (face manifolds), 3 k_w_finish (contact list, groups, prep,
 * colouring, cost class), 4 k_w_solve.                                                                                  */
int slhip_settle_timing_enable(int on);
int slhip_settle_timings(float avg_ms_out[5], uint32_t launches_out[5]);
/* The same records step by step (profiles/rNN/solve_by_step.csv): slhip_settle_timing_every(k) times every k-th step (default 8);
 * slhip_settle_timings_by_step synchronises the recorded events and writes, for up to `capacity` timed steps since the last read-out,
 * ms_out[5 * i + kernel] and steps_out[i] (may be NULL) = the step's index within its settle call; *n_out = rows written.          */
int slhip_settle_timing_every(uint32_t every);
int slhip_settle_timings_by_step(float* ms_out, uint32_t* steps_out, uint32_t capacity, uint32_t* n_out);
/* LDS bytes a solver wave (k_w_solve) of the last slhip_settle call was launched with: 20 KB, more when the batch's largest scene
 * shape needs it, SLHIP_SOLVE_LDS_KB overrides (measurement read-out: bench.py states the configuration it measured).             */
int slhip_settle_solver_wave_lds(void);
/* scratch for n_scenes scenes: accumulators + the per-scene pair cache, sized from the hints in
 * `params` (NULL or zero hints: the worst case)                                                      */
int slhip_settle_scratch_bytes(uint32_t n_scenes, const slhip_settle_params* params, uint64_t* bytes_out);

/* Boolean any-overlap query per body against all OTHER bodies of its scene (and the plane if
 * present): d_flags[body] = 1 if it collides.  Replaces Scene::isObjectColliding /
 * checkCollisions (scene.cpp:355-385, :914-925).                                             */
int slhip_overlap_any(const slhip_settle_scene* d_scenes, uint32_t n_scenes,
                      const slhip_body* d_bodies, const slhip_hull* d_hulls,
                      const float* d_hull_verts, uint8_t* d_flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * sl.diff half (replaces python/src/diff.cu + bridge_diff.cpp and fuses diff.py:355-523)
 * ------------------------------------------------------------------------------------------- */

/* Every entry of this half returns -1 with an error text, before any launch, for H <= 0, W <= 0 or H * W > 0x7fffffff
 * (pixels are indexed with int), and the pose backward for more than 256 objects (its accumulators live in LDS).   */

/* generate_sobel_valid_mask (bridge_diff.cpp:13-69, CPU-loop semantics: the 1-px border stays
 * valid).  d_inst i16[H,W]; d_depth f32 with `depth_stride` floats between pixels (1 for a
 * dense [H,W] image, 4 to read channel 3 of the coordinate target in place); d_valid u8[H,W].  */
int slhip_diff_sobel_valid(const int16_t* d_inst, const float* d_depth, int depth_stride, int H, int W,
                           uint8_t* d_valid, void* stream);

/* dilate_object_mask (bridge_diff.cpp:71-157).  d_coords f32 xyz with `coord_stride` floats
 * between pixels (3 or 4); outputs u8[H,W] and f32[H,W,3]; the 1-px border reads 0.            */
int slhip_diff_dilate(const uint8_t* d_mask, const uint8_t* d_valid, const float* d_coords, int coord_stride,
                      int H, int W, uint8_t* d_out_mask, float* d_out_coords, void* stream);

/* compute_image_space_gradients (diff.py:73-127): d_rgb u8[H,W,4] -> grad_x, grad_y f32[3,H,W],
 * zero where !valid.                                                                           */
int slhip_diff_image_gradients(const uint8_t* d_rgb, const uint8_t* d_valid, int H, int W, float* d_grad_x,
                               float* d_grad_y, void* stream);

/* backpropagate_gradient_to_poses (diff.py:355-523), fused.  d_coord f32[H,W,4] (object xyz,
 * depth), d_inst i16[H,W], d_grad_img f32[3,H,W], h_proj HOST float[16] (row-major projection),
 * d_poses f32[n_obj,16], d_obj_inst i32[n_obj]; scratch d_valid u8[H,W], d_acc f64[n_obj*6];
 * d_out f32[n_obj,6].                                                                          */
int slhip_diff_pose_backward(const uint8_t* d_rgb, const float* d_coord, const int16_t* d_inst,
                             const float* d_grad_img, const float* h_proj, const float* d_poses,
                             const int32_t* d_obj_inst, int n_obj, int H, int W, uint8_t* d_valid,
                             double* d_acc, float* d_out, void* stream);
/* The same for K pose hypotheses of one scene in ONE launch sequence (BASELINE config C5): d_rgb / d_coord / d_inst are the
 * [K,H,W,..] targets of the hypotheses' renders, d_poses f32 [K,n_obj,16], d_grad_img one image for all (grad_stride_floats
 * = 0) or one per hypothesis (= 3 * H * W); scratch d_valid u8 [K,H,W], d_acc f64 [K,n_obj,6]; d_out f32 [K,n_obj,6].
 * The reference loops hypothesis by hypothesis through its renderer and python/stillleben/diff.py:355-523.       */
int slhip_diff_pose_backward_batch(const uint8_t* d_rgb, const float* d_coord, const int16_t* d_inst,
                                   const float* d_grad_img, uint64_t grad_stride_floats, const float* h_proj,
                                   const float* d_poses, const int32_t* d_obj_inst, int n_obj, int n_hyp, int H, int W,
                                   uint8_t* d_valid, double* d_acc, float* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image-based lighting precompute (replaces LightMap::load's GL passes, light_map.cpp:360-606, and
 * src/shaders/cubemap_shader_{equirectangular,irradiance,prefilter}.frag, brdf_shader.frag)
 * ------------------------------------------------------------------------------------------- */
/* floats needed for the four buffers of a light map with the given sizes: out[0..3] = env,
 * irradiance, prefilter, BRDF LUT                                                              */
int slhip_light_map_floats(uint32_t env_size, uint32_t env_levels, uint32_t irr_size, uint32_t pre_size,
                           uint32_t pre_levels, uint32_t lut_size, uint64_t out[4]);
/* d_equirect: f32 [H][W][3] equirectangular radiance, row 0 = top (+z up, azimuth atan2(y, x) along
 * the row); fills every buffer of *lm (a HOST struct holding DEVICE pointers).  The image is read
 * bilinearly at u = atan2(y, x) * 0.1591 + 0.5, w = asin(z) * 0.3183 + 0.5 (w = 1: top row) and clamped
 * to its edge in both directions, as the reference's ClampToEdge sampler: not wrapped at azimuth +-pi.
 * The irradiance pass keeps the reference's tangent frame right = (0, 1, 0) x N, up = N x right WITHOUT
 * normalising either (cubemap_shader_irradiance.frag:22-24).  tests/ibl_analytic.py restates these rules
 * in float64.                                                                                      */
int slhip_light_map_build(const float* d_equirect, int H, int W, const slhip_light_map* lm, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera model ('next' row f4 of SURVEY.md 8f): the step after the render in every data-generation
 * loop.  Replaces python/stillleben/camera_model.py:222-263 (process_deterministic): chromatic
 * aberration (:47-74, affine_grid + bilinear grid_sample, reflection padding) -> 5x5 Gaussian blur
 * (:77-118, zero padding) -> re-exposure (:120-130) -> Poissonian-Gaussian noise (:132-163) ->
 * clamp -> hue jitter (:165-220) -> 5x5 post blur (sigma 0.4) -> clamp, fused into two kernels.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float translation[6];   /* (tx, ty) of R, G, B in normalised [-1,1] image coordinates          */
    float scaling[3];       /* scale of R, G, B                                                    */
    float blur_kernel[25];  /* 5x5 weights of the first blur, row-major (camera_model.py:77-104);
                               used when blur_enabled                                             */
    float post_kernel[25];  /* 5x5 weights of the post blur (sigma = 0.4)                          */
    float exposure_gain;    /* exp(deltaS), rounded to f32 (camera_model.py:130)                   */
    float noise_a, noise_b; /* signal-dependent variance factor, signal-independent std            */
                            /* noise_a: 0 or >= 2^-24 -- the entry does not check it; below that the   */
                            /* counts rgb / noise_a are no whole numbers in float32 any more          */
    float hue_shift;        /* -0.5 .. 0.5                                                         */
    uint32_t blur_enabled;  /* blur_sigma > 0                                                      */
    uint32_t noise_enabled; /* do_noise                                                            */
    uint32_t seed_lo, seed_hi; /* counter-based RNG key of this image (noise stage)               */
} slhip_camera_params;      /* 268 bytes */

/* d_in / d_out: f32 [n_images, 3, H, W] (the reference's CHW layout, values in [0,1]); d_tmp:
 * scratch of the same size; d_params: DEVICE array of n_images records.  d_out may alias d_in.   */
int slhip_camera_model(const float* d_in, float* d_out, float* d_tmp, uint32_t n_images, int H, int W,
                       const slhip_camera_params* d_params, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth sensor model: the depth sibling of the camera model.  This project's addition -- the
 * reference has no counterpart (its camera_model.py treats the colour image only).  It turns the
 * rasteriser's exact camera z into what a rectified structured-light / active-stereo sensor
 * (projector at +baseline along camera x) delivers: range limits, holes at grazing angles, the
 * projector's shadow band beside every object, holes where the matching window straddles a
 * discontinuity, lateral jitter, disparity noise, 1/subpixel px disparity quantisation, dropout.
 * Two kernels: pass 1 builds one projector line per image row in LDS and writes a disparity and a
 * flag plane to scratch; pass 2 works on 32 x 8 tiles with a halo of 2 + window_radius in LDS.
 * DESIGN.md "Depth sensor model" states the model step by step; tests/depth_sensor_ref.py restates
 * it in NumPy in the same operation order.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_DEPTH_FLAG_RANGE    1u   /* z outside [z_min, z_max] or NaN; noisy disparity <= 0 */
#define SLHIP_DEPTH_FLAG_GRAZING  2u   /* |n.v| < cos_min                                       */
#define SLHIP_DEPTH_FLAG_SHADOW   4u   /* the projector does not see the surface                */
#define SLHIP_DEPTH_FLAG_SUPPORT  8u   /* fewer than min_support window pixels agree            */
#define SLHIP_DEPTH_FLAG_DROPOUT  16u  /* random dropout                                        */
#define SLHIP_DEPTH_SENSOR_MAX_LINE   4096   /* W + Dmax, Dmax = ceil(fb / z_min): the projector line in LDS */
#define SLHIP_DEPTH_SENSOR_MAX_RADIUS 4

typedef struct {
    float fb;               /* fx * baseline (px * m), rounded once to f32 on the host             */
    float z_min, z_max;     /* working range of the sensor, metres                                 */
    float shadow_margin;    /* px of disparity an occluder must be in front by to cast a shadow     */
    float cos_min;          /* grazing limit on |n.v|; 0 switches the stage off                    */
    uint32_t window_radius; /* r of the (2r+1)^2 matching window, 0..4                             */
    float window_tol;       /* px of disparity within which a window pixel supports the centre     */
    uint32_t min_support;   /* fewer supporting pixels (the centre counts) -> SUPPORT              */
    float sigma_lateral;    /* px; the source pixel is jittered by round(sigma * N(0,1)), +-2 at most */
    float sigma_disparity;  /* px of Gaussian noise on the disparity                               */
    uint32_t subpixel;      /* quantisation steps per px of disparity; 0 = none                    */
    float dropout_p;        /* probability of a random hole                                        */
    float depth_scale;      /* millimetres per unit of the uint16 output (BOP's depth_scale)       */
    uint32_t seed_lo, seed_hi; /* counter-based RNG key of this image                              */
} slhip_depth_sensor_params;   /* 60 bytes */

/* Host-side check of n_images HOST records against an image width: fb, z_min, depth_scale > 0, z_max >= z_min,
 * window_radius <= 4, W + ceil(fb / z_min) <= 4096.  Needs no device.  slhip_depth_sensor reads its records on the device and
 * cannot fail on them: an image whose record breaks a limit comes out all RANGE (flags 1, depth 0).   */
int slhip_depth_sensor_check_params(const slhip_depth_sensor_params* h_params, uint32_t n_images, int W);
/* bytes of d_scratch: the disparity plane f32 [n,H,W] followed by the flag plane u8 [n,H,W].  Needs no device. */
int slhip_depth_sensor_scratch_bytes(uint32_t n_images, int W, int H, uint64_t* bytes);
/* d_depth: z of pixel (i, y, x) at d_depth[((i * H + y) * W + x) * depth_stride] (stride in floats: 4 for the w of
 * slhip_render_out.d_coord, 1 for a dense plane); d_ndotv likewise (the w of d_normals), NULL = no grazing stage.
 * d_params: DEVICE array of n_images records.  Outputs, each NULL when not wanted: d_out_f32 f32 [n,H,W] metres, 0 where
 * invalid; d_out_u16 u16 [n,H,W] = min(65535, floor(z * 1000 / depth_scale + 0.5)), 0 where invalid; d_flags u8 [n,H,W],
 * SLHIP_DEPTH_FLAG_* bits, 0 = valid.  d_scratch: slhip_depth_sensor_scratch_bytes, 16-byte aligned; the inputs must not
 * alias the outputs.  Asynchronous on `stream`.                                                     */
int slhip_depth_sensor(const float* d_depth, uint32_t depth_stride, const float* d_ndotv, uint32_t ndotv_stride,
                       uint32_t n_images, int H, int W, const slhip_depth_sensor_params* d_params, float* d_out_f32,
                       uint16_t* d_out_u16, uint8_t* d_flags, void* d_scratch, void* stream);
/* Developer hook (tools/time_depth_sensor.py): with timing on, a call records HIP events around its two passes;
 * slhip_depth_sensor_timings waits for the last timed call and gives ms_out[0] = pass 1, ms_out[1] = pass 2.   */
int slhip_depth_sensor_timing_enable(int on);
int slhip_depth_sensor_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Object crops: one fixed-size square window per visible object of a render, the input of an
 * object-centric network ("dynamic zoom-in": the object's 2D box, enlarged, randomly scaled and
 * shifted).  This project's addition, the reference has no counterpart.  Two steps on the device:
 * slhip_object_crops_select turns the statistics of a render (slhip_object_stats) into a compact
 * list of crop records in ascending (scene, slot) order; slhip_object_crops_gather resamples the
 * render targets into N x N windows, one thread per output pixel.  All arithmetic is float32, one
 * rounded IEEE operation at a time (no fma); tests/object_crops_ref.py restates it in NumPy bit
 * for bit.  DESIGN.md "Object crops" states the rules.
 *
 * Eligible: the chosen box is non-empty, px_visib >= min_px, (float)px_visib >= min_visib_fract *
 * (float)px_all; slot 0 never.  With (x, y, w, h) the chosen box and u0, u1, u2 the first three
 * uniforms of stream 5 ("Randomness" below; the draw is always made):
 *   side = (float)max(w, h) * pad * (1 + jitter_scale * (2 u0 - 1))
 *   cx_b = (float)x + 0.5 (float)w + jitter_shift * (float)w * (2 u1 - 1)      (cy_b likewise, h and u2)
 *   x0 = cx_b - 0.5 side, y0 = cy_b - 0.5 side, step = side / (float)N
 *   K' = (fx / step, fy / step, (cx - x0) / step, (cy - y0) / step)
 * Output pixel (u, v) samples the picture at sx = x0 + ((float)u + 0.5) step, sy likewise (image x runs from edge 0 to edge W,
 * pixel j covers [j, j + 1)).  Everything but rgb takes the NEAREST pixel (floor(sx), floor(sy)), 0 outside the picture.
 * rgb is BILINEAR on all four bytes: tx = sx - 0.5, ix = floor(tx), ax = tx - ix (y likewise), taps outside count as 0,
 * top = (1 - ax) p00 + ax p10, bot = (1 - ax) p01 + ax p11, val = (1 - ay) top + ay bot, byte = min(255, floor(val + 0.5)).
 * There is no anti-aliasing filter for step > 1 (a window larger than N source pixels is point-sampled).
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_CROP_RGB      1u    /* u8  [n,N,N,4] */
#define SLHIP_CROP_COORD    2u    /* f32 [n,N,N,4] object xyz, camera z */
#define SLHIP_CROP_NORMALS  4u    /* f32 [n,N,N,4] */
#define SLHIP_CROP_INSTANCE 8u    /* i16 [n,N,N]   */
#define SLHIP_CROP_MASK     16u   /* u8  [n,N,N]: bit 0 visible (the nearest sample's instance output is the slot), bit 1
                                     amodal (the kind-0 bit of the slot's tiles at the nearest sample; 0 without masks) */
#define SLHIP_OBJECT_CROPS_MAX_SIZE 1024
#define SLHIP_OBJECT_CROPS_CAPACITY 3   /* status of slhip_object_crops_select: d_crops is too small */

typedef struct {
    uint32_t size;             /* N: the windows are N x N, 1..1024                                         */
    uint32_t box;              /* 0: bbox_visib, 1: bbox_obj                                                */
    float pad;                 /* side of the window / longer side of the box, > 0                         */
    float jitter_scale;        /* [0, 1): the side is scaled by 1 +- this                                   */
    float jitter_shift;        /* [0, 1]: the centre moves by +- this share of the box's width / height     */
    uint32_t min_px;           /* >= 1: fewer visible pixels -> no crop                                      */
    float min_visib_fract;     /* [0, 1]: a smaller visible share of the silhouette -> no crop               */
    float fx, fy, cx, cy;      /* intrinsics the picture was rendered with (Scene.set_camera_intrinsics)     */
    uint32_t seed_lo, seed_hi; /* Philox key of the jitter                                                   */
    uint32_t scene_id_base;    /* scene id of scene 0 of d_stats                                            */
    uint32_t outputs;          /* SLHIP_CROP_* bits, at least one                                           */
    uint32_t isolate;          /* 1: coord and normals are zero wherever mask bit 0 is clear                */
} slhip_object_crop_params;    /* 64 bytes */

typedef struct {
    uint32_t scene, slot;
    float x0, y0, side, step;  /* the window's top-left corner, side and source pixels per output pixel    */
    float K[4];                /* fx', fy', cx', cy' of the window                                          */
    uint32_t _pad[2];
} slhip_object_crop;           /* 48 bytes */

typedef struct {               /* outputs of slhip_object_crops_gather; those not named in `outputs` are not touched */
    uint8_t* d_rgb;
    float*   d_coord;
    float*   d_normals;
    int16_t* d_instance;
    uint8_t* d_mask;
} slhip_object_crops_out;

/* Every rule of the parameter record against a W x H picture; a negative error with slhip_last_error text.  No device. */
int slhip_object_crops_check_params(const slhip_object_crop_params* params, int W, int H);
/* bytes of the d_scratch of slhip_object_crops_select (8-byte aligned).  No device. */
int slhip_object_crops_scratch_bytes(uint32_t n_scenes, uint64_t* bytes);
/* d_stats: slhip_object_stats [n_scenes][n_slots] (device).  Writes the records of all eligible (scene, slot), slot >= 1, in
 * ascending (scene, slot) order to d_crops (device, `capacity` records; n_scenes * (n_slots - 1) always suffices) and their
 * number to *n_out (host).  Returns 0, SLHIP_OBJECT_CROPS_CAPACITY when the number exceeds `capacity` (*n_out is still the
 * needed count; nothing is promised about d_crops), or a negative error.  Synchronises `stream` once.                   */
int slhip_object_crops_select(const slhip_object_crop_params* params, const slhip_object_stats* d_stats, uint32_t n_scenes,
                              uint32_t n_slots, int W, int H, slhip_object_crop* d_crops, uint64_t capacity, void* d_scratch,
                              uint64_t* n_out, void* stream);
/* buffers: the render targets of the picture ([n_scenes,H,W,...]); only those a requested output reads must be non-NULL
 * (d_rgb, d_coord, d_normals; d_instance for SLHIP_CROP_INSTANCE, SLHIP_CROP_MASK and isolate).  d_masks / d_words: the records
 * and bit tiles of slhip_render_object_masks of the same picture, or both NULL (mask bit 1 then stays 0).  A record whose
 * scene or slot lies outside [n_scenes][n_slots] gives an all-zero window.  n_crops == 0 returns 0 without a launch.
 * Asynchronous on `stream`.                                                                                              */
int slhip_object_crops_gather(const slhip_object_crop_params* params, const slhip_object_crop* d_crops, uint64_t n_crops,
                              const slhip_render_out* buffers, uint32_t n_scenes, int W, int H,
                              const slhip_object_mask* d_masks, const uint64_t* d_words, uint32_t n_slots,
                              const slhip_object_crops_out* out, void* stream);
/* Developer hook (tools/time_object_crops.py): with timing on, the two calls record HIP events around their kernels;
 * slhip_object_crops_timings waits for them and gives ms_out[0] = the last select, ms_out[1] = the last gather.   */
int slhip_object_crops_timing_enable(int on);
int slhip_object_crops_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Object points: K pixels of every visible object of a render, drawn inside its visible mask, and
 * what the render shows there -- the input of networks that take a fixed number of points per
 * object (the "choose" indices, the camera-frame point cloud, the dense correspondence target).
 * This project's addition, the reference has no counterpart.  Two steps on the device, as for the
 * crops: slhip_object_points_select turns the statistics and mask records of a render into a
 * compact list of point sets in ascending (scene, slot) order; slhip_object_points_gather finds
 * the pixels in the kind-1 bit tiles of slhip_render_object_masks and gathers there, one workgroup
 * per set.  The choice is integer arithmetic, the camera point float32 with one rounded IEEE
 * operation at a time (no fma); tests/object_points_ref.py restates both in NumPy bit for bit.
 * DESIGN.md "Object points" states the rules.
 *
 * Eligible: slot >= 1, px_visib >= min_px, (float)px_visib >= min_visib_fract * (float)px_all, and
 * the slot has tiles (tile_box tx0 <= tx1).
 * Tile order of a slot's visible pixels: the tiles of its box row-major, inside a tile the rising bit
 * index of the kind-1 word (bit (y & 7) * 8 + (x & 7) = pixel (x, y)).  n = the set's n_visib
 * (px_visib, the popcount of those words); the RANK of a visible pixel is its position in that order.
 * Point j of K = n_points is a stratified draw, all integer (products in 64 bits):
 *   lo = floor(j n / K), hi = floor((j + 1) n / K), width = hi - lo
 *   rank = lo + (uint32_t)(((uint64_t)x_j * width) >> 32)                  (= lo when width == 0)
 * with x_j word j & 3 of stream 6, index (slot << 12) | (j >> 2) ("Randomness" below); point j is the
 * pixel of that rank.  Ranks rise with j and stay below n; for n >= K the K pixels are distinct and
 * spread over the whole mask, for n <= K every visible pixel appears, for n == K point j is pixel j.
 * When the words hold fewer than rank + 1 set bits (statistics and masks of different pictures), when
 * the pixel lies outside the W x H picture or the tile box outside its tiles, or when the set's scene
 * or slot lies outside [n_scenes][n_slots], every output of the point is zero and nothing is read
 * out of bounds of the picture.
 * The camera point of pixel (x, y): z = d_depth[((scene * H + y) * W + x) * depth_stride] as in
 * slhip_depth_sensor (stride 4 on the w of d_coord, 1 on a dense plane such as the sensor's float
 * output, whose holes are 0); valid iff z is finite and > 0; then
 *   X = ((((float)x + 0.5f) - cx) * z) / fx,  Y likewise with y, cy, fy,  Z = z,  valid = 1.0f
 * in the renderer's camera frame (OpenCV's: x right, y down, z forward); an invalid point is
 * (0, 0, 0, 0).  Pixel j covers [j, j + 1), as for the crops: the rasteriser samples at j + 0.5.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_POINTS_PIXEL   1u   /* i16 [n,K,2] (x, y) */
#define SLHIP_POINTS_CAMERA  2u   /* f32 [n,K,4] (X, Y, Z, valid) */
#define SLHIP_POINTS_COORD   4u   /* f32 [n,K,4] d_coord at the pixel, bit for bit (object xyz, camera z) */
#define SLHIP_POINTS_NORMALS 8u   /* f32 [n,K,4] d_normals at the pixel, bit for bit */
#define SLHIP_POINTS_RGB     16u  /* u8  [n,K,4] d_rgb at the pixel */
#define SLHIP_OBJECT_POINTS_MAX 16384
#define SLHIP_OBJECT_POINTS_CAPACITY 4   /* status of slhip_object_points_select: d_sets is too small */

typedef struct {
    uint32_t n_points;         /* K, 1..SLHIP_OBJECT_POINTS_MAX                                              */
    uint32_t min_px;           /* >= 1: fewer visible pixels -> no set                                       */
    float min_visib_fract;     /* [0, 1]: a smaller visible share of the silhouette -> no set                */
    float fx, fy, cx, cy;      /* intrinsics the picture was rendered with (Scene.set_camera_intrinsics)     */
    uint32_t seed_lo, seed_hi; /* Philox key of the draw                                                     */
    uint32_t scene_id_base;    /* scene id of scene 0 of d_stats                                            */
    uint32_t outputs;          /* SLHIP_POINTS_* bits, at least one                                          */
    uint32_t _pad;
} slhip_object_point_params;   /* 48 bytes */

typedef struct {
    uint32_t scene, slot;
    uint32_t n_visib;          /* px_visib of the slot when it was selected: the n of the rank rule         */
    uint32_t _pad;
} slhip_object_point_set;      /* 16 bytes */

typedef struct {               /* outputs of slhip_object_points_gather; those not named in `outputs` are not touched */
    int16_t* d_pixel;
    float*   d_camera;
    float*   d_coord;
    float*   d_normals;
    uint8_t* d_rgb;
} slhip_object_points_out;

/* Every rule of the parameter record against a W x H picture (sides 1..32768): 1 <= n_points <= SLHIP_OBJECT_POINTS_MAX, min_px >= 1,
 * min_visib_fract in [0, 1], fx, fy > 0 and all four intrinsics finite, known output bits and at least one.  select and gather
 * also refuse n_slots > 65536 (the slot shares the counter's index word with j >> 2).  A negative error with slhip_last_error
 * text.  No device. */
int slhip_object_points_check_params(const slhip_object_point_params* params, int W, int H);
/* bytes of the d_scratch of slhip_object_points_select (8-byte aligned).  No device. */
int slhip_object_points_scratch_bytes(uint32_t n_scenes, uint64_t* bytes);
/* d_stats, d_masks: slhip_object_stats and slhip_object_mask [n_scenes][n_slots] (device) of one slhip_render_object_masks.
 * Writes the records of all eligible (scene, slot) in ascending (scene, slot) order to d_sets (device, `capacity` records;
 * n_scenes * (n_slots - 1) always suffices) and their number to *n_out (host).  Returns 0, SLHIP_OBJECT_POINTS_CAPACITY when
 * the number exceeds `capacity` (*n_out is still the needed count; nothing is promised about d_sets), or a negative error.
 * Synchronises `stream` once.                                                                                           */
int slhip_object_points_select(const slhip_object_point_params* params, const slhip_object_stats* d_stats,
                               const slhip_object_mask* d_masks, uint32_t n_scenes, uint32_t n_slots,
                               slhip_object_point_set* d_sets, uint64_t capacity, void* d_scratch, uint64_t* n_out, void* stream);
/* buffers: the render targets of the picture ([n_scenes,H,W,...]); only those a requested output reads must be non-NULL
 * (d_coord, d_normals, d_rgb).  d_depth / depth_stride (in floats): the z plane of SLHIP_POINTS_CAMERA, required with that
 * output only.  d_masks / d_words: the records and bit tiles of slhip_render_object_masks of the same picture, always
 * required.  Null pointers and bad sizes are refused before anything touches the device; n_sets == 0 returns 0 without a
 * launch.  Asynchronous on `stream`.                                                                                      */
int slhip_object_points_gather(const slhip_object_point_params* params, const slhip_object_point_set* d_sets, uint64_t n_sets,
                               const slhip_render_out* buffers, const float* d_depth, uint32_t depth_stride, uint32_t n_scenes,
                               int W, int H, const slhip_object_mask* d_masks, const uint64_t* d_words, uint32_t n_slots,
                               const slhip_object_points_out* out, void* stream);
/* The pixels of ONE set on the host, by the same lookup (csrc/slhip_mask_select.h) on host words: tile_box and h_words are
 * the slot's tile box and its kind-1 words (word 0 = the box's first tile); out_xy receives n_points pairs (x, y), (0, 0)
 * where the words run out before the rank.  Host only, no device: the handle by which the lookup is tested without one.   */
int slhip_object_points_host_pixels(const slhip_object_point_params* params, uint32_t scene, uint32_t slot, uint32_t n_visib,
                                    const int32_t tile_box[4], const uint64_t* h_words, int16_t* out_xy);
/* Developer hook (tools/time_object_points.py): with timing on, the two calls record HIP events around their kernels;
 * slhip_object_points_timings waits for them and gives ms_out[0] = the last select, ms_out[1] = the last gather.   */
int slhip_object_points_timing_enable(int on);
int slhip_object_points_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Object keypoints: the targets of keypoint-voting pose networks (PVN3D, FFB6D: per-point offsets to
 * 3D keypoints of the object's class; PVNet: per-pixel vectors towards the projected keypoints), from
 * what a batch keeps in HBM -- the mesh pool, object_to_camera of slhip_synth_place_view and the
 * instance target.  This project's addition, the reference has no counterpart.  Three steps: a bank
 * of keypoints per class by farthest point sampling (once per asset table), their projection per
 * (scene, object), and the per-pixel field.  All float32, one rounded IEEE operation at a time (no
 * fma), the parenthesisation below is the contract; csrc/slhip_keypoint_rules.h holds the rules for
 * host and device, tests/object_keypoints_ref.py restates them in NumPy bit for bit.  DESIGN.md
 * "Object keypoints".
 *
 * 1. FPS, per class.  Its vertices are d_pos[vtx_base .. vtx_base + n_verts), vtx_base that of
 * d_templates[asset.draw_begin]; a class with draw_count == 0 or n_verts == 0 has none (nor one whose
 * template or vertices lie outside the tables, or with more than max_verts vertices).
 *   p_v = rows 0..2 of mesh_to_object applied to (x, y, z, 1), each ((m0*x + m1*y) + m2*z) + m3: the
 *         object frame, the frame of the coord target
 *   o = (bbox_min + bbox_max) * 0.5f per component
 *   d2(a, b) = ((ax-bx)*(ax-bx) + (ay-by)*(ay-by)) + (az-bz)*(az-bz)
 *   dmin[v] = d2(p_v, o); then for k = 0 .. n_fps-1:
 *     i_k = the lowest v whose dmin[v] is the maximum (a scan upwards from -inf with a strict >: a NaN
 *           never wins; when nothing wins, vertex 0),  kp_k = p_{i_k},
 *     dmin[v] = d2(p_v, kp_k) < dmin[v] ? d2(p_v, kp_k) : dmin[v]
 * With fewer distinct positions than n_fps the rule repeats the lowest index: that is the defined
 * result.  With no vertices every keypoint is o and every index -1.
 *
 * 2. Projection, per (scene, object, k) with (x, y, z) = bank[object's asset][k] and r, t the rows of
 * object_to_camera:  X = ((r00*x + r01*y) + r02*z) + t0, Y and Z likewise;
 *   u = (fx * X) / Z + cx,  v = (fy * Y) / Z + cy      (pixel index x covers [x, x + 1), as for points and crops)
 * Flags: SLHIP_KEYPOINT_IN_FRONT  X, Y, Z finite and Z > 0
 *        SLHIP_KEYPOINT_INSIDE    in front, 0 <= u < W and 0 <= v < H
 *        SLHIP_KEYPOINT_UNOCCLUDED  only with a depth plane: inside, the plane's z at pixel (floor(u), floor(v))
 *                                 finite and > 0, and Z <= z + depth_tol
 * Without IN_FRONT, u = v = 0 and the camera point is (0, 0, 0, 0); an asset >= n_assets gives all-zero outputs.
 *
 * 3. Field.  A pixel (x, y) with instance i, 1 <= i <= n_objects, belongs to object i - 1; for keypoint k
 *   dx = u_k - ((float)x + 0.5f),  dy = v_k - ((float)y + 0.5f)
 *   OFFSET: (dx, dy)      UNIT: l = sqrt(dx*dx + dy*dy), (dx / l, dy / l), (0, 0) when l == 0
 * (sqrt and / correctly rounded), (0, 0) in both modes when the keypoint is not IN_FRONT.  Every other
 * pixel (instance 0, negative, above n_objects) gets zeros in all 2 Kp floats.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_KEYPOINTS_MAX 32
#define SLHIP_KEYPOINT_IN_FRONT   1u
#define SLHIP_KEYPOINT_INSIDE     2u
#define SLHIP_KEYPOINT_UNOCCLUDED 4u
#define SLHIP_KEYPOINT_FIELD_OFFSET 0u
#define SLHIP_KEYPOINT_FIELD_UNIT   1u

typedef struct {
    float fx, fy, cx, cy;      /* intrinsics the picture was rendered with; fx, fy > 0, all finite          */
    int32_t W, H;              /* picture size, each side 1..32768                                           */
    float depth_tol;           /* metres, finite and >= 0: how far behind the plane a keypoint still shows   */
    uint32_t n_keypoints;      /* Kp, 1..SLHIP_KEYPOINTS_MAX                                                 */
    uint32_t n_objects;        /* objects per scene, 1..SLHIP_SYNTH_MAX_OBJECTS                              */
    uint32_t mode;             /* SLHIP_KEYPOINT_FIELD_* (slhip_object_keypoints_field only)                 */
    uint32_t _pad[2];
} slhip_object_keypoint_params; /* 48 bytes */

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_object_keypoints_check_params(const slhip_object_keypoint_params* params);
/* bytes of the d_scratch of slhip_object_keypoints_fps: dmin, one row of max_verts floats per class.  No device. */
int slhip_object_keypoints_fps_bytes(uint32_t n_assets, uint64_t max_verts, uint64_t* bytes);
/* slhip_object_keypoints_fps, _fps_host and _project take records of the synthesis section and are declared there, below.
 * d_instance i16 [n_scenes, H, W], d_uv and d_flags of the projection, scenes [first, first + count) of them into d_out f32
 * [count, H, W, Kp, 2] (8-byte aligned): every float of the slice is written exactly once, nothing outside it.  A scene's
 * field must stay below 2^31 (pixel, keypoint) pairs, count below 65536; a range past n_scenes, null pointers and bad
 * parameters are refused before anything touches the device.  Asynchronous on `stream`.                                  */
int slhip_object_keypoints_field(const slhip_object_keypoint_params* params, const int16_t* d_instance, const float* d_uv,
                                 const uint8_t* d_flags, uint32_t n_scenes, uint32_t first, uint32_t count, float* d_out,
                                 void* stream);
/* Developer hook (tools/time_object_keypoints.py): with timing on, the three calls record HIP events around their kernels;
 * slhip_object_keypoints_timings waits for them and gives the ms of the last fps, project and field (-1: not run).   */
int slhip_object_keypoints_timing_enable(int on);
int slhip_object_keypoints_timings(float ms_out[3]);

/* ---------------------------------------------------------------------------------------------
 * Object regions: the targets of pose networks that classify every pixel into a surface region of its
 * object and regress inside it (GDR-Net's surface region attention, EPOS' surface fragments and
 * fragment-local coordinates, SO-Pose, the coarse levels of ZebraPose).  This project's addition, the
 * reference has no counterpart.  A bank of R region centres per class by the farthest point sampling
 * of "Object keypoints" (once per asset table), the region of every mesh vertex with per-region counts
 * and extents, and per pixel of a render the region of its object coordinate.  All float32, one
 * rounded IEEE operation at a time (no fma); csrc/slhip_region_rules.h holds the rules for host and
 * device, tests/object_regions_ref.py restates them in NumPy bit for bit.  DESIGN.md "Object regions".
 *
 * Nearest centre of a point p among the R centres c_0 .. c_{R-1} of a class, with d2 of "Object keypoints":
 *   best = +inf, region = 0;  for r = 0 .. R-1 upwards:  d = d2(p, c_r);  if (d < best) { best = d; region = r; }
 * A strict <: ties, duplicated centres included, go to the lowest index; a NaN distance never wins; when
 * nothing wins (every d NaN or +inf) the region is 0.
 *
 * 1. Centres, per class: exactly the FPS of "Object keypoints" step 1 with n_fps = R, R in
 * [1, SLHIP_REGIONS_MAX]: the first 32 centres are, bit for bit, the keypoint FPS.
 *
 * 2. Vertices.  Every vertex v of every class a (the ranges of step 1 of "Object keypoints", no row limit)
 * gets r = nearest centre of p_v among the centres of a;  count[a][r] += 1;  with c = centre r of a
 *   extent[a][r] = max over the region's vertices of (|p.x - c.x|, |p.y - c.y|, |p.z - c.z|, d2(p, c))
 * each maximum taken on the bit patterns with the sign cleared (the order of non-negative floats; a NaN
 * sorts above +inf), zeros for an empty region: integer maxima and sums, so the result does not depend
 * on the order.  vertex_region[v] = r; SLHIP_REGION_NONE for a vertex of no class; a vertex inside the
 * ranges of several classes carries the region of the highest such class (count and extent take it
 * for every class).
 *
 * 3. Label, per pixel with instance i and coord (x, y, z, w; w is not read):  region = SLHIP_REGION_NONE
 * when i < 1 or i > n_objects, when cls = classes[(image * n_objects + i - 1) * class_stride] is outside
 * [0, n_assets), or when x, y or z is not finite; otherwise the nearest centre of (x, y, z) among the
 * centres of cls.  local = (x - cx, y - cy, z - cz, d2((x, y, z), c)) of the winning centre c, zeros
 * where region is NONE.  histogram[image][i - 1][region] counts the pixels that have a region.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_REGIONS_MAX 255
#define SLHIP_REGION_NONE 255
#define SLHIP_REGIONS_OUT_LOCAL     1u
#define SLHIP_REGIONS_OUT_HISTOGRAM 2u

typedef struct {
    int32_t W, H;              /* picture size, each side 1..32768                                            */
    uint32_t n_images;         /* N; N * H * W must stay below 2^32 - 2048 (split larger batches)             */
    uint32_t n_objects;        /* O, objects per image, 1..SLHIP_SYNTH_MAX_OBJECTS                             */
    uint32_t n_regions;        /* R, 1..SLHIP_REGIONS_MAX                                                      */
    uint32_t n_assets;         /* A, classes of the bank, 1..SLHIP_SYNTH_MAX_ASSETS                            */
    uint32_t outputs;          /* SLHIP_REGIONS_OUT_* bits; `region` is always written                         */
    uint32_t _pad;
} slhip_object_region_params; /* 32 bytes */

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_object_regions_check_params(const slhip_object_region_params* params);
/* bytes of the d_scratch of slhip_object_regions_centres: one row of max_verts floats per class.  No device. */
int slhip_object_regions_centres_bytes(uint32_t n_assets, uint64_t max_verts, uint64_t* bytes);
/* slhip_object_regions_centres, _centres_host, _vertices and _vertices_host take records of the synthesis section and are
 * declared there, below.
 * Label: d_instance i16 [N, H, W]; d_coord f32 [N, H, W, 4] (16-byte aligned); d_classes i32, read at
 * (image * O + object) * class_stride (1: a plain [N, O] tensor, 4: the asset of slhip_synth_object records in place);
 * d_centres f32 [A, R, 4] (16-byte aligned).  d_region u8 [N, H, W], any alignment: every byte is written exactly once.
 * d_local f32 [N, H, W, 4] (16-byte aligned) with SLHIP_REGIONS_OUT_LOCAL, d_histogram u32 [N, O, R] (4-byte aligned) with
 * SLHIP_REGIONS_OUT_HISTOGRAM: the entry zeroes the histogram on `stream` before the kernel, the caller need not.  Without
 * their bit the two pointers are not read.  An image whose pixels are all NONE never reads d_centres.  n_images == 0 does
 * nothing; null pointers, misaligned buffers and bad parameters are refused before anything touches the device.
 * Asynchronous on `stream`.                                                                                              */
int slhip_object_regions_label(const slhip_object_region_params* params, const int16_t* d_instance, const float* d_coord,
                               const int32_t* d_classes, uint32_t class_stride, const float* d_centres, uint8_t* d_region,
                               float* d_local, uint32_t* d_histogram, void* stream);
/* The same rules on host arrays through csrc/slhip_region_rules.h; h_histogram is zeroed first.  Host only, no device: the
 * handle the CPU tests use.                                                                                              */
int slhip_object_regions_label_host(const slhip_object_region_params* params, const int16_t* h_instance, const float* h_coord,
                                    const int32_t* h_classes, uint32_t class_stride, const float* h_centres, uint8_t* h_region,
                                    float* h_local, uint32_t* h_histogram);
/* Developer hook (tools/time_object_regions.py): with timing on, the three device calls record HIP events around their
 * work; slhip_object_regions_timings waits for them and gives the ms of the last centres, vertices and label (-1: not run). */
int slhip_object_regions_timing_enable(int on);
int slhip_object_regions_timings(float ms_out[3]);

/* ---------------------------------------------------------------------------------------------
 * Pose errors: ADD, ADD-S (PoseCNN, DenseFusion), BOP's MSSD and MSPD of pose estimates against a
 * batch's ground truth object_to_camera, with the symmetries of every class; the arg-min of MSSD is
 * the symmetric equivalent of the ground truth nearest the estimate, the target of symmetry-aware
 * losses.  This project's addition, the reference has no counterpart.  All float32, one rounded IEEE
 * operation at a time (no fma); csrc/slhip_pose_rules.h holds the rules for host and device,
 * tests/pose_error_ref.py restates them in NumPy bit for bit.  DESIGN.md "Pose errors".
 *
 * The bank: per class a (0 <= a < n_assets) count[a] points (x, y, z, 1) in the object frame -- row a of
 * points, n_points floats4 long -- and n_sym[a] symmetry transforms, 3 x 4 row-major, entry 0 the identity
 * -- row a of symmetries, n_symmetries long.  A class with count outside [1, n_points] or n_sym outside
 * [1, n_symmetries], and a class index outside the bank, has no points: its errors are +inf and its
 * indices -1 (never 0, which would read as a perfect pose).  The points must be finite.
 *
 * Per (scene, object, hypothesis) with g = the object's ground truth and e the estimate (3 x 4 row-major):
 *   D = e - g, all twelve entries (the translations cancel before anything is multiplied).  When an entry of D
 * is not finite, every error of the hypothesis is NaN and every index -1.  Otherwise, with M p = the rows
 * ((m0*x + m1*y) + m2*z) + m3, dist2(a, b) = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2 and p_i the class's points:
 *   w_i = D p_i                      the camera-frame displacement x_e(p_i) - x_g(p_i)
 *   v_i[c] = (g[0][c]*w_i[0] + g[1][c]*w_i[1]) + g[2][c]*w_i[2]      R_g^T w_i (the rotation of g is taken as orthonormal)
 *   q_i = p_i + v_i per component    the estimate's point in the ground truth's object frame
 *   add   = sum_i sqrt((w_i[0]^2 + w_i[1]^2) + w_i[2]^2) / (float)count
 *   adds  = sum_i sqrt(min_j dist2(q_i, p_j)) / (float)count
 *   mssd  = sqrt(min_s max_i dist2(q_i, S_s p_i)),  mssd_sym = the lowest s that reaches the minimum
 *   mspd  = sqrt(min_s max_i ((ue_i - ug_si)^2 + (ve_i - vg_si)^2)),  mspd_sym likewise, where
 *           (X, Y, Z) = e p_i,  ue = (fx * X) / Z + cx,  ve = (fy * Y) / Z + cy,  and ug, vg the same of g (S_s p_i);
 *           when a Z of either side (any i, any s < n_sym) is not > 0:  mspd = +inf, mspd_sym = -1
 * sqrt and / correctly rounded; min and max are order-free.  The order of the two sums: lane l of 256
 * adds the terms of points l, l + 256, ... upwards from 0.0f; the 64 lanes of a wave combine by
 * v[l] = v[l] + v[l ^ off] for off = 32, 16, 8, 4, 2, 1, the four waves as ((w0 + w1) + w2) + w3.
 * An estimate equal to the ground truth has D = 0 and q_i = p_i to the bit: every error is exactly 0.
 * The diameter of a class is sqrt(max_ij dist2(p_i, p_j)), 0 for a class without points.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_POSE_POINTS_MAX     4096
#define SLHIP_POSE_SYMMETRIES_MAX 1024
#define SLHIP_POSE_OUT_ADD  1u
#define SLHIP_POSE_OUT_ADDS 2u
#define SLHIP_POSE_OUT_MSSD 4u      /* mssd and mssd_sym */
#define SLHIP_POSE_OUT_MSPD 8u      /* mspd and mspd_sym */

typedef struct {
    float fx, fy, cx, cy;      /* intrinsics of MSPD; fx, fy > 0, all finite                                  */
    uint32_t n_objects;        /* O, objects per scene, 1..SLHIP_SYNTH_MAX_OBJECTS                            */
    uint32_t n_hypotheses;     /* Hy >= 1, estimates per object                                               */
    uint32_t outputs;          /* SLHIP_POSE_OUT_* bits, at least one                                         */
    uint32_t _pad;
} slhip_pose_error_params; /* 32 bytes */

typedef struct {
    const float* points;       /* f32 [n_assets, n_points, 4], 16-byte aligned                                */
    const int32_t* count;      /* i32 [n_assets]                                                              */
    const float* symmetries;   /* f32 [n_assets, n_symmetries, 3, 4], 16-byte aligned                         */
    const int32_t* n_sym;      /* i32 [n_assets]                                                              */
    uint32_t n_assets;         /* 1..SLHIP_SYNTH_MAX_ASSETS                                                   */
    uint32_t n_points;         /* N, the row length: 1..SLHIP_POSE_POINTS_MAX                                 */
    uint32_t n_symmetries;     /* S, the row length: 1..SLHIP_POSE_SYMMETRIES_MAX                             */
    uint32_t _pad;
} slhip_pose_bank; /* 48 bytes; the four arrays on the device, or on the host for the _host entries */

typedef struct {               /* each [n_scenes, n_objects, n_hypotheses]; read only when its bit is set    */
    float* add;
    float* adds;
    float* mssd;
    int32_t* mssd_sym;
    float* mspd;
    int32_t* mspd_sym;
} slhip_pose_error_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_error_check_params(const slhip_pose_error_params* params);
/* d_diameter f32 [n_assets]: the entry zeroes it on `stream`, then all pairs of every class's points.  Runs once per table.
 * A null pointer, a misaligned bank and row lengths out of range are refused before anything touches the device.
 * Asynchronous on `stream`.                                                                                              */
int slhip_pose_error_diameter(const slhip_pose_bank* bank, float* d_diameter, void* stream);
/* The same rule on host arrays.  Host only, no device. */
int slhip_pose_error_diameter_host(const slhip_pose_bank* h_bank, float* h_diameter);
/* d_classes i32, read at (scene * O + object) * class_stride (1: a plain [n_scenes, O] tensor, 4: the asset of
 * slhip_synth_object records in place); d_gt f32 [n_scenes, O, 3, 4] (object_to_camera of slhip_synth_place_view); d_est f32
 * [n_scenes, O, Hy, 3, 4].  Every output named in params->outputs is written exactly once per hypothesis, the others are not
 * touched.  n_scenes == 0 does nothing; null pointers (an output named in the mask included), a misaligned bank, row lengths
 * out of range, class_stride 0, Hy == 0 and bad parameters are refused before anything touches the device.  One workgroup
 * holds a class's points in LDS and takes one or several hypotheses of an object.  Asynchronous on `stream`.             */
int slhip_pose_error(const slhip_pose_error_params* params, const slhip_pose_bank* bank, const int32_t* d_classes,
                     uint32_t class_stride, const float* d_gt, const float* d_est, uint32_t n_scenes,
                     const slhip_pose_error_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_pose_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_error_host(const slhip_pose_error_params* params, const slhip_pose_bank* h_bank, const int32_t* h_classes,
                          uint32_t class_stride, const float* h_gt, const float* h_est, uint32_t n_scenes,
                          const slhip_pose_error_out* out);
/* Developer hook (tools/time_pose_error.py): with timing on, the two device calls record HIP events around their work;
 * slhip_pose_error_timings waits for them and gives the ms of the last diameter and the last errors (-1: not run).       */
int slhip_pose_error_timing_enable(int on);
int slhip_pose_error_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Pose VSD: BOP's Visible Surface Discrepancy of pose estimates against a batch's ground truth, the
 * one pose error that looks at the picture.  The object is drawn as depth at the ground truth and at
 * the estimate, both are compared where either is visible in the scene's depth image.  This project's
 * addition, the reference has no counterpart.  All float32, one rounded IEEE operation at a time (no
 * fma), the coverage in exact integers; csrc/slhip_vsd_rules.h holds the rules for host and device,
 * tests/pose_vsd_ref.py restates them in NumPy bit for bit.  DESIGN.md "Pose VSD".
 *
 * The surface bank: vertices (x, y, z, 1) in the object frame and triangles of absolute vertex indices;
 * class a owns triangles [tri_begin[a], tri_begin[a] + tri_count[a]).  A class with tri_count 0 or a range
 * that leaves the table, and a class index outside the bank, has no surface: vsd = +inf, counts -1.  A
 * triangle with an index >= n_vertices is dropped.
 *
 * Rasterising a pose M (3 x 4 row-major, object to camera, +Z forward) of a class, per triangle:
 *   (X, Y, Z) = M p per vertex, rows ((m0*x + m1*y) + m2*z) + m3.  A vertex with a non-finite X, Y or Z or
 *   without Z > z_near is clipped: its triangles are dropped and the hypothesis gets SLHIP_VSD_CLIPPED (a
 *   triangle of the ground truth's pose: every hypothesis of the object).  There is no clip-space path.
 *   u = (fx * X) / Z + cx,  v = (fy * Y) / Z + cy,  Xs = (int)clamp(floorf(u * 256.0f + 0.5f), -2^26, 2^26)
 *   (a NaN gives 0), Ys likewise of v; the centre of pixel (px, py) is (256 px + 128, 256 py + 128).
 *   area2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); 0: dropped; flipped = area2 < 0, area2 = |area2|.
 *   e_i = slhip_raster::edge_value(i) at the centre; covered when e_0, e_1, e_2 >= 0 (no ownership bias, no
 *   culling).  b_i = (float)e_i / (float)area2, iz_k = 1.0f / Z_k,
 *   z = 1.0f / ((b_0 * iz_0 + b_1 * iz_1) + b_2 * iz_2); the pose's depth is the minimum over its triangles.
 * Comparing, per pixel, with z_g, z_e the two depths (present_g, present_e: covered at all) and t the scene's
 * depth at d_test_depth[((scene * H + py) * W + px) * depth_stride]:
 *   absent_t = !(t > 0) || t - t != 0
 *   xn = (((float)px + 0.5f) - cx) / fx, yn likewise, ray = sqrtf((xn*xn + yn*yn) + 1.0f)
 *   D_g = z_g * ray, D_e = z_e * ray, D_t = t * ray
 *   vis(m) = present_m && (absent_t || (D_m - D_t) <= delta)
 *   V_g = vis(g), V_e = vis(e) || (V_g && present_e), inter = V_g && V_e, uni = V_g || V_e
 *   cost_t = inter && fabsf(D_g - D_e) >= thr_t,  thr_t = taus[t], or taus[t] * diameter[class] with
 *   SLHIP_VSD_NORMALIZED
 * and over the picture the int32 counts n_visib_gt, n_visib_est, n_inter, n_union, n_cost[t]:
 *   vsd[t] = n_union == 0 ? 1.0f : (float)(n_cost[t] + (n_union - n_inter)) / (float)n_union
 * A pose (ground truth or estimate) with an entry that is not finite: vsd NaN, counts and n_cost -1, flags 0.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_VSD_TAUS_MAX   16
#define SLHIP_VSD_WIDTH_MAX  4096u    /* a row of the picture must fit the smallest LDS band             */
#define SLHIP_VSD_NORMALIZED 1u       /* params.flags: thresholds are taus[t] * diameter[class]          */
#define SLHIP_VSD_CLIPPED    1u       /* output flags: a triangle had a vertex at or behind z_near       */
#define SLHIP_VSD_OUT_VSD    1u
#define SLHIP_VSD_OUT_COUNTS 2u
#define SLHIP_VSD_OUT_COST   4u
#define SLHIP_VSD_OUT_FLAGS  8u

typedef struct {
    float fx, fy, cx, cy;      /* fx, fy > 0, all finite                                                      */
    int32_t W, H;              /* the picture: W 1..SLHIP_VSD_WIDTH_MAX, H 1..32768                           */
    uint32_t n_objects;        /* O, 1..SLHIP_SYNTH_MAX_OBJECTS                                               */
    uint32_t n_hypotheses;     /* Hy >= 1                                                                     */
    uint32_t n_taus;           /* T, 1..SLHIP_VSD_TAUS_MAX                                                    */
    float delta;               /* tolerance of the visibility test, >= 0 and finite                           */
    float z_near;              /* > 0 and finite                                                              */
    uint32_t flags;            /* SLHIP_VSD_NORMALIZED or 0                                                   */
    uint32_t outputs;          /* SLHIP_VSD_OUT_* bits, at least one (slhip_pose_depth does not read them)    */
    uint32_t _pad[3];
    float taus[SLHIP_VSD_TAUS_MAX];   /* the first n_taus finite and >= 0                                     */
} slhip_pose_vsd_params; /* 128 bytes */

typedef struct {
    const float* vertices;     /* f32 [n_vertices, 4], 16-byte aligned                                        */
    const uint32_t* triangles; /* u32 [n_triangles, 3]                                                        */
    const uint32_t* tri_begin; /* u32 [n_assets]                                                              */
    const uint32_t* tri_count; /* u32 [n_assets]                                                              */
    const float* diameter;     /* f32 [n_assets]; required with SLHIP_VSD_NORMALIZED, else may be NULL        */
    uint32_t n_assets;         /* 1..SLHIP_SYNTH_MAX_ASSETS                                                   */
    uint32_t n_vertices;       /* 1..2^31 - 1                                                                 */
    uint32_t n_triangles;      /* 1..2^31 - 1                                                                 */
    uint32_t _pad;
} slhip_pose_surface; /* 56 bytes; the arrays on the device, or on the host for the _host entries */

typedef struct {               /* read only when its bit is set                                               */
    float* vsd;                /* f32 [n_scenes, O, Hy, T]                                                    */
    int32_t* counts;           /* i32 [n_scenes, O, Hy, 4]: visib_gt, visib_est, inter, union                 */
    int32_t* n_cost;           /* i32 [n_scenes, O, Hy, T]                                                    */
    uint32_t* flags;           /* u32 [n_scenes, O, Hy]                                                       */
} slhip_pose_vsd_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_vsd_check_params(const slhip_pose_vsd_params* params);
/* d_classes i32, read at (scene * O + object) * class_stride (1: a plain tensor, 4: slhip_synth_object records in place);
 * d_gt f32 [n_scenes, O, 3, 4]; d_est f32 [n_scenes, O, Hy, 3, 4]; d_test_depth read with depth_stride floats between
 * pixels (4 on the w of d_coord, 1 on a dense plane).  Every output named in params->outputs is written exactly once per
 * hypothesis, the others are not touched.  n_scenes == 0 does nothing; null pointers, misalignment, class_stride or
 * depth_stride 0 and bad parameters are refused before anything touches the device.  One workgroup per (scene, object,
 * hypothesis); the two depth planes live in LDS only.  Asynchronous on `stream`.                                          */
int slhip_pose_vsd(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* d_classes,
                   uint32_t class_stride, const float* d_gt, const float* d_est, const float* d_test_depth,
                   uint32_t depth_stride, uint32_t n_scenes, const slhip_pose_vsd_out* out, void* stream);
/* The raster alone: d_poses f32 [n_scenes, O, Hy, 3, 4] drawn into d_depth f32 [n_scenes, O, Hy, H, W], 0 where nothing is
 * covered (and everywhere for a class without a surface or a pose that is not finite); d_flags u32 [n_scenes, O, Hy] or
 * NULL.  Every float of d_depth is written exactly once.  The whole record must pass slhip_pose_vsd_check_params, though
 * outputs, n_taus, taus, delta and flags do not enter the raster.                                                         */
int slhip_pose_depth(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* d_classes,
                     uint32_t class_stride, const float* d_poses, uint32_t n_scenes, float* d_depth, uint32_t* d_flags,
                     void* stream);
/* The same rules on host arrays through csrc/slhip_vsd_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_vsd_host(const slhip_pose_vsd_params* params, const slhip_pose_surface* h_surface, const int32_t* h_classes,
                        uint32_t class_stride, const float* h_gt, const float* h_est, const float* h_test_depth,
                        uint32_t depth_stride, uint32_t n_scenes, const slhip_pose_vsd_out* out);
int slhip_pose_depth_host(const slhip_pose_vsd_params* params, const slhip_pose_surface* h_surface, const int32_t* h_classes,
                          uint32_t class_stride, const float* h_poses, uint32_t n_scenes, float* h_depth, uint32_t* h_flags);
/* The pixels one LDS band of k_pose_vsd holds (two uint32 planes of that size).  No device. */
int slhip_pose_vsd_band_pixels(void);
/* Developer hook (tools/time_pose_vsd.py): HIP events round the last slhip_pose_vsd [0] and slhip_pose_depth [1]. */
int slhip_pose_vsd_timing_enable(int on);
int slhip_pose_vsd_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Pose PnP: the pose of every set of K 2D-3D correspondences (a pixel position and a point in the
 * object frame) by P3P inside RANSAC and Gauss-Newton on the inliers -- the step between the
 * correspondence targets (`coord`, slhip_object_points_gather) and the pose errors above.  This
 * project's addition, the reference has no counterpart.  All float32, one rounded IEEE operation at a
 * time (no fma), only + - * / sqrt fabs min max and comparisons; csrc/slhip_pnp_rules.h holds the rules
 * for host and device, so slhip_pose_pnp_host gives the device's outputs bit for bit.  DESIGN.md
 * "Pose PnP" states them operation by operation; in short, per set:
 *   1. valid list: correspondence j counts when u, v, x, y, z are finite and w > 0; the valid ones are
 *      taken in ascending j, n_valid of them; fewer than 4: SLHIP_PNP_INSUFFICIENT.  The centre of pixel
 *      (x, y) is (x + 0.5, y + 0.5); bearings are a = (u - cx) / fx, b = (v - cy) / fy.
 *   2. hypothesis h draws Philox counter (set_id_base + set, 7, h, 0x51DE5EED) under (seed_lo, seed_hi)
 *      ("Randomness" below); word k picks min(n_valid - 1, (uint32_t)(uniform(x_k) * (float)n_valid)) of
 *      the valid list; the first three are the sample, the fourth disambiguates; a repeated pick: void.
 *   3. P3P on the three bearings and points (a quartic free of cosines, its roots by sign changes and a
 *      fixed number of halvings, three Newton steps on the distances); a solution is kept when every
 *      entry is finite, the three distances are > 0 and the squared sides are met within 2^-10 of
 *      themselves; of the kept the smallest squared pixel error of the fourth point wins (one not in
 *      front counts +inf), ties to the lower root; none kept: void.
 *   4. score = the number of valid correspondences with Z > 0 and ((fx*X)/Z + cx - u)^2 +
 *      ((fy*Y)/Z + cy - v)^2 <= threshold_px^2, (X, Y, Z) the rows ((m0*x + m1*y) + m2*z) + m3; a void
 *      hypothesis scores 0.  The winner: highest score, ties to the lowest index, d_init as index -1.
 *      A winner below min_inliers: SLHIP_PNP_NO_MODEL.
 *   5. refine_iters Gauss-Newton steps on the pixel residuals of the inliers of the current pose,
 *      (omega, t) applied on the left through the Cayley map of omega / 2; the 27 sums in the order of the
 *      pose errors' means (lane l of 256 over valid points l, l + 256, ..; the butterfly; ((w0 + w1) + w2)
 *      + w3); L D L^T without pivoting; a pivot not positive and finite: SLHIP_PNP_REFINE_STOPPED, the
 *      pose of the step before stays.
 *   6. inliers, count and rms = sqrt(sum of squared errors / (float)count) of the refined pose over the
 *      correspondences j in their own order (lane j % 256); fewer inliers than the winner's score: the
 *      winner's pose and figures with SLHIP_PNP_REFINE_REJECTED.
 * INSUFFICIENT and NO_MODEL give a NaN pose, 0 inliers, NaN rms, best -2 and zero bits -- never an
 * identity pose, which would read as an answer.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_PNP_POINTS_MAX      4096u
#define SLHIP_PNP_HYPOTHESES_MAX  4096u
#define SLHIP_PNP_REFINE_MAX      16u
#define SLHIP_PNP_OUT_POSE      1u
#define SLHIP_PNP_OUT_N_INLIERS 2u
#define SLHIP_PNP_OUT_RMS       4u
#define SLHIP_PNP_OUT_INLIERS   8u
#define SLHIP_PNP_OUT_BEST      16u
#define SLHIP_PNP_OUT_FLAGS     32u
#define SLHIP_PNP_INSUFFICIENT    1      /* flags: fewer than 4 valid correspondences                          */
#define SLHIP_PNP_NO_MODEL        2      /* flags: no hypothesis reached min_inliers                           */
#define SLHIP_PNP_REFINE_STOPPED  4      /* flags: a pivot of the normal equations was not positive and finite */
#define SLHIP_PNP_REFINE_REJECTED 8      /* flags: the refined pose held fewer inliers; the winner is returned */

typedef struct {
    float fx, fy, cx, cy;      /* intrinsics of every set without a row in d_intrinsics; fx, fy > 0, all finite */
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* K, 4..SLHIP_PNP_POINTS_MAX                                                  */
    uint32_t n_hypotheses;     /* Hy, 0..SLHIP_PNP_HYPOTHESES_MAX; 0 needs d_init (a pure refinement)         */
    float threshold_px;        /* inlier threshold in pixels, > 0 and finite                                  */
    uint32_t refine_iters;     /* 0..SLHIP_PNP_REFINE_MAX                                                     */
    uint32_t min_inliers;      /* >= 4                                                                        */
    uint32_t seed_lo, seed_hi; /* Philox key                                                                  */
    uint32_t set_id_base;      /* set i draws as set_id_base + i                                              */
    uint32_t outputs;          /* SLHIP_PNP_OUT_* bits, at least one                                          */
    uint32_t _pad[2];
} slhip_pose_pnp_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set                                               */
    float* pose;               /* f32 [M, 3, 4], object to camera                                             */
    int32_t* n_inliers;        /* i32 [M]                                                                     */
    float* rms;                /* f32 [M], reprojection RMS of the inliers in pixels                          */
    uint32_t* inliers;         /* u32 [M, ceil(K / 32)], bit j & 31 of word j >> 5                            */
    int32_t* best;             /* i32 [M], the winning hypothesis; -1: d_init; -2: none                       */
    int32_t* flags;            /* i32 [M], SLHIP_PNP_* flag bits                                              */
} slhip_pose_pnp_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_pnp_check_params(const slhip_pose_pnp_params* params);
/* d_uv f32 [M, K, 2] (8-byte aligned); d_xyz f32 [M, K, 4]: the object-frame point and a weight word (16-byte aligned;
 * slhip_object_points_gather's d_coord works as it is, its w is the camera depth); d_intrinsics NULL or f32 [M, 4] (fx, fy, cx,
 * cy) per set, 16-byte aligned (a crop has its own); d_init NULL or f32 [M, 3, 4], a pose that competes as index -1 and wins
 * ties.  Every output named in params->outputs is written exactly once per set, the others are not touched.  n_sets == 0 does
 * nothing; null pointers (an output named in the mask included), misalignment, Hy == 0 without d_init and bad parameters are
 * refused before anything touches the device.  One workgroup per set.  Asynchronous on `stream`.                          */
int slhip_pose_pnp(const slhip_pose_pnp_params* params, const float* d_uv, const float* d_xyz, const float* d_intrinsics,
                   const float* d_init, const slhip_pose_pnp_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_pnp_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_pnp_host(const slhip_pose_pnp_params* params, const float* h_uv, const float* h_xyz, const float* h_intrinsics,
                        const float* h_init, const slhip_pose_pnp_out* out);
/* The minimal solver alone: uv f32 [3, 2], xyz f32 [3, 3], intrinsics f32 [4], poses_out f32 [4, 3, 4].  Returns the number of
 * solutions kept (0..4), written to the front of poses_out, or a negative error.  Host only, no device.                  */
int slhip_pose_pnp_p3p_host(const float* uv, const float* xyz, const float* intrinsics, float* poses_out);
/* Developer hook (tools/time_pose_pnp.py): HIP events round the last slhip_pose_pnp [0] and the last one that sampled
 * hypotheses, n_hypotheses > 0 [1] (-1: not run).                                                                        */
int slhip_pose_pnp_timing_enable(int on);
int slhip_pose_pnp_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Keypoint voting: one 2D position, with an uncertainty, per (set, keypoint) from a predicted field of
 * per-pixel unit vectors -- PVNet's RANSAC voting layer, the step between the vector-field target
 * (slhip_object_keypoints_field) and slhip_pose_pnp.  This project's addition, the reference has no
 * counterpart.  All float32, one rounded IEEE operation at a time (no fma), only + - * / sqrt fabs and
 * comparisons; csrc/slhip_vote_rules.h holds the rules for host and device, so slhip_keypoint_vote_host
 * gives the device's outputs bit for bit.  DESIGN.md "Keypoint voting" states them operation by
 * operation; in short, per set m and keypoint k:
 *   1. valid list: voter j counts when its pixel lies in [0, W) x [0, H), its scene lies in the field
 *      (dense mode; nothing is read otherwise), (vx, vy) is finite and l = sqrtf(vx*vx + vy*vy) > 0; then
 *      d = (vx / l, vy / l), p = ((float)x + 0.5f, (float)y + 0.5f).  The valid ones are taken in ascending
 *      j, n_valid of them; fewer than 2: SLHIP_VOTE_INSUFFICIENT.
 *   2. hypothesis h draws Philox counter (set_id_base + m, 8, h, k) under (seed_lo, seed_hi)
 *      ("Randomness" below); words 0 and 1 pick a and b, each min(n_valid - 1, (uint32_t)(uniform(x) *
 *      (float)n_valid)).  Void when a == b, p_a == p_b, det = d_a.x*d_b.y - d_a.y*d_b.x has fabsf(det) <=
 *      min_sin, or q is not finite; else s = ((p_b.x - p_a.x)*d_b.y - (p_b.y - p_a.y)*d_b.x) / det and
 *      q = (p_a.x + s*d_a.x, p_a.y + s*d_a.y).
 *   3. score: with e = q - p_j, dot = e.x*d.x + e.y*d.y, n2 = e.x*e.x + e.y*e.y, voter j is an inlier when
 *      n2 == 0 or (dot > 0 and dot*dot >= (inlier_cos*inlier_cos) * n2).  A void hypothesis scores 0.  The
 *      winner: highest count, ties to the lowest h.  A winner below min_inliers: SLHIP_VOTE_NO_MODEL.
 *   4. distribution over the non-void hypotheses, w_h = (float)count_h / (float)n_valid: mean = (sum(w*q.x)
 *      / sum(w), sum(w*q.y) / sum(w)); cov = the sums of (w*gx)*gx, (w*gx)*gy, (w*gy)*gy, g = q - mean, each
 *      / sum(w).  Every sum in the order of the pose errors' means: lane h % 256 takes its hypotheses
 *      upwards from 0.0f, the butterfly in a wave, ((w0 + w1) + w2) + w3.
 *   5. refinement: one least-squares step on the winner's inliers of the valid list (lane i % 256):
 *      n = (-d.y, d.x), c = n . (p - q) by line_offset of slhip_vote_rules.h (the differences, the products
 *      and their sum formed error-free from rounded + - *, the lost parts added back smallest first: c is
 *      the small rest of two products of the size of |p - q| and would otherwise keep their rounding); the
 *      sums a00 n.x*n.x, a01 n.x*n.y, a11 n.y*n.y, b0 n.x*c, b1 n.y*c; det = a00*a11 - a01*a01 not finite or
 *      not > 0: SLHIP_VOTE_REFINE_STOPPED and uv = q; else uv = (q.x + (b0*a11 - a01*b1) / det, q.y +
 *      (a00*b1 - a01*b0) / det).
 *   6. inliers and count of uv by rule 3 over the voters in their own order; fewer than the winner's
 *      score: q and its figures with SLHIP_VOTE_REFINE_REJECTED.
 * INSUFFICIENT and NO_MODEL give NaN uv, mean and cov, 0 inliers, best -2 and zero bits -- a position is
 * never zero-filled.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_VOTE_POINTS_MAX      4096u
#define SLHIP_VOTE_HYPOTHESES_MAX  1024u
#define SLHIP_VOTE_OUT_UV        1u
#define SLHIP_VOTE_OUT_N_INLIERS 2u
#define SLHIP_VOTE_OUT_BEST      4u
#define SLHIP_VOTE_OUT_FLAGS     8u
#define SLHIP_VOTE_OUT_MEAN      16u
#define SLHIP_VOTE_OUT_COV       32u
#define SLHIP_VOTE_OUT_INLIERS   64u
#define SLHIP_VOTE_INSUFFICIENT    1     /* flags: fewer than 2 valid voters                                    */
#define SLHIP_VOTE_NO_MODEL        2     /* flags: no hypothesis reached min_inliers                            */
#define SLHIP_VOTE_REFINE_STOPPED  4     /* flags: the normal equations were singular; uv is the winner's q     */
#define SLHIP_VOTE_REFINE_REJECTED 8     /* flags: the refined position held fewer inliers; q is returned       */

typedef struct {
    uint32_t W, H;             /* the picture the pixels lie in, each side 1..32768                           */
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* K voters per set, 2..SLHIP_VOTE_POINTS_MAX                                  */
    uint32_t n_keypoints;      /* Kp, 1..SLHIP_KEYPOINTS_MAX                                                  */
    uint32_t n_hypotheses;     /* Hy, 1..SLHIP_VOTE_HYPOTHESES_MAX                                            */
    float inlier_cos;          /* in (0, 1): the smallest cosine between a voter's vector and its view of q   */
    uint32_t min_inliers;      /* >= 2                                                                        */
    float min_sin;             /* >= 0 and finite: the smallest |d_a x d_b| a sampled pair may have           */
    uint32_t outputs;          /* SLHIP_VOTE_OUT_* bits, at least one                                         */
    uint32_t seed_lo, seed_hi; /* Philox key                                                                  */
    uint32_t set_id_base;      /* set m draws as set_id_base + m                                              */
    uint32_t _pad[3];
} slhip_keypoint_vote_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    float* uv;                 /* f32 [M, Kp, 2], the keypoint's pixel position                               */
    int32_t* n_inliers;        /* i32 [M, Kp]                                                                 */
    int32_t* best;             /* i32 [M, Kp], the winning hypothesis; -2: none                               */
    int32_t* flags;            /* i32 [M, Kp], SLHIP_VOTE_* flag bits                                         */
    float* mean;               /* f32 [M, Kp, 2], the weighted mean of the hypotheses                         */
    float* cov;                /* f32 [M, Kp, 3], their weighted covariance (xx, xy, yy)                      */
    uint32_t* inliers;         /* u32 [M, Kp, ceil(K / 32)], bit j & 31 of word j >> 5                        */
} slhip_keypoint_vote_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_keypoint_vote_check_params(const slhip_keypoint_vote_params* params);
/* d_pixel i16 [M, K, 2] (x, y), 4-byte aligned: the `pixel` of slhip_object_points_gather.  With d_scene (i32 [M]) non-null
 * d_vectors is a dense field f32 [n_field_scenes, H, W, Kp, 2] (slhip_object_keypoints_field's layout, or a network's) and
 * voter j of set m is read at (d_scene[m], y, x); a scene outside [0, n_field_scenes) or a pixel outside the picture reads
 * nothing.  With d_scene null d_vectors is already gathered, f32 [M, K, Kp, 2] (networks that run on crops).  d_vectors is
 * 8-byte aligned.  Every output named in params->outputs is written for every (set, keypoint), the others are not
 * touched.  n_sets == 0 does nothing; null pointers (an output named in the mask included), misalignment, n_field_scenes < 1
 * in dense mode and bad parameters are refused before anything touches the device.  One workgroup per (set, keypoint).
 * Asynchronous on `stream`.                                                                                              */
int slhip_keypoint_vote(const slhip_keypoint_vote_params* params, const int16_t* d_pixel, const float* d_vectors,
                        const int32_t* d_scene, uint32_t n_field_scenes, const slhip_keypoint_vote_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_vote_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_keypoint_vote_host(const slhip_keypoint_vote_params* params, const int16_t* h_pixel, const float* h_vectors,
                             const int32_t* h_scene, uint32_t n_field_scenes, const slhip_keypoint_vote_out* out);
/* Developer hook (tools/time_keypoint_vote.py): HIP events round the last slhip_keypoint_vote [0] and the last one that read
 * a dense field [1] (-1: not run).                                                                                       */
int slhip_keypoint_vote_timing_enable(int on);
int slhip_keypoint_vote_timings(float ms_out[2]);

/* ---------------------------------------------------------------------------------------------
 * Keypoint voting in 3D: one camera-frame position, with an uncertainty, per (set, keypoint) from
 * per-point predicted 3D offsets (the layout of ObjectKeypoints.offsets) -- the decoder of PVN3D /
 * FFB6D, by mean shift over the candidates and the mode with the most support.  This project's addition,
 * the reference has no counterpart.  All float32, one rounded IEEE operation at a time (no fma), only
 * + - * / and comparisons (no exp: the kernel of the mean shift is compact, not Gaussian);
 * csrc/slhip_vote3d_rules.h holds the rules for host and device, so slhip_keypoint_vote3d_host gives the
 * device's outputs bit for bit.  Nothing is random.  Per set m and keypoint k, with h = bandwidth,
 * h2 = h*h, inv_h2 = 1 / (h*h), tol2 = tol*tol:
 *   1. candidate c_j = (camera_j.x + offset_jk.x, .y + .y, .z + .z), valid when camera_j.w != 0 and the three
 *      sums are finite.  The valid ones keep their ascending order in j, n_valid of them; none:
 *      SLHIP_VOTE3D_INSUFFICIENT.
 *   2. seeds: S_eff = min(n_seeds, n_valid); seed s starts at the valid candidate of rank
 *      ((2 s + 1) * n_valid) / (2 * S_eff) in integers -- with n_seeds >= n_valid every candidate is a seed.
 *   3. one step of seed x: over the valid candidates in ascending order, one after the other from 0.0f
 *      (acc = acc + term): d = c_j - x per component, t = ((d.x*d.x + d.y*d.y) + d.z*d.z) * inv_h2,
 *      w = t < 1 ? 1 - t : 0, and the four sums of w, w*d.x, w*d.y, w*d.z.  Then m = (sum w*d) / (sum w) per
 *      component and x = x + m.  The seed stops when (m.x*m.x + m.y*m.y) + m.z*m.z <= tol2, or after
 *      max_iters steps.  (sum w > 0 for a seed that started on a candidate: slhip_vote3d_rules.h.)
 *   4. support of a finished seed: the valid candidates with ((d.x*d.x + d.y*d.y) + d.z*d.z) <= h2.  The
 *      winner: highest support, ties to the lowest s.  A winner below min_support: SLHIP_VOTE3D_NO_MODEL.
 *      A winner that took max_iters steps without stopping: SLHIP_VOTE3D_NOT_CONVERGED, its outputs are
 *      written all the same.
 *   5. over the winner's supporters: mean = sum(c) / (float)n_support per component; cov = the sums of
 *      g.x*g.x, g.x*g.y, g.x*g.z, g.y*g.y, g.y*g.z, g.z*g.z, g = c - mean, each / (float)n_support.  Every
 *      sum in the order of the pose errors' means over the valid list: lane i % 256 takes its supporters
 *      i upwards from 0.0f, the butterfly in a wave, ((w0 + w1) + w2) + w3.
 * INSUFFICIENT and NO_MODEL give NaN xyz, mean and cov, 0 supporters, best -2, 0 iterations and zero bits --
 * a position is never zero-filled.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_VOTE3D_POINTS_MAX  4096u
#define SLHIP_VOTE3D_SEEDS_MAX   1024u
#define SLHIP_VOTE3D_ITERS_MAX   64u
#define SLHIP_VOTE3D_OUT_XYZ       1u
#define SLHIP_VOTE3D_OUT_N_SUPPORT 2u
#define SLHIP_VOTE3D_OUT_BEST      4u
#define SLHIP_VOTE3D_OUT_ITERS     8u
#define SLHIP_VOTE3D_OUT_FLAGS     16u
#define SLHIP_VOTE3D_OUT_MEAN      32u
#define SLHIP_VOTE3D_OUT_COV       64u
#define SLHIP_VOTE3D_OUT_SUPPORT   128u
#define SLHIP_VOTE3D_INSUFFICIENT  1     /* flags: no valid voter                                               */
#define SLHIP_VOTE3D_NO_MODEL      2     /* flags: no mode reached min_support                                  */
#define SLHIP_VOTE3D_NOT_CONVERGED 4     /* flags: the winner took max_iters steps without meeting tol          */

typedef struct {
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* K voters per set, 1..SLHIP_VOTE3D_POINTS_MAX                                */
    uint32_t n_keypoints;      /* Kp, 1..SLHIP_KEYPOINTS_MAX                                                  */
    uint32_t n_seeds;          /* S, 1..SLHIP_VOTE3D_SEEDS_MAX                                                */
    float bandwidth;           /* h > 0 and finite, in the unit of the camera points (metres)                 */
    uint32_t max_iters;        /* 1..SLHIP_VOTE3D_ITERS_MAX                                                   */
    float tol;                 /* >= 0 and finite: a seed stops when its shift squared is <= tol*tol          */
    uint32_t min_support;      /* >= 1                                                                        */
    uint32_t outputs;          /* SLHIP_VOTE3D_OUT_* bits, at least one                                       */
    uint32_t _pad[7];
} slhip_keypoint_vote3d_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    float* xyz;                /* f32 [M, Kp, 3], the winner's mode in the camera frame                       */
    int32_t* n_support;        /* i32 [M, Kp]                                                                 */
    int32_t* best;             /* i32 [M, Kp], the winning seed; -2: none                                     */
    int32_t* iters;            /* i32 [M, Kp], the steps the winner took                                      */
    int32_t* flags;            /* i32 [M, Kp], SLHIP_VOTE3D_* flag bits                                       */
    float* mean;               /* f32 [M, Kp, 3], the mean of the winner's supporters                         */
    float* cov;                /* f32 [M, Kp, 6], their covariance (xx, xy, xz, yy, yz, zz)                   */
    uint32_t* support;         /* u32 [M, Kp, ceil(K / 32)], bit j & 31 of word j >> 5                        */
} slhip_keypoint_vote3d_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_keypoint_vote3d_check_params(const slhip_keypoint_vote3d_params* params);
/* d_camera f32 [M, K, 4] (x, y, z, w), 16-byte aligned: the `camera` of slhip_object_points_gather.  d_offsets f32
 * [M, K, Kp, 3], 4-byte aligned.  Every output named in params->outputs is written for every (set, keypoint), the others are
 * not touched.  n_sets == 0 does nothing; null pointers (an output named in the mask included), misalignment and bad
 * parameters are refused before anything touches the device.  One workgroup per (set, keypoint).  Asynchronous on `stream`. */
int slhip_keypoint_vote3d(const slhip_keypoint_vote3d_params* params, const float* d_camera, const float* d_offsets,
                          const slhip_keypoint_vote3d_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_vote3d_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_keypoint_vote3d_host(const slhip_keypoint_vote3d_params* params, const float* h_camera, const float* h_offsets,
                               const slhip_keypoint_vote3d_out* out);
/* Developer hook (tools/time_keypoint_vote3d.py): HIP events round the last slhip_keypoint_vote3d [0] (-1: not run). */
int slhip_keypoint_vote3d_timing_enable(int on);
int slhip_keypoint_vote3d_timings(float ms_out[1]);

/* ---------------------------------------------------------------------------------------------
 * Rigid fit: the pose (object to camera) of every set of N 3D-3D correspondences in the least-squares
 * sense, by Horn's unit-quaternion form -- bank keypoints onto voted keypoints (the PVN3D pose), or
 * predicted object coordinates onto camera points (the depth counterpart of slhip_pose_pnp).  This
 * project's addition.  All float32, one rounded IEEE operation at a time, only + - * / sqrt fabs and
 * comparisons; csrc/slhip_fit_rules.h holds the rules for host and device, so slhip_pose_fit_host gives
 * the device's outputs bit for bit.  Per set:
 *   1. correspondence j counts when src.w > 0 and dst.w != 0 and the six coordinates are finite; n_used of
 *      them; fewer than 3: SLHIP_FIT_INSUFFICIENT.
 *   2. centroids cs, cd = sum / (float)n_used; then the nine sums M[3 i + j] of (src_i - cs_i) * (dst_j -
 *      cd_j).  Every sum in the order of the pose errors' means: lane j % 256 takes its correspondences
 *      upwards from 0.0f, the butterfly in a wave, ((w0 + w1) + w2) + w3.
 *   3. Horn's symmetric matrix in quaternion order (w, x, y, z): diagonal (Sxx + Syy) + Szz, (Sxx - Syy) -
 *      Szz, (Syy - Sxx) - Szz, (Szz - Sxx) - Syy; N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy
 *      + Syx, N13 = Szx + Sxz, N23 = Syz + Szy.  Then 8 cyclic Jacobi sweeps over the pairs (0,1) (0,2) (0,3)
 *      (1,2) (1,3) (2,3): a pair whose off-diagonal is exactly 0 is skipped; theta = (aqq - app) / (2 apq),
 *      t = sign(theta) / (fabsf(theta) + sqrtf(theta*theta + 1)) with sign(0) = +1, c = 1 / sqrtf(t*t + 1),
 *      s = t*c; app -= t*apq, aqq += t*apq, apq = 0; for the other k: akp' = c*akp - s*akq, akq' = s*akp +
 *      c*akq; the eigenvector columns likewise.
 *   4. the quaternion is the column of the largest diagonal entry (ties to the lowest column), divided by
 *      its length sqrtf(((q0*q0 + q1*q1) + q2*q2) + q3*q3), negated when w < 0.
 *   5. R = (1 - 2(yy + zz), 2(xy - wz), 2(xz + wy); 2(xy + wz), 1 - 2(xx + zz), 2(yz - wx); 2(xz - wy),
 *      2(yz + wx), 1 - 2(xx + yy)) and t_i = cd_i - ((R_i0*cs.x + R_i1*cs.y) + R_i2*cs.z): a proper rotation
 *      always, flat point sets included -- there is no reflection branch.
 *   6. when the two largest eigenvalues differ by no more than min_gap * the sum of the four absolute
 *      eigenvalues (collinear or coincident points): SLHIP_FIT_DEGENERATE.
 *   7. rms = sqrtf(sum(|R src + t - dst|^2) / (float)n_used), each row ((R_i0*x + R_i1*y) + R_i2*z) + t_i,
 *      the sum in the order of rule 2.
 * INSUFFICIENT and DEGENERATE give a NaN pose and rms -- never an identity; n_used is the count in
 * every case.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_FIT_POINTS_MAX   4096u
#define SLHIP_FIT_OUT_POSE     1u
#define SLHIP_FIT_OUT_N_USED   2u
#define SLHIP_FIT_OUT_RMS      4u
#define SLHIP_FIT_OUT_FLAGS    8u
#define SLHIP_FIT_INSUFFICIENT 1     /* flags: fewer than 3 correspondences count                               */
#define SLHIP_FIT_DEGENERATE   2     /* flags: collinear or coincident points                                   */

typedef struct {
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* N correspondences per set, 1..SLHIP_FIT_POINTS_MAX                          */
    float min_gap;             /* in [0, 1): rule 6                                                           */
    uint32_t outputs;          /* SLHIP_FIT_OUT_* bits, at least one                                          */
    uint32_t _pad[12];
} slhip_pose_fit_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    float* pose;               /* f32 [M, 3, 4], object to camera                                             */
    int32_t* n_used;           /* i32 [M]                                                                     */
    float* rms;                /* f32 [M], in the unit of the points                                          */
    int32_t* flags;            /* i32 [M], SLHIP_FIT_* flag bits                                              */
} slhip_pose_fit_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_fit_check_params(const slhip_pose_fit_params* params);
/* d_src f32 [M, N, 4] object frame, d_dst f32 [M, N, 4] camera frame, both 16-byte aligned.  Every output named in
 * params->outputs is written for every set, the others are not touched.  n_sets == 0 does nothing; null pointers,
 * misalignment and bad parameters are refused before anything touches the device.  One workgroup per set.  Asynchronous
 * on `stream`.                                                                                                           */
int slhip_pose_fit(const slhip_pose_fit_params* params, const float* d_src, const float* d_dst, const slhip_pose_fit_out* out,
                   void* stream);
/* The same rules on host arrays through csrc/slhip_fit_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_fit_host(const slhip_pose_fit_params* params, const float* h_src, const float* h_dst, const slhip_pose_fit_out* out);
/* Developer hook: HIP events round the last slhip_pose_fit [0] (-1: not run). */
int slhip_pose_fit_timing_enable(int on);
int slhip_pose_fit_timings(float ms_out[1]);

/* ---------------------------------------------------------------------------------------------
 * Robust alignment: the pose (object to camera) of every set of K 3D-3D correspondences that has the
 * most inliers, refitted on them -- RANSAC round the rigid fit above, for predicted object coordinates
 * or voted keypoints of which some are wrong by the size of the object (slhip_pose_fit is plain least
 * squares and is ruined by one of them).  This project's addition.  All float32, one rounded IEEE
 * operation at a time, only + - * / sqrt fabs and comparisons; csrc/slhip_align_rules.h holds the rules
 * for host and device, so slhip_pose_align_host gives the device's outputs bit for bit.  DESIGN.md
 * "Robust alignment" states them operation by operation; in short, per set:
 *   1. valid list: correspondence j counts by rule 1 of "Rigid fit" (src.w > 0, dst.w != 0, the six
 *      coordinates finite); the valid ones are taken in ascending j, n_valid of them; fewer than 3:
 *      SLHIP_ALIGN_INSUFFICIENT.
 *   2. hypothesis h draws Philox counter (set_id_base + set, 9, h, 0x51DE5EED) under (seed_lo, seed_hi)
 *      ("Randomness" below); words 0, 1, 2 each pick min(n_valid - 1, (uint32_t)(uniform(x) *
 *      (float)n_valid)) of the valid list; two equal picks: void.
 *   3. rules 2 to 6 of "Rigid fit" on the three pairs: centroids ((p0 + p1) + p2) / 3.0f, the nine moments
 *      (a0_i*b0_j + a1_i*b1_j) + a2_i*b2_j of the centred pairs, Horn's matrix, 8 Jacobi sweeps, the
 *      quaternion and min_gap.  A degenerate sample (collinear or coincident) or a pose entry that is
 *      not finite: void.
 *   4. score = the number of valid correspondences with |R s + t - d|^2 <= threshold * threshold, the
 *      residual of rule 7 of "Rigid fit"; a NaN compares false, a void hypothesis scores 0.  Slot 0 is
 *      d_init (not finite: scores 0), slot h + 1 hypothesis h; the winner is the arg-max of (count << 13) |
 *      (4097 - slot): highest score, ties to the lowest slot, so d_init (index -1) wins ties.  A winner
 *      below min_inliers: SLHIP_ALIGN_NO_MODEL.
 *   5. refine_iters times: the inliers of the current pose among the valid list, then rules 2 to 6 of
 *      "Rigid fit" on them, lanes over the list index i (lane i % 256 upwards, the butterfly, ((w0 + w1) +
 *      w2) + w3).  Fewer than 3 inliers or a degenerate fit: SLHIP_ALIGN_REFINE_STOPPED, the pose stays
 *      and the loop ends.
 *   6. inliers, count and rms = sqrtf(sum of squared residuals / (float)count) of the refitted pose over
 *      the correspondences j in their own order (lane j % 256); fewer inliers than the winner's score:
 *      the winner's pose and figures with SLHIP_ALIGN_REFINE_REJECTED.
 * INSUFFICIENT and NO_MODEL give a NaN pose, 0 inliers, NaN rms, best -2 and zero bits -- never an
 * identity pose and never d_init.  Rigid motions only: a similarity scale (Umeyama) is not estimated.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_ALIGN_POINTS_MAX      4096u
#define SLHIP_ALIGN_HYPOTHESES_MAX  4096u
#define SLHIP_ALIGN_REFINE_MAX      16u
#define SLHIP_ALIGN_OUT_POSE      1u
#define SLHIP_ALIGN_OUT_N_INLIERS 2u
#define SLHIP_ALIGN_OUT_RMS       4u
#define SLHIP_ALIGN_OUT_INLIERS   8u
#define SLHIP_ALIGN_OUT_BEST      16u
#define SLHIP_ALIGN_OUT_FLAGS     32u
#define SLHIP_ALIGN_INSUFFICIENT    1      /* flags: fewer than 3 valid correspondences                        */
#define SLHIP_ALIGN_NO_MODEL        2      /* flags: no hypothesis reached min_inliers                         */
#define SLHIP_ALIGN_REFINE_STOPPED  4      /* flags: a refit had fewer than 3 inliers or was degenerate        */
#define SLHIP_ALIGN_REFINE_REJECTED 8      /* flags: the refitted pose held fewer inliers; the winner is returned */

typedef struct {
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* K, 3..SLHIP_ALIGN_POINTS_MAX                                                */
    uint32_t n_hypotheses;     /* Hy, 0..SLHIP_ALIGN_HYPOTHESES_MAX; 0 needs d_init (a pure refit)            */
    float threshold;           /* inlier threshold in the unit of the points, > 0 and finite                  */
    float min_gap;             /* in [0, 1): rule 6 of "Rigid fit", for the samples and the refits            */
    uint32_t refine_iters;     /* 0..SLHIP_ALIGN_REFINE_MAX                                                   */
    uint32_t min_inliers;      /* >= 3                                                                        */
    uint32_t seed_lo, seed_hi; /* Philox key                                                                  */
    uint32_t set_id_base;      /* set i draws as set_id_base + i                                              */
    uint32_t outputs;          /* SLHIP_ALIGN_OUT_* bits, at least one                                        */
    uint32_t _pad[5];
} slhip_pose_align_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    float* pose;               /* f32 [M, 3, 4], object to camera                                             */
    int32_t* n_inliers;        /* i32 [M]                                                                     */
    float* rms;                /* f32 [M], RMS of |R src + t - dst| over the inliers, in the unit of the points */
    uint32_t* inliers;         /* u32 [M, ceil(K / 32)], bit j & 31 of word j >> 5                            */
    int32_t* best;             /* i32 [M], the winning hypothesis; -1: d_init; -2: none                       */
    int32_t* flags;            /* i32 [M], SLHIP_ALIGN_* flag bits                                            */
} slhip_pose_align_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_align_check_params(const slhip_pose_align_params* params);
/* d_src f32 [M, K, 4] object frame, d_dst f32 [M, K, 4] camera frame, both 16-byte aligned (the layouts of slhip_pose_fit);
 * d_init NULL or f32 [M, 3, 4], 4-byte aligned: a pose that competes as index -1 and wins ties.  Every output named in
 * params->outputs is written exactly once per set, the others are not touched.  n_sets == 0 does nothing; null pointers (an
 * output named in the mask included), misalignment, Hy == 0 without d_init and bad parameters are refused before anything
 * touches the device.  One workgroup per set, the valid list in 24 * K bytes of LDS.  Asynchronous on `stream`.          */
int slhip_pose_align(const slhip_pose_align_params* params, const float* d_src, const float* d_dst, const float* d_init,
                     const slhip_pose_align_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_align_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_align_host(const slhip_pose_align_params* params, const float* h_src, const float* h_dst, const float* h_init,
                          const slhip_pose_align_out* out);
/* Developer hook (tools/time_pose_align.py): HIP events round the last slhip_pose_align [0] (-1: not run). */
int slhip_pose_align_timing_enable(int on);
int slhip_pose_align_timings(float ms_out[1]);

/* ---------------------------------------------------------------------------------------------
 * ICP: the pose (object to camera) of every set of K camera points refined against the points of its
 * class in a slhip_pose_bank, point to point, from an initial pose -- the refinement step of DenseFusion,
 * PVN3D, FFB6D, PoseCNN+ICP and the BOP baselines.  This project's addition.  The loop round two rules
 * that exist: the nearest-neighbour walk of the pose errors' ADD-S and the rigid fit.  All float32, one
 * rounded IEEE operation at a time; csrc/slhip_icp_rules.h holds the rules for host and device, so
 * slhip_pose_icp_host gives the device's outputs bit for bit.  Per set i, class c = classes[i]:
 *   1. the set can start when 0 <= c < n_assets and 1 <= count[c] <= n_points of the bank (else
 *      SLHIP_ICP_BAD_CLASS) and the 12 entries of init[i] are finite (else SLHIP_ICP_NO_INIT).  A set that
 *      cannot start has a NaN pose and rms, iters 0, n_pairs 0 and nearest -1 throughout.
 *   2. camera point j counts when its w != 0 and x, y, z are finite.
 *   3. into the object frame with the current pose (R, t):  d = c - t per component,
 *      q_k = (R[0][k]*d0 + R[1][k]*d1) + R[2][k]*d2  (R transposed).  The bank is never transformed.
 *   4. the nearest bank point: m scans [0, count[c]) upwards from (best = +inf, no index); point m replaces
 *      the best when dist2(q, p_m) < best, dist2 = (dx*dx + dy*dy) + dz*dz of the pose errors -- the
 *      smallest distance, among equals the lowest index.  A distance of NaN or +inf never wins; rows past
 *      count[c] are never read.
 *   5. the pair (j, m) counts when the point counts, an index won and best <= gate * gate (+inf passes, NaN
 *      fails).  gate_0 = max_dist; after every fit gate = max(gate * dist_scale, min_dist).  n_pairs of
 *      them; nearest[j] = m, or -1 without a pair.  Fewer than min_pairs: SLHIP_ICP_INSUFFICIENT.
 *   6. the rigid fit of the pairs, src = the bank point, dst = the camera point, by rules 2 to 6 of "Rigid
 *      fit" unchanged (centroids, moments, Horn, 8 Jacobi sweeps, quaternion, min_gap); lane j % 256
 *      takes its pairs upwards, the butterfly in a wave, ((w0 + w1) + w2) + w3.  The result is the new
 *      absolute pose -- poses are never composed, every iterate is a proper rotation.  A degenerate fit:
 *      SLHIP_ICP_DEGENERATE.
 *   7. rms = sqrtf(sum(|R src + t - dst|^2) / (float)n_pairs) of the new pose over the pairs of the fit, the
 *      sum in the order of rule 6.
 *   8. the loop ends when every |R_new - R_old| entry <= tol_rot and every |t_new - t_old| entry <= tol_trans
 *      (SLHIP_ICP_CONVERGED, not a failure), or after max_iters fits.  iters = the fits done.
 * INSUFFICIENT and DEGENERATE end the loop with a NaN pose and rms -- never an identity, never the init;
 * n_pairs and nearest are those of the last association in every case.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_ICP_POINTS_MAX    4096u
#define SLHIP_ICP_ITERS_MAX     64u
#define SLHIP_ICP_OUT_POSE      1u
#define SLHIP_ICP_OUT_N_PAIRS   2u
#define SLHIP_ICP_OUT_RMS       4u
#define SLHIP_ICP_OUT_ITERS     8u
#define SLHIP_ICP_OUT_FLAGS     16u
#define SLHIP_ICP_OUT_NEAREST   32u
#define SLHIP_ICP_BAD_CLASS     1     /* flags: the class lies outside the bank or has no points                 */
#define SLHIP_ICP_NO_INIT       2     /* flags: the initial pose is not finite                                   */
#define SLHIP_ICP_INSUFFICIENT  4     /* flags: fewer than min_pairs pairs                                       */
#define SLHIP_ICP_DEGENERATE    8     /* flags: the pairs' bank points are collinear or coincident               */
#define SLHIP_ICP_CONVERGED     16    /* flags: the pose moved by no more than the tolerances (not a failure)    */
#define SLHIP_ICP_FAILED        15    /* the failure bits                                                        */

typedef struct {
    uint32_t n_sets;           /* M                                                                           */
    uint32_t n_points;         /* K camera points per set, 1..SLHIP_ICP_POINTS_MAX                            */
    uint32_t max_iters;        /* 1..SLHIP_ICP_ITERS_MAX fits                                                 */
    uint32_t min_pairs;        /* >= 3                                                                        */
    float max_dist;            /* >= 0, +inf: no gate; rule 5                                                 */
    float dist_scale;          /* in (0, 1]                                                                   */
    float min_dist;            /* >= 0                                                                        */
    float min_gap;             /* in [0, 1): rule 6 of "Rigid fit"                                            */
    float tol_rot;             /* >= 0                                                                        */
    float tol_trans;           /* >= 0                                                                        */
    uint32_t outputs;          /* SLHIP_ICP_OUT_* bits, at least one                                          */
    uint32_t _pad[5];
} slhip_pose_icp_params; /* 64 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    float* pose;               /* f32 [M, 3, 4], object to camera                                             */
    int32_t* n_pairs;          /* i32 [M]                                                                     */
    float* rms;                /* f32 [M], in the unit of the points                                          */
    int32_t* iters;            /* i32 [M]                                                                     */
    int32_t* flags;            /* i32 [M], SLHIP_ICP_* flag bits                                              */
    int32_t* nearest;          /* i32 [M, K]                                                                  */
} slhip_pose_icp_out;

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_pose_icp_check_params(const slhip_pose_icp_params* params);
/* d_camera f32 [M, K, 4] (the layout of the point sets' camera output) and d_init f32 [M, 3, 4], both 16-byte aligned;
 * d_classes i32 [M]; of the bank only points and count are read.  Every output named in params->outputs is written for
 * every set, the others are not touched.  n_sets == 0 does nothing; null pointers, misalignment, a bank out of range and
 * bad parameters are refused before anything touches the device.  One workgroup per set, the class's points in LDS.
 * Asynchronous on `stream`.                                                                                              */
int slhip_pose_icp(const slhip_pose_icp_params* params, const float* d_camera, const float* d_init, const int32_t* d_classes,
                   const slhip_pose_bank* bank, const slhip_pose_icp_out* out, void* stream);
/* The same rules on host arrays through csrc/slhip_icp_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_pose_icp_host(const slhip_pose_icp_params* params, const float* h_camera, const float* h_init, const int32_t* h_classes,
                        const slhip_pose_bank* h_bank, const slhip_pose_icp_out* out);
/* Developer hook (tools/time_pose_icp.py): HIP events round the last slhip_pose_icp [0] (-1: not run). */
int slhip_pose_icp_timing_enable(int on);
int slhip_pose_icp_timings(float ms_out[1]);

/* ---------------------------------------------------------------------------------------------
 * Render flow: where every pixel of one render (picture a) lands in another render of the same scene
 * (picture b) -- optical flow, scene flow and an occlusion flag, the targets of flow networks (RAFT)
 * and of flow-based 6D refiners (Coupled Iterative Refinement, SCFlow, PFA, GenFlow, DeepIM's flow
 * head), and the co-visibility of a view pair.  Stands in for nothing on the reference's side: this
 * project's addition, the reference has no counterpart.  Exact geometry and exact motion: the depth of
 * a (the w of its coord target), its instance plane and, per instance slot, the rigid motion from
 * camera frame a to camera frame b.  Both pictures share the intrinsics and the size.  All float32,
 * one rounded IEEE operation at a time (no fma), the parenthesisation below is the contract;
 * csrc/slhip_flow_rules.h holds the rules for host and device (with row_point, project, is_finite and
 * unoccluded of "Object keypoints"), tests/render_flow_ref.py restates them in NumPy bit for bit.
 * DESIGN.md "Render flow".
 *
 * Motion table: f32 [B, n_slots, 3, 4], row-major; row i maps a point of camera frame a to camera
 * frame b for the pixels of instance i.  Slot 0 is the plane and the background: the camera's own motion.
 *
 * Pixel (x, y) of scene b of picture a, with z = its depth, i = its instance (read as u16), M = row i:
 *   VALID   z finite and 0 < z < max_depth;  i < n_slots;  all 12 entries of M finite;  the moved point in
 *           front (X', Y', Z' finite and Z' > 0).  The renderer writes 3000 where nothing was hit, so
 *           max_depth = 3000 drops the background and keeps the plane.
 *   X = (((x + 0.5f) - cx) * z) / fx;   Y = (((y + 0.5f) - cy) * z) / fy             (the camera point of "Object points")
 *   X' = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3], Y' and Z' by rows 1 and 2;
 *   u = (fx * X') / Z' + cx;   v = (fy * Y') / Z' + cy
 *   INSIDE  VALID, 0 <= u < W and 0 <= v < H
 *   flow = (u - (x + 0.5f), v - (y + 0.5f));   scene_flow = (X' - X, Y' - Y, Z' - z)
 *   VISIBLE only with a depth plane of picture b:  x0 = floor(u - 0.5f), y0 = floor(v - 0.5f); of the
 *           pixels (x0 + dx, y0 + dy), dx, dy in {0, 1} -- the bilinear footprint of (u, v), tried in the order
 *           (0,0), (1,0), (0,1), (1,1) -- those inside the picture; one passes when (with
 *           SLHIP_FLOW_MATCH_INSTANCE and an instance plane of b) its instance in b equals i, and its depth z_b
 *           is finite, z_b > 0 and Z' <= z_b + (depth_tol + depth_rel * Z').  VISIBLE = VALID, INSIDE and any passes.
 * A pixel that is not VALID gets zeros and flags 0: the flags plane is the mask.
 * counts[b][i] = (pixels of a with instance i, of those the VALID, the INSIDE, the VISIBLE ones): integer
 * sums, the same in any order.
 *
 * Motion of one rigid frame, slhip_render_flow_motion: out = to o inv_rigid(from) on rows 0-2 of two
 * row-major 3 x 4 matrices (R, t):  inv_rigid = (R^T, -(R^T t)), every dot product summed as
 * (a*b + c*d) + e*f, the product's rotation entries the same way, its translation by the row rule of X'
 * above.  A non-finite entry among the 24 gives 12 NaNs (so those pixels are not VALID).  Rigid inputs are
 * assumed and not checked.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_FLOW_SLOTS_MAX 256
#define SLHIP_FLOW_VALID   1u
#define SLHIP_FLOW_INSIDE  2u
#define SLHIP_FLOW_VISIBLE 4u
#define SLHIP_FLOW_OUT_FLOW   1u
#define SLHIP_FLOW_OUT_SCENE  2u
#define SLHIP_FLOW_OUT_FLAGS  4u
#define SLHIP_FLOW_OUT_COUNTS 8u
#define SLHIP_FLOW_MATCH_INSTANCE 1u

typedef struct {
    float fx, fy, cx, cy;      /* intrinsics of both pictures: fx, fy > 0, all four finite                    */
    int32_t W, H;              /* size of both pictures, each side 1..32768                                   */
    uint32_t n_slots;          /* rows of a scene's motion table, 1..SLHIP_FLOW_SLOTS_MAX                     */
    float max_depth;           /* > 0, may be +inf: a pixel of a at or beyond it is not VALID                 */
    float depth_tol;           /* finite and >= 0: how far behind b's surface a moved point still shows       */
    float depth_rel;           /* finite and >= 0: the same as a share of Z'                                  */
    uint32_t outputs;          /* SLHIP_FLOW_OUT_* bits, at least one                                         */
    uint32_t flags;            /* SLHIP_FLOW_MATCH_INSTANCE                                                   */
} slhip_render_flow_params; /* 48 bytes */

/* Every rule of the record, in the order of its fields.  A negative error with slhip_last_error text.  No device. */
int slhip_render_flow_check_params(const slhip_render_flow_params* params);
/* d_depth_a / stride_a: the depth of picture a, read at pixel * stride (1: a float plane [B, H, W]; 4: d_coord + 3, the w
 * of the coord target in place), d_depth_b / stride_b the same of picture b or NULL: VISIBLE is then never set and its count
 * is 0.  d_instance_a u16 [B, H, W]; d_instance_b the same or NULL: no instance condition.  d_motion f32 [B, n_slots, 3, 4].
 * Outputs, each only with its SLHIP_FLOW_OUT_* bit (without it the pointer is not read): d_flow f32 [B, H, W, 2] (8-byte
 * aligned), d_scene_flow f32 [B, H, W, 3], d_flags u8 [B, H, W], d_counts i32 [B, n_slots, 4], zeroed by the call itself on
 * `stream`.  B == 0 does nothing; B > 65535, null pointers, a zero stride, misalignment and bad parameters are refused before
 * anything touches the device.  One lane per pixel, the scene's motion table in LDS.  Asynchronous on `stream`.             */
int slhip_render_flow(const slhip_render_flow_params* params, const float* d_depth_a, uint32_t stride_a,
                      const uint16_t* d_instance_a, const float* d_motion, const float* d_depth_b, uint32_t stride_b,
                      const uint16_t* d_instance_b, uint32_t B, float* d_flow, float* d_scene_flow, uint8_t* d_flags,
                      int32_t* d_counts, void* stream);
/* d_from, d_to, d_out: f32 [n, 3, 4]; one lane per frame.  n == 0 does nothing.  Asynchronous on `stream`. */
int slhip_render_flow_motion(const float* d_from, const float* d_to, uint32_t n, float* d_out, void* stream);
/* The same rules on host arrays through csrc/slhip_flow_rules.h.  Host only, no device: the handles the CPU tests use. */
int slhip_render_flow_host(const slhip_render_flow_params* params, const float* h_depth_a, uint32_t stride_a,
                           const uint16_t* h_instance_a, const float* h_motion, const float* h_depth_b, uint32_t stride_b,
                           const uint16_t* h_instance_b, uint32_t B, float* h_flow, float* h_scene_flow, uint8_t* h_flags,
                           int32_t* h_counts);
int slhip_render_flow_motion_host(const float* h_from, const float* h_to, uint32_t n, float* h_out);

/* ---------------------------------------------------------------------------------------------
 * Point neighbours: for every query point of a set its k nearest reference points of the same set, as
 * lists of indices and squared distances sorted by (distance, index).  This project's addition, the
 * reference has no counterpart: it renders, and leaves the networks' data pipeline to their loaders.
 * What the entry replaces there is the CPU kd-tree of the FFB6D / PVN3D-with-RandLA data pipeline, per
 * frame and encoder level (dataset's DP.knn_search, a nanoflann wrapper):
 *   cld_nei_idx     = knn(cloud_l, cloud_l, 16)        a self-search of the first N_l points
 *   cld_sub_idx     = the first N_l / ratio rows        no search: the reference prefix below
 *   cld_interp_idx  = knn(cloud_l+1, cloud_l, 1)        k = 1, references = the prefix of N_l+1 points
 *   r2p_ds_nei_idx  = knn(pixel_xyz, cloud, 16),   p2r_ds_nei_idx = knn(cloud, pixel_xyz, 1)
 * and the k-NN grouping of PointNet++ / DGCNN style refiners on the point sets of "Object points".
 * All float32, one rounded IEEE operation at a time (no fma), only - * + and comparisons;
 * csrc/slhip_knn_rules.h holds the rules for host and device, so slhip_point_knn_host gives the device's
 * outputs bit for bit, and tests/point_knn_ref.py restates them in NumPy.  DESIGN.md "Point neighbours".
 * Per set i, query q in [0, n_queries), reference r in [0, n_refs):
 *   1. a point (x, y, z, w) counts when w != 0 and x, y, z are finite (rule 2 of "ICP").
 *   2. d(q, r) = dist2(query, ref) = (dx*dx + dy*dy) + dz*dz of "Pose errors", dx = query.x - ref.x.
 *   3. r is a candidate of q when both points count, d is finite (a NaN or +inf distance is never a
 *      neighbour), d <= max_dist * max_dist (+inf: no gate; the gate's own distance passes) and, with
 *      skip_same, r != q -- decided by index, never by coordinates: duplicated points are normal.
 *   4. the list of q is the first k candidates in the total order (d, r): the smaller distance first, among
 *      equal distances the lower index; stored in that order.  As a scan upwards in r: a candidate enters
 *      when d < the list's last distance (strictly) and goes behind every entry with d' <= d.  The order
 *      is total, so the lists depend neither on the tiles nor on the slots of the kernel's instantiation.
 *   5. a slot without a candidate holds idx -1 and dist2 NaN -- never 0, never a repeated neighbour;
 *      count[q] = the filled slots, 0 for a query that does not count.
 * A set's points lie query_stride (ref_stride) points apart in memory, stride >= count: the first n_refs
 * points of a longer row are a reference set of their own (RandLA's sub-sample is a prefix).
 * Bounds: n_sets * n_queries * k <= 2^31 - 1 (the elements of a list output) and
 * n_sets * max(query_stride, ref_stride) * 4 <= 2^31 - 1 (the floats of an input); so a reference index
 * and the 1-D grid of n_sets * ceil(n_queries / 256) workgroups fit 31 bits.  Offsets are 64-bit inside.
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_KNN_K_MAX     32u
#define SLHIP_KNN_BLOCK     256u      /* queries per workgroup, one per lane                                  */
#define SLHIP_KNN_TILE      1024u     /* references per LDS tile (16 KiB)                                     */
#define SLHIP_KNN_OUT_IDX   1u
#define SLHIP_KNN_OUT_DIST2 2u
#define SLHIP_KNN_OUT_COUNT 4u

typedef struct {
    uint32_t n_sets;           /* n                                                                           */
    uint32_t n_queries;        /* Q >= 1 queries per set                                                      */
    uint32_t n_refs;           /* R >= 1 references per set                                                   */
    uint32_t query_stride;     /* points from one set's queries to the next set's, >= n_queries               */
    uint32_t ref_stride;       /* the same of the references, >= n_refs                                       */
    uint32_t k;                /* 1..SLHIP_KNN_K_MAX neighbours per query                                     */
    float max_dist;            /* >= 0, +inf: no gate; rule 3                                                 */
    uint32_t skip_same;        /* 0 or 1: rule 3; 1 needs queries == refs and query_stride == ref_stride      */
    uint32_t outputs;          /* SLHIP_KNN_OUT_* bits, at least one                                          */
    uint32_t _pad[3];
} slhip_point_knn_params; /* 48 bytes */

typedef struct {               /* read only when its bit is set; every pointer 4-byte aligned                 */
    int32_t* idx;              /* i32 [n, Q, k], -1 in an empty slot                                          */
    float* dist2;              /* f32 [n, Q, k], NaN in an empty slot                                         */
    int32_t* count;            /* i32 [n, Q]                                                                  */
} slhip_point_knn_out;

/* Every rule of the record, in the order of its fields, then the two bounds above.  A negative error with
 * slhip_last_error text.  No device. */
int slhip_point_knn_check_params(const slhip_point_knn_params* params);
/* d_queries f32 [n, query_stride, 4] and d_refs f32 [n, ref_stride, 4] (the layout of the point sets' camera and coord
 * outputs), both 16-byte aligned; they may be the same pointer (a self-search), and must be with skip_same.  Every output
 * named in params->outputs is written for every query, the others are not touched.  n_sets == 0 does nothing; null pointers
 * (an output named in the mask included), misalignment and bad parameters are refused before anything touches the device.
 * One workgroup of 256 lanes per set and 256 queries, the references through LDS in tiles of SLHIP_KNN_TILE; k = 1 is the
 * same kernel.  Asynchronous on `stream`.                                                                                 */
int slhip_point_knn(const slhip_point_knn_params* params, const float* d_queries, const float* d_refs,
                    const slhip_point_knn_out* out, void* stream);
/* The plain scan of rule 4 on host arrays through csrc/slhip_knn_rules.h.  Host only, no device: the handle the CPU tests use. */
int slhip_point_knn_host(const slhip_point_knn_params* params, const float* h_queries, const float* h_refs,
                         const slhip_point_knn_out* out);
/* Developer hook (tools/time_point_knn.py): HIP events round the last slhip_point_knn [0] (-1: not run). */
int slhip_point_knn_timing_enable(int on);
int slhip_point_knn_timings(float ms_out[1]);

/* bp_to_vertices_and_colors (diff.py:215-352, row D6), dense form: for every pixel that belongs to one
 * of the n_obj objects, the negated gradient of the objective w.r.t. the three vertices of its triangle
 * (-bary_k * dL/dX, X = object coordinates of the pixel) and w.r.t. their colours (-bary_k * dL/dI).
 * d_bary f32[H,W,4] (the barycentric target); outputs f32[H,W,3,3], zero where no object matches; the
 * caller selects the rows of one object's pixels (row-major, as the reference's boolean indexing does)
 * and pairs them with the vertex-index target.  d_valid u8[H,W] is scratch.                       */
int slhip_diff_vertex_backward(const uint8_t* d_rgb, const float* d_coord, const int16_t* d_inst,
                               const float* d_bary, const float* d_grad_img, const float* h_proj,
                               const float* d_poses, const int32_t* d_obj_inst, int n_obj, int H, int W,
                               uint8_t* d_valid, float* d_grad_vertices, float* d_grad_colors, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Library
 * ------------------------------------------------------------------------------------------- */
int slhip_abi_version(void);
const char* slhip_last_error(void);
/* hipSetDevice + sanity check that the device is gfx950.  Replaces Context::CreateCUDA's
 * device selection (reference src/context.cpp:411-560).                                      */
int slhip_device_init(int device_index);

/* Streams confined to a range of compute units of the current device (additive: the reference has
 * one GL context per process and nothing to partition).  A data-generation loop runs the settle of
 * batch k+1 and the render of batch k at the same time; the two halves have opposite resource
 * shapes (settle: 256 VGPRs + 20 KiB LDS per single-wave workgroup held for ~100 ms; render: short
 * 256-thread workgroups), and sharing CUs between them fragments both.  Giving each half its own CU
 * range removes the interference.  Consecutive CUs of the mask order are dealt round-robin over
 * the XCDs, so a contiguous range takes the same share of every XCD.  `*stream_out` is a
 * hipStream_t usable as the `stream` argument of every call above.                              */
int slhip_stream_create_cu_range(uint32_t first_cu, uint32_t n_cus, void** stream_out);
int slhip_stream_destroy(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene synthesis on the device: the host work either side of the settle, moved into HBM.
 *
 * In the reference every scene is built by host C++ behind pybind11: the tabletop set-up of
 * Scene::simulateTableTopScene (src/scene.cpp:612-678: plane yaw, the stack of randomly oriented
 * objects), after the settle Scene::chooseRandomCameraPose (scene.cpp:472-610) and
 * chooseRandomLightDirection (scene.cpp:453-470), and per render the shadow matrices
 * (render_pass.cpp:69-211) and the per-drawable uniforms (render_pass.cpp:534-621,
 * render_shader.cpp:233-265).  For a batch that is ~4 ms of host time per scene against 0.15 ms of
 * device time, so a batch is described ONCE by an asset table (one record per sl.Mesh in use) and two
 * kernels write the records the settle and render kernels consume -- nothing crosses PCIe per scene.
 *
 * Randomness: Philox4x32-10 keyed by (seed_lo, seed_hi), counter (scene id, stream, index,
 * 0x51DE5EED); uniform = ((x >> 8) + 0.5) * 2^-24; normals by Box-Muller on deterministic log /
 * sin / cos polynomials (the DISTRIBUTIONS of the reference are the contract, its libstdc++ streams are
 * not reproducible: it seeds from std::random_device, scene.cpp:147-148).
 * Streams: 0 scene (plane yaw, camera azimuth / elevation, light direction), 1 classes, 2 orientations, 3 metallic /
 * roughness, 4 environment (slhip_synth_place_env only; no draw of streams 0-3 depends on it).  Stream 4, index 0:
 * x[0] gates the light set, x[1] picks it, x[2] gates the background image, x[3] picks it; index 1: x[0] gates the plane
 * texture, x[1] picks it.  Gate: uniform(x) < p.  Pick: min(n - 1, (uint32_t)(uniform(x) * (float)n)), float32 throughout.
 * Stream 5, crop jitter (slhip_object_crops_select only; its key and scene id base are the caller's): index = the slot,
 * x[0] scales the window, x[1] and x[2] shift it along x and y.
 * Stream 6, point ranks (slhip_object_points_gather only; its key and scene id base are the caller's): index =
 * (slot << 12) | (j >> 2), x[j & 3] places point j inside its stratum of the visible pixels ("Object points" above).
 * Stream 7, correspondence samples (slhip_pose_pnp only; its key and set id base are the caller's, the set id stands where
 * the scene id does): index = the hypothesis h, x[0], x[1], x[2] pick the three correspondences of the minimal sample, x[3]
 * the fourth that disambiguates, each by the pick rule above over the n_valid correspondences ("Pose PnP" above).
 * Stream 8, voter samples (slhip_keypoint_vote only; its key and set id base are the caller's, the set id stands where the
 * scene id does, and the keypoint k stands where 0x51DE5EED does): index = the hypothesis h, x[0] and x[1] pick the two voters
 * whose lines are intersected, each by the pick rule above over the n_valid voters ("Keypoint voting" above).
 * Stream 9, alignment samples (slhip_pose_align only; its key and set id base are the caller's, the set id stands where the
 * scene id does): index = the hypothesis h, x[0], x[1], x[2] pick the three correspondences of the minimal sample, each by the
 * pick rule above over the n_valid correspondences ("Robust alignment" above); x[3] is not used.
 * Views (slhip_synth_place_view): azimuth and elevation of view v >= 1 are the draw of view 0 -- stream 0, index 0, words 1 and
 * 2, the same scene id, the same formulas -- under the key (seed_lo + v * 0x9E3779B9, seed_hi + v * 0xBB67AE85), each sum
 * wrapping at 32 bits.  No other draw uses the view's key: the light's normals, the environment's gates and picks and everything
 * of slhip_synth_stage keep the batch's key in every view.
 * ------------------------------------------------------------------------------------------- */

/* One mesh class: what sl.Mesh (+ the defaults of sl.Object) contributes to a scene. */
typedef struct {
    float mesh_to_object[16];   /* Mesh::pretransform, row-major                                     */
    float bbox_min[4], bbox_max[4]; /* Mesh::bbox() incl. quirk q6 (mesh.cpp:1075-1081), object frame  */
    float com[4];               /* centre of mass (object frame) at the default density               */
    float inv_inertia[12];      /* inverse inertia about the COM, object axes, rows padded to 4       */
    float mass;                 /* density 1000 (object.h:287) x hull volumes                         */
    float mu_s, mu_d, restitution;  /* default material 0.3 / 0.2 / 0.1 (context.cpp:250-252)       */
    float bsphere[4];           /* bounding sphere of all hulls                                       */
    uint32_t hull_begin, hull_end;  /* range in the hull table handed to slhip_settle                */
    uint32_t draw_begin, draw_count; /* sub-mesh draw templates of this class in d_templates          */
    uint32_t n_verts;           /* vertices of the mesh (every draw of the class indexes all of them) */
    uint32_t n_chunks;          /* sum over the class's draws of ceil(n_tris / SLHIP_CHUNK_TRIS)      */
    uint32_t _pad[2];
} slhip_asset;                  /* 224 bytes */

#define SLHIP_SYNTH_SAMPLE_DISTINCT 1u  /* draw each scene's n_objects classes without replacement
                                           (examples/ycb.py:60: random.sample(meshes, 20)); needs
                                           n_objects <= n_assets <= SLHIP_SYNTH_MAX_ASSETS; otherwise
                                           d_asset_ids names every object's class                     */
#define SLHIP_SYNTH_RANDOM_PBR      2u  /* metallic, roughness ~ U(0,1) per object (examples/ycb.py:63-64:
                                           obj.metallic / obj.roughness); otherwise the file's values   */
#define SLHIP_SYNTH_SHADOWS         4u  /* fill shadow_mat of the active light(s) (render_pass.cpp:131-211) */
#define SLHIP_SYNTH_MAX_ASSETS   1024u
#define SLHIP_SYNTH_MAX_OBJECTS    64u  /* == SLHIP_MAX_BODIES */

typedef struct {
    uint32_t n_scenes, n_objects, n_assets, flags;
    uint32_t seed_lo, seed_hi;
    uint32_t scene_id_base;     /* global id of scene 0: shards and steps draw disjoint random streams  */
    uint32_t render_chunk;      /* scenes per slhip_render call: `scene`, `draw`, draw_begin/end and
                                   clip_base in the written records are relative to the first scene of
                                   the call's chunk (scene s belongs to chunk s / render_chunk)         */
    uint32_t max_draws_per_scene;      /* record strides: scene s owns draws [s*max_draws, ...), chunks */
    uint32_t max_chunks_per_scene;     /* [s*max_chunks, ...) and clip vertices [s*max_clip, ...)        */
    uint32_t max_clip_verts_per_scene; /* (chunk-relative); unused slots are written with zero counts   */
    float plane_z;              /* top of the table box: BOX_HALF_EXTENTS.z = 0.04 (scene.cpp:638)       */
    float proj[16];             /* Scene::projectionMatrix, row-major (scene.cpp:222-253)                */
    float proj_inv[16];         /* its inverse (render_pass.cpp:73)                                      */
    float plane_size[2];        /* Scene::backgroundPlaneSize; 0,0 = no plane drawn                      */
    float manual_exposure;
    float _pad0;
    float light_color[4];       /* light 0; its direction is drawn per scene (scene.cpp:453-470)         */
    float ambient[4];
} slhip_synth_params;           /* 224 bytes */

typedef struct {
    uint32_t asset;             /* class of the object                                                  */
    uint32_t instance_index;    /* 1 + position in the scene (scene.cpp:285-287)                         */
    float metallic, roughness;  /* per-object override, < 0 = the file's value (render_shader.cpp:355-377) */
} slhip_synth_object;

typedef struct {
    float plane_pose[16];       /* Scene::backgroundPlanePose set by the tabletop set-up (scene.cpp:650-657) */
    float camera_pose[16];      /* out of slhip_synth_place: Scene::cameraPose                            */
} slhip_synth_scene;

/* Object keypoints ("Object keypoints" above), the entries that take the records of this section. */
/* d_pos: float4 [n_vertices], the pool's positions; d_assets [n_assets] (1..SLHIP_SYNTH_MAX_ASSETS), d_templates
 * [n_templates]; n_fps 1..SLHIP_KEYPOINTS_MAX; max_verts: the most vertices of a class (the row length of d_scratch).
 * d_keypoints f32 [n_assets, n_fps, 4] = (x, y, z, 1), d_vertex i32 [n_assets, n_fps] = i_k.  One workgroup per class (this
 * runs once per asset table).  Bad counts and null pointers are refused before anything touches the device.  Asynchronous
 * on `stream`.                                                                                                            */
int slhip_object_keypoints_fps(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                               const slhip_draw* d_templates, uint32_t n_templates, uint32_t n_fps, uint64_t max_verts,
                               void* d_scratch, float* d_keypoints, int32_t* d_vertex, void* stream);
/* The same rule on host arrays through csrc/slhip_keypoint_rules.h (no row limit, no scratch).  A class whose template or
 * vertices lie outside the tables has no vertices here too.  Host only, no device: the handle the CPU tests use.        */
int slhip_object_keypoints_fps_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets, uint32_t n_assets,
                                    const slhip_draw* h_templates, uint32_t n_templates, uint32_t n_fps, float* h_keypoints,
                                    int32_t* h_vertex);
/* [n_scenes, n_objects, Kp] keypoints: d_bank f32 [n_assets, Kp, 4] (any bank, not only FPS), d_objects
 * slhip_synth_object [n_scenes * n_objects] (only .asset is read), d_object_to_camera f32 [n_scenes, n_objects, 3, 4],
 * d_depth / depth_stride as in slhip_object_points_gather, or NULL: no SLHIP_KEYPOINT_UNOCCLUDED.  Outputs: d_camera f32
 * [.., 4] = (X, Y, Z, 1), d_uv f32 [.., 2], d_flags u8 [..].  Null pointers and bad sizes are refused before anything touches
 * the device.  Asynchronous on `stream`.                                                                                  */
int slhip_object_keypoints_project(const slhip_object_keypoint_params* params, const float* d_bank, uint32_t n_assets,
                                   const slhip_synth_object* d_objects, const float* d_object_to_camera, uint32_t n_scenes,
                                   const float* d_depth, uint32_t depth_stride, float* d_camera, float* d_uv, uint8_t* d_flags,
                                   void* stream);

/* Object regions ("Object regions" above), the entries that take the records of this section. */
/* The arguments of slhip_object_keypoints_fps with n_regions 1..SLHIP_REGIONS_MAX in place of n_fps (the same kernel, the
 * same rule): d_centres f32 [n_assets, n_regions, 4] = (x, y, z, 1), d_vertex i32 [n_assets, n_regions].  Asynchronous on
 * `stream`.                                                                                                               */
int slhip_object_regions_centres(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                                 const slhip_draw* d_templates, uint32_t n_templates, uint32_t n_regions, uint64_t max_verts,
                                 void* d_scratch, float* d_centres, int32_t* d_vertex, void* stream);
/* The same on host arrays (no row limit, no scratch).  Host only, no device. */
int slhip_object_regions_centres_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets, uint32_t n_assets,
                                      const slhip_draw* h_templates, uint32_t n_templates, uint32_t n_regions, float* h_centres,
                                      int32_t* h_vertex);
/* Step 2: d_centres f32 [n_assets, n_regions, 4] (16-byte aligned; any bank, not only FPS) -> d_vertex_region u8 [n_vertices]
 * (n_vertices below 2^32), d_count i32 [n_assets, n_regions], d_extent f32 [n_assets, n_regions, 4] (4-byte aligned).  The
 * entry fills d_vertex_region with SLHIP_REGION_NONE and zeroes d_count and d_extent on `stream` before the kernel.  Bad
 * counts and null pointers are refused before anything touches the device.  Asynchronous on `stream`.                     */
int slhip_object_regions_vertices(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                                  const slhip_draw* d_templates, uint32_t n_templates, const float* d_centres, uint32_t n_regions,
                                  uint8_t* d_vertex_region, int32_t* d_count, float* d_extent, void* stream);
/* The same on host arrays.  Host only, no device. */
int slhip_object_regions_vertices_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets, uint32_t n_assets,
                                       const slhip_draw* h_templates, uint32_t n_templates, const float* h_centres,
                                       uint32_t n_regions, uint8_t* h_vertex_region, int32_t* h_count, float* h_extent);

/* Tabletop set-up of every scene of the batch (scene.cpp:612-678): d_bodies [n_scenes * n_objects],
 * d_settle_scenes [n_scenes] (has_plane = 1), d_objects [n_scenes * n_objects], d_scenes [n_scenes].
 * d_asset_ids: u16 [n_scenes * n_objects] or NULL with SLHIP_SYNTH_SAMPLE_DISTINCT.                   */
int slhip_synth_stage(const slhip_synth_params* params, const slhip_asset* d_assets, const uint16_t* d_asset_ids,
                      slhip_body* d_bodies, slhip_settle_scene* d_settle_scenes, slhip_synth_object* d_objects,
                      slhip_synth_scene* d_scenes, void* stream);

/* After the settle: camera pose, light direction, shadow matrix, and the slhip_scene / slhip_draw /
 * slhip_chunk records of the batch (strides from `params`), ready for slhip_render chunk by chunk.
 * d_templates: the sub-mesh draws of every class with all static fields filled (materials, textures,
 * vertex / index ranges, class index); transforms, ids and bases are written here.                    */
int slhip_synth_place(const slhip_synth_params* params, const slhip_asset* d_assets, const slhip_draw* d_templates,
                      const slhip_body* d_bodies, const slhip_synth_object* d_objects, slhip_synth_scene* d_scenes,
                      slhip_scene* d_out_scenes, slhip_draw* d_out_draws, slhip_chunk* d_out_chunks, void* stream);

/* The environment bank of a batch: what examples/ycb.py binds per scene with --ibl (:64-67, Scene::setLightMap) and
 * --plane-texture (:73-74, Scene::setBackgroundPlaneTexture), and Scene::setBackgroundImage (py_scene.cpp:131-140),
 * uploaded once like the asset table.  The textures live in the texel pool handed to slhip_render (d_tex).        */
typedef struct {            /* one light map as a scene uses it (render_pass.cpp:412-418, render_shader.cpp:270-296) */
    uint32_t light_map;     /* 1 + index into slhip_mesh_pool.d_light_maps                                   */
    uint32_t n_lights;      /* <= SLHIP_NUM_LIGHTS (more are cut, render_pass.cpp:417-418): Sun / Light1 / Light2 of
                               the .ibl file (light_map.cpp:310-345)                                          */
    uint32_t _pad[2];
    float light_dir[SLHIP_NUM_LIGHTS][4], light_color[SLHIP_NUM_LIGHTS][4];   /* world frame (xyz)            */
} slhip_env_light_set;      /* 112 bytes */

typedef struct {            /* a texture of the texel pool: Scene::backgroundImage (render_pass.cpp:637-646) or   */
    uint32_t offset, w, h;  /* Scene::backgroundPlaneTexture (render_pass.cpp:555-573); byte offset, size          */
    uint32_t sampler;       /* SLHIP_SAMPLER_* of the plane draw's base texture (low 8 bits); unused for backgrounds */
} slhip_env_texture;        /* 16 bytes */

typedef struct {
    const slhip_env_light_set* d_light_sets;     /* Scene::lightMap candidates (scene.h:174-176)                */
    const slhip_env_texture*   d_backgrounds;    /* rectangle textures, one level (py_scene.cpp:131-140)       */
    const slhip_env_texture*   d_plane_textures; /* 2D textures with mip chain (py_scene.cpp:414-415)          */
    const int32_t* d_env_ids;   /* NULL: draw from stream 4.  Else [n_scenes][3] = (light set, background, plane
                                   texture) of every scene, -1 = none; an id beyond its bank makes the scene EMPTY
                                   (no draws -- as for record strides that do not fit), nothing is read out of bounds */
    uint32_t n_light_sets, n_backgrounds, n_plane_textures;
    float p_light_map, p_background, p_plane_texture;   /* probability that a scene gets one, each in [0, 1]
                                   (examples/ycb.py:64-74 takes all or none per run); ignored with d_env_ids     */
} slhip_synth_env;          /* 56 bytes */

/* slhip_synth_place with an environment per scene.  Camera, draws of the objects and chunks are those of
 * slhip_synth_place bit for bit.  A scene WITHOUT a light set gets the drawn light, params->light_color and
 * params->ambient as there; WITH one, light l < n_lights = the set's direction / colour, the others off, ambient 0,
 * light_map = the set's (render_pass.cpp:412-418; RenderShader::setLightMap, render_shader.cpp:270-296).  With
 * SLHIP_SYNTH_SHADOWS every active light gets its shadow matrix (render_pass.cpp:131-211, 426-436), by the arithmetic
 * light 0 has in slhip_synth_place.  bg_tex and the plane draw's base texture (colour 1, SLHIP_DRAW_HAS_BASE_TEX;
 * render_pass.cpp:555-573) come from the bank entries.  d_env_out [n_scenes][3]: what each scene got, -1 = none.
 * Refused before any launch: a null bank with a non-zero count, a probability outside [0, 1] or not finite, a
 * probability above zero for an empty bank (when drawing), a null d_env_out.                                    */
int slhip_synth_place_env(const slhip_synth_params* params, const slhip_synth_env* env, const slhip_asset* d_assets,
                          const slhip_draw* d_templates, const slhip_body* d_bodies, const slhip_synth_object* d_objects,
                          slhip_synth_scene* d_scenes, slhip_scene* d_out_scenes, slhip_draw* d_out_draws,
                          slhip_chunk* d_out_chunks, int32_t* d_env_out, void* stream);

/* Another camera on the SAME settled scenes: a view.  Poses, lights, environment, every slhip_draw and slhip_chunk and
 * light_color / ambient / light_map / bg_tex of slhip_scene carry the bits slhip_synth_place (env NULL) or
 * slhip_synth_place_env writes; world_to_cam, cam_position, shadow_mat[*] and slhip_synth_scene.camera_pose are the view's
 * (camera_pose is overwritten: a hand-over sees the view placed last).  The shadow matrices are fitted to the view's frustum
 * by the arithmetic of slhip_synth_place (render_pass.cpp:69-211 runs per render).  A scene without a light set keeps, in
 * every view, the world-space light_dir slhip_synth_place writes for it: the reference draws the light in the camera frame,
 * and the scene's camera is view 0's (scene.cpp:453-470).  View 0 without d_camera_poses is slhip_synth_place /
 * slhip_synth_place_env bit for bit. */
typedef struct {
    uint32_t view;                /* 0: the camera slhip_synth_place gives the scene.  v >= 1: the same draw under the key
                                     of view v ("Randomness"), the same fit to the objects (scene.cpp:472-610)            */
    uint32_t _pad;
    const float* d_camera_poses;  /* NULL, or [n_scenes][16] camera-to-world, row-major (Scene::cameraPose): taken as it
                                     is -- no draw, no fit; `view` is ignored.  A pose with an entry that is not finite
                                     makes the scene EMPTY (no draws -- as for record strides that do not fit) under
                                     the identity camera                                                                */
    float* d_object_to_camera;    /* NULL, or out [n_scenes][n_objects][12]: rows of world_to_cam * pose (3x4)             */
} slhip_synth_view;         /* 24 bytes */

/* env NULL: the plain form (d_env_out NULL as well); else the form of slhip_synth_place_env with its refusals.  Refused
 * before any launch besides: a null view; d_env_out and env not both null or both set.                               */
int slhip_synth_place_view(const slhip_synth_params* params, const slhip_synth_env* env, const slhip_synth_view* view,
                           const slhip_asset* d_assets, const slhip_draw* d_templates, const slhip_body* d_bodies,
                           const slhip_synth_object* d_objects, slhip_synth_scene* d_scenes, slhip_scene* d_out_scenes,
                           slhip_draw* d_out_draws, slhip_chunk* d_out_chunks, int32_t* d_env_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host side of the per-object API (sl.Scene / sl.RenderPass): record assembly in C++, one call per batch.
 * The reference does this work in C++ as well -- renderer.render(scene) (python/src/py_render_pass.cpp:252-258) runs
 * RenderPass::render (src/render_pass.cpp:303-796), which computes the shadow matrices (:69-211) and uploads the
 * per-drawable uniforms (:534-621; RenderShader::setTransformations / setMaterial, render_shader.cpp:233-265, :326-417).
 * Inputs are flat HOST arrays; nothing here touches the device.
 * ------------------------------------------------------------------------------------------- */
/* An object of a scene: pose + what sl.Object overrides of its mesh's draw templates.        */
typedef struct {
    float pose[16];              /* object to world, row-major (Object::pose)                  */
    float bbox_center[4];        /* mesh bbox centre (object frame); w = bbox diagonal / 2 (shadow fit, render_pass.cpp:87,180) */
    float color[4];              /* Object options "color" ...                                 */
    uint32_t force_color;        /* ... used instead of the material's base colour when set ("force_color") */
    uint32_t tmpl_begin, tmpl_count;   /* the mesh's draw templates (one per sub-mesh) in `templates` */
    uint32_t instance_index;
    float metallic, roughness;   /* per-object override, < 0: the material's (render_shader.cpp:355-377) */
    uint32_t casts_shadows;
    uint32_t _pad;
} slhip_host_object;             /* 128 bytes */

/* A scene: camera, lights, background plane, its objects [obj_begin, obj_end).               */
typedef struct {
    float proj[16], proj_inv[16];    /* projection (Scene::projectionMatrix) and its inverse (float64 inverse rounded) */
    float camera_pose[16];           /* camera to world                                        */
    float light_dir[SLHIP_NUM_LIGHTS][4], light_color[SLHIP_NUM_LIGHTS][4];
    float ambient[4];
    float plane_pose[16];            /* background plane pose (scene.cpp:629-663)              */
    float plane_size[2];
    int32_t plane_template;          /* draw template of the background plane in `templates`, -1: no plane */
    float manual_exposure;
    uint32_t obj_begin, obj_end;
    uint32_t light_map;
    uint32_t bg_tex[3];
} slhip_host_scene;                  /* 408 bytes */

/* Shadow-map matrices of one scene (computeFrustumCorners + computeShadowMapMatrix, render_pass.cpp:69-211):
 * out48 = NUM_LIGHTS row-major 4x4 (identity for inactive lights or a non-finite fit).      */
int slhip_host_shadow_matrices(const slhip_host_scene* scene, const slhip_host_object* objects, float* out48);
/* Matrix4::normalMatrix(): inverse transpose of the upper 3x3 of m16 (float64 cofactors), 3 rows padded to 4. */
int slhip_host_normal_matrix(const float* m16, float* out12);
/* Records a batch needs: draws (plane + one per object sub-mesh) and raster chunks (<= SLHIP_CHUNK_TRIS triangles each). */
int slhip_records_count(const slhip_host_scene* scenes, uint32_t n_scenes, const slhip_host_object* objects,
                        const slhip_draw* templates, uint32_t* n_draws, uint32_t* n_chunks);
/* Fills srec[n_scenes], drec[<= draw_capacity], crec[<= chunk_capacity] in scene / object / sub-mesh order: the draw
 * templates with scene, prim_base, clip_base, object_to_world, normal_to_world, the per-object overrides; the scene
 * records with world_to_cam, cam_position, lights and (with_shadows) the shadow matrices.   */
int slhip_records_build_render(const slhip_host_scene* scenes, uint32_t n_scenes, const slhip_host_object* objects,
                               const slhip_draw* templates, uint32_t with_shadows, slhip_scene* srec, slhip_draw* drec,
                               uint32_t draw_capacity, slhip_chunk* crec, uint32_t chunk_capacity);

/* Host geometry of the collision-shape stage (Mesh::loadPhysics, src/mesh.cpp:335-470, where the reference calls its
 * vendored V-HACD and PhysX's convex cooking; csrc/slhip_hull.cpp).
 * slhip_host_convex_hull: quick-hull of n points (xyz, double): up to tri_capacity index triples into `points` (a hull of n points has
 * at most 2 n - 4 triangles), outward oriented.  Returns 0; 1 when the points span no volume (*n_tris_out = 0); -1 on error.
 * slhip_host_fill_holes: solid fill of a voxel grid [nx][ny][nz] (bytes, C order, in place): every empty cell that cannot be reached
 * from the border through empty face neighbours becomes 1 -- V-HACD's inside / outside classification.                           */
int slhip_host_convex_hull(const double* points, uint32_t n, uint32_t* tris_out, uint32_t tri_capacity, uint32_t* n_tris_out);
int slhip_host_fill_holes(uint8_t* grid, uint32_t nx, uint32_t ny, uint32_t nz);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU exchange: scenes are independent, every rank (one process per GPU, as
 * the reference runs it: python/src/py_context.cpp:34-52) settles and renders its own shard; the one
 * exchange step is the all-gather of rendered batches, RCCL over xGMI.  RCCL is bound at run time
 * (the copy the process already maps -- PyTorch's -- else librccl.so.1 of the ROCm install).
 * ------------------------------------------------------------------------------------------- */
#define SLHIP_COMM_ID_BYTES 128   /* == NCCL_UNIQUE_ID_BYTES */
typedef struct slhip_comm slhip_comm;
/* Rank 0 draws an id and hands it to the other ranks out of band (the host layer uses the
 * torch.distributed store; a file or MPI works as well).                                            */
int slhip_comm_unique_id(uint8_t id_out[SLHIP_COMM_ID_BYTES]);
/* Collective over all ranks; binds the communicator to the calling thread's current HIP device.     */
int slhip_comm_create(const uint8_t id[SLHIP_COMM_ID_BYTES], int n_ranks, int rank, slhip_comm** comm_out);
int slhip_comm_destroy(slhip_comm* comm);
int slhip_comm_info(const slhip_comm* comm, int* n_ranks, int* rank);
/* d_recv (n_ranks * bytes) receives every rank's d_send (bytes) in rank order; asynchronous on `stream`. */
int slhip_allgather(slhip_comm* comm, const void* d_send, void* d_recv, uint64_t bytes, void* stream);
/* The buffers of one rendered chunk (rgb, coord, class, instance, normals) in ONE fused RCCL group:
 * d_recv[i] (n_ranks * bytes[i]) <- all ranks' d_send[i].                                           */
int slhip_allgather_group(slhip_comm* comm, uint32_t n_buffers, const void* const* d_send, void* const* d_recv,
                          const uint64_t* bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLHIP_H */
