/* mi355rt.h — C ABI of the MI355X path-tracing renderer (libmi355rt.so).
 *
 * Drop-in boundary: these entry points are what an FFI binding of the reference's
 * `class WebGPURenderer` (src/renderer/WebGPURenderer.ts:7-138) would call; each one
 * cites the TypeScript method it replaces.  Plain pointers and sizes only.
 *
 * Ownership: the caller owns every input array; the callee copies during the call
 * (queue.writeBuffer semantics, ResourceManager.ts:282,318-320,340-341), so inputs may
 * be freed or mutated right after return.  The callee owns all device memory.
 * Threading: one HIP stream per context; calls on one context are not re-entrant;
 * rt_compute / rt_present only enqueue, rt_sync fences (device.queue.onSubmittedWorkDone).
 * Errors: int status, 0 = ok, > 0 = informational (e.g. "buffer was reallocated"),
 * < 0 = failure with rt_last_error(ctx) holding the message.  Like the reference's
 * passes (RaytracePass.ts:38-46,94; RasterizerPass.ts:55,97; PostProcessPass.ts:32-38,60),
 * rt_compute / rt_present silently skip (return RT_SKIPPED) while resources are missing.
 */
#ifndef MI355RT_H
#define MI355RT_H

#include <stddef.h>
#include <stdint.h>

#include "mi355rt_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

enum {
  RT_OK = 0,
  RT_REALLOCATED = 1, /* updateBuffer & co. return `needsRebind` */
  RT_SKIPPED = 2,     /* pass skipped: resources not ready */
  RT_ERR_INVALID = -1,
  RT_ERR_HIP = -2,
  RT_ERR_NOT_READY = -3,
  RT_ERR_NO_DEVICE = -4,
  RT_ERR_INTERNAL = -5,
  RT_ERR_RCCL = -6 /* librccl could not be loaded, or one of its calls failed (sharded image, below) */
};

/* updateBuffer(type, data) kinds — WebGPURenderer.ts:55-60 */
typedef enum rt_kind {
  RT_KIND_TOPOLOGY = 0,     /* Uint32Array, 20 u32 per triangle  */
  RT_KIND_INSTANCE = 1,     /* Float32Array, 36 f32 per instance */
  RT_KIND_LIGHTS = 2,       /* Uint32Array, 2 u32 per light      */
  RT_KIND_DRAW_COMMANDS = 3 /* Uint32Array, 4 u32 per instance   */
} rt_kind;

/* device counters (SURVEY.md §8d "Ray definition") */
typedef struct rt_counters {
  uint64_t primary_rays;   /* primary-visibility casts                        */
  uint64_t extension_rays; /* intersect_tlas calls,        Raytracer.wgsl:732 */
  uint64_t shadow_rays;    /* intersect_tlas_shadow calls, Raytracer.wgsl:688 */
  uint64_t nodes_visited;  /* BVH node fetches (TLAS + BLAS)                  */
  uint64_t tris_tested;    /* hit_triangle_raw calls                          */
  uint64_t shaded_hits;    /* bounce-loop iterations (one shaded hit each)    */
} rt_counters;

/* constructor(canvas) + init() — WebGPURenderer.ts:17-32, WebGPUContext.ts:14-36.
 * Returns NULL when no HIP device / the ordinal is invalid (init() throws there). */
rt_ctx* rt_create(int device_ordinal);
void rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx); /* ctx may be NULL: error of the last failed rt_create */

/* buildPipeline(depth, spp) — WebGPURenderer.ts:34-39, RaytracePass.ts:18-36
 * (pipeline-override constants MAX_DEPTH, SPP). */
int rt_set_pipeline(rt_ctx* ctx, uint32_t max_depth, uint32_t spp);

/* updateScreenSize(w, h) — WebGPURenderer.ts:41-45, ResourceManager.ts:97-142:
 * (re)allocates render target, G-buffer, accumulation buffer and both history textures. */
int rt_resize(rt_ctx* ctx, uint32_t width, uint32_t height);

/* resetAccumulation() — WebGPURenderer.ts:47-49, ResourceManager.ts:144-151 */
int rt_reset_accum(rt_ctx* ctx);

/* loadTexturesFromWorld(bridge) — WebGPURenderer.ts:51-53, ResourceManager.ts:153-198.
 * Takes the already decoded + resized 1024x1024 RGBA8 layers (decode/resize is the
 * browser's job in the reference).  layers == 0 binds the 1x1 white default texture. */
int rt_upload_textures(rt_ctx* ctx, const uint8_t* rgba, uint32_t layers);
/* The same method fed with images at their own size: the host decodes each blob
 * (include/mi355tex.h), the GPU resizes it into its layer — createImageBitmap(blob, {resizeWidth: 1024,
 * resizeHeight: 1024}) + copyExternalImageToTexture, ResourceManager.ts:162-196; resize rule: mi355rt_math.h
 * rt_resize_coord / rt_bilinear_u8.
 *   rt_alloc_texture_layers   createTexture({size: [1024, 1024, layers]}); every layer starts as the white fallback
 *   rt_upload_texture_image   layer <- width x height straight-alpha RGBA8; rgba == NULL writes the white fallback
 *                             bitmap the reference substitutes when decoding fails (:169-175, 200-208)
 *   rt_read_texture_layer     1024*1024*4 bytes back to the host (tests) */
int rt_alloc_texture_layers(rt_ctx* ctx, uint32_t layers);
int rt_upload_texture_image(rt_ctx* ctx, uint32_t layer, const uint8_t* rgba, uint32_t width, uint32_t height);
int rt_read_texture_layer(rt_ctx* ctx, uint32_t layer, uint8_t* out_rgba, size_t cap);

/* BLAS build for World::update(t) on the GPU: the binned-SAH builder of bvh/blas.rs
 * (BVHBuilder::build_with_ids, called per geometry per frame at rebuilder.rs:93-98) — same tree, same triangle order
 * as the scene compiler's CPU restatement, byte for byte.
 *   verts4      4 f32 per vertex (the skinned positions rebuilder.rs hands to the builder), n_verts of them
 *   indices     3 u32 per triangle
 *   nodes_out   8 f32 per node: {min.xyz, bits(skip)} {max.xyz, bits(data)}, BLAS-local skip pointers, leaf data =
 *               (first << 3) | count with `first` an index into order_out; room for nodes_cap nodes (2 * n_tris is enough)
 *   order_out   n_tris u32: position in the BLAS's triangle order -> original triangle id
 * The signature (ctx first) is the one ms_world_set_blas_builder (mi355scene.h) takes as its hook. */
int rt_build_blas(rt_ctx* ctx, const float* verts4, uint32_t n_verts, const uint32_t* indices, uint32_t n_tris,
                  float* nodes_out, uint32_t nodes_cap, uint32_t* n_nodes_out, uint32_t* order_out);

/* updateBuffer(type, data) -> needsRebind — WebGPURenderer.ts:55-60, ResourceManager.ts:230-284 */
int rt_upload(rt_ctx* ctx, rt_kind kind, const void* data, size_t bytes);

/* updateCombinedGeometry(v, n, uv) -> needsRebind — WebGPURenderer.ts:62-68, ResourceManager.ts:286-323 */
int rt_upload_geometry(rt_ctx* ctx, const float* pos4, const float* nrm4, const float* uv2, uint32_t vertex_count);

/* updateCombinedBVH(tlas, blas) -> needsRebind — WebGPURenderer.ts:70-72, ResourceManager.ts:325-346 */
int rt_upload_bvh(rt_ctx* ctx, const float* tlas, uint32_t n_tlas_nodes, const float* blas, uint32_t n_blas_nodes);

/* updateSceneUniforms(cameraData, frameCount, lightCount) — WebGPURenderer.ts:74-80, ResourceManager.ts:359-405 */
int rt_set_scene(rt_ctx* ctx, const float camera[24], uint32_t frame_count, uint32_t light_count);

/* recreateBindGroup() — WebGPURenderer.ts:82-86.  Nothing to rebind on HIP; kept for call parity. */
int rt_recreate_bind_group(rt_ctx* ctx);

/* The first compute() after an upload checks every index the kernels follow (vertex ids, skip pointers, leaf ranges,
 * instance BLAS offsets, light references) on the GPU and returns RT_ERR_INVALID with the reason for a malformed scene —
 * the stand-in for WebGPU's robust buffer access, which a HIP kernel does not have.
 * compute(frameCount) — WebGPURenderer.ts:88-102: totalFrames++, frame uniforms (Halton jitter),
 * primary-visibility pass, path-trace pass.  Enqueues on the context stream. */
int rt_compute(rt_ctx* ctx, uint32_t frame_count);

/* n consecutive compute() calls as ONE dispatch of each kernel — the recorder's batch loop
 * `for (k < batch) renderer.compute(samplesDone + k)` (VideoRecorder.ts:278-280, batch <= 50 there, <= 64 here).
 * Host state (totalFrames, jitter) and every output are bit-identical to calling rt_compute n times; each frame keeps
 * its own G-buffer (24 B/px extra per frame but the last). Needs the persistent kernel form (the default). */
int rt_compute_batch(rt_ctx* ctx, const uint32_t* frame_counts, uint32_t n);

/* present() — WebGPURenderer.ts:104-129: post pass -> render target, swap history. */
int rt_present(rt_ctx* ctx);

/* captureFrame() — WebGPURenderer.ts:131-137, WebGPUContext.ts:38-107: tight RGBA8 rows of the
 * render target (blocking). cap = capacity of out_rgba in bytes (>= width*height*4). */
int rt_capture(rt_ctx* ctx, uint8_t* out_rgba, size_t cap);

/* device.queue.onSubmittedWorkDone() — main.ts:115, VideoRecorder.ts:167,293 */
int rt_sync(rt_ctx* ctx);

/* ---- additions for parity tests, checkpointing and multi-GPU sharding (no reference counterpart) ---- */
int rt_read_accum(rt_ctx* ctx, float* out_rgba32f, size_t cap_bytes);
int rt_write_accum(rt_ctx* ctx, const float* in_rgba32f, size_t bytes);
/* any of the three outputs may be NULL */
int rt_read_gbuffer(rt_ctx* ctx, uint8_t* albedo_rgba8, float* normal_id_rgba32f, float* depth_f32);
int rt_read_history(rt_ctx* ctx, uint16_t* out_rgba16f, size_t cap_bytes); /* last written history texture */
int rt_read_uniforms(rt_ctx* ctx, void* out256);                            /* the 256-byte scene uniform block */
int rt_get_counters(rt_ctx* ctx, rt_counters* out);                         /* blocking; both kernels */
/* counters of one kernel only: 0 = primary-visibility kernel, 1 = path-trace kernel */
int rt_get_kernel_counters(rt_ctx* ctx, int kernel, rt_counters* out);
int rt_reset_counters(rt_ctx* ctx);
/* count nodes/tris/shaded hits too (slower kernel variant); rays are always counted */
int rt_set_counting(rt_ctx* ctx, int detailed);
/* Restrict compute() to rows y with (y / stripe_rows) % count == rank (interleaved row stripes).
 * count <= 1 renders everything.  present() is never sharded. */
int rt_set_stripes(rt_ctx* ctx, uint32_t stripe_rows, uint32_t rank, uint32_t count);
/* Raw device pointer of the float4 accumulation buffer (width*height*16 bytes) so the caller
 * can hand it to a collective (RCCL) without a host round trip. */
void* rt_accum_device_ptr(rt_ctx* ctx);
/* Use caller-owned device memory (width*height*16 bytes, same device) as the accumulation buffer,
 * e.g. a tensor the caller will hand to RCCL; NULL returns to the context's own buffer.
 * Call after rt_resize; a later rt_resize drops the binding and compute() / present() fail until it is renewed. */
int rt_bind_accum(rt_ctx* ctx, void* device_ptr);
/* present() reads this caller-owned float4 buffer (width*height*16 bytes, same device) instead of the accumulation
 * buffer; NULL returns to the accumulation buffer.  The sharded renderer reduces the ranks' stripe accumulators into
 * such a display buffer, so the per-rank accumulators stay disjoint and a progressive render can go on after a
 * gather.  Like rt_bind_accum, the binding is dropped by rt_resize; staleness is tracked PER BINDING: compute() and
 * present() fail with RT_ERR_INVALID until rt_bind_accum is called again (if an accumulator was bound), and present()
 * also until rt_bind_present_source is called again (if a present source was bound) — NULL included; re-binding one
 * does not acknowledge the other. */
int rt_bind_present_source(rt_ctx* ctx, void* device_ptr);
/* Run every subsequent enqueue on a caller-provided hipStream_t (NULL = context's own stream). */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);
/* Average duration in ms of the path-trace kernel over the launches since the last call
 * (HIP events recorded on the context stream around each launch); also returns the launch count. */
int rt_kernel_time_ms(rt_ctx* ctx, double* avg_pathtrace_ms, double* avg_primary_ms, uint32_t* launches);
/* Speculative lookahead for the live loop (src/main.ts:168-173: compute(frameCount); present() per displayed frame).  With
 * max_frames > 1, a compute(f) that continues a run of consecutive frame counts traces the frames f .. f+L-1 as ONE batched
 * dispatch (L doubles along the run, up to max_frames <= 64) and accumulates only frame f; the compute(f+1) ... that follow
 * find their frame ready and only add it.  Images, G-buffer read-backs and the accumulation buffer are bit for bit those of
 * one dispatch per frame; any call that changes what a frame looks like (uploads, rt_set_scene, rt_resize, rt_set_pipeline,
 * ...) drops what was traced ahead.  While it is on, the ray counters count a frame when it is TRACED (ahead of its compute()
 * call), and the detailed-counter build does not trace ahead.  0 (default) / 1 = off. */
int rt_set_lookahead(rt_ctx* ctx, uint32_t max_frames);
/* A caller that knows when its run of consecutive frames ends - renderFrame advances the world every updateInterval frames
 * (main.ts:127-131) - says so: the next rt_compute traces at most `frames_left` frames (itself included), so nothing is
 * traced ahead in vain across the end of the run.  0 = unknown (the default).  Changes no result and discards nothing. */
int rt_set_lookahead_limit(rt_ctx* ctx, uint32_t frames_left);
/* Traversal of the wavefront trace kernels: 1 = child-pair records (csrc/k_pairwalk.hip.h: one 64-byte record per inner
 * node, both children tested per fetch, quad-cooperative LDS-DMA fetch, short per-lane stack); 0 = one 32-byte node per step
 * with skip pointers only (rounds 1-2); 2 (default) = auto: pairs for a scene of one instance, nodes otherwise (where each
 * was measured faster).  Same results bit for bit, same counters.  MI355RT_WALK=node|pairs|auto sets the
 * default of new contexts. */
int rt_set_walk(rt_ctx* ctx, int walk);
int rt_set_kernel_timing(rt_ctx* ctx, int enabled);
/* Per-kernel timers (HIP events on the context stream around every launch while timing is enabled): sum of the
 * durations in ms and launch count per RT_TIMER_* since the last read; n = number of entries the arrays hold. */
enum {
  RT_TIMER_PRIMARY = 0,         /* k_primary_visibility                                                    */
  RT_TIMER_PATHTRACE = 1,       /* k_pathtrace_persistent, or one whole wavefront dispatch (all depths)    */
  RT_TIMER_WF_SHADE = 2,        /* k_wf_shade, one entry per depth                                         */
  RT_TIMER_WF_TRACE_SHADOW = 3, /* k_wf_trace<any hit>                                                     */
  RT_TIMER_WF_TRACE_EXT = 4,    /* k_wf_trace<closest hit>                                                 */
  RT_TIMER_POST = 5,            /* k_postprocess                                                           */
  RT_TIMER_COUNT = 6
};
int rt_kernel_times(rt_ctx* ctx, double* sum_ms, uint32_t* launches, uint32_t n);
/* Diagnostic build (-DRT_CLOCK_STAMP) only: {delta s_memtime, delta s_memrealtime} of each workgroup of the last
 * k_pathtrace_persistent launch (in-kernel clock = ratio x 100 MHz).  Returns the number of pairs written, 0 in the
 * product build, where no stamp executes. */
int rt_debug_clock_stamps(rt_ctx* ctx, uint64_t* out_pairs, uint32_t cap_pairs);
/* The derived traversal array of the uploaded scene (csrc/k_treelet.hip.h) for tests: 8 f32 per node in the new order,
 * the original-index -> new-index table, and the per-instance BLAS roots (any pointer may be NULL).  Returns the node count. */
int rt_debug_read_traversal_nodes(rt_ctx* ctx, float* tnodes_out, uint32_t* new_index_out, uint32_t* inst_root_out,
                                  uint32_t cap_nodes);
/* Diagnostics of the last rt_build_blas: tree levels the breadth-first build went through (nodes of at most 64 triangles
 * are finished inside one wave and do not count) | levels that held a node above 4 096 triangles << 16. */
int rt_build_blas_levels(const rt_ctx* ctx);
/* Device-resident World::update(t): derive EVERY bridge array of this frame on the GPU, inside the
 * renderer's own scene buffers, from the static scene description and the frame's joint matrices (rt_world_frame,
 * mi355rt_layout.h): linear-blend skinning (rebuilder.rs:36-91), the binned-SAH BLAS of every geometry (bvh/blas.rs,
 * without host synchronisation between tree levels), topology / light / draw-command packing (rebuilder.rs:121-168,
 * lib.rs:237-270), the median-split TLAS (bvh/tlas.rs:58-111) and the packed instances - byte for byte the arrays
 * World::update would have produced, which therefore need no upload: it replaces update(t) + updateCombinedGeometry +
 * updateBuffer(topology / instance / lights / draw commands) + updateCombinedBVH of the live loop (src/main.ts:133-163).
 * The signature (with the rt_ctx* as `user`) is ms_device_updater's of mi355scene.h.  The static description is copied
 * to the device when frame->static_epoch differs from the last call's; the pointers need only live during the call.
 * One stream synchronisation at the end (node counts, the TLAS root).  Returns RT_OK / RT_REALLOCATED, or < 0: a
 * description this path does not take (an instance of an empty geometry, a NaN instance box; the caller then runs the
 * host update and uploads as before) or an error.  The update writes into the live scene buffers: after a failure that
 * came when its kernels had started (a NaN instance box, a tree that did not settle) those hold a mix of two scenes and
 * rt_compute refuses with RT_ERR_INVALID until the scene has been uploaded again (rt_upload* / rt_upload_geometry /
 * rt_upload_bvh); a refusal of the arguments (null arrays, a skin table that does not match the static description) is made
 * before anything is written and leaves the previous scene renderable. */
int rt_world_update(rt_ctx* ctx, const rt_world_frame* frame);
/* A geometry without a skin has the same vertices in every frame of a static description, hence the same BLAS, topology
 * rows and emissive list: after the first update rt_world_update leaves its rows in place and copies its node block from a
 * cache (World::update rebuilds it every frame - the same bytes).  Any host upload into the scene buffers (rt_upload*,
 * a new static_epoch) drops the cache.  enabled = 0 rebuilds everything every frame (measurements); default 1. */
int rt_world_set_static_cache(rt_ctx* ctx, int enabled);
/* Stream time (ms, HIP events) of the last rt_world_update: kernels and the small copies, without host work. */
double rt_world_last_ms(const rt_ctx* ctx);
/* ... and of its TLAS kernel alone (k_tlas: instance boxes, median-split tree, packed instances). */
double rt_world_last_tlas_ms(const rt_ctx* ctx);
/* Read a bridge array back from the device-resident world (tests; a host that wants the arrays after all).  out == NULL:
 * only *bytes_out is set. */
typedef enum rt_world_array {
  RT_WORLD_VERTICES = 0, RT_WORLD_NORMALS, RT_WORLD_UVS, RT_WORLD_TOPOLOGY, RT_WORLD_TLAS, RT_WORLD_BLAS, RT_WORLD_INSTANCES,
  RT_WORLD_LIGHTS, RT_WORLD_DRAW_COMMANDS,
  RT_WORLD_INSTANCE_ORDER   /* n_instances u32: the declaration index of the instance at each TLAS position (frame motion's ids) */
} rt_world_array;
int rt_world_read(rt_ctx* ctx, int which, void* out, size_t cap_bytes, size_t* bytes_out);
/* Debug / test read-back of the child-pair records the trace kernels walk (csrc/k_pairs.hip.h): pairs_out receives
 * 16 floats per inner node, root_rec_out 8 floats per instance plus 8 for the TLAS root (either may be NULL).  Returns the
 * number of pair records, or < 0 (cap_pairs too small, no scene). */
int rt_debug_read_pairs(rt_ctx* ctx, float* pairs_out, float* root_rec_out, uint32_t cap_pairs);
/* Diagnostic build (-DRT_TRACE_STAMPS) only: s_memtime cycles the waves of k_wf_trace spent in its three sections,
 * summed over all launches since the last reset: out16[queue][k], queue 0 = closest hit, 1 = any hit; k = 0..2 cycles in
 * {retire / pull, node step, triangle flush}, 3..5 how often each did work, 6 waves, 7 loop trips.  Returns 1 in the
 * diagnostic build, 0 in the product build (where no stamp executes and the array stays zero). */
int rt_debug_trace_sections(rt_ctx* ctx, uint64_t* out16, int reset);
/* Diagnostic build (-DRT_PT_STAMPS) only: the same for k_pathtrace_persistent: out8[0..4] = cycles in {regenerate + start,
 * shade, shadow traversal, extension traversal + surface frame, finish}, [5] trips, [6] waves.  The one-leaf forms make the
 * surface frame of new samples and new hits in one pass between "start" and "shade": its cycles are out8[7], and in neither
 * [0] nor [3]. */
int rt_debug_pt_sections(rt_ctx* ctx, uint64_t* out8, int reset);
/* Shape of the last launch of the persistent path-trace kernel: out4 = {threads per workgroup (256, or 512 for the wide
 * one-leaf form), workgroups, dynamic LDS bytes per workgroup, resident workgroups per CU from the occupancy query}.  All
 * zero before the first such launch. */
int rt_debug_pt_launch(rt_ctx* ctx, uint32_t* out4);
/* Which materials the path-trace kernel of the last compute() dispatch carried code for: RT_PT_FORM_PLAIN when the host knew
 * from the uploaded topology that every triangle is an untextured Lambertian surface or a light and ran the wide one-leaf
 * form compiled for those alone (MI355RT_PLAIN_MATERIALS=0 in the environment of rt_create switches that off),
 * RT_PT_FORM_GENERIC for every other launch of the persistent kernel, RT_PT_FORM_NONE before the first dispatch and after a
 * dispatch that ran another kernel (wavefront, one pixel per lane).  RT_PT_FORM_GENERIC_SWEEP and RT_PT_FORM_PLAIN_SWEEP are
 * those two in the form whose walks test the BLAS leaves alone, in wave lock-step: the host takes it for a batched dispatch
 * of a one-leaf scene when the BLAS bytes of rt_upload_bvh are a canonical pre-order tree of finite, nested boxes with at
 * most 16 leaves of 1-7 triangles (MI355RT_LEAF_SWEEP=0 in the environment of rt_create switches that off;
 * MI355RT_LEAF_SWEEP_GUARD=1 sends every walk of such a form through the sweep over all nodes of the tree that it keeps for
 * rays with a non-finite reciprocal direction).  The images of all forms are the same, bit for bit. */
enum { RT_PT_FORM_NONE = 0, RT_PT_FORM_GENERIC = 1, RT_PT_FORM_PLAIN = 2, RT_PT_FORM_GENERIC_SWEEP = 3, RT_PT_FORM_PLAIN_SWEEP = 4 };
int rt_debug_pt_form(const rt_ctx* ctx);
/* Diagnostic build (-DRT_LANE_STATS) only: lane utilisation of the parts of a trip of k_pathtrace_persistent:
 * out32[2 k] = times part k ran (wave level), out32[2 k + 1] = active lanes summed; k = 0 shade, 1 / 2 node step / triangle
 * chunk of the shadow walk, 3 / 4 of the extension walk, 5 surface frame of a new hit, 6 start of a sample, 7 end of a sample;
 * in the one-leaf forms 5 only records the hit, 6 makes the camera ray and loads the G-buffer words, and 8 is the one pass that
 * makes the surface frame of both; in the sweep forms, per walk with a walking lane, 9 counts every walk, 10 those that sweep
 * the node records and 11 those with a lane of a non-finite slab operand (and those lanes).
 * Returns 1 in the diagnostic build, 0 in the product build (no counter executes, the array stays zero). */
int rt_debug_lane_stats(rt_ctx* ctx, uint64_t* out32, int reset);
/* Proof obligation of the device build's short division / reciprocal / square-root sequences (csrc/k_ieee.hip.h): run
 * them on the GPU against the compiler's correctly rounded IEEE expansions over inputs [first, first + count) of the
 * input set of `op` (csrc/k_ieee_inputs.h: RT_IEEE_OP_*; one-operand ops: index = bit pattern, 2^32 of them; divisions:
 * 2^24 mantissa samples x 2^8 exponent classes).  n = inputs checked; guard_pass = inputs the guard sends down the short
 * sequence, wrong_fast = of those, results that differ from IEEE (must be 0); wrong_fn = results of the composed function
 * (guard + wave-uniform fallback, what the kernels call) that differ (must be 0); checksum = sum of
 * rt_ieee_mix(IEEE result, index), to be compared with the host CPU's own IEEE results (tests/model/ieee_ref.cpp);
 * bad = operand a, operand b, got, ieee of the first mismatches.  No renderer state is touched.  Returns RT_OK, or
 * RT_ERR_INVALID for an unknown op / a build with -DRT_IEEE_PLAIN (nothing to check). */
typedef struct rt_ieee_report {
  uint64_t n, guard_pass, wrong_fast, wrong_fn, checksum;
  uint32_t n_bad;
  uint32_t bad[32];
} rt_ieee_report;
int rt_debug_ieee_check(rt_ctx* ctx, int op, uint64_t first, uint64_t count, rt_ieee_report* out);
/* Path-trace kernel form (all four are bit-identical; tests/test_gpu_parity.py::test_kernel_forms_agree_bitwise):
 *   3 = auto (default): wavefront form when the scene's records do not fit LDS, SPP == 1 and the dispatch carries
 *       >= 4 frames (rt_compute_batch); the persistent kernel otherwise
 *   2 = wavefront: shade / trace stages per depth, path state in HBM, ray-level regeneration in the trace kernels
 *       (SPP != 1 falls back to the persistent kernel)
 *   1 = persistent waves with per-lane path regeneration
 *   0 = one pixel per lane, one 8x8 tile per wave (the reference's dispatch shape; kept for A/B timing; no batches) */
int rt_set_kernel_variant(rt_ctx* ctx, int variant);
int rt_device_count(void);

/* ---- ray queries against the uploaded scene: "what does this ray hit?" (picking, line of sight, bakes, placement) ----
 * The rays go through the acceleration structure the renderer keeps on the device - after rt_upload* as after
 * rt_world_update, whose arrays never reach the host - with the walks of the wavefront trace kernels (k_ray_query,
 * csrc/k_rayquery.hip.h).  Results are those of intersect_tlas / intersect_tlas_shadow (Raytracer.wgsl:496-528, 566-600):
 *   RT_RAYS_CLOSEST  {t, tri, inst, hit = 1} of the closest hit with t_min < t < t_max; a miss is {the ray's t_max, bits
 *                    unchanged, -1, -1, 0}
 *   RT_RAYS_ANY      {0, -1, -1, hit = 1 when anything lies in (t_min, t_max), else 0}
 * tri is the global triangle index and inst the TLAS-order instance index, the numbers rt_read_gbuffer and the topology
 * array use.  Directions need not be normalised; t counts in units of the direction's length.  t_max is per ray (rt_ray),
 * t_min one value per call, >= 0 (the renderer's own rays use 0.001).  A scene with blas_base_idx == 0 (no TLAS) is missed
 * by every ray.
 * The floats of a ray are not validated: both walks terminate for any bit pattern (node order is strictly increasing,
 * k_validate_scene; the pair walk's stack is finite), and a NaN, an infinity or a zero direction gets whatever the
 * reference's arithmetic gives it.
 * The form of the kernel is picked as for the wavefront trace kernels (rt_set_walk / MI355RT_WALK, MI355RT_NO_LDS_STAGING,
 * MI355RT_WF_RAYREG, the size of the scene), in 256-thread workgroups; rt_set_kernel_variant does not matter.
 * A query leaves the renderer as it was: accumulation, jitter and frame counts, the rt_counters, the G-buffer and the frames
 * traced ahead under rt_set_lookahead are untouched, and a render interrupted by queries is bit for bit the uninterrupted one.
 *   rt_trace_rays          blocking: copies n rays in, traces, copies n hits out (staging buffers are kept and grown).  stats
 *                          != NULL also runs the node / triangle counting kernel and fills *stats.  n == 0 is RT_OK; n >= 2^31,
 *                          a NULL pointer, an unknown mode or a t_min that is negative or NaN is RT_ERR_INVALID; without a
 *                          valid scene (nothing uploaded, a scene k_validate_scene refused, the state after a failed
 *                          rt_world_update) RT_ERR_NOT_READY with the reason in rt_last_error.
 *   rt_trace_rays_device   the same on device-accessible arrays (n rt_ray in, n rt_ray_hit out; 16-byte aligned, on the
 *                          context's device): only enqueues on the context's stream (rt_set_stream respected), no host
 *                          synchronisation - the entry for torch tensors.  Counts nodes and triangles while
 *                          rt_set_counting(ctx, 1) is on.
 *   rt_ray_query_stats     stats of the last query (blocking: fences the stream). */
enum { RT_RAYS_CLOSEST = 0, RT_RAYS_ANY = 1 };
int rt_trace_rays(rt_ctx* ctx, const rt_ray* rays, uint32_t n, int mode, float t_min, rt_ray_hit* out, rt_ray_stats* stats);
int rt_trace_rays_device(rt_ctx* ctx, const void* dev_rays, uint32_t n, int mode, float t_min, void* dev_out);
int rt_ray_query_stats(rt_ctx* ctx, rt_ray_stats* out);

/* ---- radiance queries: "what radiance arrives along this ray?" (light probes, irradiance and lightmap bakes, reflection
 * captures, panorama / fisheye / orthographic cameras, renderers that make their own primary rays) ----
 * The renderer's shading - materials, textures, next-event estimation with MIS, Russian roulette: ray_color
 * (Raytracer.wgsl:607-783) - on rays the caller supplies, by the path-query loop over the path state machine
 * (path_query_loop with the policy RadianceItem: k_radiance_query, csrc/k_radiance.hip.h).  For ray i (rt_ray) and sample s
 * in 0 .. spp-1:
 *   rng     init_rng(rays[i].pad, seed * spp + s) in u32 arithmetic: `main`'s init_rng(pixel, frame_count * spp + sample)
 *           (:798-800) with both numbers chosen by the caller.  pad, which rt_trace_rays ignores, is the ray's RNG stream id.
 *   sample  ray_color with the depth-0 surface taken from the TRACED hit, exactly as at every later depth (:738-779): no
 *           G-buffer, no octahedral normal, no unorm8 albedo, no lens offset, no jitter.  The first segment is the closest
 *           hit in (0.001, rays[i].t_max); every later segment uses 0.001 / 1e30 (:6-7) and shadow rays are traced as in a
 *           frame.  Directions are not normalised by the library (the reference's camera rays are not either).  The light
 *           count is that of the last rt_set_scene; light_count above the uploaded lights buffer is RT_ERR_INVALID, as for a
 *           frame.
 *   result  rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp the way `main` does (:811; no division for spp
 *           == 1); t = the first segment's hit distance.  A miss is rgb = +0 and t = the ray's t_max, bits unchanged (the
 *           reference has no environment light).  max_depth == 0: the first segment is traced and t reported, rgb = +0.
 * The first segment does not depend on the sample: it is traced once per ray and counts as one extension ray.  A result
 * depends on (scene, ray, pad, seed, spp, max_depth) only - never on the ray's position in the array, its neighbours, n or
 * the form of the kernel (whole scene in LDS when it fits, as for the persistent path tracer, else global memory;
 * MI355RT_NO_LDS_STAGING respected; rt_set_kernel_variant and rt_set_walk do not matter).
 * A query leaves the renderer as it was, exactly like rt_trace_rays: it has its own chunk counter, counter shards and event
 * pair, and the accumulation, jitter and frame counts, the rt_counters, the G-buffer and the frames traced ahead under
 * rt_set_lookahead are untouched.
 *   rt_trace_radiance         blocking: copies n rays in, traces, copies n results out (staging buffers are kept and
 *                             grown).  stats != NULL runs the counting kernel and fills *stats.  n == 0 is RT_OK; n >= 2^31,
 *                             a NULL pointer, spp == 0 or spp > 65536 is RT_ERR_INVALID; without a valid scene
 *                             RT_ERR_NOT_READY with the reason in rt_last_error.
 *   rt_trace_radiance_device  the same on device-accessible arrays (n rt_ray in, n rt_radiance out; 16-byte aligned, on the
 *                             context's device): only enqueues on the context's stream (rt_set_stream respected).  Counts
 *                             while rt_set_counting(ctx, 1) is on.
 *   rt_radiance_query_stats   stats of the last radiance query (blocking: fences the stream). */
int rt_trace_radiance(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                      rt_radiance* out, rt_radiance_stats* stats);
int rt_trace_radiance_device(rt_ctx* ctx, const void* dev_rays, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                             void* dev_out);
int rt_radiance_query_stats(rt_ctx* ctx, rt_radiance_stats* out);

/* ---- irradiance gathers: "how much light arrives at this surface point?" (lightmap and light-probe bakes, ambient
 * occlusion) ----
 * A radiance query traces the same ray for all spp samples of an entry; an irradiance estimate needs another direction per
 * sample.  Here the work item is a surface point (rt_gather_point): the hemisphere directions are drawn on the device, the
 * renderer's path tracing runs behind them and only the per-point mean comes back, by the radiance query's loop with the
 * policy GatherItem (k_irradiance_gather, csrc/k_gather.hip.h).  For point i and sample s in 0 .. spp-1, with f = seed * spp
 * + s in u32 arithmetic:
 *   direction  the .dir of the reference's Lambert sampler (sample_diffuse, Raytracer.wgsl:228-233, 191-199: build_onb, phi =
 *              2 pi r1, cos(theta) = sqrt(1 - r2), sin(theta) = sqrt(r2), to_world) on n = normalize(points[i].normal), and
 *              nothing else of it; its two rand_pcg draws come from a direction stream of their own, init_rng(pad ^
 *              0x80000000, f).  The direction is not normalised again.  The normal is not validated: a zero or non-finite
 *              normal gets whatever the arithmetic gives, and both walks terminate for any bit pattern, as for ray queries.
 *   sample     exactly what rt_trace_radiance returns for the ray {position, t_max, that direction, pad} with spp = 1 and
 *              seed = f: the path's rng is init_rng(pad, f), the first segment is the closest hit in (0.001, t_max), the
 *              depth-0 surface comes from the traced hit, later segments use 0.001 / 1e30, and the light count is that of the
 *              last rt_set_scene.  A gather is thereby the composition of things this header already defines:
 *              gather(i, s) == radiance query on a host-made ray, bit for bit.  Keep pad < 2^31, so that direction streams
 *              and path streams stay apart.
 *   result     rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp the way `main` does (:811; no division for
 *              spp == 1).  This is the cosine-weighted mean incoming radiance, E / pi: no factor pi is applied - multiply by
 *              pi for irradiance, or by the albedo for the outgoing radiance of a Lambert texel.  hit_fraction = hits / spp,
 *              hits = the samples whose first segment hit something in (0.001, t_max).  max_depth == 0: all spp first
 *              segments are still traced, rgb = +0, and 1 - hit_fraction is ambient occlusion of radius t_max.
 * Every sample's first segment counts as one extension ray, so the stats of a gather (an rt_radiance_stats with rays = n
 * points and samples = n * spp) are the sums of the stats of the radiance queries it is composed of.  A result depends on
 * (scene, point, pad, seed, spp, max_depth) only - never on n, the point's position in the array, its neighbours or the
 * form of the kernel (picked as for radiance queries; MI355RT_NO_LDS_STAGING respected).  A lane keeps its point for all
 * spp samples, so few points with a very large spp fill few lanes: replicate the point with different pads and average the
 * results, which is exact.
 * A gather leaves the renderer as it was, exactly like the two queries above: it has its own staging, chunk counter,
 * counter shards and event pair, and the accumulation, jitter and frame counts, the rt_counters, the G-buffer and the frames
 * traced ahead under rt_set_lookahead are untouched.
 *   rt_gather_irradiance         blocking: copies n points in, gathers, copies n results out (staging buffers are kept and
 *                                grown).  stats != NULL runs the counting kernel and fills *stats.  n == 0 is RT_OK; n >=
 *                                2^31, a NULL pointer, spp == 0 or spp > 65536 is RT_ERR_INVALID; without a valid scene
 *                                RT_ERR_NOT_READY with the reason in rt_last_error; light_count above the uploaded lights
 *                                buffer is RT_ERR_INVALID.
 *   rt_gather_irradiance_device  the same on device-accessible arrays (n rt_gather_point in, n rt_irradiance out; 16-byte
 *                                aligned, on the context's device): only enqueues on the context's stream (rt_set_stream
 *                                respected).  Counts while rt_set_counting(ctx, 1) is on.
 *   rt_irradiance_gather_stats   stats of the last gather (blocking: fences the stream). */
int rt_gather_irradiance(rt_ctx* ctx, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                         rt_irradiance* out, rt_radiance_stats* stats);
int rt_gather_irradiance_device(rt_ctx* ctx, const void* dev_points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                                void* dev_out);
int rt_irradiance_gather_stats(rt_ctx* ctx, rt_radiance_stats* out);

/* ---- probe gathers: "which radiance arrives at this point, from every direction?" as nine spherical-harmonic
 * coefficients per colour (light-probe grids for dynamic objects, irradiance volumes) ----
 * A probe (rt_probe) is a point in space.  Its spp directions are drawn uniformly on the sphere on the device, the
 * renderer's path tracing runs behind each, and the samples are projected onto the real spherical harmonics of bands 0 ..
 * 2; only the 27 coefficients and the hit fraction come back (rt_probe_sh9).  The unit of path work is the (probe,
 * sample) pair, not the probe: a call is k_probe_rays (one rt_ray per pair) -> the radiance query's kernel on those rays at
 * spp = 1 -> k_probe_project (one wave per probe; csrc/k_probe.hip.h), so a grid of few probes with very many samples
 * fills the device, which a lane-per-point gather does not.
 *
 * THE PROBE RULE.  All arithmetic is f32, unfused, in the order written, with rt_sqrt / rt_max / rt_sincos / rt_div of
 * mi355rt_math.h.  For probe i and sample s in 0 .. spp-1, with f = seed * spp + s in u32 arithmetic:
 *   direction  from the gather's direction stream, rng_d = init_rng(pad ^ 0x80000000, f): u1 = rand_pcg(rng_d), u2 =
 *              rand_pcg(rng_d); z = 1.0f - 2.0f * u1; r = rt_sqrt(rt_max(0.0f, 1.0f - z * z)); rt_sincos(RT_TWO_PI * u2, &sp,
 *              &cp); d = (r * cp, r * sp, z).  Uniform on the sphere; not normalised again.
 *   sample     {r, g, b, t}: exactly what rt_trace_radiance returns for the ray {position, t_max, d, pad} with spp = 1 and
 *              seed = f.  It is a hit iff t < t_max as a float comparison (false for NaN).  Keep pad < 2^31, as for a gather.
 *   basis      for d = (x, y, z): Y0 = 0.282094792f; Y1 = 0.488602512f * y; Y2 = 0.488602512f * z; Y3 = 0.488602512f * x;
 *              Y4 = 1.092548431f * (x * y); Y5 = 1.092548431f * (y * z); Y6 = 0.315391565f * (3.0f * (z * z) - 1.0f);
 *              Y7 = 1.092548431f * (x * z); Y8 = 0.546274215f * (x * x - y * y).  The term of (k, c) is radiance[c] * Yk.
 *   sum        a fixed tree, the same for each of the 27 sums: the partial P[l], l = 0 .. 63, is ((+0 + term(l)) + term(l +
 *              64)) + ... over the samples s = l (mod 64), ascending; then for m = 32, 16, 8, 4, 2, 1, in all l at once, P[l]
 *              = P[l] + P[l ^ m] (own value first); the sum is P[0].
 *   result     sh[k][c] = rt_div(sum, (float)spp) * 12.566370614f, the Monte-Carlo estimate of the integral of L(w) Yk(w)
 *              over the sphere;  hit_fraction = rt_div((float)hits, (float)spp).  max_depth == 0: every first segment is
 *              still traced and the coefficients are whatever the arithmetic gives from radiance +0.
 * A result depends on (scene, probe, pad, seed, spp, max_depth) only - never on n, the probe's position in the array or how
 * the library splits the work: a call is cut into batches of whole probes of at most RT_PROBE_BATCH_SAMPLES samples, whose
 * rays and radiances live in scratch of the probe gather's own, kept and grown (at most 48 B per sample of a batch, 192
 * MiB).  The rgb irradiance at a normal n follows from the coefficients by the cosine-lobe convolution (band factors pi, 2
 * pi / 3, pi / 4), a host one-liner; a probe grid with that convolution, a window against ringing and a device sampler is an
 * irradiance volume (below).
 * The stats are an rt_radiance_stats: rays = n probes, samples = n * spp; the ray, hit, node and triangle counters and
 * workgroups are the sums over the radiance launches the call makes - hence the sums of the composed queries' counters -
 * lds is the form that was picked, and kernel_ms is the summed time of the RADIANCE launches only (k_probe_rays and
 * k_probe_project are not in it).
 * A probe gather leaves the renderer as it was, like the queries above, and it has a state of its own: the stats and
 * staging of radiance queries and irradiance gathers are untouched.
 *   rt_gather_probes         blocking: copies n probes in, gathers, copies n results out.  stats != NULL runs the counting
 *                            kernel and fills *stats.  n == 0 is RT_OK; n >= 2^31, a NULL pointer, spp == 0 or spp > 65536 is
 *                            RT_ERR_INVALID; without a valid scene RT_ERR_NOT_READY; light_count above the uploaded lights
 *                            buffer is RT_ERR_INVALID.  Messages begin with "probe gather:".
 *   rt_gather_probes_device  the same on device-accessible arrays (n rt_probe in, n rt_probe_sh9 out; 16-byte aligned, on
 *                            the context's device): only enqueues on the context's stream (rt_set_stream respected).
 *                            Counts while rt_set_counting(ctx, 1) is on.
 *   rt_probe_gather_stats    stats of the last probe gather (blocking: fences the stream). */
#define RT_PROBE_BATCH_SAMPLES (1u << 22)
int rt_gather_probes(rt_ctx* ctx, const rt_probe* probes, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                     rt_probe_sh9* out, rt_radiance_stats* stats);
int rt_gather_probes_device(rt_ctx* ctx, const void* dev_probes, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                            void* dev_out);
int rt_probe_gather_stats(rt_ctx* ctx, rt_radiance_stats* out);

/* ---- irradiance volumes: "how much light arrives at this point of space, on a surface facing this way?" for dynamic
 * objects that have no lightmap ----
 * A volume is an axis-aligned grid of probes (rt_volume_desc, mi355rt_layout.h): nx * ny * nz records of rt_probe_sh9,
 * probe-major, probe (x, y, z) at p = (z * ny + y) * nx + x.  rt_bake_volume makes the grid's probes on the device, runs
 * the probe gather's device path on them and finishes the coefficients in place; rt_sample_volume turns (position,
 * normal) pairs into irradiance from the eight surrounding probes; rt_encode_volume exports the volume as seven texel
 * layers for consumers that upload 3D textures (csrc/k_volume.hip.h).  The volume stays probe-major for the library's own
 * sampler: a record is one 112-byte run and the x-neighbour of a corner the next one, so a point reads four runs of 224
 * bytes; layers would make the same read 56 separate 16-byte pieces.
 *
 * THE VOLUME RULE.  All arithmetic is f32, unfused, in the order written, with rt_div / rt_min / rt_max / rt_normalize of
 * mi355rt_math.h.
 *   probes     of the grid, for probe (x, y, z): position[a] = origin[a] + (float)idx_a * step[a], the product rounded first;
 *              t_max = desc.t_max; unused = +0; pad = pad_first + p.
 *   finish     sh'[k][c] = (sh[k][c] * A_band(k)) * window[band(k)] on what the probe rule gives for those probes, with A =
 *              3.141592654f, 2.094395102f, 0.785398163f for bands 0 (k = 0), 1 (k = 1 .. 3) and 2 (k = 4 .. 8); hit_fraction
 *              keeps its bits.  The volume therefore holds IRRADIANCE coefficients: E(n) = sum_k sh'[k] Y_k(n).  window =
 *              {1, 1, 1} is none; a Hanning window of width w is (1 + cos(pi l / w)) / 2 for band l.
 *   sample     at {position, normal} of an rt_gather_point (t_max and pad are not read):
 *     cell       per axis a with N = n_a: g = rt_div(position[a] - origin[a], step[a]); if !(g > 0) then g = +0 (NaN too); g =
 *                rt_min(g, (float)(N - 1)); i0 = (uint32_t)g; if N > 1 and i0 > N - 2 then i0 = N - 2; i1 = i0 + 1 (i1 = i0
 *                when N == 1); f = g - (float)i0 (f = +0 when N == 1); w0 = 1.0f - f, w1 = f.
 *     corners    c = 0 .. 7 with dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2: w_c = (wx[dx] * wy[dy]) * wz[dz], replaced by +0
 *                when the corner probe is invalid: !(hit_fraction <= max_hit_fraction), so a NaN hit_fraction is invalid.
 *     weight     W = ((+0 + w_0) + w_1) + ... in corner order.  If !(W > 0) the result is {+0, +0, +0, +0}.
 *     coefs      for each of the 27 (k, ch): S = +0, then S = S + w_c * sh'_c[k][ch] for every corner with w_c != 0, in
 *                corner order; corners of weight zero are SKIPPED, not multiplied, so a NaN or an infinity in an invalid or
 *                zero-weight probe never reaches a result.  coef = rt_div(S, W).
 *     evaluate   nrm = rt_normalize(normal); Y_k(nrm) with the nine constants and the operation order of the probe rule;
 *                E[ch] = ((+0 + coef[0][ch] * Y0) + coef[1][ch] * Y1) + ... for k = 0 .. 8; rgb[ch] = rt_max(0.0f, E[ch]);
 *                the hit_fraction slot = W, the valid share of the interpolation weight (1 when all eight corners are
 *                valid).
 *   layers     layer j = 0 .. 6 of the export holds the floats 4 j .. 4 j + 3 of each record, n texels per layer in probe
 *              order: RT_LIGHTMAP_F32, 16 B per texel, the words unchanged; RT_LIGHTMAP_F16, 8 B, four rt_f32_to_f16 as in
 *              rt_encode_atlas.  RT_LIGHTMAP_RGBE8 is refused: coefficients are signed.
 * A sample depends on (volume, desc, point) only - never on n, the point's place in the array or the launch shape.  A
 * baked volume depends on (scene, desc, seed, spp, max_depth) only, as the probe rule says of its probes.
 * Refusals (RT_ERR_INVALID, every message begins with "volume:"): a dimension 0 or above 1024; nx * ny * nz > 2^24;
 * pad_first + nx * ny * nz > 2^31; a step that is not finite and > 0; a window that is not finite and >= 0; a NaN
 * max_hit_fraction; a non-zero reserved word.  The descriptor is checked before the context, and without one the message is
 * what rt_last_error(NULL) returns.
 * A bake runs on the probe gather's state: its probes and, for the blocking entry, its results live in the probe gather's
 * staging, its stats are the probe gather's (rays = probes; kernel_ms the radiance launches only), and
 * rt_probe_gather_stats reports the last bake like the last gather.  Sampling and encoding need no scene - they work on a
 * context with nothing uploaded - and have staging of their own, kept and grown.  Baking, sampling and encoding leave the
 * renderer and the other queries' state as they were.
 *   rt_bake_volume           blocking: probes, gather (cut into batches as a probe gather is), finish, one copy of n
 *                            records back.  stats != NULL runs the counting kernel and fills *stats.  spp as for a probe
 *                            gather; without a valid scene RT_ERR_NOT_READY.
 *   rt_bake_volume_device    the same into a device-accessible array of n records (16-byte aligned, on the context's
 *                            device): only enqueues on the context's stream (rt_set_stream respected).
 *   rt_sample_volume         blocking: copies the volume and n points in, samples, copies n results out.  n == 0 is RT_OK; n
 *                            >= 2^31 or a NULL pointer is RT_ERR_INVALID.  It uploads the whole volume on every call and keeps
 *                            that staging: a caller sampling every frame should keep the volume on the device and use
 *   rt_sample_volume_device  the same on device-accessible arrays (16-byte aligned): only enqueues.
 *   rt_encode_volume         blocking: the volume into seven layers at out, layer j at out + j * n * texel bytes; cap is the
 *                            capacity of out in bytes.  format is RT_LIGHTMAP_F32 or RT_LIGHTMAP_F16.
 *   rt_encode_volume_device  the same on device-accessible arrays; dev_out must not be dev_volume.  Only enqueues. */
int rt_bake_volume(rt_ctx* ctx, const rt_volume_desc* desc, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_probe_sh9* out,
                   rt_radiance_stats* stats);
int rt_bake_volume_device(rt_ctx* ctx, const rt_volume_desc* desc, uint32_t max_depth, uint32_t spp, uint32_t seed, void* dev_out);
int rt_sample_volume(rt_ctx* ctx, const rt_volume_desc* desc, const rt_probe_sh9* volume, const rt_gather_point* points,
                     uint32_t n, rt_irradiance* out);
int rt_sample_volume_device(rt_ctx* ctx, const rt_volume_desc* desc, const void* dev_volume, const void* dev_points, uint32_t n,
                            void* dev_out);
int rt_encode_volume(rt_ctx* ctx, const rt_volume_desc* desc, uint32_t format, const rt_probe_sh9* volume, void* out, size_t cap);
int rt_encode_volume_device(rt_ctx* ctx, const rt_volume_desc* desc, uint32_t format, const void* dev_volume, void* dev_out,
                            size_t cap);

/* ---- reflection probes: "which radiance arrives at this point from that direction, seen through a lobe of this
 * roughness?" for glossy surfaces, which lightmaps and irradiance volumes do not serve ----
 * A reflection probe is the radiance arriving at an rt_probe from every direction as an octahedral map of size * size texels
 * {r, g, b, hit_fraction} (rt_reflection_desc, mi355rt_layout.h), and behind it a chain of smaller maps, level m pre-convolved
 * with the renderer's own GGX lobe (sample_ggx: a = roughness, a2 = roughness * roughness) at the roughness m / (levels - 1).
 * rt_capture_reflection makes level 0 by the renderer's path tracing; rt_filter_reflection makes the levels >= 1 of a chain
 * from level 0 and needs no scene; rt_bake_reflection captures straight into level 0 of each chain and filters in place
 * (csrc/k_reflection.hip.h).  A chain holds chain_texels = sum over m of (size >> m)^2 texels, level m at the texel offset
 * sum over k < m of (size >> k)^2; n chains lie one behind the other.
 *
 * THE REFLECTION RULE.  All arithmetic is f32, unfused, in the order written, with rt_div / rt_rcp / rt_sqrt / rt_rsqrt /
 * rt_sincos / rt_max / rt_min / rt_floor / rt_abs / rt_saturate / rt_normalize of mi355rt_math.h.
 *   octahedral   unpack(px, py), a direction from a point of [-1, 1]^2: n = (px, py, 1.0f - rt_abs(px) - rt_abs(py)); t =
 *                rt_saturate(-n.z); n.x += (n.x >= 0 ? -t : t); n.y likewise with n.y; the result is rt_normalize(n).
 *                pack(v), its inverse: s = rt_rcp(rt_abs(v.x) + rt_abs(v.y) + rt_abs(v.z)); p = (v.x * s, v.y * s); if v.z <
 *                0 then p = ((1.0f - rt_abs(p.y)) * (p.x >= 0 ? 1.0f : -1.0f), (1.0f - rt_abs(p.x)) * (p.y >= 0 ? 1.0f :
 *                -1.0f)), both from the p before.
 *   frame        onb(n): sign = n.z >= 0 ? 1.0f : -1.0f; a = -rt_rcp(sign + n.z); b = n.x * n.y * a; u = (1.0f + sign * n.x *
 *                n.x * a, sign * b, -sign * n.x); v = (b, sign + n.y * n.y * a, -n.y); w = n.  to_world(onb, t) = t.x * u + t.y
 *                * v + t.z * w, per component (t.x * u_c + t.y * v_c) + t.z * w_c.
 *   capture      texel t = j * size + i of a probe, sample s in 0 .. spt - 1, f = seed * spt + s in u32 arithmetic:
 *                pad_t = pad + t; rng_d = init_rng(pad_t ^ 0x80000000, f), the gathers' direction stream; jx = rand_pcg(rng_d),
 *                jy = rand_pcg(rng_d); px = rt_div((float)i + jx, (float)size) * 2.0f - 1.0f, py likewise from j and jy; d =
 *                unpack(px, py).  The sample {r, g, b, t} is exactly what rt_trace_radiance returns for the ray {position,
 *                t_max, d, pad_t} with spp = 1 and seed = f; it is a hit iff t < t_max (false for NaN).  The texel's rgb is
 *                ((+0 + r_0) + r_1) + ... in sample order, divided by (float)spt (three quotients; no division for spt == 1);
 *                its fourth word is rt_div((float)hits, (float)spt).  Keep pad + size * size <= 2^31.
 *   filter       level 0 of a chain is the map, word for word.  Level m >= 1 has the side S = size >> m and the roughness a =
 *                rt_div((float)m, (float)(levels - 1)).  Output texel (i, j): n = unpack(cx, cy) with cx = rt_div((float)i +
 *                0.5f, (float)S) * 2.0f - 1.0f, cy likewise from j; o = onb(n).  Sample s in 0 .. K - 1, K = filter_samples:
 *                  ux = rt_div((float)s + 0.5f, (float)K); uy = (float)(bitreverse32(s) >> 8) * 0x1p-24f (exact);
 *                  phi = RT_TWO_PI * ux; cos_theta = rt_sqrt(rt_max(0.0f, rt_div(1.0f - uy, 1.0f + (a * a - 1.0f) * uy)));
 *                  sin_theta = rt_sqrt(rt_max(0.0f, 1.0f - cos_theta * cos_theta)); rt_sincos(phi, &sp, &cp);
 *                  h = (sin_theta * cp, sin_theta * sp, cos_theta), as sample_ggx forms it in the tangent frame;
 *                  with the view along the normal, l_t = (2.0f * (h.z * h.x), 2.0f * (h.z * h.y), 2.0f * (h.z * h.z) - 1.0f)
 *                  and the weight w = l_t.z.  If !(w > 0), all five terms of the sample are +0.  Else l = to_world(o, l_t), q
 *                  = pack(l); per axis u = (q * 0.5f + 0.5f) * (float)size, u = +0 if !(u > 0), index =
 *                  min((uint32_t)rt_floor(u), size - 1); the source is texel (index_x, index_y) of LEVEL 0, nearest, no
 *                  interpolation; the five terms are w * r, w * g, w * b, w * hit_fraction, w.
 *                Each of the five sums is the probe rule's fixed tree: 64 strided partials ((+0 + term(l)) + term(l + 64)) +
 *                ..., then P[l] = P[l] + P[l ^ m] for m = 32 .. 1, the sum P[0].  The texel is four rt_div(sum_c, sum_w), or
 *                four +0 if !(sum_w > 0).  Source texels are not sanitised: a NaN in level 0 reaches what samples it.  h, l_t
 *                and w depend on (level, s) only.
 * A result depends on (scene, probe, desc, seed, max_depth) only - never on n, the probe's place in the array or how a call
 * is cut: the unit of path work is the (texel, sample) pair, and a capture is cut into batches of whole texels of at most
 * RT_PROBE_BATCH_SAMPLES samples in the composed gathers' shared scratch; a probe may span several batches and a batch
 * several probes.  A bake is word for word rt_filter_reflection of rt_capture_reflection; levels >= 1 read level 0 only.
 * Export needs no entry of its own: every level is a width * height array of 16-byte texels whose fourth word is never -1,
 * which is what rt_encode_atlas(_device) takes as it stands, in all three formats - RT_LIGHTMAP_RGBE8 included, radiance
 * not being signed.  A consumer picks the level of a roughness r as r * (levels - 1).
 * Refusals (RT_ERR_INVALID, every message begins with "reflection:", checked before the context; without one the message is
 * what rt_last_error(NULL) returns): size not a power of two in 8 .. 512; levels < 2; size >> (levels - 1) < 4; spt 0 or
 * above 65536 (capture and bake); filter_samples not a multiple of 64 in 64 .. 4096 (filter and bake); a non-zero reserved
 * word; n * chain_texels >= 2^31.  The host entries of capture and bake also refuse a probe with pad + size * size > 2^31;
 * for the device entries that is the caller's duty.  Then as for a probe gather: a NULL or unaligned array; without a
 * valid scene RT_ERR_NOT_READY; light_count above the uploaded lights buffer.  n == 0 is RT_OK.
 * The stats are an rt_radiance_stats with rays = n * size * size texels and samples = rays * spt, summed over the radiance
 * launches as a probe gather's are.  Reflection probes have a path-query state and staging of their own, kept and grown:
 * capture, filter and bake leave the renderer and the other queries' state as they were.
 *   rt_capture_reflection         blocking: n probes in, n maps of size * size texels out.  stats != NULL runs the counting
 *                                 kernel and fills *stats.
 *   rt_filter_reflection          blocking: n maps in, n chains out.  Needs no scene.
 *   rt_bake_reflection            blocking: n probes in, n chains out.
 *   rt_capture_reflection_device, rt_bake_reflection_device
 *                                 the same on device-accessible arrays (16-byte aligned, on the context's device): only
 *                                 enqueue on the context's stream.  Count while rt_set_counting(ctx, 1) is on.
 *   rt_filter_reflection_device   dev_maps: n maps one behind the other - or dev_chains itself, and then map p is read in
 *                                 place as level 0 of chain p (the layout of a bake).  Only enqueues.
 *   rt_reflection_stats           stats of the last capture or bake (blocking: fences the stream). */
int rt_capture_reflection(rt_ctx* ctx, const rt_reflection_desc* desc, const rt_probe* probes, uint32_t n, uint32_t max_depth,
                          uint32_t seed, float* out_maps, rt_radiance_stats* stats);
int rt_capture_reflection_device(rt_ctx* ctx, const rt_reflection_desc* desc, const void* dev_probes, uint32_t n,
                                 uint32_t max_depth, uint32_t seed, void* dev_maps);
int rt_filter_reflection(rt_ctx* ctx, const rt_reflection_desc* desc, const float* maps, uint32_t n, float* out_chains);
int rt_filter_reflection_device(rt_ctx* ctx, const rt_reflection_desc* desc, const void* dev_maps, uint32_t n, void* dev_chains);
int rt_bake_reflection(rt_ctx* ctx, const rt_reflection_desc* desc, const rt_probe* probes, uint32_t n, uint32_t max_depth,
                       uint32_t seed, float* out_chains, rt_radiance_stats* stats);
int rt_bake_reflection_device(rt_ctx* ctx, const rt_reflection_desc* desc, const void* dev_probes, uint32_t n, uint32_t max_depth,
                              uint32_t seed, void* dev_chains);
int rt_reflection_stats(rt_ctx* ctx, rt_radiance_stats* out);

/* ---- the reflection sampler: "which radiance does this surface point reflect at this roughness?" read from baked chains on
 * the device, as rt_sample_volume reads a baked volume ----
 * A query (rt_reflection_query, mi355rt_layout.h) names a probe, the reflected direction and a roughness, and - for the
 * parallax correction - the position of the shaded point; the result is one 16-byte texel {r, g, b, hit_fraction}: a bilinear
 * fetch that follows the octahedral map across its seams, from the two levels of the chain around the roughness, mixed
 * linearly.  With RT_REFLECTION_SAMPLE_PARALLAX the direction is first bent to where it leaves the probe's proxy box
 * (rt_reflection_box), seen from the probe (Lagarde & Zanuttini 2012): a probe captured in the middle of a room then serves
 * points near its walls (csrc/k_reflection_sample.hip.h).  The second factor of the split sum, the BRDF integral, stays the
 * consumer's.
 *
 * THE REFLECTION SAMPLE RULE.  All arithmetic is f32, unfused, in the order written, with rt_div / rt_min / rt_floor of
 * mi355rt_math.h; pack is THE REFLECTION RULE's.  The chains are n_probes chains laid out as a bake lays them: chain p at the
 * texel p * chain_texels, its level m of side S = size >> m at the texel offset sum over k < m of (size >> k)^2, texel (i, j)
 * at j * S + i.
 *   probe      p = query.probe.  If p >= n_probes the result is {+0, +0, +0, +0} and nothing is loaded for the query.
 *   direction  d = query.direction, as given (not normalised).  Without RT_REFLECTION_SAMPLE_PARALLAX d' = d: the position,
 *              probes and boxes are never read, and the two arrays may be NULL.
 *   parallax   with the flag: x = query.position, c = probes[p].position, lo and hi of boxes[p].  inside = for every axis
 *              lo[a] <= x[a] && x[a] <= hi[a] (false with a NaN).  If !inside then d' = d.  Else per axis a: if d[a] > 0 then
 *              t_a = rt_div(hi[a] - x[a], d[a]); else if d[a] < 0 then t_a = rt_div(lo[a] - x[a], d[a]); else t_a = +inf (a
 *              zero and a NaN d[a] too).  t = rt_min(rt_min(t_x, t_y), t_z).  If !(t < +inf) then d' = d (a NaN t too).  Else
 *              h[a] = x[a] + d[a] * t, the product rounded before the sum, and d'[a] = h[a] - c[a].
 *   level      r = query.roughness; if !(r > 0) then r = +0 (a NaN too); r = rt_min(r, 1.0f).  xl = r * (float)(levels - 1);
 *              m0 = (uint32_t)xl, and if m0 > levels - 2 then m0 = levels - 2; m1 = m0 + 1; g = xl - (float)m0.  Level m0 has
 *              the weight 1.0f - g and level m1 the weight g.
 *   fold       a tap (i, j) with i and j in -1 .. S of a level of side S is folded across the octahedral seam, x first, then y:
 *              if i < 0 then i = -1 - i and j = S - 1 - j, else if i >= S then i = 2 S - 1 - i and j = S - 1 - j; then if j <
 *              0 then j = -1 - j and i = S - 1 - i, else if j >= S then j = 2 S - 1 - j and i = S - 1 - i.  (THE VISIBILITY
 *              RULE's wrap.)  The corner (-1, -1) becomes (S - 1, S - 1).
 *   fetch      of a level of side S at d': q = pack(d'), once for both levels.  Per axis u = (q * 0.5f + 0.5f) * (float)S -
 *              0.5f; if !(u >= -0.5f) then u = -0.5f (a NaN too); u = rt_min(u, (float)S - 0.5f); fl = rt_floor(u); i0 =
 *              (int)fl, in -1 .. S - 1; f = u - fl.  With (i0, fx) from q.x and (j0, fy) from q.y, wx = {1.0f - fx, fx}, wy =
 *              {1.0f - fy, fy}, the tap t_ab is the folded texel (i0 + a, j0 + b) and its weight w_ab = wx[a] * wy[b].  Per
 *              channel the level's value is (((+0 + w00 * t00) + w10 * t10) + w01 * t01) + w11 * t11, and a tap whose weight
 *              is exactly zero (+0 or -0) is left out of the sum, not multiplied: a NaN texel never reaches a result it has
 *              no weight in.  Every index is inside the map for every input.
 *   mix        out[ch] = (+0 + (1.0f - g) * A[ch]) + g * B[ch] for all four channels, A the value fetched from level m0 and B
 *              from level m1; a level whose weight is exactly zero is left out: it does not contribute, whatever it holds.
 *              (An implementation may still load the texels of a tap or a level it leaves out and drop them: every texel of
 *              every chain must be readable memory.)  Source texels are not sanitised.
 * A result depends on (chains, desc, probes[p], boxes[p], query) only - never on n or on the query's place in the array.
 * Refusals (RT_ERR_INVALID, every message begins with "reflection:", the descriptor checked before the context - without one
 * the message is what rt_last_error(NULL) returns): a NULL descriptor; size, levels and the smallest level as for
 * rt_reflection_desc; an unknown flag; a non-zero reserved word; n_probes == 0 with n > 0; n_probes * chain_texels >= 2^31;
 * n >= 2^31; a NULL array, or a device array that is not 16-byte aligned - probes and boxes only with
 * RT_REFLECTION_SAMPLE_PARALLAX.  n == 0 is RT_OK.  The sampler needs no scene, has staging of its own, kept and grown, and
 * leaves the renderer, rt_reflection_stats and every other query's state as they were.
 *   rt_sample_reflection         blocking: copies the n_probes chains (and with the flag the probes and boxes) and n queries
 *                                in, samples, copies n results of four floats out.  It uploads the chains on every call: a
 *                                caller sampling every frame keeps them on the device and uses
 *   rt_sample_reflection_device  the same on device-accessible arrays (16-byte aligned): only enqueues on the context's
 *                                stream. */
int rt_sample_reflection(rt_ctx* ctx, const rt_reflection_sample_desc* desc, const float* chains, uint32_t n_probes,
                         const rt_probe* probes, const rt_reflection_box* boxes, const rt_reflection_query* queries, uint32_t n,
                         float* out);
int rt_sample_reflection_device(rt_ctx* ctx, const rt_reflection_sample_desc* desc, const void* dev_chains, uint32_t n_probes,
                                const void* dev_probes, const void* dev_boxes, const void* dev_queries, uint32_t n, void* dev_out);

/* ---- probe visibility maps: "does this probe of the volume see the point it is about to light?" - the weight that keeps a
 * probe behind a wall from lighting the room in front of it ----
 * rt_sample_volume blends the eight surrounding probes by their trilinear weight alone, so indoors light leaks through
 * walls.  A visibility volume (rt_volume_visibility_desc, mi355rt_layout.h) holds, per probe of an irradiance volume, an
 * octahedral map of the mean and the mean square of the distance to the nearest surface; the sampler turns the two moments
 * into a Chebyshev bound on the share of the probe's surroundings that lies at least as far as the point, and multiplies the
 * trilinear weight by it (Majercik et al. 2019).  rt_bake_volume_visibility captures the maps with closest-hit ray queries;
 * rt_sample_volume_visible is rt_sample_volume with that weight; rt_encode_volume_visibility exports bordered tiles for
 * consumers that sample with a texture unit (csrc/k_volume_visibility.hip.h).
 *
 * THE VISIBILITY RULE.  All arithmetic is f32, unfused, in the order written, with rt_div / rt_rcp / rt_sqrt / rt_min / rt_max /
 * rt_abs / rt_floor / rt_normalize of mi355rt_math.h; pack, unpack, init_rng and the jitter are THE REFLECTION RULE's.
 *   capture    for probe p of the grid, texel t = j * size + i and sample s = 0 .. spt - 1: f = seed * spt + s (u32); pad_t =
 *              pad_first + p * size * size + t; the position is THE VOLUME RULE's; rng_d = init_rng(pad_t ^ 0x80000000, f), jx
 *              and jy its first two draws, px = rt_div((float)i + jx, (float)size) * 2 - 1, py alike, d = unpack(px, py).  The
 *              sample is x = rt_min(hit.t, max_distance), hit being what rt_trace_rays returns in RT_RAYS_CLOSEST mode at
 *              t_min = 0.001f for the ray {position, max_distance, d, pad_t}: a miss contributes max_distance, a NaN t too.
 *              Word 0 of the texel is ((+0 + x_0) + x_1) + ... in sample order, divided (rt_div) by (float)spt unless spt ==
 *              1; word 1 the same sum of x_s * x_s.  A map depends on (scene, desc, volume desc, seed) only - never on how the
 *              call is cut into batches.
 *   wrap       a tap (i, j) outside the map folds back across the octahedral edge, x first, then y: if i < 0 then i = -1 - i
 *              and j = size - 1 - j, else if i >= size then i = 2 size - 1 - i and j = size - 1 - j; then the same for j,
 *              mirroring i.
 *   fetch      at a unit direction v: q = pack(v); per axis u = (q * 0.5f + 0.5f) * (float)size - 0.5f; fl = rt_floor(u); if
 *              !(fl >= -1) then fl = -1 (a NaN u too); fl = rt_min(fl, (float)(size - 1)); i0 = (int)fl, fx = u - fl.  So
 *              every u, finite or not, names a tap in -1 .. size - 1 and its neighbour, which the wrap puts inside the map; a
 *              non-finite u only makes the weight fx non-finite.  The four wrapped taps t00 (i0, j0), t10, t01, t11 are read;
 *              for each of the two words a = t00 + fx * (t10 - t00), b = t01 + fx * (t11 - t01), the result a + fy * (b - a):
 *              a constant map fetches its constant exactly.
 *   sample     at {position, normal}: cell, corners, the trilinear weight tri_c, validity, W, the 27 sums, the division, the
 *              evaluation and the result layout are THE VOLUME RULE's with w_c = vis_c * tri_c in place of w_c = tri_c, the
 *              product rounded once; the replacement by +0 for an invalid probe still comes last.  With n =
 *              rt_normalize(normal), B = position + n * normal_bias and P_c the position of corner probe c:
 *                e = B - P_c, len = rt_sqrt(dot(e, e)).  If !(len > 0) then vis = 1 (a NaN len too).  Otherwise (m1, m2) =
 *                fetch(map_c, e * rt_rcp(len)); if len <= m1 then vis = 1; otherwise var = rt_abs(m1 * m1 - m2), g = len - m1,
 *                c = rt_div(var, var + g * g), if !(c > 0) then c = +0, c = (c * c) * c, vis = rt_max(c, min_visibility).
 *                With RT_VOLUME_VIS_BACKFACE: h = rt_normalize(P_c - position), b = (dot(h, n) + 1.0f) * 0.5f, vis = vis *
 *                (b * b + 0.2f).  (A point exactly on a probe has no h: that corner's weight is NaN, W is, and the result is
 *                {+0, +0, +0, +0} by the volume rule's !(W > 0).)
 *                If crush_threshold > 0 and vis < crush_threshold then vis = rt_div((vis * vis) * vis, crush_threshold *
 *                crush_threshold).
 *   export     every map becomes a tile of (size + 2)^2 texels whose one-texel border is the wrapped neighbour; the tiles lie
 *              nx per row in ny * nz rows, probe p at tile (p % nx, p / nx), in one image of nx (size + 2) by ny nz (size + 2)
 *              texels, rows top down: RT_LIGHTMAP_F32, 8 B per texel, the words unchanged; RT_LIGHTMAP_F16, 4 B, two
 *              rt_f32_to_f16.  RT_LIGHTMAP_RGBE8 is refused.
 * Refusals (RT_ERR_INVALID, every message begins with "volume visibility:", checked before the context - without one the
 * message is what rt_last_error(NULL) returns): a size that is no power of two in 4 .. 32; spt outside 1 .. 65536 (bake); a
 * max_distance that is not finite and > 0; a normal_bias that is not finite and >= 0; min_visibility or crush_threshold
 * outside [0, 1]; an unknown flag; a non-zero reserved word; nx * ny * nz * size * size >= 2^31; pad_first + nx * ny * nz * size
 * * size > 2^31 (bake); a NULL array; a device array that is not 16-byte aligned; dev_out == dev_visibility for the export.
 * The volume descriptor is checked first, by the volume's own check and with its messages.
 * A bake has a state of its own - counter shards, an event pair per ray launch, staging - and shares only the scratch of a
 * batch with the composed gathers: items are cut into batches of whole texels of at most RT_PROBE_BATCH_SAMPLES samples.  Its
 * stats are an rt_ray_stats summed over the batches (kernel_ms: the ray launches only).  Sampling and export need no scene
 * and have staging of their own.  All three leave the renderer and every other query's state, rt_ray_query_stats included,
 * as they were.
 *   rt_bake_volume_visibility          blocking: n * size * size texels back.  stats != NULL runs the counting kernel and
 *                                      fills *stats.  Without a valid scene RT_ERR_NOT_READY.
 *   rt_bake_volume_visibility_device   the same into a device-accessible array: only enqueues on the context's stream.
 *   rt_sample_volume_visible           blocking: copies the volume, the maps and n points in, samples, copies n results out.
 *                                      n == 0 is RT_OK; n >= 2^31 is RT_ERR_INVALID.
 *   rt_sample_volume_visible_device    the same on device-accessible arrays: only enqueues.
 *   rt_encode_volume_visibility        blocking: the maps into the tiled image at out; cap is its capacity in bytes.
 *   rt_encode_volume_visibility_device the same on device-accessible arrays.  Only enqueues. */
int rt_bake_volume_visibility(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t seed,
                              float* out, rt_ray_stats* stats);
int rt_bake_volume_visibility_device(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t seed,
                                     void* dev_out);
int rt_volume_visibility_stats(rt_ctx* ctx, rt_ray_stats* out);
int rt_sample_volume_visible(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis,
                             const rt_probe_sh9* volume, const float* visibility, const rt_gather_point* points, uint32_t n,
                             rt_irradiance* out);
int rt_sample_volume_visible_device(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis,
                                    const void* dev_volume, const void* dev_visibility, const void* dev_points, uint32_t n,
                                    void* dev_out);
int rt_encode_volume_visibility(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t format,
                                const float* visibility, void* out, size_t cap);
int rt_encode_volume_visibility_device(rt_ctx* ctx, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis,
                                       uint32_t format, const void* dev_visibility, void* dev_out, size_t cap);

/* ---- directional gathers: "which radiance arrives at this surface point, from which side?" as four spherical-harmonic
 * coefficients per colour over the hemisphere of the normal (directional lightmaps for normal-mapped surfaces) ----
 * An irradiance gather returns one colour per point, the cosine-weighted mean at the interpolated normal; a renderer that
 * perturbs that normal with a normal map needs the radiance as a function of direction.  Here the work item is again a
 * surface point (rt_gather_point, unchanged) and the result (rt_directional) is the projection of the radiance over the
 * hemisphere above it onto the real spherical harmonics of bands 0 .. 1, in world space.  It is the probe gather's
 * composition at surface points: k_dir_rays (one rt_ray per (point, sample)) -> the radiance query's kernel on those rays
 * at spp = 1 -> k_dir_project (one wave per point; csrc/k_directional.hip.h).  A lane of the irradiance gather keeps its
 * point for all spp samples, and twelve accumulators do not fit beside its path state.
 *
 * THE DIRECTIONAL RULE.  All arithmetic is f32, unfused, in the order written, with the rt_* functions of mi355rt_math.h.
 * For point i and sample s in 0 .. spp-1, with f = seed * spp + s in u32 arithmetic:
 *   direction  d0 = the probe rule's direction for (pad, f): uniform on the sphere, from rng_d = init_rng(pad ^ 0x80000000,
 *              f).  With N the point's normal as given (not normalised): c = (d0.x * N.x + d0.y * N.y) + d0.z * N.z;  d = (c <
 *              0.0f) ? (-d0.x, -d0.y, -d0.z) : d0 as a float comparison (a NaN does not flip).  Uniform on the hemisphere of
 *              N; not normalised again.
 *   sample     {r, g, b, t}: exactly what rt_trace_radiance returns for the ray {position, t_max, d, pad} with spp = 1 and
 *              seed = f.  It is a hit iff t < t_max (false for NaN).  Keep pad < 2^31, as for a gather.
 *   basis      bands 0 and 1 of the probe rule: for d = (x, y, z): Y0 = 0.282094792f; Y1 = 0.488602512f * y; Y2 =
 *              0.488602512f * z; Y3 = 0.488602512f * x.  The term of (k, c) is radiance[c] * Yk.
 *   sum        the probe rule's fixed tree, for each of the 12 sums and for the hit count: the partial P[l], l = 0 .. 63, is
 *              ((+0 + term(l)) + term(l + 64)) + ... over the samples s = l (mod 64), ascending; then for m = 32, 16, 8, 4, 2,
 *              1, in all l at once, P[l] = P[l] + P[l ^ m] (own value first); the sum is P[0].
 *   result     layer[k][c] = rt_div(sum, (float)spp) * RT_TWO_PI, the Monte-Carlo estimate of the integral of L(w) Yk(w)
 *              over the hemisphere, c = 0 .. 2;  layer[k][3] = rt_div((float)hits, (float)spp) for all four k.  max_depth ==
 *              0: every first segment is still traced, and the twelve coefficients come out +0.
 * Every row layer[k] has the shape of an rt_irradiance - a 16-byte texel whose fourth word >= 0 says "covered" - so that
 * scattering a result into four atlas layers is four plain copies and the filter, the gutter fill and the encode read each
 * layer as the texel they know.  The irradiance at a unit normal n follows by the cosine-lobe convolution of bands 0 .. 1:
 * E(n) = pi * Y0 * c0 + (2 pi / 3) * 0.488602512 * (c1 n.y + c2 n.z + c3 n.x), a host (or shader) one-liner.
 * A result depends on (scene, point, pad, seed, spp, max_depth) only - never on n, the point's position in the array or how
 * the library splits the work: a call is cut into batches of whole points of at most RT_DIRECTIONAL_BATCH_SAMPLES samples,
 * whose rays and radiances live in the scratch the probe gather uses too (per-call scratch on the one stream).
 * The stats are an rt_radiance_stats as for a probe gather: rays = n points, samples = n * spp; the counters and workgroups
 * are the sums over the radiance launches, and kernel_ms is the summed time of the RADIANCE launches only.
 * A directional gather leaves the renderer as it was and has a state of its own: the stats and staging of radiance queries,
 * irradiance gathers and probe gathers are untouched.
 *   rt_gather_directional         blocking: copies n points in, gathers, copies n results out.  stats != NULL runs the
 *                                 counting kernel and fills *stats.  n == 0 is RT_OK; n >= 2^31, a NULL pointer, spp == 0 or
 *                                 spp > 65536 is RT_ERR_INVALID; without a valid scene RT_ERR_NOT_READY; light_count above the
 *                                 uploaded lights buffer is RT_ERR_INVALID.  Messages begin with "directional gather:".
 *   rt_gather_directional_device  the same on device-accessible arrays (n rt_gather_point in, n rt_directional out; 16-byte
 *                                 aligned, on the context's device): only enqueues on the context's stream.  Counts while
 *                                 rt_set_counting(ctx, 1) is on.
 *   rt_directional_gather_stats   stats of the last directional gather (blocking: fences the stream).
 * Not built: band 2 (five more layers per atlas), tangent-space bases (the coefficients are world-space; band 1 rotates as
 * the vector (layer[3], layer[1], layer[2])). */
#define RT_DIRECTIONAL_BATCH_SAMPLES (1u << 22)
int rt_gather_directional(rt_ctx* ctx, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp,
                          uint32_t seed, rt_directional* out, rt_radiance_stats* stats);
int rt_gather_directional_device(rt_ctx* ctx, const void* dev_points, uint32_t n, uint32_t max_depth, uint32_t spp,
                                 uint32_t seed, void* dev_out);
int rt_directional_gather_stats(rt_ctx* ctx, rt_radiance_stats* out);

/* ---- lightmap bakes: "the gather points of this instance's atlas", rasterised on the device ----
 * An irradiance gather wants surface points; a lightmap wants one per covered texel of an instance's UV atlas.  The scene
 * holds what that takes on the device (uv, pos, nrm, topology, the instances' forward transforms, the draw commands with
 * each instance's triangle range) - also after rt_world_update, when the skinned vertices exist nowhere else - so the
 * UV-space rasteriser runs there (csrc/k_bake.hip.h) and its points feed rt_gather_irradiance without leaving HBM.
 *
 * THE TEXEL RULE.  All arithmetic is f32, unfused (no FMA contraction), in the order written, with rt_div / rt_normalize
 * of mi355rt_math.h for division and square root.  Inputs: an rt_bake_desc d {inst, width W, height H, pad_base, t_max}
 * (mi355rt_layout.h) and optionally an override array atlas_uv of 2 f32 per vertex of the WHOLE scene (lightmap UVs are
 * rarely the texture UVs).  uv(j), the atlas UV of global vertex j, is atlas_uv[j] when the array is given, else the
 * scene's uv[j].
 *   triangles   of instance d.inst: the global triangles k in [dc.z / 3, dc.z / 3 + dc.x / 3) of its draw command dc = {3
 *               n_tris, 1, 3 first_tri, i} (integer division), in ascending k.  A k at or beyond the topology's triangle
 *               count is skipped and never read.
 *   vertices    in texel space, with (v0, v1, v2) the topology row's vertex ids: a = (uv(v0).x * (float)W, uv(v0).y *
 *               (float)H), b and c likewise from v1, v2.
 *   texel       (x, y), 0 <= x < W, 0 <= y < H, has index y * W + x and centre p = ((float)x + 0.5f, (float)y + 0.5f).
 *               Row 0 is v near 0: nothing is flipped.
 *   E(q, r, s)  = (r.x - q.x) * (s.y - q.y) - (r.y - q.y) * (s.x - q.x), and A = E(a, b, c).
 *   coverage    triangle k covers the texel iff (1) a.x, a.y, b.x, b.y, c.x, c.y and A are all finite and A != 0; (2)
 *               min(a.x, b.x, c.x) <= p.x <= max(a.x, b.x, c.x) and the same in y; (3) with sg = A > 0 ? 1.0f : -1.0f: sg *
 *               E(a, b, p) >= 0, sg * E(b, c, p) >= 0 and sg * E(c, a, p) >= 0.  (2) makes a sweep over the triangle's
 *               bounding box exact, also for needles whose edge values all round to 0.
 *   owner       of a texel: the LOWEST global triangle index that covers it, or none.  This settles overlapping charts,
 *               both windings, duplicate triangles and centres on shared edges.
 *   point       of a texel with owner k: bu = rt_div(E(c, a, p), A) (the weight of v1), bv = rt_div(E(a, b, p), A) (of v2),
 *               bw = 1.0f - bu - bv;  V0, V1, V2 = rt_mat_mul_point(instance transform, pos[v*]) (the world-space triangle
 *               light sampling makes);  position = (bw * V0 + bu * V1) + bv * V2;  normal = rt_normalize(rt_vec_mul_mat_dir(
 *               rt_normalize((nrm[v0] * bw + nrm[v1] * bu) + nrm[v2] * bv), instance inverse)) (the shading normal of a
 *               traced hit, without the normal map);  t_max = d.t_max;  pad = d.pad_base + y * W + x.
 *   output      the covered texels in ASCENDING TEXEL INDEX, compacted: points[j] (rt_gather_point) and texels[j] (u32),
 *               j = 0 .. n-1.  The optional owner map holds W * H i32: the owner's global triangle index, -1 for none.
 * The rule has no run-time freedom: two bakes of one scene give the same words, and a CPU restatement (tests/model/
 * bake_model.cpp) gives them too.  Out of scope: chart packing, conservative rasterisation.  Several instances per call: atlas
 * bakes, below; a gutter of copied colour around the charts: atlas dilation, below them; the filter of a noisy bake, guided
 * by these points: atlas denoise, below that.
 * Limits, all RT_ERR_INVALID: a NULL descriptor, reserved != 0, W or H == 0, W * H > 2^24, pad_base + W * H > 2^31 (the
 * gather's pad rule), inst >= the instance count, a NULL output that is needed.  Without a valid scene: RT_ERR_NOT_READY;
 * also when the scene has no draw command for every instance (rt_upload(RT_KIND_DRAW_COMMANDS) was never called).
 * A bake leaves the renderer as it was, like the queries above; it has staging arrays of its own, kept and grown.
 *   rt_bake_points         blocking, one fence.  atlas_uv: host array or NULL = the scene's uvs; when given, n_uv_vertices
 *                          must be the scene's vertex count.  Writes min(n, cap) records to points_out / texels_out and
 *                          sets *n_out = n; cap < n is RT_OK with *n_out > cap; cap == 0 (outputs may be NULL) only counts.
 *                          owner_out: W * H i32 or NULL.  The price of the single fence: min(cap, W * H) records (36 B each)
 *                          are staged on the device and cross to a host buffer before n is known, whatever the coverage -
 *                          about 600 MB at 4096 x 4096.  A caller who minds counts first (cap == 0) and passes cap = n.
 *   rt_bake_points_device  the same on device-accessible arrays (16-byte aligned, on the context's device; dev_atlas_uv: 2
 *                          f32 per scene vertex or NULL; dev_count: one u32; dev_owner: W * H u32 or NULL; dev_points /
 *                          dev_texels may be NULL when cap == 0): only enqueues on the context's stream (rt_set_stream
 *                          respected).
 *   rt_bake_irradiance     the whole bake: points -> rt_gather_irradiance's kernel on them (max_depth, spp, seed as there) ->
 *                          scatter.  atlas_out[texels[j]] is, bit for bit, what rt_gather_irradiance returns for points[j];
 *                          every uncovered texel is {+0, +0, +0, -1.0f} (hit_fraction lies in [0, 1], so -1 says "no
 *                          surface").  *n_covered_out (may be NULL) = n.  stats (may be NULL) are the gather's: the
 *                          counting kernel runs, and rt_irradiance_gather_stats reports this gather afterwards.  One host
 *                          read of the count between the point pass and the gather.  The values are E / pi: multiply by pi *
 *                          albedo for the outgoing radiance of a Lambert texel.  An enqueue-only form of the whole bake is
 *                          not offered: chain rt_bake_points_device and rt_gather_irradiance_device; the whole pipeline
 *                          with one read of the count is rt_bake_atlas_lightmap, below. */
int rt_bake_points(rt_ctx* ctx, const rt_bake_desc* desc, const float* atlas_uv, uint32_t n_uv_vertices,
                   rt_gather_point* points_out, uint32_t* texels_out, uint32_t cap, uint32_t* n_out, int32_t* owner_out);
int rt_bake_points_device(rt_ctx* ctx, const rt_bake_desc* desc, const void* dev_atlas_uv, void* dev_points, void* dev_texels,
                          uint32_t cap, void* dev_count, void* dev_owner);
int rt_bake_irradiance(rt_ctx* ctx, const rt_bake_desc* desc, const float* atlas_uv, uint32_t n_uv_vertices, uint32_t max_depth,
                       uint32_t spp, uint32_t seed, rt_irradiance* atlas_out, uint32_t* n_covered_out, rt_radiance_stats* stats);

/* ---- atlas bakes: "the lightmap of these instances, each in its rectangle of one atlas", in one call ----
 * Instances of one geometry share their triangles and vertices, hence their UV chart: what tells their texels apart is a
 * rectangle of the atlas per instance.  An atlas bake is one point pass, one gather and one scatter over a list of them.
 *
 * THE ATLAS RULE.  Inputs: an rt_bake_atlas_desc d {width W, height H, pad_base, t_max, n_entries} and n_entries records
 * rt_bake_rect {inst, x, y, width w, height h} (mi355rt_layout.h), entry e being the e-th; optionally atlas_uv as above.
 *   local bake  of entry e: by definition THE TEXEL RULE for the rt_bake_desc {inst, w, h}: texel-space vertices are uv *
 *               ((float)w, (float)h), local texels (lx, ly) with 0 <= lx < w, 0 <= ly < h and centres + 0.5f; coverage,
 *               owner triangle k and point as written there.  Nothing is offset in float: a chart that runs outside [0, 1]
 *               is clipped to its rectangle by construction and never reaches a neighbour's texels.
 *   placement   entry e covers atlas texel (X, Y) = (x + lx, y + ly) with triangle k when its local bake covers (lx, ly)
 *               with k.  The atlas texel has index Y * W + X.
 *   owner       of an atlas texel: the lexicographically LOWEST (e, k) that covers it, or none.  This settles overlapping
 *               rectangles, one instance listed twice, and everything the lowest-k sentence settles.
 *   point       of an atlas texel with owner (e, k): the local rule's point for (lx, ly), k and the entry's instance -
 *               position and normal as there, t_max = d.t_max - with pad = d.pad_base + Y * W + X.
 *   output      the covered atlas texels in ASCENDING ATLAS TEXEL INDEX, compacted: points[j] and texels[j].  The optional
 *               owner map holds W * H pairs {i32 entry, i32 triangle}, {-1, -1} for none.
 * Two identities follow.  (A) One entry {inst, 0, 0, W, H} gives, word for word with the pads, what rt_bake_points gives for
 * {inst, W, H, pad_base, t_max}.  (B) Any atlas bake is the composition of its entries' single-instance bakes:
 * rt_bake_points per entry, placed at the rectangle, the lowest entry winning, the pads re-based.
 * Out of scope: chart packing (the caller chooses the rectangles), a t_max per entry, an enqueue-only form of the whole bake (the
 * gather would have to take its count from the device; with one read of the count: rt_bake_atlas_lightmap_device, below).
 * Limits, all RT_ERR_INVALID: a NULL descriptor or NULL entries, reserved != 0 (descriptor or any entry), n_entries == 0 or
 * > 65536, W or H == 0, W * H > 2^24, pad_base + W * H > 2^31, any w or h == 0, any rectangle not inside the atlas (x + w
 * <= W and y + h <= H, taken without u32 overflow), any inst >= the instance count, and what the bake entries above say about
 * NULL outputs and n_uv_vertices.  RT_ERR_NOT_READY as for a bake.  Messages begin with "bake atlas:".
 * The entries are a HOST array in all three forms, and the library has copied them when it returns.  cap, n_out, the stats,
 * {+0, +0, +0, -1.0f} in uncovered texels and "leaves the renderer as it was" are as in the three entries above.
 *   rt_bake_atlas_points         blocking, one fence.  owner_out: 2 i32 per atlas texel {entry, triangle}, or NULL.
 *   rt_bake_atlas_points_device  device-accessible arrays as in rt_bake_points_device; dev_owner: W * H u64, (entry << 32) |
 *                                triangle, all ones for none (the map as the kernels keep it), or NULL.  Only enqueues on
 *                                the context's stream: the entries go through a pinned staging buffer of the bake's own.
 *   rt_bake_atlas_irradiance     the whole bake: ONE gather over all entries' points.  atlas_out[texels[j]] is, bit for bit,
 *                                what rt_gather_irradiance returns for points[j].  One host read of the count. */
int rt_bake_atlas_points(rt_ctx* ctx, const rt_bake_atlas_desc* desc, const rt_bake_rect* entries, const float* atlas_uv,
                         uint32_t n_uv_vertices, rt_gather_point* points_out, uint32_t* texels_out, uint32_t cap,
                         uint32_t* n_out, int32_t* owner_out);
int rt_bake_atlas_points_device(rt_ctx* ctx, const rt_bake_atlas_desc* desc, const rt_bake_rect* entries, const void* dev_atlas_uv,
                                void* dev_points, void* dev_texels, uint32_t cap, void* dev_count, void* dev_owner);
int rt_bake_atlas_irradiance(rt_ctx* ctx, const rt_bake_atlas_desc* desc, const rt_bake_rect* entries, const float* atlas_uv,
                             uint32_t n_uv_vertices, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_irradiance* atlas_out,
                             uint32_t* n_covered_out, rt_radiance_stats* stats);

/* ---- atlas dilation: "a gutter of copied colour around every chart", the nearest covered texel into the uncovered ones ----
 * A baked atlas holds {0, 0, 0, -1} wherever no chart covers a texel, and a renderer that samples it bilinearly or through
 * mip maps blends every chart border with that black.  Dilation copies, into every uncovered texel within `radius` texels of
 * a chart, the colour of the nearest covered texel.  One ring is simple on the host; a gutter of 4 .. 16 texels, which mip
 * chains need, is a nearest-source search, and after rt_bake_atlas_points_device plus rt_gather_irradiance_device the atlas
 * is in HBM and nowhere else - so the search runs there, on a coverage bitmap (csrc/k_dilate.hip.h).
 *
 * THE DILATION RULE.  All of it is integer arithmetic; no float is computed, only compared and copied.  Inputs: an
 * rt_dilate_desc {width W, height H, radius R} (mi355rt_layout.h) and an atlas of W * H texels of 4 f32 {x, y, z, w},
 * row-major, texel (x, y) at index i = y * W + x.
 *   coverage   a texel is covered iff w >= 0.0f as a float comparison: NaN is uncovered, -0.0f and +inf are covered, -1.0f
 *              (no surface) and -2.0f (filled, below) are uncovered.
 *   source     of an uncovered texel (x, y): among the covered texels (sx, sy) of the atlas with d2 = (sx - x)^2 + (sy - y)^2
 *              <= R * R, the one with the smallest d2, and among equals the one with the lowest texel index sy * W + sx.
 *              Texels outside the atlas do not exist.
 *   result     in place.  A covered texel is untouched.  An uncovered texel with a source receives the source's first three
 *              words bit for bit and w = -2.0f: "no surface here, colour copied".  An uncovered texel without a source is
 *              untouched, whatever it holds.
 *   source map (optional) W * H u32: a covered texel holds its own index, a filled texel its source's index, any other
 *              texel 0xffffffff.  With it a caller applies the same fill to other layers of the same atlas.
 *   count      (optional) one u32: the number of filled texels.
 * Three things follow.  (1) The result does not depend on scheduling: every word is a function of the input alone.  (2)
 * Dilating a dilated atlas again with the same R gives the same words: filled texels stay uncovered (w = -2.0f) and find the
 * same sources.  (3) Covered texels are only read and uncovered texels are only written, so in place is safe.
 * Limits, all RT_ERR_INVALID with messages that begin "dilate atlas:": a NULL descriptor or a NULL atlas, reserved != 0, W or
 * H == 0, W * H > 2^24 (the bakes' limit), R > RT_DILATE_MAX_RADIUS (24).  R == 0 is valid and fills nothing.
 * No scene is needed: the calls work on a fresh context, and they leave the renderer and the state of every query as they
 * were.  Dilation has staging arrays of its own, kept and grown: the bitmap (8 bytes per 64 texels of a row) and, unless the
 * caller supplies one, the source map.
 *   rt_dilate_atlas         blocking, host arrays: copies the atlas in, dilates, copies it back; src_out (W * H u32) and
 *                           filled_out (one u32) may be NULL.
 *   rt_dilate_atlas_device  the same on device-accessible arrays (16-byte aligned - the single count word too - and on the
 *                           context's device); dev_src and dev_filled may be NULL.  Only enqueues on the context's stream
 *                           (rt_set_stream respected). */
int rt_dilate_atlas(rt_ctx* ctx, const rt_dilate_desc* desc, float* atlas, uint32_t* src_out, uint32_t* filled_out);
int rt_dilate_atlas_device(rt_ctx* ctx, const rt_dilate_desc* desc, void* dev_atlas, void* dev_src, void* dev_filled);

/* ---- atlas denoise: "the filter between the gather and the gutter fill", an edge-stopped a-trous blur of a baked atlas ----
 * A bake a user can afford is tens of samples per texel and visibly noisy.  A plain blur bleeds one wall into the next, for
 * neighbouring texels of an atlas are often unrelated surfaces; the world position and shading normal that the bake entries
 * emit for every covered texel say which neighbours lie on the same surface.  After rt_bake_*_points_device and
 * rt_gather_irradiance_device atlas and points are in HBM and nowhere else - so the filter runs there (csrc/k_denoise.hip.h).
 *
 * THE DENOISE RULE.  All arithmetic is f32, unfused (no FMA contraction), in the order written; rt_div of mi355rt_math.h does
 * the one division.  The weights use no exp: every output word is reproducible.  Inputs: an rt_denoise_desc {width W, height
 * H, step, passes, normal_cos, plane_eps, max_dist} (mi355rt_layout.h); atlas_in, W * H texels of 4 f32, row-major, texel (x,
 * y) at index i = y * W + x; points, n rt_gather_point, and texels, n u32 - points[j] and texels[j] exactly as the bake
 * entries emit them; atlas_out, W * H texels.
 *   guide      texel i is GUIDED iff some j < n has texels[j] == i; its guide is points[j] for the LOWEST such j (position P,
 *              normal N, taken as given and not re-normalised).  An entry with texels[j] >= W * H is ignored.  The atlas's own
 *              fourth component is never consulted.
 *   one pass   at step s, out of place.  An unguided texel's 16 bytes are copied bit for bit.  A guided texel (x, y) visits
 *              the taps (dx, dy), dy = -2 .. 2 outer and dx = -2 .. 2 inner, both ascending; the tap texel is q = (x + dx *
 *              s, y + dy * s) and the tap weight h = k[|dx|] * k[|dy|] with k = {0.375f, 0.25f, 0.0625f}.
 *   accepted   the centre tap always.  Any other tap iff all of these hold as float comparisons (a NaN fails every one), with
 *              md2 = max_dist * max_dist:  q is inside the atlas;  q is guided, with guide position Pq and normal Nq;
 *              (N.x * Nq.x + N.y * Nq.y) + N.z * Nq.z >= normal_cos;  with d = Pq - P,
 *              |(N.x * d.x + N.y * d.y) + N.z * d.z| <= plane_eps;  (d.x * d.x + d.y * d.y) + d.z * d.z <= md2.
 *   result     acc[0 .. 3] and wsum start at +0; for every accepted tap in visiting order, for each channel c = 0 .. 3,
 *              acc[c] = acc[c] + h * in[q][c], and wsum = wsum + h.  out[c] = rt_div(acc[c], wsum).  All four channels are
 *              filtered alike: hit_fraction stays in [0, 1], and a max_depth = 0 ambient-occlusion bake is denoised too.
 *   a call     runs `passes` passes, pass p at step `step << p`: in -> ... -> out, by ping-pong through one scratch atlas the
 *              library owns.  atlas_in is never written.
 * Three things follow.  (1) {step 1, passes 3} is the composition of {1, 1}, {2, 1} and {4, 1}, word for word.  (2) n == 0
 * copies the atlas.  (3) A result texel depends only on the inputs, never on tile shape or scheduling: the guide index is an
 * integer minimum and every sum has a fixed order.
 * Limits, all RT_ERR_INVALID with messages that begin "denoise atlas:": a NULL descriptor or a NULL array (points and texels
 * may be NULL only when n == 0), reserved != 0, W or H == 0, W * H > 2^24 (the bakes' limit), step == 0, passes == 0, step <<
 * (passes - 1) > RT_DENOISE_MAX_STEP (4), n > W * H.  The float parameters are not validated: a normal_cos above 1, or a NaN,
 * simply rejects every tap but the centre.
 * Not built: a luminance or variance stop, other texel formats, steps above 4.  (The filter inside a
 * whole bake, on the guides the bake already holds in HBM: rt_bake_atlas_lightmap, below.)
 * No scene is needed: the calls work on a fresh context, and they leave the renderer and the state of every query as they
 * were.  Denoising has staging arrays of its own, kept and grown: the guide index map (4 bytes per texel), the scratch atlas
 * and, for the host entry, the staged inputs and output.
 *   rt_denoise_atlas         blocking, host arrays: copies atlas, points and texels in, filters, copies the result to
 *                            atlas_out, which may equal atlas_in.
 *   rt_denoise_atlas_device  the same on device-accessible arrays (16-byte aligned, on the context's device).  dev_out ==
 *                            dev_in is refused; any other overlap is the caller's fault.  Only enqueues on the context's
 *                            stream (rt_set_stream respected): one index build, then `passes` launches. */
int rt_denoise_atlas(rt_ctx* ctx, const rt_denoise_desc* desc, const float* atlas_in, const rt_gather_point* points,
                     const uint32_t* texels, uint32_t n, float* atlas_out);
int rt_denoise_atlas_device(rt_ctx* ctx, const rt_denoise_desc* desc, const void* dev_in, const void* dev_points,
                            const void* dev_texels, uint32_t n, void* dev_out);

/* ---- frame denoise: "a clean frame from one sample per pixel", an edge-stopped a-trous filter of the frame ahead of present()
 * ----
 * The live loop shows a 1-spp image almost all the time, and the post pass has a 3 x 3 bilateral only.  After every compute()
 * the guides an edge-stopped filter needs are in HBM: the octahedral normal with triangle and instance id, the clip depth and
 * the unorm8 albedo, 24 B per pixel.  The filter runs there (csrc/k_frame_denoise.hip.h) and writes an image in the
 * accumulator's format, which present() can read through rt_bind_present_source or by itself (rt_set_present_denoise).
 *
 * THE FRAME DENOISE RULE.  All arithmetic is f32, unfused (no FMA contraction), in the order written, with rt_div / rt_sqrt /
 * rt_exp / rt_max / rt_abs / rt_normalize / rt_length / rt_from_unorm8 of mi355rt_math.h; `/` below is the language's division
 * where the post pass uses it.  Inputs: an rt_frame_denoise_desc {passes, step, flags, normal_cos, plane_eps, sigma_lum}
 * (mi355rt_layout.h); the context's accumulation buffer A (a bound one included), W x H texels {r, g, b, a}, pixel (x, y) at i
 * = y * W + x; the G-buffer of the last compute() - the planes rt_read_gbuffer reads, the slot of a frame traced ahead
 * included: albedo word alb[i], normal_id[i] = {ox, oy, bits(tri), bits(inst)}, depth[i]; and U, the uniform block of that
 * frame (rt_read_uniforms).  lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b.
 *   background  pixel i is BACKGROUND iff the alpha byte of alb[i] is 0 (k_primary_visibility writes 0 for a miss, 255 for a
 *               hit), else a SURFACE.
 *   radiance    rad(x, y), coordinates clamped to the image: get_radiance of the post pass, a <= 0 ? (0, 0, 0) : (r / a, g / a,
 *               b / a).
 *   modulation  m[i] = (1, 1, 1) without RT_FRAME_DENOISE_DEMODULATE and on the background; else m[i][c] =
 *               rt_max(rt_from_unorm8(byte c of alb[i]), RT_FRAME_DENOISE_MIN_ALBEDO), c = 0 .. 2.  alpha[i] = a > 0 ? 1 : 0.
 *   quantity    q(x, y), coordinates clamped: (rt_div(rad[0], m[0]), rt_div(rad[1], m[1]), rt_div(rad[2], m[2])) - what the
 *               passes filter.
 *   variance    m1 = m2 = +0; for dy = -1 .. 1 outer, dx = -1 .. 1 inner: l = lum(q(x + dx, y + dy)); m1 = m1 + l; m2 = m2 + l
 *               * l.  mean = rt_div(m1, 9.0f); var = rt_max(rt_div(m2, 9.0f) - mean * mean, 0.0f), as the post pass forms it.
 *   guide       of a surface: the normal N = n / |n| by rt_normalize of n = (ox, oy, 1.0f - rt_abs(ox) - rt_abs(oy)) with t =
 *               rt_saturate(-n.z) and n.x += (n.x >= 0 ? -t : t), n.y likewise (unpack_normal of the path tracer); the
 *               instance, the bits of normal_id[i].w; the world position P, the inverse of k_primary_visibility's depth on the
 *               pixel's own jittered pinhole ray: center = ll + hor * 0.5f + ver * 0.5f; focal = rt_length(center - eye); u =
 *               ((float)x + 0.5f + U.jitter[0] * (float)W) / (float)W; v = 1.0f - ((float)y + 0.5f + U.jitter[1] * (float)H) /
 *               (float)H; d = ll + u * hor + v * ver - eye (left to right, per component); ca = 10000.0f / (10000.0f -
 *               0.001f); cb = (10000.0f * 0.001f) / (10000.0f - 0.001f); z_view = rt_div(cb, ca - depth[i]); t = rt_div(z_view,
 *               focal); P[c] = eye[c] + d[c] * t.  The stored depth is ca - cb / z_view with ca one ulp above 1, so z_view
 *               comes back in steps of z^2 * 2^-24 / cb = 6e-5 z^2: DESIGN.md 4.3b.  The guide of a background pixel is all
 *               zero.  A guide is 32 bytes, {P.xyz, bits(inst)} {N.xyz, bits(surface ? 1 : 0)}: the unit normal as three f32,
 *               so that no tap decodes anything.
 *   prepare     one pass over the image, out of place: colour texel col[i] = {q(x, y), var}, guide[i], modulation texel {m[i],
 *               alpha[i]}.
 *   one pass    at spacing s, out of place.  A background pixel's 16 bytes are copied bit for bit.  A surface pixel p = (x, y)
 *               with centre values lum_p = lum(col[p].rgb), den = sigma_lum * rt_sqrt(col[p].w) + 1e-4f visits the taps (dx,
 *               dy), dy = -2 .. 2 outer and dx = -2 .. 2 inner; the tap pixel is q = (x + dx * s, y + dy * s) and h = k[|dx|] *
 *               k[|dy|] with k = {0.375f, 0.25f, 0.0625f}, as in the atlas rule.
 *   accepted    the centre tap always.  Any other tap iff all of these hold (a NaN fails each float comparison):  q is inside
 *               the image and a surface;  with RT_FRAME_DENOISE_SAME_INSTANCE, q's instance word equals p's;  (N.x * Nq.x +
 *               N.y * Nq.y) + N.z * Nq.z >= normal_cos;  with e = Pq - P, rt_abs((N.x * e.x + N.y * e.y) + N.z * e.z) <=
 *               plane_eps.
 *   weight      of an accepted tap, the centre included: w = h when !(sigma_lum > 0) - no exponential is evaluated - else w =
 *               h * rt_exp(rt_div(-rt_abs(lum(col[q].rgb) - lum_p), den)).
 *   result      acc[0 .. 2], vacc and wsum start at +0; for every accepted tap in visiting order acc[c] = acc[c] + w *
 *               col[q][c], vacc = vacc + (w * w) * col[q].w, wsum = wsum + w.  out = {rt_div(acc[c], wsum), rt_div(vacc, wsum
 *               * wsum)}: the weighted mean and the variance of that mean.
 *   finish      after the last pass: out[i] = {col[i][0] * m[i][0], col[i][1] * m[i][1], col[i][2] * m[i][2], alpha[i]} - the
 *               accumulator's format with weight 1, so present() can read it as it stands.
 *   a call      prepare, then `passes` passes, pass p at spacing `step << p`, by ping-pong through two colour images the
 *               library owns, then finish.  The accumulation buffer and the G-buffer are never written.
 * Three things follow.  (1) {step 1, passes 3} is prepare, the passes at 1, 2 and 4 and finish, word for word.  (2) A result
 * word depends only on the inputs, never on the form of a pass, tile shape or scheduling: no atomics, no cross-lane sums,
 * every sum in a fixed order.  (3) Background radiance passes through bit for bit (rad * 1) and never enters a surface.
 * The forms of a pass: k_frame_pass_lds stages the tile's window in LDS (spacings 1 .. 4, where the window fits),
 * k_frame_pass_direct reads its taps through L1 / L2 (every spacing).  rt_set_frame_denoise_form: 0 = auto (per spacing, what
 * was measured faster, DESIGN.md 4.3b: the LDS form at spacings 1 .. 3, the direct form from 4), 1 = LDS, 2 = direct; 1 is
 * refused by a call with a spacing above 4.
 * THE ALBEDO PLANE IS THE RENDER TARGET: present() overwrites it.  The outputs of the prepare stage are therefore kept, keyed
 * on a per-context count of dispatches that wrote a G-buffer: after a present() with no compute() between, the calls reuse
 * them when flags has the same DEMODULATE bit and the accumulation buffer has not been written through the API since
 * (rt_write_accum, rt_reset_accum, rt_bind_accum drop them, as do rt_resize, the uploads and rt_set_scene); else they fail with
 * RT_ERR_NOT_READY, "frame denoise: the albedo plane was overwritten by present(); call compute first".
 * Refusals, all RT_ERR_INVALID with messages that begin "frame denoise:", made before anything is enqueued: a NULL
 * descriptor or output, passes == 0 or > 5, step == 0, step << (passes - 1) > RT_FRAME_DENOISE_MAX_STEP (16), an unknown flag
 * bit, a non-zero reserved word, an output that is the accumulation buffer, a capacity below W * H * 16, a forced LDS form with
 * a spacing above 4.  Without a screen or a G-buffer (no rt_resize, no compute() yet): RT_ERR_NOT_READY.  The float
 * parameters are not validated: a NaN normal_cos rejects every tap but the centre.
 * Temporal reprojection and moment history (SVGF's temporal half) are the optional stage of "frame temporal" below.
 * Not built: separate treatment of specular and emissive surfaces under demodulation (a light's radiance is
 * divided by its albedo like any other); stripes and ranks (a rank's G-buffer covers only its own rows: refused).
 * The two explicit calls leave accumulation, history, counters, the G-buffer, frames traced ahead and every query's state
 * unchanged.
 *   rt_denoise_frame          blocking, one fence: filters into a buffer of the library's and copies W * H * 16 bytes out.
 *   rt_denoise_frame_device   enqueue only, on the context's stream: dev_out is W * H float4 on the context's device, may
 *                             afterwards be given to rt_bind_present_source, and must not be the accumulation buffer.
 *   rt_set_present_denoise    desc != NULL: from now on rt_present filters into a buffer the context owns and the post pass
 *                             reads that; NULL (the default) restores the plain path exactly.  Refused, with an explicit
 *                             message, while a present source is bound, on a rank (rt_dist_init) and with stripes on; and
 *                             while it is set, rt_bind_present_source(non-NULL), rt_dist_init and rt_set_stripes(count > 1)
 *                             are refused.
 *   rt_set_frame_denoise_form see above.
 *   rt_frame_denoise_stats    blocking: stream times of the last call's stages (an event pair of its own: no RT_TIMER_* entry),
 *                             the form of every pass and whether the cache was hit. */
int rt_denoise_frame(rt_ctx* ctx, const rt_frame_denoise_desc* desc, float* out_rgba32f, size_t cap_bytes);
int rt_denoise_frame_device(rt_ctx* ctx, const rt_frame_denoise_desc* desc, void* dev_out);
int rt_set_present_denoise(rt_ctx* ctx, const rt_frame_denoise_desc* desc_or_null);
int rt_set_frame_denoise_form(rt_ctx* ctx, int form);
int rt_frame_denoise_stats(rt_ctx* ctx, rt_frame_denoise_report* out);

/* ---- frame temporal: "carry last frame's result to this frame's pixels", an optional stage of the frame denoiser ----
 * Whenever the camera moves or the world updates the accumulator starts over, and the spatial filter above then has one sample
 * per pixel to work on.  With this stage on, the frame denoiser keeps, per pixel, a history colour with its length n, the first
 * two moments of its luminance and the guide of the frame the history was made from; between the prepare stage and the first
 * pass, one gather kernel (csrc/k_frame_temporal.hip.h) reprojects every surface pixel into the previous frame, tests what it
 * finds there against the previous guide and blends it with the current colour.  The passes and the finish are unchanged: they
 * read the integrated image where they read the prepare stage's colour image, the current guide and the current modulation.
 * The stage is OFF by default, and with it off every word the library produces is what it produced without the stage.
 *
 * THE FRAME TEMPORAL RULE.  All arithmetic is f32, unfused (no FMA contraction), in the order written, with rt_div / rt_floor /
 * rt_max / rt_abs of mi355rt_math.h.  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; cross(a, b) = (a.y * b.z - a.z * b.y,
 * a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); lum as in the frame denoise rule.  Inputs: an rt_frame_temporal_desc {flags,
 * max_history, var_history, normal_cos, plane_eps} (mi355rt_layout.h); of the CURRENT frame the outputs of the prepare stage,
 * colour texel col[p] = {c.rgb, vs} and guide {P, inst} {N, surface flag}; of the PREVIOUS frame - the last frame this stage
 * ran on - the history texel hist[q] = {q.rgb, n}, n a whole number stored as f32, the moments texel {m1, m2}, the guide {Pq,
 * instq} {Nq, flagq}, and of the uniform block k_frame_prepare was given for it the pinhole eye', ll', hor', ver' (origin,
 * lower_left, horizontal, vertical) and the jitter j'.  Per pixel p = (x, y), l = lum(c):
 *   background  (surface flag 0): the integrated texel is col[p] bit for bit, the history {c, 0}, the moments {0, 0}.
 *   no history  when none is kept (the first frame after a drop), when max_history == 1, or when `reproject` accepts no tap:
 *               the integrated texel is col[p] bit for bit, the history {c, 1}, the moments {l, l * l}.
 *   reproject   the world is taken as static, so the surface point was at P in the previous frame too.  e = P - eye'; c0 = ll'
 *               - eye'; nrm = cross(hor', ver'); s = rt_div(dot(c0, nrm), dot(e, nrm)); r = e * s - c0 (per component); u =
 *               rt_div(dot(r, hor'), dot(hor', hor')); v = rt_div(dot(r, ver'), dot(ver', ver')) - THE CAMERA'S hor AND ver ARE
 *               ORTHOGONAL (look-at cameras make them so), which is what makes these two quotients the plane coordinates; fx
 *               = (u * (float)W - 0.5f) - j'.x * (float)W; fy = ((1.0f - v) * (float)H - 0.5f) - j'.y * (float)H: the exact
 *               inverse of the u, v k_frame_prepare forms.  Required: s > 0 && fx >= -1 && fx < W && fy >= -1 && fy < H (a
 *               NaN fails each).  x0 = (int)rt_floor(fx), tx = fx - rt_floor(fx), y0 and ty likewise.  The taps are (x0, y0),
 *               (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) in that order, their weights w = (1.0f - tx) * (1.0f - ty), tx *
 *               (1.0f - ty), (1.0f - tx) * ty, tx * ty.  A tap is VISITED iff w > 0.
 *   accepted    a visited tap q iff all of these hold (a NaN fails each float comparison): q is inside the image; flagq != 0;
 *               n >= 1.0f; with RT_FRAME_TEMPORAL_SAME_INSTANCE, instq equals inst; dot(N, Nq) >= normal_cos; with d = Pq -
 *               P (per component), rt_abs(dot(N, d)) <= plane_eps.
 *   sums        wsum, acc[0 .. 2], s1, s2 start at +0; for every accepted tap in visiting order wsum = wsum + w; acc[c] =
 *               acc[c] + w * hist[q][c]; s1 = s1 + w * m1; s2 = s2 + w * m2.  n_prev is the n of the first accepted tap,
 *               replaced by a later accepted tap's n iff that is < n_prev: the least.  hq[c] = rt_div(acc[c], wsum); hm1 =
 *               rt_div(s1, wsum); hm2 = rt_div(s2, wsum).
 *   blend       n' = n_prev + 1.0f, replaced by (float)max_history unless n' < (float)max_history; a = rt_div(1.0f, n'); q'[c]
 *               = hq[c] + a * (c[c] - hq[c]); m1' = hm1 + a * (l - hm1); m2' = hm2 + a * (l * l - hm2); var' = n' >=
 *               (float)var_history ? rt_max(m2' - m1' * m1', 0.0f) : vs.  The integrated texel is {q', var'}, the history
 *               {q', n'}, the moments {m1', m2'}.
 * The history holds PRE-FILTER colour, in the filtered quantity of the prepare stage (radiance / albedo under DEMODULATE).
 * WHEN IT RUNS: exactly when the prepare stage runs - on a miss of its cache - never otherwise: one run of prepare is one
 * frame of history.  A second call on the same G-buffer reuses the integrated image and does not advance the history.  Colour,
 * moments and guide are double-buffered: the stage reads the previous set and writes the next, into which k_frame_prepare has
 * written its guide.
 * THE HISTORY IS DROPPED (the next frame is a first frame) by rt_set_frame_temporal, rt_reset_frame_history, rt_resize and a
 * change of the DEMODULATE bit between runs, since the stored quantity changes; the first two also drop the prepare stage's
 * cache, so the next call runs both stages.  It is NOT dropped by rt_set_scene, rt_world_update, the uploads or rt_reset_accum:
 * a moved camera and a rebuilt world are the cases it exists for.  A caller who swaps the whole scene calls
 * rt_reset_frame_history.
 * Refusals, RT_ERR_INVALID with messages that begin "frame temporal:", made before the context is looked at: an unknown flag
 * bit, a non-zero reserved word, max_history == 0 or > RT_FRAME_TEMPORAL_MAX_HISTORY (256), var_history == 0.  The float
 * parameters are not validated: a NaN rejects every tap.  The rank and stripe refusals of the frame denoiser apply as they
 * stand.
 * Motion of instances and skinned vertices is the optional "frame motion" below (RT_FRAME_TEMPORAL_MOTION); without that flag
 * a moved surface fails the plane test and restarts at n = 1, correct but noisy.
 * Not built: SVGF's 3 x 3 search when all four
 * taps fail; neighbourhood clamping of the history; feeding back the first pass's filtered colour; weighting by the
 * accumulator's sample count (with a growing accumulator the history averages successive means).
 *   rt_set_frame_temporal     desc != NULL: every later rt_denoise_frame, rt_denoise_frame_device and filtered present() runs
 *                             the stage; NULL (the default) restores the plain path exactly.  Any call drops the history.
 *   rt_reset_frame_history    drops the history.
 *   rt_read_frame_history     blocking, for tests and tools: the current history colour (W * H x 4 f32) and moments (W * H x 2
 *                             f32), either may be NULL; cap_pixels >= W * H.  frames_out (may be NULL): the frames integrated
 *                             since the last drop.  With both arrays NULL only that count is read.  RT_ERR_NOT_READY while
 *                             there is no history.
 * rt_frame_denoise_stats reports the stage in `temporal` (0 off, 1 ran, 2 its image was reused) and `temporal_ms`. */
int rt_set_frame_temporal(rt_ctx* ctx, const rt_frame_temporal_desc* desc_or_null);
int rt_reset_frame_history(rt_ctx* ctx);
int rt_read_frame_history(rt_ctx* ctx, float* colour_rgba32f, float* moments_rg32f, size_t cap_pixels, uint32_t* frames_out);

/* ---- frame motion: "follow the surface point, not the place", RT_FRAME_TEMPORAL_MOTION in rt_frame_temporal_desc.flags ----
 * The temporal rule takes the world as static.  In the loop it exists for - a world rebuilt every frame - that fails three
 * ways: a surface that leaves its plane restarts at n = 1 every frame; a surface that slides within its plane passes every
 * test and blends the history of another surface point; and SAME_INSTANCE compares TLAS positions, which every update
 * re-sorts.  With the flag set, one more kernel (csrc/k_frame_motion.hip.h) runs between the prepare stage and
 * k_frame_temporal: it finds where the pixel's own point of its own triangle was in the previous frame, from a snapshot of
 * that frame's vertex positions and instance transforms, and the temporal stage reprojects THAT point.  With the flag clear
 * every word the library produces is what it produced before the flag existed.
 *
 * THE FRAME MOTION RULE.  f32, unfused, in the order written, with rt_div / rt_normalize / rt_abs / rt_mat_mul_point of
 * mi355rt_math.h; dot and cross as in the temporal rule.  Inputs per surface pixel p (surface flag of its guide != 0): tri =
 * bits(normal_id[p].z), inst = bits(normal_id[p].w) of the G-buffer; P and N of this frame's guide; the scene arrays as they
 * are now: n_tris topology rows, n_verts positions, n_inst instance records in TLAS order; ids, n_inst words (below: IDENTITY);
 * the SNAPSHOT of the previous frame - the last frame this stage ran on - when one is kept: n_verts positions by vertex id, the
 * forward transforms of that frame's instances BY STABLE ID, and per pixel the stable id that frame recorded.
 *   ids         sid = ids[inst] when inst < n_inst and ids[inst] < n_inst, else RT_FRAME_MOTION_NO_ID (0xffffffff).  The id
 *               the frame records for the pixel is sid; for a background pixel NO_ID.
 *   untracked   the pixel is UNTRACKED when tri >= n_tris; or inst >= n_inst; or sid == NO_ID; or one of v0, v1, v2 - the first
 *               three words of topology row tri - is >= n_verts; or no snapshot is kept; or, below, !(den > 0) or a word of P'
 *               is not finite (its exponent field is all ones).  Every index is compared BEFORE the load it guards; a load
 *               that fails its guard is not made through that index.  An untracked pixel takes the temporal rule's
 *               no-history path.  Its carry is {P, UNTRACKED} {N, sid}.
 *   corners     M = the 16 words of transform of instance record inst; M' = the snapshot's transform of sid.  A =
 *               rt_mat_mul_point(M, pos[v0]), B of v1, C of v2 - what the kernels' world_triangle gives; A', B', C' the same
 *               of M' and the snapshot's positions of the same three vertex ids.
 *   unmoved     when the nine words of A, B, C equal those of A', B', C' bit for bit: P' = P, N' = N, status UNMOVED: the
 *               temporal rule then applies word for word.
 *   moved       else e1 = B - A, e2 = C - A, ep = P - A (per component); d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2,
 *               e2), dp1 = dot(ep, e1), dp2 = dot(ep, e2); den = d11 * d22 - d12 * d12; b1 = rt_div(d22 * dp1 - d12 * dp2, den);
 *               b2 = rt_div(d11 * dp2 - d12 * dp1, den) - the barycentrics of the foot of P in the triangle's plane, by the 2 x 2
 *               normal equations; e1' = B' - A', e2' = C' - A'; P'[c] = A'[c] + (b1 * e1'[c] + b2 * e2'[c]); N' =
 *               rt_normalize(cross(e1', e2')), every component negated when dot(cross(e1, e2), N) < 0; status MOVED.  A
 *               previous triangle of no area gives a NaN N', which fails every tap's normal test: no history.
 *   carry       per pixel 32 bytes, {P'.xyz, bits(status)} {N'.xyz, bits(sid)}; a background pixel: {0, 0, 0, BACKGROUND}
 *               {0, 0, 0, NO_ID}.  rt_read_frame_motion reads it; P' - P is the pixel's world-space motion vector.
 *   temporal    the temporal rule with these changes: an UNTRACKED pixel takes the no-history path; `reproject` starts from e
 *               = P' - eye'; `accepted` tests dot(N', Nq) >= normal_cos and, with d = Pq - P', rt_abs(dot(N', d)) <=
 *               plane_eps; with RT_FRAME_TEMPORAL_SAME_INSTANCE the tap's id AS THE PREVIOUS FRAME RECORDED IT must equal sid
 *               (the guides' TLAS positions are not compared).  Sums and blend are unchanged.
 * LIMITATION: the shading normal is not carried.  N' is the GEOMETRIC normal of the previous triangle, Nq the previous
 * frame's shading normal: on a smoothly shaded mesh normal_cos has to tolerate the angle between the two, up to half a facet
 * angle.  An UNMOVED pixel keeps its shading normal.
 * IDENTITY.  ids[p] is the stable id of the instance at TLAS position p.  rt_world_update supplies it on the device: the
 * declaration index of the instance its TLAS builder put at position p (RT_WORLD_INSTANCE_ORDER of rt_world_read).  On the
 * upload path ids is the identity mapping after every upload of RT_KIND_INSTANCE, until rt_set_frame_motion_ids declares the
 * ids of the instance array now uploaded: a permutation of 0 .. n - 1 with n the instance count, else RT_ERR_INVALID, "frame
 * motion: ...".
 * THE SNAPSHOT is taken on the context's stream right after the temporal stage has run, and only while the flag is set:
 * the vertex positions (16 B per vertex, a device copy), the transforms scattered by stable id (64 B per instance), the id
 * plane (4 B per pixel, double-buffered with the history).  The history is dropped, as by rt_reset_frame_history, when the
 * vertex count or the instance count differs from the snapshot's, and by every rt_set_frame_temporal.
 * THE SCENE MUST BE THE G-BUFFER'S.  The stage follows G-buffer indices into the scene arrays, so with the flag set a frame
 * denoise call is refused with RT_ERR_NOT_READY, "frame motion: the scene changed since the last compute()", when geometry,
 * topology, instances or BVH were uploaded, or rt_world_update ran, after the compute() that made the G-buffer.  A camera
 * change alone does not trigger it.  Frames traced ahead are dropped by everything that rewrites the scene.
 * rt_set_frame_temporal refuses the flag, "frame temporal: RT_FRAME_TEMPORAL_MOTION needs an uploaded scene ...", on a context
 * that has no triangles, vertices or instances yet (and without a context): set it after the first upload or world update.
 * Not built: carrying the shading normal; motion of the camera's lens; motion vectors for anything but the primary hit.
 *   rt_set_frame_motion_ids   see IDENTITY.  n must equal the instance count of the context.  Does not drop the history.
 *   rt_read_frame_motion      blocking, for tests and for callers who want motion vectors: the carry plane of the last run,
 *                             W * H x 8 f32; cap_pixels >= W * H.  RT_ERR_NOT_READY before the first run with the flag set.
 * rt_frame_denoise_stats reports the stage in `motion` (1: k_frame_motion ran in that call) and `motion_ms`. */
int rt_set_frame_motion_ids(rt_ctx* ctx, const uint32_t* ids, uint32_t n);
int rt_read_frame_motion(rt_ctx* ctx, float* carry_2xrgba32f, size_t cap_pixels);

/* ---- lightmaps: "the finished lightmap of these instances, in the texel format a renderer loads", in one call ----
 * The four sections above are the stages of a lightmap: points, gather, filter, gutter.  A caller who chains their host
 * entries pays a second point pass for the filter's guides and two more round trips of the atlas, and receives 16 bytes per
 * texel of f32 where a renderer loads half floats or a shared-exponent HDR image.  Here the stages run back to back on the
 * context's stream, from the entries to the encoded atlas without leaving HBM: one point pass, one host read of the point
 * count, one copy back of the encoded size (csrc/k_encode.hip.h is the one new kernel).
 *
 * THE LIGHTMAP RULE is an identity; there is no new arithmetic but the encoding.  Inputs: an rt_lightmap_desc d
 * (mi355rt_layout.h) - the five fields of rt_bake_atlas_desc; the gather's max_depth, spp, seed; the filter's passes, step,
 * normal_cos, plane_eps, max_dist; dilate_radius; format - the entries and optionally atlas_uv, as for an atlas bake.
 *   f32 atlas   word for word the composition, in this order, of (1) rt_bake_atlas_irradiance for {width, height, pad_base,
 *               t_max, n_entries}, the entries, atlas_uv, max_depth, spp and seed;  (2) unless passes == 0: rt_denoise_atlas of
 *               that atlas for {width, height, step, passes, normal_cos, plane_eps, max_dist}, with the points and texels that
 *               rt_bake_atlas_points gives for the same arguments;  (3) unless dilate_radius == 0: rt_dilate_atlas of the result
 *               for {width, height, dilate_radius}.
 *   counts      *n_covered_out = the bake's count n;  *n_filled_out = the dilation's count, 0 when dilate_radius == 0;  the
 *               stats are the gather's, and rt_irradiance_gather_stats reports this gather afterwards.  Each may be NULL.
 *   result      RT_LIGHTMAP_F32: that atlas.  Any other format: rt_encode_atlas of it.
 *   n == 0      (no entry covers a texel) is valid: every texel is {+0, +0, +0, -1.0f}, nothing is filled.
 *
 * THE ENCODING RULE.  Texel by texel {r, g, b, w}; every step is exact, and there is no division, no log and no exp.
 *   F32         the 16 bytes unchanged.
 *   F16         8 bytes: the four halves rt_f32_to_f16(r), (g), (b), (w) of mi355rt_math.h in this order (round to nearest
 *               even, overflow to infinity, NaN stays a NaN).  -1 and -2 are exact halves: coverage survives.
 *   RGBE8       4 bytes, the little-endian word R | G << 8 | B << 16 | E << 24: a Radiance .hdr pixel.  A texel with w ==
 *               -1.0f (no surface, not filled) is the word 0.  Otherwise each colour is sanitised, c' = (c > 0) ? min(c,
 *               0x1.fffffep+126f) : 0 as float comparisons, so that a NaN, a negative value and either zero give +0;  v = the
 *               largest c' and b = its biased exponent field (bits 23 .. 30);  b < 32 (v < 2^-95) is the word 0;  else E = b +
 *               2 and each byte is floor(c' * 2^(134 - b)) - the scale is a representable power of two for b = 32 .. 253, the
 *               product is exact and below 256, the largest channel lands in 128 .. 255, and a product that would be
 *               denormal floors to 0 whether or not it is flushed.  A decoder reads c = (byte + 0.5) * 2^(E - 136): every
 *               channel comes back within 2^(E - 137) of c'.  (1, 1, 1) is (128, 128, 128, 129), as in Radiance.
 *               rt_rgbe8 of mi355rt_math.h is this rule on the host and on the device.
 * Limits, all RT_ERR_INVALID and all raised before anything is enqueued, with messages that begin "lightmap:" (the encode
 * entries: "encode atlas:"): a NULL descriptor, reserved != 0, a format that is none of the three, passes > 3, and with passes
 * >= 1 a step of 0 or step << (passes - 1) > RT_DENOISE_MAX_STEP, dilate_radius > RT_DILATE_MAX_RADIUS, a NULL out, out_bytes
 * below width * height * {16, 8, 4}, a dev_out that is not a 16-byte-aligned array the context's device can reach, and
 * everything an atlas bake and an irradiance gather refuse for the same arguments (their message follows the prefix).
 * RT_ERR_NOT_READY as for a bake.  The encode entries: width or height == 0, width * height > 2^24, a NULL array.
 * A lightmap bake leaves the renderer as it was, like every bake.  It runs in the staging arrays of the stages it is made of
 * and three of its own (the filtered atlas, the filled count, the encoded atlas), kept and grown, all sized before the first
 * launch.
 *   rt_bake_atlas_lightmap         blocking; entries, atlas_uv and out are host arrays.  One host read of the count between
 *                                  the point pass and the gather, one copy of width * height * {16, 8, 4} bytes, one fence.
 *   rt_bake_atlas_lightmap_device  dev_atlas_uv (or NULL) and dev_out are device-accessible arrays; the entries stay a host
 *                                  array.  NOT enqueue-only: it still reads the count once, which fences the stream in the
 *                                  middle of the call; behind that read it only enqueues, unless n_filled_out or stats is
 *                                  asked for, which costs a second fence at the end.  An enqueue-only whole bake would need
 *                                  the gather to take its count from the device, and is not built.
 *   rt_encode_atlas                the encode stage alone, blocking, on host arrays: any atlas of 16-byte texels, such as one
 *                                  rt_dilate_atlas returned.  No scene is needed; out may not overlap atlas_in unless the
 *                                  format is RT_LIGHTMAP_F32 and they are equal.
 *   rt_encode_atlas_device         the same on device-accessible arrays (16-byte aligned, on the context's device); dev_out
 *                                  must not overlap dev_in.  Only enqueues on the context's stream. */
int rt_bake_atlas_lightmap(rt_ctx* ctx, const rt_lightmap_desc* desc, const rt_bake_rect* entries, const float* atlas_uv,
                           uint32_t n_uv_vertices, void* out, size_t out_bytes, uint32_t* n_covered_out, uint32_t* n_filled_out,
                           rt_radiance_stats* stats);
int rt_bake_atlas_lightmap_device(rt_ctx* ctx, const rt_lightmap_desc* desc, const rt_bake_rect* entries,
                                  const void* dev_atlas_uv, void* dev_out, size_t out_bytes, uint32_t* n_covered_out,
                                  uint32_t* n_filled_out, rt_radiance_stats* stats);
int rt_encode_atlas(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t format, const float* atlas_in, void* out,
                    size_t out_bytes);
int rt_encode_atlas_device(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t format, const void* dev_in, void* dev_out,
                           size_t out_bytes);

/* ---- directional lightmaps: "the four SH layers of these instances' lightmap", the atlas bake and the finished lightmap
 * around the directional gather ----
 * Both entries are identities, like their flat siblings; there is no new arithmetic.  The atlas has four LAYERS of W * H
 * texels of 16 bytes, layer-major: layer k holds {sh[k].r, sh[k].g, sh[k].b, hit_fraction}, an rt_irradiance in shape.
 *   rt_bake_atlas_directional           desc, entries, atlas_uv as for rt_bake_atlas_irradiance; blocking, on host arrays.
 *                                       The atlas point pass, one host read of the count, ONE directional gather on the
 *                                       points in HBM, one scatter (k_dir_scatter).  layers_out is 4 * W * H rt_irradiance:
 *                                       layers_out[k * W * H + texels[j]] is, bit for bit, rt_gather_directional(points[j])
 *                                       .layer[k], and every uncovered texel of every layer is {+0, +0, +0, -1.0f}.
 *                                       *n_covered_out (may be NULL) = n.  The stats (may be NULL) are the directional
 *                                       gather's, and rt_directional_gather_stats reports this gather afterwards.  Limits
 *                                       and messages are an atlas bake's and a directional gather's, behind the prefix "bake
 *                                       directional:".
 *   rt_bake_atlas_directional_lightmap  rt_lightmap_desc unchanged; blocking, host arrays.  For each layer k the encoded
 *                                       layer is word for word the composition of (1) layer k of rt_bake_atlas_directional;
 *                                       (2) unless passes == 0, rt_denoise_atlas of it with the points and texels of
 *                                       rt_bake_atlas_points - the filter's weights come from the guides alone, so filtering
 *                                       each layer is filtering the SH vector; (3) unless dilate_radius == 0, rt_dilate_atlas
 *                                       of the result; (4) rt_encode_atlas in `format`.  Layer k is written at out + k * W * H
 *                                       * texel bytes; out_bytes below four layers is RT_ERR_INVALID.  RT_LIGHTMAP_RGBE8 is
 *                                       RT_ERR_INVALID: band-1 coefficients are signed and the shared-exponent rule zeroes
 *                                       negatives.  *n_filled_out is layer 0's count; all four are equal, the fourth word
 *                                       being the same in every layer before and after the filter.  One point pass, one read
 *                                       of the count, one copy back; every atlas-sized array is sized before the first
 *                                       launch.  Messages begin with "directional lightmap:".
 * Not built: _device forms of the two bakes (chain rt_bake_atlas_points_device and rt_gather_directional_device), band 2,
 * tangent-space bases, an RGBE-style signed encoding. */
int rt_bake_atlas_directional(rt_ctx* ctx, const rt_bake_atlas_desc* desc, const rt_bake_rect* entries, const float* atlas_uv,
                              uint32_t n_uv_vertices, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_irradiance* layers_out,
                              uint32_t* n_covered_out, rt_radiance_stats* stats);
int rt_bake_atlas_directional_lightmap(rt_ctx* ctx, const rt_lightmap_desc* desc, const rt_bake_rect* entries,
                                       const float* atlas_uv, uint32_t n_uv_vertices, void* out, size_t out_bytes,
                                       uint32_t* n_covered_out, uint32_t* n_filled_out, rt_radiance_stats* stats);

/* ---- the sharded image: one picture rendered by `world` contexts ("ranks"), assembled on rank 0 ----
 * Rank k owns the image rows y with (y / stripe_rows) % world == k and traces only those (rt_set_stripes).  Its COMPACT
 * BLOCK holds the rows it owns in ascending y, width float4 each, padded with zero rows to max_rows = the largest share
 * over all ranks, so all blocks are rt_dist_block_bytes long: row j of block k is image row
 * ((j / stripe_rows) * world + k) * stripe_rows + j % stripe_rows when that is < height, a padding row otherwise.
 * A gather is pack (accumulator -> this rank's block), exchange (every block to rank 0) and unpack (rank 0: the world
 * blocks -> its display buffer, which rt_present then reads).  Pack, exchange and unpack are copies: the display buffer is
 * bit for bit the accumulation buffer one context would hold.  The gather is out of place - the accumulators are only
 * read - so a progressive render goes on after it (render, gather, render, gather ...).  The exchange is either RCCL on
 * the context's stream (rt_gather_stripes; needs a communicator) or the host's own: rt_dist_read_block on every rank,
 * any transport, rt_dist_write_block on rank 0 (ranks that share a GPU, ranks on other machines).
 * The context owns every buffer of it (send block; on rank 0 `world` receive blocks and the display buffer).  rt_resize
 * allocates them anew for the new size (display buffer and blocks zeroed) - nothing goes stale, nothing is re-bound.
 * While a context is a rank, rt_bind_accum and rt_bind_present_source are refused (the rank reads the context's own
 * accumulator and presents from its own display buffer) and so is an rt_set_stripes that says anything else than
 * rt_dist_init did. */

/* ncclGetUniqueId: rank 0 calls it and the host hands the 128 bytes to the other ranks (pipe, file, IPC message).
 * Loads librccl on first use (see rt_dist_init).  No context: on failure the message is rt_last_error(NULL). */
int rt_dist_unique_id(uint8_t out[128]);
/* Make the context rank `rank` of `world` (<= 65535) with stripes of `stripe_rows` rows: sets the stripes as
 * rt_set_stripes(stripe_rows, rank, world) would and allocates the buffers for the current size (none yet: at the first
 * rt_resize).  unique_id128 != NULL: also ncclCommInitRank on the context's device - collective, every rank of the id must
 * call it.  NULL: no communicator; the host moves the blocks.
 * RCCL is never linked: it is dlopen'ed here, in this order: MI355RT_RCCL=<path> when set; the librccl.so.1 that is already
 * mapped into the process (a process that has loaded PyTorch has PyTorch's copy, built against the HIP runtime it
 * shares with this library); the system's librccl.so.1.  A library that cannot be loaded or a failing ncclCommInitRank
 * is RT_ERR_RCCL with the file in use named in the message, and leaves the context a plain one.
 * RT_ERR_INVALID: rank >= world, world == 0 or > 65535, stripe_rows == 0, a context that is a rank already, or one with
 * an rt_bind_accum / rt_bind_present_source binding. */
int rt_dist_init(rt_ctx* ctx, uint32_t rank, uint32_t world, uint32_t stripe_rows, const uint8_t* unique_id128);
/* Back to a plain context that renders every row and presents its accumulator: frees the buffers and the communicator.
 * Fences the stream first.  rt_destroy does the same.  RT_OK on a context that is no rank. */
int rt_dist_shutdown(rt_ctx* ctx);
/* max_rows * width * 16 at the current size; 0 when the context is no rank or has no size yet. */
size_t rt_dist_block_bytes(const rt_ctx* ctx);
/* Enqueue: accumulator -> this rank's compact block (k_pack_stripes). */
int rt_pack_stripes(rt_ctx* ctx);
/* This rank's block as the last rt_pack_stripes left it -> host (blocking).  cap >= rt_dist_block_bytes. */
int rt_dist_read_block(rt_ctx* ctx, void* host_out, size_t cap);
/* Rank 0: host -> the receive block of rank `from_rank` (rank 0's own block included: it takes the same way as everyone
 * else's).  bytes must be rt_dist_block_bytes.  The source may be reused on return. */
int rt_dist_write_block(rt_ctx* ctx, uint32_t from_rank, const void* host_in, size_t bytes);
/* Rank 0, enqueue: the `world` receive blocks -> display buffer, one launch (k_unpack_stripes). */
int rt_unpack_stripes(rt_ctx* ctx);
/* pack -> every rank ncclSend's its block to rank 0, rank 0 ncclRecv's `world` blocks (one group) -> unpack on rank 0,
 * all enqueued on the context's stream (rt_set_stream respected) without host synchronisation.  Collective: every rank
 * calls it once per gather.  world == 1 still runs the send / receive pair.  Without a communicator: RT_ERR_INVALID (move the
 * blocks with rt_dist_read_block / rt_dist_write_block instead). */
int rt_gather_stripes(rt_ctx* ctx);
/* Rank 0: the display buffer (the assembled float4 image of the last unpack; zero before the first) -> host (blocking). */
int rt_read_display(rt_ctx* ctx, float* out_rgba32f, size_t cap_bytes);

#ifdef __cplusplus
}
#endif
#endif
