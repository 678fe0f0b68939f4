// kernels.hip.h — hand-written gfx950 kernels of the path-tracing hot path.
//
//   lds_sizes.h               per-wave LDS blocks and the LdsPlan / PairPlan records, shared with the host's launch_plan.h
//   k_common.hip.h            helpers, texture fetch, RNG
//   k_block_scan.hip.h        block_count / block_rank / block_scan_inclusive / array_scan_exclusive: the block-level count,
//                             rank and prefix sum of the build-path kernels, and k_scan_counts, their one-workgroup u32 scan
//   k_intersect.hip.h         rays, slab / triangle tests, per-lane stackless walk
//   k_shading.hip.h           surface frame, BSDFs, light sampling, counters
//   k_prepare_primary.hip.h   k_prepare_tris / _tri_shade / _instances / _lights / _world_tris (upload-time re-layout and
//                             per-triangle world records of one-leaf-TLAS scenes, device_scene.h) and
//                             k_primary_visibility: the hardware-raster G-buffer pass (Rasterizer.wgsl:81-173,
//                             RasterizerPass.ts:97-140) as one closest-hit cast per pixel
//   k_treelet.hip.h           upload-time re-layout of the node array: explicit successors, most-visited nodes first
//   k_pairs.hip.h             upload-time re-layout into CHILD-PAIR records (one 64-byte record per inner node)
//   k_traverse.hip.h          the wave-level TLAS / BLAS walk (node step + LDS triangle queue) of the persistent kernel
//   k_pairwalk.hip.h          per-ray state machine of the walk over pair records (plain C++: also run on the host by the tests)
//   k_pairtrav.hip.h          its wave-level side: quad-cooperative record fetch, LDS stack, batched entry, triangle flush
//   k_pathtrace.hip.h         Raytracer.wgsl `main` + ray_color (:607-819) as a per-path state machine (start_sample,
//                             shade_bounce, ...) and its drivers k_pathtrace (one pixel per lane), k_pathtrace_persistent
//   k_wavefront.hip.h         the same bounce as shade / trace stages over device queues (large scenes)
//   k_rayquery.hip.h          k_ray_query: the trace stage over a caller's flat ray array (rt_trace_rays)
//   k_radiance.hip.h          path_query_loop: the path state machine over a caller's flat item array, one persistent loop
//                             with a policy per kind, and k_radiance_query: the items are rays (rt_trace_radiance)
//   k_gather.hip.h            k_irradiance_gather: the same loop behind hemisphere directions drawn at a caller's surface
//                             points (rt_gather_irradiance)
//   k_probe.hip.h             k_probe_rays / k_probe_project: uniform-sphere rays per (probe, sample) in front of
//                             k_radiance_query and the SH9 projection behind it (rt_gather_probes)
//   k_directional.hip.h       k_dir_rays / k_dir_project: the same around k_radiance_query at surface points, directions on the
//                             hemisphere of the normal, bands 0 .. 1 (rt_gather_directional), and k_dir_scatter: the results
//                             into the four layers of an atlas (rt_bake_atlas_directional)
//   k_bake.hip.h              k_bake_owner / _count / _emit: the UV-space rasteriser that makes such points from the
//                             texels of an instance's atlas (rt_bake_points), and k_bake_scatter, the way back
//   k_dilate.hip.h            k_dilate_mask / _source / _apply: the nearest-texel gutter fill of a baked atlas on a coverage
//                             bitmap (rt_dilate_atlas)
//   k_denoise.hip.h           k_denoise_index / _pass: the edge-stopped a-trous filter of a baked atlas, guided by the bake's
//                             points, on LDS windows (rt_denoise_atlas)
//   k_frame_denoise.hip.h     k_frame_prepare / _pass_lds / _pass_direct / _finish: the edge-stopped a-trous filter of a FRAME,
//                             guided by the G-buffer of the last compute(), staged in LDS or read through L2 per spacing
//                             (rt_denoise_frame, rt_set_present_denoise)
//   k_frame_temporal.hip.h    k_frame_temporal: the temporal stage between k_frame_prepare and the first pass: last frame's
//                             history reprojected through last frame's camera, tested against last frame's guide and blended
//                             (rt_set_frame_temporal); k_frame_temporal_motion: the same body on the carry plane
//   k_frame_motion.hip.h      k_frame_motion / _scatter: where a pixel's own point of its own triangle was in the previous frame,
//                             from a snapshot of that frame's vertices and transforms (RT_FRAME_TEMPORAL_MOTION)
//   k_encode.hip.h            k_encode_atlas: a finished f32 atlas as half floats or shared-exponent RGBE8 words
//                             (rt_encode_atlas, the last stage of rt_bake_atlas_lightmap)
//   k_volume.hip.h            k_volume_probes / _finish / _sample / _layers: the probes of a grid, SH9 radiance into windowed
//                             irradiance coefficients, the trilinear sampler (eight lanes per point) and the export into
//                             seven texel layers (rt_bake_volume, rt_sample_volume, rt_encode_volume)
//   k_reflection.hip.h        k_reflection_rays / _texels: octahedral rays per (texel, sample) in front of k_radiance_query and
//                             the texel mean behind it; k_reflection_filter: the GGX-filtered chain of a map, one wave per
//                             output texel; k_reflection_copy (rt_capture_reflection, rt_filter_reflection, rt_bake_reflection)
//   k_volume_visibility.hip.h k_visibility_rays / _texels: octahedral rays per (texel, sample) in front of k_ray_query and the
//                             distance moments behind it; k_volume_sample_visible: the sampler with a Chebyshev weight per
//                             corner; k_visibility_tiles: bordered tiles (rt_bake_volume_visibility, rt_sample_volume_visible,
//                             rt_encode_volume_visibility)
//   k_texture_post.hip.h      k_resize_texture; k_postprocess = PostProcess.wgsl `main` (:103-176)
//   k_validate.hip.h          k_validate_scene: every index the kernels follow, checked once per upload
//   k_stripes.hip.h           k_pack_stripes / k_unpack_stripes: the copies of the sharded image's gather
//
// (k_reflection_sample.hip.h, the reflection sampler of rt_sample_reflection, is not of this set: it needs nothing of it and
// is the translation unit reflection_sample.hip.)
//
// All arithmetic is unfused IEEE f32 (-ffp-contract=off) with the builtin semantics of
// include/mi355rt_math.h, in the evaluation order of the WGSL source, so that every path
// takes the same branches as the CPU oracle and results agree bit for bit.
#ifndef MI355RT_KERNELS_HIP_H
#define MI355RT_KERNELS_HIP_H

#include "device_scene.h"
#include "lds_sizes.h"   // per-wave LDS blocks and the plan records, shared with the host's launch planner (launch_plan.h)

#define RT_T_MIN 0.001f
#define RT_T_MAX 1e30f
#define RT_COUNTER_SHARDS 1024

#include "k_common.hip.h"
#include "k_block_scan.hip.h"
#include "k_intersect.hip.h"
#include "k_shading.hip.h"
#include "k_prepare_primary.hip.h"
#include "k_treelet.hip.h"
#include "k_pairwalk.hip.h"
#include "k_pairs.hip.h"
#include "k_traverse.hip.h"
#include "k_pairtrav.hip.h"
#include "k_pathtrace.hip.h"
#include "k_radiance.hip.h"
#include "k_gather.hip.h"
#include "k_probe.hip.h"
#include "k_directional.hip.h"
#include "k_bake.hip.h"
#include "k_dilate.hip.h"
#include "k_denoise.hip.h"
#include "k_frame_denoise.hip.h"
#include "k_frame_temporal.hip.h"
#include "k_frame_motion.hip.h"
#include "k_encode.hip.h"
#include "k_volume.hip.h"
#include "k_reflection.hip.h"
#include "k_volume_visibility.hip.h"
#include "k_wavefront.hip.h"
#include "k_rayquery.hip.h"
#include "k_texture_post.hip.h"
#include "k_validate.hip.h"
#include "k_stripes.hip.h"

#endif
