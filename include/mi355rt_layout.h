/* mi355rt_layout.h — byte-exact layouts of the buffers that cross the drop-in
 * boundary.  Produced by the scene compiler
 * (rust-shader-tools/src/rebuilder.rs, bvh/blas.rs, bvh/tlas.rs, lib.rs in the reference),
 * consumed unchanged by the renderer.  Little-endian f32/u32 throughout.
 */
#ifndef MI355RT_LAYOUT_H
#define MI355RT_LAYOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Raytracer.wgsl:40-49 `MeshTopology`; rebuilder.rs:140-161. 80 bytes. */
typedef struct rt_topology {
  uint32_t v0, v1, v2; /* global vertex ids */
  uint32_t pad;        /* = geometry index (rebuilder.rs:155) */
  float data0[4];      /* base colour rgb, material type as float */
  float data1[4];      /* metallic, roughness, ior, 0 */
  float data2[4];      /* baseTex, metRoughTex, normalTex, emissiveTex (-1 = none) */
  float data3[4];      /* emissive rgb, occlusionTex */
} rt_topology;

/* Raytracer.wgsl:56-59 `BVHNode`; bvh/mod.rs:9-16. 32 bytes.
 * data == 0: internal (first child = curr+1); else leaf: first = data>>3, count = data&7.
 * skip: TLAS absolute, BLAS relative to the BLAS root. */
typedef struct rt_node {
  float min_b[3];
  uint32_t skip;
  float max_b[3];
  uint32_t data;
} rt_node;

/* Raytracer.wgsl:61-74 `Instance`; bvh/mod.rs:18-27. 144 bytes. */
typedef struct rt_instance {
  float transform[16]; /* column-major */
  float inverse[16];   /* column-major */
  uint32_t blas_node_offset; /* node units, relative to blas_base_idx */
  uint32_t attr_offset;
  uint32_t instance_id; /* geometry index */
  uint32_t pad;
} rt_instance;

/* Raytracer.wgsl:51-54 `LightRef`. 8 bytes. */
typedef struct rt_light_ref {
  uint32_t inst_idx;
  uint32_t tri_idx;
} rt_light_ref;

/* Raytracer.wgsl:16-38 `SceneUniforms`; ResourceManager.ts:63-67,374-403.
 * 240 bytes used of a 256-byte buffer. */
typedef struct rt_camera {
  float origin[4]; /* w = lens_radius */
  float lower_left[4];
  float horizontal[4];
  float vertical[4];
  float u[4];
  float v[4];
} rt_camera;

typedef struct rt_scene_uniforms {
  rt_camera camera;      /* @0   */
  rt_camera prev_camera; /* @96  */
  uint32_t frame_count;  /* @192 */
  uint32_t blas_base_idx;
  uint32_t vertex_count;
  uint32_t rand_seed; /* uploaded, never read by any shader */
  uint32_t light_count;
  uint32_t width;
  uint32_t height;
  uint32_t pad;
  float jitter[2];
  float average_jitter[2]; /* @232, ends @240 */
  uint32_t tail_pad[4];    /* buffer is 256 bytes (ResourceManager.ts:65) */
} rt_scene_uniforms;


/* ---- device-resident World::update(t): what the scene compiler hands the renderer so that the
 * per-frame half of World::update (lib.rs:149-270) runs on the GPU and the bridge arrays never leave HBM.
 *
 * STATIC part (changes only when `static_epoch` does: scene load / animation file load): per geometry the skinning
 * input of rebuilder.rs:36-91 (base positions / normals / uvs, joints, weights), its index list and its per-triangle
 * attribute rows (geometry.rs:6-25), and the instance list of lib.rs:194-230 in DECLARATION order with the transforms
 * the update would leave in place.  PER-FRAME part: the joint matrices global(joint) * inverse_bind of every skin
 * (rebuilder.rs:40-47) after the animation was sampled at t and the scene graph re-evaluated (lib.rs:149-184) - a few
 * hundred bytes.  Everything else of update(t) - skinning, BLAS build (bvh/blas.rs), topology / light / draw-command
 * packing (rebuilder.rs:121-168, lib.rs:237-270), TLAS (bvh/tlas.rs:58-111), instance packing - is derived from these
 * on the device by rt_world_update (include/mi355rt.h). */
typedef struct rt_world_geometry {
  const float* positions;     /* 3 f32 per vertex (base pose) */
  const float* normals;       /* 3 f32 per vertex */
  const float* uvs;           /* 2 f32 per vertex, n_uvs of them (vertices beyond get 0, 0) */
  const uint32_t* joints;     /* 4 per vertex */
  const float* weights;       /* 4 per vertex */
  const uint32_t* indices;    /* 3 per triangle, geometry-local vertex ids */
  const float* attributes;    /* 16 f32 per triangle (the 64 bytes after rt_topology.pad) */
  uint32_t n_verts, n_uvs, n_tris;
  int32_t skin;               /* index into the frame's skins, -1 = not skinned */
} rt_world_geometry;

typedef struct rt_world_frame {
  uint64_t static_epoch;               /* the static part below is unchanged while this is */
  uint32_t n_geometries, n_instances, n_skins, pad;
  const rt_world_geometry* geometries; /* n_geometries */
  const rt_instance* instances;        /* n_instances, declaration order; blas_node_offset is filled in on the device */
  const uint32_t* skin_first;          /* n_skins + 1: first joint matrix of each skin in joint_mats */
  const float* joint_mats;             /* 16 f32 each (column-major), this frame */
} rt_world_frame;

/* ---- ray queries (rt_trace_rays, mi355rt.h) ---- */
typedef struct rt_ray {       /* 32 B: the trace kernels' own queue record {o, t_max} {d, -} */
  float origin[3];
  float t_max;
  float dir[3];               /* need not be normalised */
  uint32_t pad;
} rt_ray;
typedef struct rt_ray_hit {   /* 16 B */
  float t;
  int32_t tri;                /* global triangle index (the topology array's, rt_read_gbuffer's), -1 = none */
  int32_t inst;               /* TLAS-order instance index, -1 = none */
  uint32_t hit;
} rt_ray_hit;
typedef struct rt_ray_stats { /* of ONE call */
  uint64_t rays, nodes_visited, tris_tested; /* the last two only from the counting kernel, else 0 */
  uint32_t walk;              /* 0 node, 1 pairs */
  uint32_t lds;               /* every traversal record staged in LDS */
  uint32_t rayreg;            /* node walk, mixed mode: RAYREG form */
  uint32_t workgroups;        /* launched */
  double kernel_ms;           /* device events around the launch while rt_set_kernel_timing is on, else 0 */
} rt_ray_stats;

/* ---- radiance queries (rt_trace_radiance, mi355rt.h) ---- */
typedef struct rt_radiance {  /* 16 B: one vector store of k_radiance_query */
  float rgb[3];               /* sum of the samples' ray_color (Raytracer.wgsl:607-783) / spp, as `main` averages (:811) */
  float t;                    /* the first segment's hit distance; a miss: the ray's t_max, bits unchanged */
} rt_radiance;
typedef struct rt_radiance_stats { /* 72 B, of ONE call */
  uint64_t rays, samples;     /* n and n * spp */
  uint64_t extension_rays, shadow_rays; /* the rt_counters of the same names; a ray's first segment is ONE extension ray */
  uint64_t shaded_hits, nodes_visited, tris_tested; /* only from the counting kernel, else 0 */
  uint32_t lds;               /* the whole scene staged in LDS (the persistent kernel's LDS form) */
  uint32_t workgroups;        /* launched */
  double kernel_ms;           /* device events around the launch while rt_set_kernel_timing is on, else 0 */
} rt_radiance_stats;

/* ---- irradiance gathers (rt_gather_irradiance, mi355rt.h); their stats are an rt_radiance_stats with rays = points ---- */
typedef struct rt_gather_point { /* 32 B: the slots of rt_ray {position, t_max} {normal, pad} */
  float position[3];
  float t_max;                /* of every sample's first segment */
  float normal[3];            /* need not be normalised; not validated */
  uint32_t pad;               /* the point's RNG stream id; keep it below 2^31 */
} rt_gather_point;
typedef struct rt_irradiance { /* 16 B: one vector store of k_irradiance_gather */
  float rgb[3];               /* cosine-weighted mean incoming radiance = E / pi: sum of the samples / spp */
  float hit_fraction;         /* samples whose first segment hit something / spp */
} rt_irradiance;

/* ---- probe gathers (rt_gather_probes, mi355rt.h); their stats are an rt_radiance_stats with rays = probes ---- */
typedef struct rt_probe {     /* 32 B: the slots of rt_ray {position, t_max} {unused, pad} */
  float position[3];
  float t_max;                /* of every sample's first segment */
  float unused[3];            /* not read; write 0 */
  uint32_t pad;               /* the probe's RNG stream id; keep it below 2^31 */
} rt_probe;
typedef struct rt_probe_sh9 { /* 112 B: seven 16-byte vector stores of k_probe_project */
  float sh[9][3];             /* coefficient-major, rgb inside: the estimate of the integral of L(w) Y_k(w) over the sphere */
  float hit_fraction;         /* samples whose first segment hit something / spp */
} rt_probe_sh9;

/* ---- irradiance volumes (rt_bake_volume / rt_sample_volume, mi355rt.h): an axis-aligned grid of nx * ny * nz probes.  The volume
 * itself is n = nx * ny * nz records of rt_probe_sh9, probe-major, probe (x, y, z) at p = (z * ny + y) * nx + x; a sample goes
 * in as an rt_gather_point (t_max and pad not read) and comes out as an rt_irradiance ---- */
typedef struct rt_volume_desc { /* 64 B */
  float origin[3];            /* position of probe (0, 0, 0) */
  uint32_t nx;                /* each dimension 1 .. 1024, nx * ny * nz <= 2^24 */
  float step[3];              /* axis-aligned spacing, finite and > 0 */
  uint32_t ny;
  float window[3];            /* per-band scale (bands 0, 1, 2), finite and >= 0; {1, 1, 1} = none */
  uint32_t nz;
  float t_max;                /* of every probe */
  uint32_t pad_first;         /* probe p gets pad = pad_first + p; pad_first + n <= 2^31 */
  float max_hit_fraction;     /* sampler only: a probe is valid iff hit_fraction <= this; a NaN hit_fraction is invalid */
  uint32_t reserved;          /* 0 */
} rt_volume_desc;

/* ---- probe visibility maps (rt_bake_volume_visibility / rt_sample_volume_visible / rt_encode_volume_visibility, mi355rt.h): a
 * visibility volume is n = nx * ny * nz maps, probe-major in the order of the volume itself; a map is size * size texels of 8
 * bytes {mean distance, mean squared distance} in octahedral layout, texel (i, j) at j * size + i; the stats of a bake are an
 * rt_ray_stats ---- */
#define RT_VOLUME_VIS_BACKFACE 1u /* flags: weight a probe down that lies behind the surface the normal belongs to */
typedef struct rt_volume_visibility_desc { /* 32 B */
  uint32_t size;              /* side of a probe's map, in texels: a power of two, 4 .. 32 */
  uint32_t spt;               /* bake: samples per texel, 1 .. 65536 */
  float max_distance;         /* finite and > 0: the t_max of every visibility ray and the clamp of every distance */
  float normal_bias;          /* finite and >= 0: the sampled point moves this far along its normal before it looks at a probe */
  float min_visibility;       /* in [0, 1]: the floor of the Chebyshev weight */
  float crush_threshold;      /* in [0, 1]: weights below it are cubed and divided by its square; 0 = no crush */
  uint32_t flags;             /* RT_VOLUME_VIS_BACKFACE; every other bit is refused */
  uint32_t reserved;          /* 0 */
} rt_volume_visibility_desc;

/* ---- reflection probes (rt_capture_reflection / rt_filter_reflection / rt_bake_reflection, mi355rt.h): rt_probe in; a map is
 * size * size texels of 16 bytes {r, g, b, hit_fraction} in octahedral layout, texel (i, j) at j * size + i; a chain is the
 * levels 0 .. levels - 1 of one probe, level m of side size >> m, concatenated in level order; their stats are an
 * rt_radiance_stats ---- */
typedef struct rt_reflection_desc { /* 32 B */
  uint32_t size;              /* side of level 0, in texels: a power of two, 8 .. 512 */
  uint32_t levels;            /* of a chain: >= 2, size >> (levels - 1) >= 4; level m has the roughness m / (levels - 1) */
  uint32_t spt;               /* capture and bake: samples per texel, 1 .. 65536 */
  uint32_t filter_samples;    /* filter and bake: lobe samples per output texel, a multiple of 64 in 64 .. 4096 */
  uint32_t reserved[4];       /* 0 */
} rt_reflection_desc;

/* ---- the reflection sampler (rt_sample_reflection, mi355rt.h "THE REFLECTION SAMPLE RULE"): chains as a bake lays them out
 * in, one 16-byte texel {r, g, b, hit_fraction} per query out ---- */
#define RT_REFLECTION_SAMPLE_PARALLAX 1u /* flags: correct the direction by the probe's box; every other bit is refused */
typedef struct rt_reflection_sample_desc { /* 32 B */
  uint32_t size;              /* side of level 0 of the chains: a power of two, 8 .. 512 */
  uint32_t levels;            /* of a chain: >= 2, size >> (levels - 1) >= 4 */
  uint32_t flags;             /* RT_REFLECTION_SAMPLE_PARALLAX */
  uint32_t reserved[5];       /* 0 */
} rt_reflection_sample_desc;
typedef struct rt_reflection_query { /* 32 B: the slots of rt_ray {position, probe} {direction, roughness} */
  float position[3];          /* of the shaded point; read only with RT_REFLECTION_SAMPLE_PARALLAX */
  uint32_t probe;             /* index of the chain; >= n_probes gives four +0 */
  float direction[3];         /* the reflected direction; need not be normalised */
  float roughness;            /* 0 .. 1 picks the level roughness * (levels - 1); clamped, a NaN is 0 */
} rt_reflection_query;
typedef struct rt_reflection_box { /* 32 B: the proxy volume of one probe, axis-aligned */
  float lo[3];
  float unused0;              /* not read; write 0 */
  float hi[3];
  float unused1;              /* not read; write 0 */
} rt_reflection_box;

/* ---- directional gathers (rt_gather_directional, mi355rt.h): rt_gather_point in; their stats are an rt_radiance_stats ---- */
typedef struct rt_directional {   /* 64 B: four 16-byte vector stores of k_dir_project */
  float layer[4][4];              /* layer[k] = {sh[k].r, sh[k].g, sh[k].b, hit_fraction}: row k is the texel of atlas layer k */
} rt_directional;

/* ---- lightmap bakes (rt_bake_points, mi355rt.h): which atlas of which instance ---- */
typedef struct rt_bake_desc { /* 32 B */
  uint32_t inst;              /* TLAS-order instance index */
  uint32_t width, height;     /* of the atlas, in texels: both >= 1, width * height <= 2^24 */
  uint32_t pad_base;          /* pad of a point = pad_base + texel index; pad_base + width * height <= 2^31 */
  float t_max;                /* of every point */
  uint32_t reserved[3];       /* 0 */
} rt_bake_desc;
/* ---- atlas bakes (rt_bake_atlas_points, mi355rt.h): one atlas, a list of (instance, rectangle) entries ---- */
typedef struct rt_bake_atlas_desc { /* 32 B */
  uint32_t width, height;     /* of the atlas, in texels: both >= 1, width * height <= 2^24 */
  uint32_t pad_base;          /* pad of a point = pad_base + atlas texel index; pad_base + width * height <= 2^31 */
  float t_max;                /* of every point */
  uint32_t n_entries;         /* 1 .. 65536 */
  uint32_t reserved[3];       /* 0 */
} rt_bake_atlas_desc;
typedef struct rt_bake_rect { /* 32 B: two 16-byte loads of k_atlas_owner / k_atlas_emit */
  uint32_t inst;              /* TLAS-order instance index */
  uint32_t x, y;              /* the rectangle's first texel in the atlas */
  uint32_t width, height;     /* of the rectangle = of the entry's local bake: both >= 1, inside the atlas */
  uint32_t reserved[3];       /* 0 */
} rt_bake_rect;

/* ---- atlas dilation (rt_dilate_atlas, mi355rt.h): the gutter fill of a baked atlas ---- */
#define RT_DILATE_MAX_RADIUS 24u
typedef struct rt_dilate_desc { /* 32 B */
  uint32_t width, height;     /* of the atlas, in texels: both >= 1, width * height <= 2^24 */
  uint32_t radius;            /* of the gutter, in texels: 0 .. RT_DILATE_MAX_RADIUS; 0 fills nothing */
  uint32_t reserved[5];       /* 0 */
} rt_dilate_desc;

/* ---- atlas denoise (rt_denoise_atlas, mi355rt.h): the edge-stopped a-trous filter of a baked atlas ---- */
#define RT_DENOISE_MAX_STEP 4u
typedef struct rt_denoise_desc { /* 32 B */
  uint32_t width, height;     /* of the atlas, in texels: both >= 1, width * height <= 2^24 */
  uint32_t step;              /* tap spacing of the first pass, in texels: >= 1 */
  uint32_t passes;            /* pass p has the spacing step << p: >= 1, step << (passes - 1) <= RT_DENOISE_MAX_STEP */
  float normal_cos;           /* a tap's normal must have at least this dot product with the centre's */
  float plane_eps;            /* a tap's position lies at most this far from the centre's tangent plane */
  float max_dist;             /* ... and at most this far from the centre's position */
  uint32_t reserved[1];       /* 0 */
} rt_denoise_desc;

/* ---- frame denoise (rt_denoise_frame, mi355rt.h): the G-buffer-guided a-trous filter of a frame ---- */
#define RT_FRAME_DENOISE_MAX_STEP 16u
#define RT_FRAME_DENOISE_MAX_PASSES 5u
#define RT_FRAME_DENOISE_DEMODULATE 1u    /* filter radiance / albedo, multiply the albedo back after the last pass */
#define RT_FRAME_DENOISE_SAME_INSTANCE 2u /* a tap must lie on the centre's instance */
#define RT_FRAME_DENOISE_MIN_ALBEDO 0.00392156886f /* f32(1 / 255): the least albedo component a radiance is divided by */
typedef struct rt_frame_denoise_desc { /* 32 B */
  uint32_t passes;            /* 1 .. 5; pass p has the spacing step << p */
  uint32_t step;              /* tap spacing of the first pass, in pixels: >= 1, step << (passes - 1) <= RT_FRAME_DENOISE_MAX_STEP */
  uint32_t flags;             /* RT_FRAME_DENOISE_*; any other bit is refused */
  float normal_cos;           /* a tap's normal must have at least this dot product with the centre's */
  float plane_eps;            /* a tap's position lies at most this far from the centre's tangent plane */
  float sigma_lum;            /* luminance stop in standard deviations; <= 0: none, no exponential is evaluated */
  uint32_t reserved[2];       /* 0 */
} rt_frame_denoise_desc;
/* what rt_frame_denoise_stats reports: stream times (ms, device events) of the last rt_denoise_frame* call or filtered present() */
typedef struct rt_frame_denoise_report { /* 48 B */
  float prepare_ms;           /* k_frame_prepare; 0 when the cache was hit */
  float pass_ms[5];           /* per pass; 0 beyond `passes` */
  float finish_ms;            /* k_frame_finish */
  uint32_t passes;
  uint8_t form[5];            /* per pass: 1 = LDS form, 2 = direct form; 0 beyond `passes` */
  uint8_t cache_hit;          /* 1: the prepare stage's outputs were those of an earlier call on the same G-buffer */
  uint8_t temporal;           /* the temporal stage (rt_set_frame_temporal): 0 = off, 1 = ran, 2 = its integrated image was reused */
  uint8_t motion;             /* the motion stage (RT_FRAME_TEMPORAL_MOTION): 1 = k_frame_motion ran in this call, else 0 */
  float temporal_ms;          /* k_frame_temporal; 0 when the stage is off or its image was reused */
  float motion_ms;            /* k_frame_motion; 0 unless `motion` is 1 */
} rt_frame_denoise_report;

/* ---- frame temporal (rt_set_frame_temporal, mi355rt.h): reprojection of last frame's history ahead of the a-trous passes ---- */
#define RT_FRAME_TEMPORAL_MAX_HISTORY 256u
#define RT_FRAME_TEMPORAL_SAME_INSTANCE 1u /* a history tap must lie on the pixel's instance */
#define RT_FRAME_TEMPORAL_MOTION 2u        /* carry every surface pixel back along its own triangle's motion before it is reprojected */
/* the status word of a carry texel (rt_read_frame_motion) and the id of a pixel that has none */
#define RT_FRAME_MOTION_BACKGROUND 0u
#define RT_FRAME_MOTION_UNTRACKED 1u
#define RT_FRAME_MOTION_UNMOVED 2u
#define RT_FRAME_MOTION_MOVED 3u
#define RT_FRAME_MOTION_NO_ID 0xffffffffu
typedef struct rt_frame_temporal_desc { /* 32 B */
  uint32_t flags;             /* RT_FRAME_TEMPORAL_*; any other bit is refused */
  uint32_t max_history;       /* 1 .. RT_FRAME_TEMPORAL_MAX_HISTORY: the blend factor never falls below 1 / max_history; 1 keeps none */
  uint32_t var_history;       /* >= 1: from this many frames of history on, the variance is the temporal one */
  float normal_cos;           /* a history tap's normal must have at least this dot product with the pixel's */
  float plane_eps;            /* a history tap's position lies at most this far from the pixel's tangent plane */
  uint32_t reserved[3];       /* 0 */
} rt_frame_temporal_desc;

/* ---- lightmaps (rt_bake_atlas_lightmap, mi355rt.h): an atlas bake, its filter, its gutter fill and its texel format ---- */
#define RT_LIGHTMAP_F32 0u    /* 16 B per texel: {r, g, b, w} as the bakes return it */
#define RT_LIGHTMAP_F16 1u    /* 8 B per texel: four halves, w included */
#define RT_LIGHTMAP_RGBE8 2u  /* 4 B per texel: R | G << 8 | B << 16 | E << 24, a Radiance .hdr pixel */
typedef struct rt_lightmap_desc { /* 64 B */
  uint32_t width, height;     /* the five fields of rt_bake_atlas_desc, with their limits */
  uint32_t pad_base;
  float t_max;
  uint32_t n_entries;
  uint32_t max_depth, spp, seed; /* of the gather, as in rt_gather_irradiance */
  uint32_t passes;            /* of the filter: 0 = no filter (the next four fields are then not read), at most 3 */
  uint32_t step;              /* as in rt_denoise_desc: >= 1, step << (passes - 1) <= RT_DENOISE_MAX_STEP */
  float normal_cos;           /* as in rt_denoise_desc */
  float plane_eps;
  float max_dist;
  uint32_t dilate_radius;     /* of the gutter fill: 0 = none, at most RT_DILATE_MAX_RADIUS */
  uint32_t format;            /* RT_LIGHTMAP_* */
  uint32_t reserved[1];       /* 0 */
} rt_lightmap_desc;

#ifdef __cplusplus
}
static_assert(sizeof(rt_lightmap_desc) == 64, "rt_lightmap_desc is 64 bytes");
static_assert(__builtin_offsetof(rt_lightmap_desc, passes) == 32 && __builtin_offsetof(rt_lightmap_desc, format) == 56,
              "rt_lightmap_desc: the filter starts at 32, the format is at 56");
static_assert(sizeof(rt_volume_desc) == 64, "rt_volume_desc is 64 bytes");
static_assert(__builtin_offsetof(rt_volume_desc, step) == 16 && __builtin_offsetof(rt_volume_desc, window) == 32 &&
                  __builtin_offsetof(rt_volume_desc, t_max) == 48 && __builtin_offsetof(rt_volume_desc, max_hit_fraction) == 56,
              "rt_volume_desc: four 16-byte rows, a dimension closing each of the first three");
static_assert(sizeof(rt_volume_visibility_desc) == 32, "rt_volume_visibility_desc is 32 bytes");
static_assert(__builtin_offsetof(rt_volume_visibility_desc, max_distance) == 8 &&
                  __builtin_offsetof(rt_volume_visibility_desc, min_visibility) == 16 &&
                  __builtin_offsetof(rt_volume_visibility_desc, flags) == 24,
              "rt_volume_visibility_desc: two 16-byte rows, size and spt opening the first, flags and reserved closing the second");
static_assert(sizeof(rt_reflection_desc) == 32, "rt_reflection_desc is 32 bytes");
static_assert(__builtin_offsetof(rt_reflection_desc, size) == 0 && __builtin_offsetof(rt_reflection_desc, levels) == 4 &&
                  __builtin_offsetof(rt_reflection_desc, spt) == 8 && __builtin_offsetof(rt_reflection_desc, filter_samples) == 12 &&
                  __builtin_offsetof(rt_reflection_desc, reserved) == 16,
              "rt_reflection_desc: four words, then four reserved ones");
static_assert(sizeof(rt_reflection_sample_desc) == 32, "rt_reflection_sample_desc is 32 bytes");
static_assert(__builtin_offsetof(rt_reflection_sample_desc, size) == 0 && __builtin_offsetof(rt_reflection_sample_desc, levels) == 4 &&
                  __builtin_offsetof(rt_reflection_sample_desc, flags) == 8 &&
                  __builtin_offsetof(rt_reflection_sample_desc, reserved) == 12,
              "rt_reflection_sample_desc: three words, then five reserved ones");
static_assert(sizeof(rt_reflection_query) == 32, "rt_reflection_query is 32 bytes");
static_assert(__builtin_offsetof(rt_reflection_query, probe) == 12 && __builtin_offsetof(rt_reflection_query, direction) == 16 &&
                  __builtin_offsetof(rt_reflection_query, roughness) == 28,
              "rt_reflection_query has the slots of rt_ray");
static_assert(sizeof(rt_reflection_box) == 32, "rt_reflection_box is 32 bytes");
static_assert(__builtin_offsetof(rt_reflection_box, lo) == 0 && __builtin_offsetof(rt_reflection_box, hi) == 16,
              "rt_reflection_box: lo in the first 16 bytes, hi in the second");
static_assert(sizeof(rt_denoise_desc) == 32, "rt_denoise_desc is 32 bytes");
static_assert(sizeof(rt_frame_denoise_desc) == 32, "rt_frame_denoise_desc is 32 bytes");
static_assert(sizeof(rt_frame_denoise_report) == 48, "rt_frame_denoise_report is 48 bytes");
static_assert(__builtin_offsetof(rt_frame_denoise_report, temporal) == 38 && __builtin_offsetof(rt_frame_denoise_report, temporal_ms) == 40,
              "rt_frame_denoise_report: the temporal stage took the first pad byte and the first reserved word");
static_assert(__builtin_offsetof(rt_frame_denoise_report, motion) == 39 && __builtin_offsetof(rt_frame_denoise_report, motion_ms) == 44,
              "rt_frame_denoise_report: the motion stage took the last pad byte and the last reserved word");
static_assert(sizeof(rt_frame_temporal_desc) == 32, "rt_frame_temporal_desc is 32 bytes");
static_assert(__builtin_offsetof(rt_frame_temporal_desc, normal_cos) == 12 && __builtin_offsetof(rt_frame_temporal_desc, reserved) == 20,
              "rt_frame_temporal_desc: three words, two floats, three reserved words");
static_assert(sizeof(rt_dilate_desc) == 32, "rt_dilate_desc is 32 bytes");
static_assert(sizeof(rt_bake_desc) == 32, "rt_bake_desc is 32 bytes");
static_assert(sizeof(rt_bake_atlas_desc) == 32, "rt_bake_atlas_desc is 32 bytes");
static_assert(sizeof(rt_bake_rect) == 32, "rt_bake_rect is 32 bytes");
static_assert(sizeof(rt_probe) == 32, "rt_probe is 32 bytes");
static_assert(__builtin_offsetof(rt_probe, t_max) == 12 && __builtin_offsetof(rt_probe, unused) == 16 &&
                  __builtin_offsetof(rt_probe, pad) == 28,
              "rt_probe has the slots of rt_ray");
static_assert(sizeof(rt_probe_sh9) == 112, "rt_probe_sh9 is 112 bytes");
static_assert(__builtin_offsetof(rt_probe_sh9, hit_fraction) == 108, "hit_fraction is the twenty-eighth word");
static_assert(sizeof(rt_directional) == 64, "rt_directional is 64 bytes");
static_assert(__builtin_offsetof(rt_directional, layer[1]) == 16 && __builtin_offsetof(rt_directional, layer[3][3]) == 60,
              "rt_directional: a row is a 16-byte texel, the hit fraction its fourth word");
static_assert(sizeof(rt_gather_point) == 32, "rt_gather_point is 32 bytes");
static_assert(__builtin_offsetof(rt_gather_point, t_max) == 12 && __builtin_offsetof(rt_gather_point, normal) == 16 &&
                  __builtin_offsetof(rt_gather_point, pad) == 28,
              "rt_gather_point has the slots of rt_ray");
static_assert(sizeof(rt_irradiance) == 16, "rt_irradiance is 16 bytes");
static_assert(__builtin_offsetof(rt_irradiance, hit_fraction) == 12, "hit_fraction is the fourth word");
static_assert(sizeof(rt_radiance) == 16, "rt_radiance is 16 bytes");
static_assert(sizeof(rt_radiance_stats) == 72, "rt_radiance_stats is 72 bytes");
static_assert(sizeof(rt_ray) == 32, "rt_ray is 32 bytes");
static_assert(sizeof(rt_ray_hit) == 16, "rt_ray_hit is 16 bytes");
static_assert(sizeof(rt_ray_stats) == 48, "rt_ray_stats is 48 bytes");
static_assert(sizeof(rt_topology) == 80, "MeshTopology is 80 bytes");
static_assert(sizeof(rt_node) == 32, "BVHNode is 32 bytes");
static_assert(sizeof(rt_instance) == 144, "Instance is 144 bytes");
static_assert(sizeof(rt_light_ref) == 8, "LightRef is 8 bytes");
static_assert(sizeof(rt_camera) == 96, "Camera is 96 bytes");
static_assert(sizeof(rt_scene_uniforms) == 256, "uniform buffer is 256 bytes");
static_assert(__builtin_offsetof(rt_scene_uniforms, frame_count) == 192, "mixed block at 192");
static_assert(__builtin_offsetof(rt_scene_uniforms, jitter) == 224, "jitter at 224");
#endif

#define RT_TEX_SIZE 1024 /* ResourceManager.ts:181-196: every layer is 1024x1024 rgba8unorm */

#endif
