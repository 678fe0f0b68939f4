// rt_api.hip — C ABI of include/mi355rt.h: resource management + kernel launches.
//
// Host-side restatement of the reference's ResourceManager / pass objects:
//   buffer growth policy (1.5x, needsRebind)    src/renderer/ResourceManager.ts:209-228
//   uniform packing + Halton jitter             src/renderer/ResourceManager.ts:348-447
//   pass order compute(): raster -> raytrace    src/renderer/WebGPURenderer.ts:88-102
//   present(): post pass, history ping-pong     src/renderer/WebGPURenderer.ts:104-129
// There is no CPU fallback anywhere in this file: without a HIP device rt_create fails.

#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <execinfo.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mi355rt.h"
#include "kernels.hip.h"
#include "reflection_sample.h"
#include "launch_plan.h"
#include "scene_facts.h"
#include "device_owned.h"
#include "bvh_build.hip.h"
#include "world_update.hip.h"
#include "k_ieee_check.hip.h"

namespace lp = launch_plan;

namespace {

using namespace owned;   // DeviceBuffer, Event, EventPair, Pinned, Stream

std::string g_create_error;

// A kernel prepared for a launch (resident_blocks): the workgroup size and dynamic LDS its attribute was last set for, and
// the workgroups of that shape a CU holds.  One entry per function.
struct PreparedKernel {
  const void* fn;
  int block;
  size_t dyn;
  int per_cu;
};

// What one kind of query (rt_trace_rays, rt_trace_radiance, rt_gather_irradiance, rt_gather_probes, rt_gather_directional) keeps
// between calls: the staging arrays of its host entry, its own counter shards with the chunk counter behind them, and the
// events around its last launch.
struct QueryState {
  DeviceBuffer in, out, counters;
  EventPair ev;
  bool timed = false;               // the last query recorded its events
  std::deque<EventPair> batch_ev;   // a batched call (run_batches) traces once per batch, each between a pair of its own (deque: a pair never moves)
  uint32_t batches_timed = 0;       // ... and the batches of the last call that recorded theirs (batch_time_ms)
};

// What lightmap bakes (rt_bake_points, rt_bake_irradiance and their atlas forms) keep between calls: their staging arrays,
// kept and grown.
struct BakeState {
  DeviceBuffer uv;                  // the caller's override atlas UVs (host entries)
  DeviceBuffer owner, blocks, count;   // owner map, per-workgroup counts / prefixes, the device count
  DeviceBuffer points, texels;      // the compacted points and their texel indices
  DeviceBuffer results, atlas;      // rt_bake_irradiance: the gather's results, the scattered atlas
  DeviceBuffer entries, items, owner64;   // atlas bakes: the rt_bake_rect list, the item counts / prefixes, the 64-bit owner map
  // pinned staging ring of the entry lists: the copy to `entries` is truly asynchronous and its source outlives it (buffer k
  // is reused only after the event recorded behind its copy has completed)
  static constexpr int kEntryRing = 4;
  Pinned ring[kEntryRing];
  size_t ring_bytes[kEntryRing] = {};
  Event ring_ev[kEntryRing];
  bool ring_used[kEntryRing] = {};
  int ring_next = 0;
};

// What atlas dilation (rt_dilate_atlas) keeps between calls, kept and grown: the staged atlas and the filled count of the host
// entry, the coverage bitmap, and the source map of a call that asks for none.
struct DilateState {
  DeviceBuffer atlas, filled, bitmap, src;
};

// What atlas denoising (rt_denoise_atlas) keeps between calls, kept and grown: the guide index map and the scratch atlas of
// the ping-pong, and the staged inputs and output of the host entry.
struct DenoiseState {
  DeviceBuffer index, scratch, in, out, points, texels;
};

// What the frame denoiser (rt_denoise_frame, rt_set_present_denoise) keeps between calls, kept and grown, and dropped by
// rt_resize: the outputs of the prepare stage (colour, guides, modulation) with the key they were made under - present()
// overwrites the albedo plane, so a call after it can only reuse them - the two colour images of the ping-pong, the filtered
// image of the host entry and of a filtered present(), the albedo plane of a frame traced ahead into the main planes
// (rt_set_lookahead), the events around every stage of the last call and its stats.
struct DenoiseFrameState {
  DeviceBuffer col, guide, mod, ping, pong, out, albedo_keep;
  bool cache_valid = false;
  uint64_t cache_gen = 0, cache_epoch = 0;
  uint32_t cache_flags = 0;
  bool keep_valid = false;          // albedo_keep holds the albedo of the last frame of the dispatch in flight
  bool wanted = false;              // a frame-denoise call was made on this context: dispatches that trace ahead keep that plane
  bool present_on = false;
  rt_frame_denoise_desc present_desc = {};
  int form = 0;                     // rt_set_frame_denoise_form
  EventPair ev[2 + RT_FRAME_DENOISE_MAX_PASSES];   // prepare, finish, the passes
  bool ev_ready = false, timed = false;
  rt_frame_denoise_report last = {};
};

// What the temporal stage of the frame denoiser (rt_set_frame_temporal) keeps between frames, beside DenoiseFrameState and
// dropped with it by rt_resize: per pixel the history colour {q.rgb, (float)n}, the moments {m1, m2} of lum(q) and the guide of
// the frame the history was made from, all double-buffered (the stage reads set `cur` and writes the other one, into which
// k_frame_prepare has written its guide); the integrated image, which takes fd.col's place as the input of pass 0; and the
// uniform block k_frame_prepare was given for the frame of set `cur`.  `have` says that set `cur` holds a history at all.
struct FrameTemporalState {
  bool on = false;
  rt_frame_temporal_desc desc = {};
  DeviceBuffer hist[2], mom[2], guide[2], integ;
  int cur = 0;
  bool have = false;
  uint32_t hist_flags = 0;          // the DEMODULATE bit the stored quantity was made under
  uint32_t frames = 0;              // frames integrated since the last drop
  rt_scene_uniforms prev_uniforms = {};
  EventPair ev;
};

// What frame motion (RT_FRAME_TEMPORAL_MOTION, mi355rt.h "THE FRAME MOTION RULE") keeps beside FrameTemporalState, and only
// while the flag is set: the carry plane of the last run; the snapshot of the frame of set `cur` - vertex positions, forward
// transforms by stable id, and the id plane, double-buffered with the history (pix_id[ft.cur] belongs to ft.hist[ft.cur]) - with
// the counts it was taken at; and where the stable ids of the instance array now on the device come from.
struct FrameMotionState {
  DeviceBuffer carry, snap_pos, snap_xf, pix_id[2], ids;
  uint32_t snap_verts = 0, snap_inst = 0;
  enum { IDS_IDENTITY, IDS_DECLARED, IDS_WORLD } ids_from = IDS_IDENTITY;
  bool ran = false;                 // `carry` holds a run at the current size
  uint64_t scene_gen = 0;           // writes of geometry, topology, instances or BVH (uploads, rt_world_update) ...
  uint64_t gbuf_scene_gen = 0;      // ... and its value when the last G-buffer was made (recorded with gbuf_gen)
  EventPair ev;
};

// What a lightmap bake (rt_bake_atlas_lightmap) and the encode entries (rt_encode_atlas) keep between calls beyond the state of
// the stages they are made of, kept and grown: the filtered atlas, the gutter fill's count, the encoded atlas and the staged
// input of the host encode entry.
struct LightmapState {
  DeviceBuffer filtered, filled, encoded, in;
};

// What irradiance volumes (rt_sample_volume, rt_encode_volume) keep between calls, kept and grown: the staged volume, points
// and results of the host entries and the encoded layers.  A bake's probes and results live in the probe gather's staging.
struct VolumeState {
  DeviceBuffer volume, points, out, encoded;
};

// What reflection probes (rt_capture_reflection, rt_filter_reflection, rt_bake_reflection) keep between calls, kept and grown:
// the staged probes, maps and chains of the host entries.  The counter shards and the event pairs of their radiance launches
// live in a QueryState of their own (rt_ctx::rf); the scratch of a batch is the composed gathers'.
struct ReflectionState {
  DeviceBuffer probes, maps, chains;
};

// What probe visibility maps (rt_bake_volume_visibility, rt_sample_volume_visible, rt_encode_volume_visibility) keep between
// calls, kept and grown: the staged maps, volume, points, results and tiles of the host entries.  The counter shards and the
// event pairs of a bake's ray launches live in a QueryState of their own (rt_ctx::vv); the scratch of a batch is the composed
// gathers'.
struct VisibilityState {
  DeviceBuffer maps, volume, points, out, encoded;
};

// What the reflection sampler (rt_sample_reflection) keeps between calls, kept and grown: the staged chains, probes, boxes,
// queries and results of the host entry.  Nothing of the reflection probes' own state is touched.
struct ReflectionSampleState {
  DeviceBuffer chains, probes, boxes, queries, out;
};

}  // namespace

struct rt_ctx {
  int device = 0;
  // the streams come before every buffer and event: members go in reverse order of declaration, so they go last
  Stream own_stream;
  hipStream_t stream = nullptr;   // own_stream, or the caller's (rt_set_stream)
  // wavefront form: the any-hit trace of a depth runs on `side_stream` beside the closest-hit trace on `stream` (the two
  // read the same shade output and write different result arrays), so the drain tail of one — a few long rays stepping
  // alone — is filled by the other.  MI355RT_WF_OVERLAP=0 puts both on `stream` again.
  Stream side_stream;
  Event side_fork, side_join;
  bool wf_overlap = true;
  int shade_per_cu = 8;          // workgroups per CU of the wavefront shade kernels (MI355RT_SHADE_BLOCKS_PER_CU); swept 4 / 8 /
                                 // 12 / 16 / 24, shade ms per image: sponza-like 64.6 / 63.9 / 63.9 / 64.3 / 64.7, instanced x1000
                                 // 35.9 / 36.4 / 36.7 / 37.4 / 38.7 (every wave may leave a partly used queue chunk per launch)
  std::string error;

  // scene buffers (raw bridge layout)
  DeviceBuffer topology, instances, lights, draw_commands, pos, nrm, uv, nodes, textures, tex_staging;
  uint32_t bv_levels = 0, bv_big_levels = 0, bv_last_tris = 0, bv_gen = 0;   // depth of the last rt_build_blas tree: how many levels the next build launches
  Pinned bv_pinned;           // 64 KB of pinned host memory for the read-back of the build's bookkeeping
  DeviceBuffer bv_in, bv_tri, bv_order, bv_nodes, bv_out, bv_counters, bv_big;  // BLAS build work space
  // device-resident World::update(t) (rt_world_update, csrc/world_update.hip.h)
  struct {
    bool valid = false;
    uint64_t epoch = 0;                   // rt_world_frame::static_epoch the static buffers were made from
    std::vector<wu::Geom> geoms;          // device pointers into `stat`
    std::vector<uint32_t> levels, big_levels;   // per geometry: tree levels / large-node levels the next build launches
    std::vector<float> inst_scale2;       // per instance (declaration order): squared linear scale (treelet weights)
    std::vector<uint32_t> inst_geom;
    uint32_t n_joints = 0, n_verts = 0, n_tris = 0, n_lights = 0, n_tlas = 0, n_inst = 0, n_skins = 0;
    DeviceBuffer stat, joints, raw_inst, geom_rows, node_base, em_flag, em_list, em_blk, tlas_scratch, stats;
    Pinned pinned;                        // joint-matrix staging and the end-of-update read-back
    size_t pinned_bytes = 0;
    wu::TlasArgs tlas;
    // static-geometry cache: a geometry without a skin has the same BLAS in every frame of a static description
    bool cache_enabled = true, static_cached = false, any_skinned = false;
    DeviceBuffer static_nodes;
    std::vector<uint32_t> static_count, static_off;   // per geometry: cached node count, first node in static_nodes
    double last_ms = 0;                   // stream time of the last update (rt_world_last_ms)
    double last_tlas_ms = 0;              // ... of its k_tlas launch alone (rt_world_last_tlas_ms)
    bool tlas_lds_set = false;
    Event ev0, ev1, ev_t0, ev_t1;
  } world;
  // derived buffers (device_scene.h)
  DeviceBuffer tri_geom, tri_shade, inst_trav, light_rec;
  DeviceBuffer tri_shade_w;   // per-triangle world records of a one-leaf-TLAS scene (k_prepare_world_tris); the path tracer's
                              // part, tri_world, lies behind the shading records in tri_shade
  DeviceBuffer tnodes, node_key, node_newidx, inst_root, root_w, treelet_work;   // k_treelet.hip.h
  DeviceBuffer pairs, pair_of, pair_parent, root_rec;                             // k_pairs.hip.h
  uint32_t n_pairs = 0;             // inner nodes of the uploaded TLAS ++ BLAS arrays (counted on the host at upload)
  rtk::TlasRoot troot = {};         // box and word of the TLAS root (node 0), passed to the trace kernels by value
  bool roots_dirty = true;          // root records: rebuilt on every instance upload (cheap); the pair records only when the
                                    // node array or the SET of BLAS roots changed
  std::vector<float> root_w_host;                                   // per entry of blas_roots: sum of squared instance scales
  bool tris_dirty = true, inst_dirty = true, lights_dirty = true, nodes_dirty = true, pairs_dirty = true;
  bool world_rec_dirty = true;      // tri_world / tri_shade_w: set with tris_dirty, inst_dirty and nodes_dirty, cleared when
                                    // prepare_scene has rebuilt them (only for a scene that takes a one-leaf LDS form)
  bool pairs_wanted = false;        // rt_debug_read_pairs: build the pair records whatever walk is selected
  bool validate_dirty = true, scene_valid = false;  // k_validate_scene: run once per upload
  std::string scene_problem;
  std::vector<uint32_t> blas_roots;                 // sorted unique BLAS-local root offsets of the instances
  DeviceBuffer val_roots, val_bad;
  uint32_t n_tris = 0, n_instances = 0, n_lights = 0, n_verts = 0, n_nodes = 0, tex_layers = 0;
  std::vector<uint32_t> draw_commands_host;  // kept like ResourceManager.drawCommandsArray

  // screen resources
  uint32_t width = 0, height = 0;
  DeviceBuffer accum, render_target, g_normal, g_depth, history[2], counters;
  void* external_accum = nullptr;
  void* present_source = nullptr;   // rt_bind_present_source: present() reads this instead of the accumulation buffer
  bool accum_stale = false;         // rt_bind_accum's buffer was sized for the screen before the last rt_resize ...
  bool present_stale = false;       // ... and so was rt_bind_present_source's: each is cleared only by its own bind call
  int history_index = 0;
  // the sharded image (rt_dist_*, k_stripes.hip.h): this context is rank `rank` of `world`
  struct {
    bool active = false;
    uint32_t rank = 0, world = 1, stripe_rows = 0;
    uint32_t max_rows = 0;             // rows of a compact block at the current size (0: no size yet)
    DeviceBuffer send, recv, display;  // this rank's block; rank 0: the world receive blocks, the assembled image
    void* comm = nullptr;              // ncclComm_t, or null: the host moves the blocks
  } dist;

  // uniforms + host state (ResourceManager fields)
  rt_scene_uniforms uniforms;
  float prev_camera[24];
  double acc_jx = 0, acc_jy = 0, jx = 0, jy = 0, avg_jx = 0, avg_jy = 0;
  uint32_t blas_offset = 0, vertex_count = 0, light_count = 0;
  uint32_t total_frames = 0;  // WebGPURenderer.totalFrames
  uint32_t max_depth = 10, spp = 1;
  bool pipeline_built = false;
  bool detailed_counters = false;
  uint32_t stripe_rows = 0, stripe_rank = 0, stripe_count = 1;
  int variant = 3;        // 3 = auto (default): persistent kernel for LDS-resident scenes, wavefront for larger ones;
                          // 0 = one-pixel-per-lane megakernel, 1 = persistent kernel, 2 = wavefront
  int num_cus = 256;      // multiProcessorCount of the device
  std::vector<PreparedKernel> prepared;   // every kernel launched with dynamic LDS so far (resident_blocks)
  lp::PlanKnobs knobs;           // what the launch planner takes from the environment and rt_set_walk (launch_plan.h)
  int treelet_order = 2;          // order of tnodes: 0 = by visit probability, 1 = the bridge's depth-first order, 2 = auto (MI355RT_TREELET_ORDER)
  bool nodes_from_device = false; // the node array was made by rt_world_update (an animated world), not uploaded
  uint32_t pt_launch[4] = {0, 0, 0, 0};   // last persistent launch: threads, workgroups, dynamic LDS, workgroups per CU
  lp::SceneFacts facts;          // materials of the topology on the device (scene_facts.h): worked out from the caller's bytes
                                 // in rt_upload(RT_KIND_TOPOLOGY), unknown after every other writer of the topology records
  int pt_form = RT_PT_FORM_NONE; // form of the last path-trace dispatch of compute() (rt_debug_pt_form)
  // The leaf sweep of a one-leaf scene (scene_facts.h walk_facts).  The host keeps the caller's bytes it is worked out from: the
  // BLAS nodes and the TLAS leaf of rt_upload_bvh when they are few enough to belong to a one-leaf LDS scene, and the BLAS
  // root of every instance of an instance upload.  A device-resident world update forgets them (walk_forget).
  std::vector<rt_node> blas_host;          // empty: not kept (too large, not a one-node TLAS, or made on the device)
  rt_node tlas0_host = {};
  std::vector<uint32_t> inst_root_host;    // empty: not kept
  lp::WalkFacts walk;                      // of the nodes and instances on the device, once walk_dirty is cleared
  bool walk_dirty = true;
  uint32_t walk_nodes = 0;                 // nodes of the sweepable BLAS, leaves included (walk.sweepable only)
  DeviceBuffer leaf_recs;                  // walk.n_leaves + 1 leaf records of 32 bytes, then walk_nodes + 1 node records
  DeviceBuffer ticket;    // tile ticket counter of the persistent kernel
  DeviceBuffer slots;     // DevFrameSlot table of the current (batched) dispatch
  // pinned staging ring for the slot tables: the H2D copy of a dispatch's table is truly asynchronous and its source
  // outlives it (entry k is reused only after the event recorded behind its copy has completed)
  static constexpr int kSlotRing = 8;
  Pinned slot_ring;                    // kSlotRing x 64 DevFrameSlot
  Event slot_ring_ev[kSlotRing];
  bool slot_ring_used[kSlotRing] = {};
  int slot_ring_next = 0;
  // Speculative lookahead of the live loop (rt_set_lookahead): a compute(f) that continues a run f-1, f traces the frames
  // f .. f+L-1 as ONE batched dispatch (L doubles while the run goes on) and accumulates only frame f; the following
  // compute(f+1) ... find their frame colours ready and only add them.  Any call that changes what a frame looks like
  // bumps `epoch` and drops what was traced ahead.
  uint32_t lookahead_max = 0;       // 0 / 1: off
  uint64_t epoch = 0;
  struct {
    bool valid = false;
    uint64_t epoch = 0;
    uint32_t n = 0, k = 0;          // frames traced, frames consumed
    uint32_t fc0 = 0, tf0 = 0;      // frame_count / totalFrames of the first traced frame
    const DevFrameSlot* dslots = nullptr;
    std::vector<DevFrameSlot> slots;   // host copy (jitter check, G-buffer planes of each frame)
    DevFrame frame;
  } spec;
  uint32_t run_len = 0, run_last_fc = 0, run_last_tf = 0;   // the run of consecutive single-frame compute() calls
  uint64_t run_epoch = 0;
  uint32_t look = 1;                // frames the next dispatch of the run traces
  uint32_t look_limit = 0;          // rt_set_lookahead_limit: frames (this one included) until the caller will end the run; 0 = unknown
  int gbuf_slot = -1;               // >= 0: the last compute() consumed this frame of the traced batch (rt_read_gbuffer)
  uint32_t acc_frames = 0;          // frames k_accumulate_frames adds at the end of a dispatch (all of them unless traced ahead)
  DeviceBuffer gbuf_batch;  // G-buffer planes of frames 0..n-2 of a batch (the last frame uses the main planes)
  DeviceBuffer frame_col;   // per-frame colours of a batch, added in frame order by k_accumulate_frames
  DeviceBuffer wf_state, wf_queues, wf_counters;  // wavefront form: path state, ray / path queues, queue counters
  // ray queries (rt_trace_rays), radiance queries (rt_trace_radiance) and irradiance gathers (rt_gather_irradiance): buffers
  // and events, shape and stats of the last query
  QueryState rq, rd, gi;
  rt_ray_stats rq_last = {};
  rt_radiance_stats rd_last = {};
  rt_radiance_stats gi_last = {};
  // The batched kinds - probe and directional gathers, reflection captures, visibility bakes - all go through the one batch
  // driver (run_batches): per batch a kernel that makes rays, a trace of them, a kernel that reduces the results.  Each has a
  // QueryState of its own (the host entry's staging, the counter shards of its trace launches, an event pair per trace launch
  // of the last call) and its last stats; the scratch of a batch is shared, pr_rays / pr_rad (one rt_ray and one 16-byte
  // result per sample, kept and grown by the driver), being per-call scratch on the one stream.
  // probe gathers (rt_gather_probes): a path-query kind of their own
  QueryState pr;
  rt_radiance_stats pr_last = {};
  DeviceBuffer pr_rays, pr_rad;
  // directional gathers (rt_gather_directional): the same composition at surface points
  QueryState dg;
  rt_radiance_stats dg_last = {};
  // directional bakes (rt_bake_atlas_directional, _lightmap): the gather's results, the four scattered layers and the four
  // encoded layers, kept and grown
  DeviceBuffer db_results, db_layers, db_encoded;
  BakeState bk;
  DilateState dl;
  DenoiseState dn;
  DenoiseFrameState fd;
  FrameTemporalState ft;
  FrameMotionState fm;
  uint64_t gbuf_gen = 0;            // dispatches and consumed frames that made a G-buffer current: the key of fd's cache
  bool albedo_plane_valid = false;  // the render target holds the albedo a compute() wrote (present() overwrites it)
  LightmapState lm;
  VolumeState vol;
  // reflection probes: a path-query kind of their own and the staging of their host entries
  QueryState rf;
  rt_radiance_stats rf_last = {};
  ReflectionState rfl;
  // probe visibility maps: their ray launches count and time on a state of their own, so rt_ray_query_stats keeps reporting
  // the caller's last rt_trace_rays (an rt_ray_hit is 16 bytes, like an rt_radiance)
  QueryState vv;
  rt_ray_stats vv_last = {};
  VisibilityState vis;
  ReflectionSampleState rfs;

  // kernel timing
  bool timing = false;
  std::deque<EventPair> ev_pool;   // deque: pointers handed out by next_events stay valid while later timers nest inside
  size_t ev_used = 0;
  std::vector<std::pair<size_t, int>> ev_tags;  // (pool index, RT_TIMER_* of mi355rt.h)

  rt_ctx() {
    std::memset(&uniforms, 0, sizeof(uniforms));
    std::memset(prev_camera, 0, sizeof(prev_camera));
  }
};

namespace {

int fail(rt_ctx* c, int code, const std::string& msg) {
  if (c) c->error = msg;
  return code;
}
// A refusal that needs no context, "<what>: <msg>": without one the message is what rt_last_error(NULL) returns.  (The
// entries of a family that has no such refusal return before they get here.)
int refuse(rt_ctx* c, const char* what, const std::string& why) {
  const std::string msg = std::string(what) + ": " + why;
  if (!c) g_create_error = msg;
  return fail(c, RT_ERR_INVALID, msg);
}
int hip_fail(rt_ctx* c, hipError_t e, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  return fail(c, RT_ERR_HIP, buf);
}
#define HIP_TRY(ctx, expr)                                   \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return hip_fail((ctx), _e, #expr); \
  } while (0)

// ensureBuffer (ResourceManager.ts:209-228): keep when large enough, else reallocate at 1.5x.
// Returns 1 when the buffer was (re)allocated, 0 when kept, <0 on error.
int ensure_buffer(rt_ctx* c, DeviceBuffer& b, size_t bytes, bool grow_policy) {
  b.size = bytes;
  if (b.ptr && b.capacity >= bytes) return 0;
  if (b.ptr) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipFree(b.ptr));
    b.ptr = nullptr;
  }
  size_t cap = bytes;
  if (grow_policy) {
    cap = (size_t)std::ceil((double)bytes * 1.5);
    cap = (cap + 3) & ~(size_t)3;
  }
  if (cap < 16) cap = 16;
  // 16 bytes of slack beyond the reported capacity: kernels stage 8-byte arrays in 16-byte slots
  HIP_TRY(c, hipMalloc(&b.ptr, cap + 16));
  b.capacity = cap;
  return 1;
}
int upload(rt_ctx* c, DeviceBuffer& b, const void* src, size_t bytes) {
  int r = ensure_buffer(c, b, bytes, true);
  if (r < 0) return r;
  if (bytes) {
    // queue.writeBuffer semantics: the source may be reused right after return
    HIP_TRY(c, hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return r;
}

double halton(uint32_t index, uint32_t base) {  // ResourceManager.ts:348-357 (JS doubles)
  double f = 1, r = 0;
  while (index > 0) {
    f = f / (double)base;
    r = r + f * (double)(index % base);
    index = index / base;
  }
  return r;
}
// jitter + running average, shared by updateSceneUniforms (:366-371,385-394) and updateFrameUniforms (:408-424)
void step_jitter(rt_ctx* c, uint32_t halton_source, uint32_t frame_count) {
  c->jx = (halton((halton_source % 16u) + 1u, 2) - 0.5) / (double)c->width;
  c->jy = (halton((halton_source % 16u) + 1u, 3) - 0.5) / (double)c->height;
  if (frame_count == 1u) {
    c->acc_jx = c->jx;
    c->acc_jy = c->jy;
  } else {
    c->acc_jx += c->jx;
    c->acc_jy += c->jy;
  }
  c->avg_jx = c->acc_jx / (double)frame_count;
  c->avg_jy = c->acc_jy / (double)frame_count;
}
void write_mixed(rt_ctx* c, uint32_t frame_count) {  // the 48 bytes at offset 192
  rt_scene_uniforms& u = c->uniforms;
  u.frame_count = frame_count;
  u.blas_base_idx = c->blas_offset;
  u.vertex_count = c->vertex_count;
  u.rand_seed = 0;  // Math.random() in the reference; no shader reads it
  u.light_count = c->light_count;
  u.width = c->width;
  u.height = c->height;
  u.pad = 0;
  u.jitter[0] = (float)c->jx;
  u.jitter[1] = (float)c->jy;
  u.average_jitter[0] = (float)c->avg_jx;
  u.average_jitter[1] = (float)c->avg_jy;
}

float4* accum_ptr(rt_ctx* c) { return (float4*)(c->external_accum ? c->external_accum : c->accum.ptr); }

// ---------------------------------------------------------------- the sharded image (rt_dist_*, k_stripes.hip.h)
// RCCL is loaded at run time, never linked: the library loads and renders on a machine without librccl.  The public NCCL
// API (nccl.h), declared here for the few calls the gather makes.
struct RcclUniqueId {
  char internal[128];
};
struct Rccl {
  void* handle = nullptr;
  std::string file;    // the file the calls resolve into (dladdr), for error messages
  std::string error;   // why it is unusable (empty: usable)
  int (*GetUniqueId)(RcclUniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclFloat32 = 7;   // ncclDataType_t

// One copy per process.  Order: MI355RT_RCCL=<path>; the librccl.so.1 already mapped (a process that has loaded PyTorch has
// PyTorch's, built against the HIP runtime it shares with this library: INTEGRATION.md "One HIP runtime per process");
// the system's.  A failure is remembered (the message says why) and never aborts.
Rccl& rccl() {
  static Rccl R;
  static std::once_flag once;
  std::call_once(once, [] {
    std::string tried;
    auto open = [&](const char* name, int flags) {
      if (R.handle) return;
      R.handle = dlopen(name, flags);
      if (!R.handle) {
        const char* e = dlerror();
        if (!(flags & RTLD_NOLOAD)) tried += std::string(tried.empty() ? "" : "; ") + (e ? e : name);
      }
    };
    const char* env = getenv("MI355RT_RCCL");
    if (env && env[0]) {
      open(env, RTLD_NOW | RTLD_LOCAL);
    } else {
      open("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
      open("librccl.so", RTLD_NOW | RTLD_NOLOAD);
      open("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
      open("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    if (!R.handle) {
      R.error = "librccl could not be loaded (" + tried + "); set MI355RT_RCCL=<path of librccl.so>";
      return;
    }
    struct {
      const char* name;
      void** slot;
    } syms[] = {{"ncclGetUniqueId", (void**)&R.GetUniqueId},   {"ncclCommInitRank", (void**)&R.CommInitRank},
                {"ncclCommDestroy", (void**)&R.CommDestroy},   {"ncclGroupStart", (void**)&R.GroupStart},
                {"ncclGroupEnd", (void**)&R.GroupEnd},         {"ncclSend", (void**)&R.Send},
                {"ncclRecv", (void**)&R.Recv},                 {"ncclGetErrorString", (void**)&R.GetErrorString}};
    for (auto& sy : syms) {
      *sy.slot = dlsym(R.handle, sy.name);
      if (!*sy.slot && R.error.empty()) R.error = std::string("librccl has no symbol ") + sy.name;
    }
    Dl_info info;
    if (R.GetUniqueId && dladdr((void*)R.GetUniqueId, &info) && info.dli_fname) R.file = info.dli_fname;
    if (!R.error.empty()) R.error += " (" + R.file + ")";
  });
  return R;
}
std::string rccl_what(const char* call, int rc) {
  Rccl& R = rccl();
  return std::string(call) + ": " + (R.GetErrorString ? R.GetErrorString(rc) : "error") + " (" + std::to_string(rc) +
         ", RCCL from " + R.file + ")";
}

// rows of the largest share - rank 0's: whole periods of stripe_rows * world rows, then the first stripe of the rest
uint32_t dist_max_rows(uint32_t height, uint32_t stripe_rows, uint32_t world) {
  const uint64_t period = (uint64_t)stripe_rows * world;
  return (uint32_t)((height / period) * stripe_rows + std::min<uint64_t>(height % period, stripe_rows));
}
rtk::StripePlan dist_plan(const rt_ctx* c) {
  rtk::StripePlan p;
  p.width = c->width;
  p.height = c->height;
  p.stripe_rows = c->dist.stripe_rows;
  p.world = c->dist.world;
  p.max_rows = c->dist.max_rows;
  p.chunks = (c->width + 255u) / 256u;
  return p;
}
size_t dist_block_bytes(const rt_ctx* c) { return (size_t)c->dist.max_rows * c->width * 16; }
void dist_free_buffers(rt_ctx* c) {
  c->dist.send.reset();
  c->dist.recv.reset();
  c->dist.display.reset();
  c->dist.max_rows = 0;
}
// (Re)allocate a rank's buffers for the current screen, zeroed; the stream is idle on return.
int dist_alloc(rt_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dist_free_buffers(c);
  if (!c->width || !c->height) return RT_OK;   // no screen yet: rt_resize comes back here
  c->dist.max_rows = dist_max_rows(c->height, c->dist.stripe_rows, c->dist.world);
  const size_t block = dist_block_bytes(c);
  struct {
    DeviceBuffer* b;
    size_t bytes;
  } items[] = {{&c->dist.send, block},
               {&c->dist.recv, c->dist.rank == 0 ? block * c->dist.world : 0},
               {&c->dist.display, c->dist.rank == 0 ? (size_t)c->width * c->height * 16 : 0}};
  for (auto& it : items) {
    if (!it.bytes) continue;
    int r = ensure_buffer(c, *it.b, it.bytes, false);
    if (r >= 0 && hipMemsetAsync(it.b->ptr, 0, it.bytes, c->stream) != hipSuccess) r = fail(c, RT_ERR_HIP, "hipMemsetAsync (sharded image buffers)");
    if (r < 0) {
      (void)hipGetLastError();
      dist_free_buffers(c);
      return r;
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
// rt_dist_shutdown / rt_destroy: the caller has fenced the stream
void dist_release(rt_ctx* c) {
  if (c->dist.comm) (void)rccl().CommDestroy(c->dist.comm);
  c->dist.comm = nullptr;
  dist_free_buffers(c);
  if (c->dist.active) {
    c->dist.active = false;
    c->stripe_rows = 0;
    c->stripe_rank = 0;
    c->stripe_count = 1;
    c->epoch++;
  }
}
// what every entry point of a rank checks first; rank0: the call is rank 0's alone
int dist_ready(rt_ctx* c, const char* what, bool rank0) {
  if (!c->dist.active) return fail(c, RT_ERR_INVALID, std::string(what) + ": the context is no rank of a sharded image (rt_dist_init)");
  if (rank0 && c->dist.rank != 0) return fail(c, RT_ERR_INVALID, std::string(what) + ": only rank 0 assembles the image");
  if (!c->dist.max_rows || !c->dist.send.ptr) return fail(c, RT_ERR_NOT_READY, std::string(what) + ": no screen size yet (rt_resize)");
  return RT_OK;
}
int dist_launch_pack(rt_ctx* c) {
  const rtk::StripePlan p = dist_plan(c);
  const uint32_t items = p.max_rows * p.chunks;
  hipLaunchKernelGGL(rtk::k_pack_stripes, dim3(std::min<uint32_t>(items, 2048u)), dim3(256), 0, c->stream,
                     (const float4*)accum_ptr(c), (float4*)c->dist.send.ptr, p, c->dist.rank);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}
int dist_launch_unpack(rt_ctx* c) {
  const rtk::StripePlan p = dist_plan(c);
  const uint64_t items = (uint64_t)p.max_rows * p.chunks * p.world;
  hipLaunchKernelGGL(rtk::k_unpack_stripes, dim3((uint32_t)std::min<uint64_t>(items, 2048u)), dim3(256), 0, c->stream,
                     (const float4*)c->dist.recv.ptr, (float4*)c->dist.display.ptr, p);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

DevScene dev_scene(const rt_ctx* c);

// Every index the kernels follow, checked on the GPU once per upload (k_validate.hip.h): a malformed scene is refused
// here instead of faulting or hanging a kernel.
static int validate_scene(rt_ctx* c) {
  if (!c->validate_dirty) return c->scene_valid ? RT_OK : fail(c, RT_ERR_INVALID, c->scene_problem.c_str());
  int r = ensure_buffer(c, c->val_bad, 32, false);
  if (r < 0) return r;
  r = ensure_buffer(c, c->val_roots, std::max<size_t>(4, c->blas_roots.size() * 4), false);
  if (r < 0) return r;
  HIP_TRY(c, hipMemsetAsync(c->val_bad.ptr, 0, 32, c->stream));
  if (!c->blas_roots.empty())
    HIP_TRY(c, hipMemcpyAsync(c->val_roots.ptr, c->blas_roots.data(), c->blas_roots.size() * 4, hipMemcpyHostToDevice, c->stream));
  rtk::ValidateArgs A;
  A.topo = (const float4*)c->topology.ptr;
  A.nodes = (const float4*)c->nodes.ptr;
  A.inst = (const float4*)c->instances.ptr;
  A.lights = (const uint2*)c->lights.ptr;
  A.roots = (const uint32_t*)c->val_roots.ptr;
  A.n_tris = c->n_tris;
  A.n_verts = c->n_verts;
  A.n_nodes = c->n_nodes;
  A.n_tlas = c->blas_offset;
  A.n_inst = c->n_instances;
  A.n_lights = c->n_lights;
  A.n_roots = (uint32_t)c->blas_roots.size();
  A.bad = (uint32_t*)c->val_bad.ptr;
  const uint32_t n = std::max(std::max(c->n_tris, c->n_nodes), std::max(c->n_instances, c->n_lights));
  if (n) hipLaunchKernelGGL(rtk::k_validate_scene, dim3((n + 255) / 256), dim3(256), 0, c->stream, A);
  HIP_TRY(c, hipGetLastError());
  uint32_t bad[5] = {0, 0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(bad, c->val_bad.ptr, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->validate_dirty = false;
  c->scene_valid = !(bad[0] | bad[1] | bad[2] | bad[3] | bad[4]);
  if (!c->scene_valid) {
    c->scene_problem = "scene arrays refer to elements out of range: " + std::to_string(bad[0]) + " triangles (vertex ids), " +
                       std::to_string(bad[1]) + " TLAS nodes, " + std::to_string(bad[2]) + " BLAS nodes, " +
                       std::to_string(bad[3]) + " instances (BLAS offset), " + std::to_string(bad[4]) + " light references";
    return fail(c, RT_ERR_INVALID, c->scene_problem.c_str());
  }
  return RT_OK;
}

// The uploaded scene as the launch planner (launch_plan.h) sees it; with c->knobs, all it reads of the context.
lp::SceneSize scene_size(const rt_ctx* c) {
  return {c->n_nodes, c->n_pairs, c->n_tris, c->n_instances, c->n_verts, c->n_lights, c->blas_offset};
}

// the nodes or the instances on the device are no longer bytes the host has seen
void walk_forget(rt_ctx* c) {
  c->blas_host.clear();
  c->inst_root_host.clear();
  c->walk = lp::WalkFacts();
  c->walk_nodes = 0;
  c->walk_dirty = true;
}

// The walk facts of the scene on the device and, when its BLAS is sweepable, the leaf records traverse_leaves reads: worked
// out again when the node or the instance array has changed.
static int walk_prepare(rt_ctx* c) {
  if (!c->walk_dirty) return RT_OK;
  c->walk = lp::WalkFacts();
  c->walk_nodes = 0;
  c->walk_dirty = false;
  if (c->nodes_from_device || c->blas_offset != 1u || c->blas_host.empty() ||
      c->blas_host.size() != (size_t)c->n_nodes - c->blas_offset || c->inst_root_host.size() != c->n_instances)
    return RT_OK;
  const uint32_t word = c->tlas0_host.data;   // the TLAS leaf: instance << 3 | 1 (k_validate_scene has seen the device's copy)
  const uint32_t inst = word >> 3;
  if (word == 0u || inst >= c->n_instances) return RT_OK;
  // the leaf records, their padding, the node records, their padding: one buffer (traverse_leaves finds the second array
  // behind the first)
  scene_facts::LeafRecord recs[scene_facts::kMaxLeafRecords + 1 + scene_facts::kMaxNodeRecords + 1];
  scene_facts::NodeRecord nodes[scene_facts::kMaxNodeRecords];
  uint32_t n_nodes = 0;
  const lp::WalkFacts f = scene_facts::walk_facts(c->blas_host.data(), c->blas_host.size(), c->inst_root_host[inst],
                                                  c->knobs.leaf_sweep_cap, recs, nodes, &n_nodes);
  if (f.known && f.sweepable) {
    // (each sweep reads one record ahead at its last one, and does not use it)
    recs[f.n_leaves] = scene_facts::padding_record();
    for (uint32_t i = 0; i < n_nodes; i++) recs[f.n_leaves + 1u + i] = nodes[i];
    recs[f.n_leaves + 1u + n_nodes] = scene_facts::padding_record();
    const size_t bytes = ((size_t)f.n_leaves + n_nodes + 2) * sizeof(scene_facts::LeafRecord);
    int r = ensure_buffer(c, c->leaf_recs, bytes, false);
    if (r < 0) return r;
    HIP_TRY(c, hipMemcpyAsync(c->leaf_recs.ptr, recs, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the source is on the stack
    c->walk_nodes = n_nodes;
  }
  c->walk = f;
  return RT_OK;
}

int prepare_scene(rt_ctx* c) {
  {
    int r = validate_scene(c);
    if (r < 0) return r;
    if ((r = walk_prepare(c)) < 0) return r;
  }
  if (c->tris_dirty && c->n_tris && c->n_verts) {
    int r = ensure_buffer(c, c->tri_geom, (size_t)c->n_tris * 16 * RT_TRI_STRIDE, true);
    if (r < 0) return r;
    hipLaunchKernelGGL(rtk::k_prepare_tris, dim3((c->n_tris + 255) / 256), dim3(256), 0, c->stream,
                       (const float4*)c->topology.ptr, (const float4*)c->pos.ptr, (float4*)c->tri_geom.ptr,
                       c->n_tris, c->n_verts);
    HIP_TRY(c, hipGetLastError());
    r = ensure_buffer(c, c->tri_shade, (size_t)c->n_tris * (128 + 32), true);   // + tri_world (k_prepare_world_tris)
    if (r < 0) return r;
    hipLaunchKernelGGL(rtk::k_prepare_tri_shade, dim3((c->n_tris + 255) / 256), dim3(256), 0, c->stream,
                       (const float4*)c->topology.ptr, (const float4*)c->nrm.ptr, (const float2*)c->uv.ptr,
                       (float4*)c->tri_shade.ptr, c->n_tris, c->n_verts);
    HIP_TRY(c, hipGetLastError());
    c->tris_dirty = false;
  }
  if (c->inst_dirty && c->n_instances) {
    int r = ensure_buffer(c, c->inst_trav, (size_t)c->n_instances * 64, true);
    if (r < 0) return r;
    hipLaunchKernelGGL(rtk::k_prepare_instances, dim3((c->n_instances + 255) / 256), dim3(256), 0, c->stream,
                       (const float4*)c->instances.ptr, (float4*)c->inst_trav.ptr, c->n_instances);
    HIP_TRY(c, hipGetLastError());
    c->inst_dirty = false;
  }
  if (c->nodes_dirty && c->n_nodes && c->n_instances) {
    // traversal copy of the node array: explicit successors, most-visited nodes first (k_treelet.hip.h); validate_scene
    // has just uploaded the sorted BLAS roots into val_roots and vouches for every pointer followed here
    int r = ensure_buffer(c, c->tnodes, (size_t)c->n_nodes * 32, true);
    if (r < 0) return r;
    if ((r = ensure_buffer(c, c->node_key, (size_t)c->n_nodes * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->node_newidx, (size_t)c->n_nodes * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->inst_root, (size_t)c->n_instances * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->root_w, std::max<size_t>(4, c->root_w_host.size() * 4), true)) < 0) return r;
    if (!c->root_w_host.empty())
      HIP_TRY(c, hipMemcpyAsync(c->root_w.ptr, c->root_w_host.data(), c->root_w_host.size() * 4, hipMemcpyHostToDevice, c->stream));
    rtk::TreeletArgs T;
    T.nodes = (const float4*)c->nodes.ptr;
    T.tnodes = (float4*)c->tnodes.ptr;
    T.key = (uint32_t*)c->node_key.ptr;
    T.new_index = (uint32_t*)c->node_newidx.ptr;
    T.roots = (const uint32_t*)c->val_roots.ptr;
    T.root_w = (const float*)c->root_w.ptr;
    T.n_nodes = c->n_nodes;
    T.n_tlas = c->blas_offset;
    T.n_roots = (uint32_t)c->blas_roots.size();
    T.k_max = (uint32_t)(c->knobs.lds_per_cu / 32);
    const dim3 grid((c->n_nodes + 255) / 256);
    const uint32_t n_blocks = (c->n_nodes + 1023u) / 1024u;
    if ((r = ensure_buffer(c, c->treelet_work, ((size_t)RT_TREELET_WORK_HEAD + n_blocks) * 4, true)) < 0) return r;
    uint32_t* work = (uint32_t*)c->treelet_work.ptr;
    HIP_TRY(c, hipMemsetAsync(work, 0, (size_t)RT_TREELET_WORK_HEAD * 4, c->stream));
    const dim3 hgrid(std::min<uint32_t>((c->n_nodes + 255) / 256, 256u));
    // A device-resident update(t) (rt_world_update) re-lays the nodes out on every displayed frame: unless a partial
    // treelet is asked for (MI355RT_TREELET_MAX) the visit-probability order buys nothing there, so it keeps the bridge's
    // depth-first order: 3 launches instead of 10 (MI355RT_TREELET_ORDER=weight / identity forces either, for measurements)
    const bool identity = c->treelet_order == 1 || (c->treelet_order == 2 && c->nodes_from_device && c->knobs.treelet_cap < 0);
    if (identity) {
      hipLaunchKernelGGL(rtk::k_treelet_iota, grid, dim3(256), 0, c->stream, T.new_index, c->n_nodes);
    } else {
      hipLaunchKernelGGL(rtk::k_treelet_weight, grid, dim3(256), 0, c->stream, T);
      hipLaunchKernelGGL(rtk::k_treelet_hist<0>, hgrid, dim3(256), 0, c->stream, T, work);
      hipLaunchKernelGGL(rtk::k_treelet_pick<0>, dim3(1), dim3(256), 0, c->stream, T, work);
      hipLaunchKernelGGL(rtk::k_treelet_hist<1>, hgrid, dim3(256), 0, c->stream, T, work);
      hipLaunchKernelGGL(rtk::k_treelet_pick<1>, dim3(1), dim3(256), 0, c->stream, T, work);
      hipLaunchKernelGGL(rtk::k_treelet_count, dim3(n_blocks), dim3(1024), 0, c->stream, T, work);
      hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, work + RT_TREELET_WORK_HEAD, n_blocks, (uint32_t*)nullptr);
      hipLaunchKernelGGL(rtk::k_treelet_number, dim3(n_blocks), dim3(1024), 0, c->stream, T, (const uint32_t*)work);
    }
    hipLaunchKernelGGL(rtk::k_treelet_remap, grid, dim3(256), 0, c->stream, T);
    hipLaunchKernelGGL(rtk::k_treelet_inst_roots, dim3((c->n_instances + 255) / 256), dim3(256), 0, c->stream,
                       (const float4*)c->instances.ptr, (const uint32_t*)c->node_newidx.ptr, (uint32_t*)c->inst_root.ptr,
                       c->n_instances, c->blas_offset, c->n_nodes);
    HIP_TRY(c, hipGetLastError());
    c->nodes_dirty = false;
  }
  // the pair records are only walked by the wavefront trace kernels under the pair walk (rt_set_walk): a scene that takes
  // the node walk does not pay for them on every update(t); they are made when a launch (or rt_debug_read_pairs) wants them
  const bool want_pairs = c->pairs_wanted || lp::walks_pairs(scene_size(c), c->knobs);
  if (want_pairs && (c->pairs_dirty || c->roots_dirty) && c->n_nodes && c->n_instances) {
    // child-pair records of the walk (k_pairs.hip.h); validate_scene has uploaded the sorted BLAS roots into val_roots and
    // vouches for every pointer followed here.  An instance upload that keeps the set of BLAS roots only redoes the root
    // records (one small launch) — what an animated scene pays per update(t).
    int r;
    if ((r = ensure_buffer(c, c->pairs, std::max<size_t>(64, (size_t)c->n_pairs * 64), true)) < 0) return r;
    if ((r = ensure_buffer(c, c->pair_of, (size_t)c->n_nodes * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->pair_parent, (size_t)c->n_nodes * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->root_rec, ((size_t)c->n_instances + 1) * 32, true)) < 0) return r;
    rtk::PairArgs P;
    P.nodes = (const float4*)c->nodes.ptr;
    P.pairs = (float4*)c->pairs.ptr;
    P.pair_of = (uint32_t*)c->pair_of.ptr;
    P.parent = (uint32_t*)c->pair_parent.ptr;
    P.roots = (const uint32_t*)c->val_roots.ptr;
    P.n_nodes = c->n_nodes;
    P.n_tlas = c->blas_offset;
    P.n_roots = (uint32_t)c->blas_roots.size();
    P.pad = 0;
    if (c->pairs_dirty) {
      const uint32_t n_blocks = (c->n_nodes + 1023u) / 1024u;
      if ((r = ensure_buffer(c, c->treelet_work, ((size_t)RT_TREELET_WORK_HEAD + n_blocks) * 4, true)) < 0) return r;
      uint32_t* work = (uint32_t*)c->treelet_work.ptr;
      const dim3 grid((c->n_nodes + 255) / 256);
      hipLaunchKernelGGL(rtk::k_pair_count, dim3(n_blocks), dim3(1024), 0, c->stream, P, work + RT_TREELET_WORK_HEAD);
      hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, work + RT_TREELET_WORK_HEAD, n_blocks, (uint32_t*)nullptr);
      hipLaunchKernelGGL(rtk::k_pair_number, dim3(n_blocks), dim3(1024), 0, c->stream, P, (const uint32_t*)(work + RT_TREELET_WORK_HEAD));
      hipLaunchKernelGGL(rtk::k_pair_parent, grid, dim3(256), 0, c->stream, P);
      hipLaunchKernelGGL(rtk::k_pair_emit, grid, dim3(256), 0, c->stream, P);
      c->pairs_dirty = false;
    }
    hipLaunchKernelGGL(rtk::k_pair_roots, dim3((c->n_instances + 256) / 256), dim3(256), 0, c->stream, P,
                       (const float4*)c->instances.ptr, (float4*)c->root_rec.ptr, c->n_instances);
    HIP_TRY(c, hipGetLastError());
    c->roots_dirty = false;
  }
  if (c->lights_dirty && c->n_lights && c->n_tris && c->n_instances && c->n_verts) {
    int r = ensure_buffer(c, c->light_rec, (size_t)c->n_lights * 64, true);
    if (r < 0) return r;
    DevScene S = dev_scene(c);
    hipLaunchKernelGGL(rtk::k_prepare_lights, dim3((c->n_lights + 255) / 256), dim3(256), 0, c->stream, S,
                       (float4*)c->light_rec.ptr, c->n_lights, c->n_tris, c->n_instances);
    HIP_TRY(c, hipGetLastError());
    c->lights_dirty = false;
  }
  // per-triangle world records: only a scene that takes a one-leaf LDS form reads them (a large animated world does not
  // pay for them on every update); the flag stays set until they are built
  if (c->world_rec_dirty && lp::one_leaf_lds(scene_size(c), c->knobs) && c->n_tris && c->n_verts && c->n_instances && c->n_nodes) {
    int r = ensure_buffer(c, c->tri_shade_w, (size_t)c->n_tris * 128, true);
    if (r < 0) return r;
    DevScene S = dev_scene(c);
    hipLaunchKernelGGL(rtk::k_prepare_world_tris, dim3((c->n_tris + 255) / 256), dim3(256), 0, c->stream, S,
                       (float4*)c->tri_shade.ptr + (size_t)8 * c->n_tris, (float4*)c->tri_shade_w.ptr, c->n_tris,
                       c->n_instances);
    HIP_TRY(c, hipGetLastError());
    c->world_rec_dirty = false;
  }
  return RT_OK;
}

// Host-side validation of everything the kernels index, so a malformed upload is refused
// instead of faulting the GPU.
bool scene_ready(const rt_ctx* c) {
  return c->pipeline_built && c->width && c->height && c->n_tris && c->n_verts && c->n_instances && c->n_nodes &&
         c->accum.ptr && c->lights.ptr;  // RaytracePass.updateBindGroup requires lightsBuffer (:38-46)
}

DevScene dev_scene(const rt_ctx* c) {
  DevScene s;
  s.nodes = (const float4*)c->nodes.ptr;
  s.tnodes = (const float4*)c->tnodes.ptr;
  s.inst_root = (const uint32_t*)c->inst_root.ptr;
  s.pairs = (const float4*)c->pairs.ptr;
  s.root_rec = (const float4*)c->root_rec.ptr;
  s.tri_geom = (const float4*)c->tri_geom.ptr;
  s.tri_shade = (const float4*)c->tri_shade.ptr;
  s.inst_trav = (const float4*)c->inst_trav.ptr;
  s.topo = (const float4*)c->topology.ptr;
  s.pos = (const float4*)c->pos.ptr;
  s.nrm = (const float4*)c->nrm.ptr;
  s.uv = (const float2*)c->uv.ptr;
  s.inst = (const float4*)c->instances.ptr;
  s.lights = (const uint2*)c->lights.ptr;
  s.light_rec = (const float4*)c->light_rec.ptr;
  s.tex = c->tex_layers ? (const uint8_t*)c->textures.ptr : nullptr;
  s.tex_layers = c->tex_layers;
  s.n_lights = c->n_lights;
  return s;
}

EventPair* next_events(rt_ctx* c, int tag) {
  if (!c->timing) return nullptr;
  if (c->ev_used == c->ev_pool.size()) {
    EventPair& p = c->ev_pool.emplace_back();
    if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) {
      c->ev_pool.pop_back();
      return nullptr;
    }
  }
  c->ev_tags.emplace_back(c->ev_used, tag);
  return &c->ev_pool[c->ev_used++];
}

// Prepare `fn` for a launch of `block` threads and `dyn` bytes of dynamic LDS per workgroup; *per_cu: the workgroups of that
// shape a CU holds (registers, LDS), at least 1.  A function has ONE entry: a launch at another size prepares it again, so
// the attribute is always that of the launch about to be made.  (The attribute belongs to the function in the process, the
// table to the context: DESIGN.md 4.1, "Launch preparation".)
int resident_blocks(rt_ctx* c, const void* fn, int block, size_t dyn, int* per_cu) {
  auto it = std::find_if(c->prepared.begin(), c->prepared.end(), [fn](const PreparedKernel& p) { return p.fn == fn; });
  if (it == c->prepared.end()) it = c->prepared.insert(it, PreparedKernel{fn, 0, 0, 0});
  if (it->per_cu == 0 || it->block != block || it->dyn != dyn) {
    it->per_cu = 0;   // a failure below leaves the entry unprepared
    HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    int n = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, block, dyn));
    it->block = block;
    it->dyn = dyn;
    it->per_cu = n < 1 ? 1 : n;
  }
  *per_cu = it->per_cu;
  return RT_OK;
}
// Grid of a kernel whose workgroups loop over their work: the resident ones (per_cu, or cap_per_cu where that is set and
// smaller: MI355RT_WF_BLOCKS_PER_CU) on every CU, no more than there is work for (`useful`), at least one.
uint32_t grid_blocks(const rt_ctx* c, int per_cu, int cap_per_cu, uint64_t useful) {
  if (cap_per_cu > 0 && per_cu > cap_per_cu) per_cu = cap_per_cu;
  const uint64_t blocks = std::min<uint64_t>((uint64_t)per_cu * (uint64_t)c->num_cus, useful);
  return blocks ? (uint32_t)blocks : 1u;
}

// ---- queries against the uploaded scene (rt_trace_rays, rt_trace_radiance, rt_gather_irradiance, rt_gather_probes,
// rt_gather_directional): what the kinds share.  `what` is the prefix of the kind's messages, "ray query", "radiance query",
// "irradiance gather", "probe gather" or "directional gather"; q its QueryState.
//
// The scene is there and its derived records are made (prepare_scene, as a compute() would); lights: the kind samples the
// lights.  Touches nothing of the renderer's frame state.
int query_scene_ready(rt_ctx* c, const char* what, bool lights) {
  const std::string w(what);
  if (!(c->n_tris && c->n_verts && c->n_instances && c->n_nodes))
    return fail(c, RT_ERR_NOT_READY, w + ": no scene (geometry, topology, instances and BVH must be uploaded first)");
  if (c->blas_offset > c->n_nodes) return fail(c, RT_ERR_NOT_READY, w + ": blas_base_idx exceeds the node buffer");
  if (lights && c->light_count > c->n_lights) return fail(c, RT_ERR_INVALID, "light_count exceeds the uploaded lights buffer");
  HIP_TRY(c, hipSetDevice(c->device));
  const int r = prepare_scene(c);
  if (r < 0 && !c->validate_dirty && !c->scene_valid) return fail(c, RT_ERR_NOT_READY, w + ": " + c->scene_problem);
  return r;
}
// One of the caller's arrays of an entry.  when: the call uses it.
struct CallerArray {
  const void* p;
  bool when;
  CallerArray(const void* p_, bool when_ = true) : p(p_), when(when_) {}
};
// an array the caller may leave out by passing NULL
CallerArray optional_array(const void* p) { return {p, p != nullptr}; }
// The caller's arrays of an entry: all there and, for a device entry, all 16-byte aligned - which needs no context, so a
// family with a context-free refusal asks here before it looks at its context - and then each of them, once, memory the
// context's device can reach.
int caller_arrays_ok(rt_ctx* c, const char* what, std::initializer_list<CallerArray> arrays, bool device = true) {
  uintptr_t bits = 0;
  for (const CallerArray& a : arrays) {
    if (!a.when) continue;
    if (!a.p) return refuse(c, what, "NULL array");
    bits |= (uintptr_t)a.p;
  }
  if (device && (bits & 15u)) return refuse(c, what, "device arrays must be 16-byte aligned");
  if (!c || !device) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  for (const CallerArray* a = arrays.begin(); a != arrays.end(); ++a) {
    if (!a->when || std::any_of(arrays.begin(), a, [a](const CallerArray& b) { return b.when && b.p == a->p; })) continue;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, a->p) != hipSuccess) {
      (void)hipGetLastError();
      return refuse(c, what, "not a device-accessible pointer");
    }
    if (at.type == hipMemoryTypeDevice && at.device != c->device)
      return refuse(c, what, "the array lives on another device than the context");
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeHost && at.type != hipMemoryTypeManaged)
      return refuse(c, what, "not a device-accessible pointer");
  }
  return RT_OK;
}
// the query's counter shards and the chunk counter behind them, zeroed on the stream; keep_counts: only the chunk counter
// is (a later launch of one call, whose counts add up in the shards)
int query_reset_counters(rt_ctx* c, QueryState& q, uint64_t** counters, uint32_t** head, bool keep_counts = false) {
  const size_t counter_bytes = (size_t)RT_COUNTER_SHARDS * 6 * 8;
  const int r = ensure_buffer(c, q.counters, counter_bytes + 16, false);
  if (r < 0) return r;
  if (keep_counts)
    HIP_TRY(c, hipMemsetAsync((char*)q.counters.ptr + counter_bytes, 0, 16, c->stream));
  else
    HIP_TRY(c, hipMemsetAsync(q.counters.ptr, 0, counter_bytes + 16, c->stream));
  *counters = (uint64_t*)q.counters.ptr;
  *head = (uint32_t*)((char*)q.counters.ptr + counter_bytes);
  return RT_OK;
}
// the query kernel (256-thread workgroups) on the context's stream, between the events of `ev` when timing is on
int query_launch(rt_ctx* c, EventPair& ev, const void* fn, uint32_t blocks, void** args, size_t dyn) {
  if (c->timing) {
    if (!ev.a) HIP_TRY(c, hipEventCreate(&ev.a));
    if (!ev.b) HIP_TRY(c, hipEventCreate(&ev.b));
    HIP_TRY(c, hipEventRecord(ev.a, c->stream));
  }
  HIP_TRY(c, hipLaunchKernel(fn, dim3(blocks), dim3(256), args, dyn, c->stream));
  if (c->timing) HIP_TRY(c, hipEventRecord(ev.b, c->stream));
  return RT_OK;
}
// The tail the query launches share, behind their choice of kernel and grid: the MI355RT_DEBUG_SHAPE line (print_shape writes
// the kind's), the counters zeroed and handed to the kernel (*counters and *head are fields of a struct that args points
// at), the launch between the events of batch_ev - a pair its caller keeps count of - or else the state's own, and `timed`.
template <class PrintShape>
int query_enqueue(rt_ctx* c, QueryState& q, const void* fn, uint32_t blocks, void** args, size_t dyn, uint64_t** counters,
                  uint32_t** head, bool keep_counts, EventPair* batch_ev, PrintShape print_shape) {
  if (getenv("MI355RT_DEBUG_SHAPE")) print_shape();
  int r = query_reset_counters(c, q, counters, head, keep_counts);
  if (r < 0) return r;
  q.timed = false;
  if ((r = query_launch(c, batch_ev ? *batch_ev : q.ev, fn, blocks, args, dyn)) < 0) return r;
  q.timed = c->timing && !batch_ev;
  return RT_OK;
}
// The six counters of the last query summed over their shards (all 0 when `launched` is false: no query yet, or an empty
// one); *kernel_ms is written when that query recorded its events.  Waits for the stream.
int query_totals(rt_ctx* c, const QueryState& q, bool launched, uint64_t sum[6], double* kernel_ms) {
  std::fill(sum, sum + 6, (uint64_t)0);
  if (!q.counters.ptr || !launched) return RT_OK;
  std::vector<uint64_t> host((size_t)RT_COUNTER_SHARDS * 6);
  HIP_TRY(c, hipMemcpyAsync(host.data(), q.counters.ptr, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t s = 0; s < RT_COUNTER_SHARDS; s++)
    for (int k = 0; k < 6; k++) sum[k] += host[s * 6 + k];
  if (q.timed) {
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, q.ev.a, q.ev.b));
    *kernel_ms = (double)ms;
  }
  return RT_OK;
}
// ---- the blocking host entries: what each stages, stated once per array.
enum : unsigned {
  STAGE_ROOM = 0,   // room for `bytes` in the buffer, which every array gets, and nothing else
  STAGE_IN = 1,     // the host's bytes are copied up before the launch
  STAGE_OUT = 2,    // the buffer's bytes are copied down behind the launch
  STAGE_MADE = 4    // (with STAGE_OUT) no room is made here: the launch makes it
};
struct Staged {
  DeviceBuffer& buf;   // of the entry's own state: kept and grown across calls
  const void* host;    // STAGE_IN: read; STAGE_OUT: the caller's writable array
  size_t bytes;
  unsigned dir;        // STAGE_*
  bool grow = true;    // ensure_buffer's grow_policy
  bool when = true;    // false: the call leaves this array out
};
// A blocking host entry behind its checks: room for every array, the inputs up, launch() enqueues the work on the arrays'
// buffers, the outputs down, one wait; the stream is idle on return and the stats of the work can be read.
template <class Launch>
int staged_call(rt_ctx* c, std::initializer_list<Staged> arrays, Launch launch) {
  HIP_TRY(c, hipSetDevice(c->device));
  int r;
  for (const Staged& a : arrays)
    if (a.when && !(a.dir & STAGE_MADE) && (r = ensure_buffer(c, a.buf, a.bytes, a.grow)) < 0) return r;
  for (const Staged& a : arrays)
    if (a.when && (a.dir & STAGE_IN)) HIP_TRY(c, hipMemcpyAsync(a.buf.ptr, a.host, a.bytes, hipMemcpyHostToDevice, c->stream));
  if ((r = launch()) < 0) return r;
  for (const Staged& a : arrays)
    if (a.when && (a.dir & STAGE_OUT))
      HIP_TRY(c, hipMemcpyAsync(const_cast<void*>(a.host), a.buf.ptr, a.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
// The host entries of the queries: n > 0 records (rt_ray, rt_gather_point) up to the query's staging array, launch(d_rays,
// d_out) enqueues the kind's kernel, n results of out_stride bytes come back.
template <class Record, class Launch>
int query_from_host(rt_ctx* c, QueryState& q, const char* what, const Record* rays, uint32_t n, void* out, size_t out_stride,
                    Launch launch) {
  if (!rays || !out) return fail(c, RT_ERR_INVALID, std::string(what) + ": NULL array");
  return staged_call(c, {{q.in, rays, (size_t)n * sizeof(Record), STAGE_IN}, {q.out, out, (size_t)n * out_stride, STAGE_OUT}},
                     [&] { return launch((const void*)q.in.ptr, q.out.ptr); });
}

// ---- the calls that trace in batches: probe and directional gathers, reflection captures (rt_radiance_stats, on the path
// query) and visibility bakes (rt_ray_stats, on the ray query).
// What the last stats of a batch's trace add to the call's: the form is that of the last batch, the workgroups add up ...
void fold_batch(rt_radiance_stats& sum, const rt_radiance_stats& b) {
  sum.lds = b.lds;
  sum.workgroups += b.workgroups;
}
void fold_batch(rt_ray_stats& sum, const rt_ray_stats& b) {
  sum.walk = b.walk;
  sum.lds = b.lds;
  sum.rayreg = b.rayreg;
  sum.workgroups += b.workgroups;
}
// ... and what the call knows itself: the items and samples of a path kind (the rays of the ray kind come from its counters)
void batches_done(rt_radiance_stats& sum, uint32_t total, uint32_t spp) {
  sum.rays = total;
  sum.samples = (uint64_t)total * spp;
}
void batches_done(rt_ray_stats&, uint32_t, uint32_t) {}
// The one batch loop.  `total` > 0 items of `spp` samples (< 2^31 in all) in batches of RT_PROBE_BATCH_SAMPLES / spp whole
// items, each of them on the stream, in this order:
//   make_rays(first, count, items)             the kind's kernel writes the count * spp = items rays of the batch to pr_rays
//   trace(rays, items, out, keep_counts, ev)   launch_path_query or launch_ray_query_on, on the state q and the stats `last`:
//                                              pr_rays to pr_rad, between the batch's own pair of events
//   reduce(first, count)                       the kind's kernel folds pr_rad into the caller's results
// Every (item, sample) is a trace item of its own, so the cut into batches cannot show in a result.  The counters of the
// batches add up in q's shards; `last` ends as the call's stats, or zeroed when a trace could not be launched.
template <class Stats, class MakeRays, class Trace, class Reduce>
int run_batches(rt_ctx* c, QueryState& q, Stats& last, uint32_t total, uint32_t spp, MakeRays make_rays, Trace trace, Reduce reduce) {
  const uint32_t per_batch = RT_PROBE_BATCH_SAMPLES / spp;   // whole items: >= 64, spp being <= 65536
  const size_t scratch_items = (size_t)std::min(total, per_batch) * spp;
  static_assert(sizeof(rt_ray_hit) == sizeof(rt_radiance), "the hits of a batch live in the radiance scratch");
  int r;
  if ((r = ensure_buffer(c, c->pr_rays, scratch_items * sizeof(rt_ray), false)) < 0) return r;
  if ((r = ensure_buffer(c, c->pr_rad, scratch_items * sizeof(rt_radiance), false)) < 0) return r;
  q.batches_timed = 0;
  Stats sum = Stats();
  uint32_t batch = 0;
  for (uint32_t first = 0; first < total; first += per_batch, batch++) {
    const uint32_t count = std::min(per_batch, total - first);
    const uint32_t items = count * spp;                       // <= RT_PROBE_BATCH_SAMPLES
    if ((r = make_rays(first, count, items)) < 0) return r;
    if (q.batch_ev.size() <= batch) q.batch_ev.emplace_back();
    if ((r = trace((const void*)c->pr_rays.ptr, items, c->pr_rad.ptr, batch != 0, &q.batch_ev[batch])) < 0) {
      last = Stats();
      return r;
    }
    if (c->timing) q.batches_timed = batch + 1;
    fold_batch(sum, last);
    if ((r = reduce(first, count)) < 0) return r;
  }
  batches_done(sum, total, spp);
  last = sum;
  return RT_OK;
}
// The stream time of the batches of q's last call that recorded their events (0.0 with timing off), added to *kernel_ms.  The
// stream has been fenced.
int batch_time_ms(rt_ctx* c, const QueryState& q, double* kernel_ms) {
  for (uint32_t b = 0; b < q.batches_timed; b++) {
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, q.batch_ev[b].a, q.batch_ev[b].b));
    *kernel_ms += (double)ms;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// MI355RT_DEBUG_TERMINATE=1: print a native backtrace when an exception escapes (the HIP runtime throws from inside
// some calls; without this only "terminate called" is seen).
static void debug_terminate() {
  void* frames[64];
  const int n = backtrace(frames, 64);
  fprintf(stderr, "mi355rt: std::terminate, native backtrace:\n");
  backtrace_symbols_fd(frames, n, 2);
  abort();
}

rt_ctx* rt_create(int device_ordinal) {
  if (const char* dbg = getenv("MI355RT_DEBUG_TERMINATE"))
    if (dbg[0] == '1') std::set_terminate(debug_terminate);
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = "no HIP device available (the MI355X renderer has no CPU fallback)";
    return nullptr;
  }
  if (device_ordinal < 0 || device_ordinal >= n) {
    g_create_error = "device ordinal out of range";
    return nullptr;
  }
  if (hipSetDevice(device_ordinal) != hipSuccess) {
    g_create_error = "hipSetDevice failed";
    return nullptr;
  }
  rt_ctx* c = new rt_ctx();
  c->device = device_ordinal;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_error = "hipStreamCreate failed";
    delete c;
    return nullptr;
  }
  c->stream = c->own_stream;
  if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming) != hipSuccess) {
    g_create_error = "hipStreamCreate / hipEventCreate (side stream) failed";
    delete c;
    return nullptr;
  }
  if (const char* e = getenv("MI355RT_WF_OVERLAP")) c->wf_overlap = atoi(e) != 0;
  if (const char* e = getenv("MI355RT_NO_LDS_STAGING")) c->knobs.no_lds_staging = atoi(e) != 0;
  if (const char* e = getenv("MI355RT_PLAIN_MATERIALS")) c->knobs.plain_materials = atoi(e) != 0;
  if (const char* e = getenv("MI355RT_LEAF_SWEEP")) c->knobs.leaf_sweep = atoi(e) != 0;
  if (const char* e = getenv("MI355RT_LEAF_SWEEP_GUARD")) c->knobs.leaf_sweep_guard = atoi(e) != 0;
  if (const char* e = getenv("MI355RT_SHADE_BLOCKS_PER_CU")) c->shade_per_cu = std::max(1, std::min(4096, atoi(e)));
  if (const char* e = getenv("MI355RT_WF_BLOCK")) {
    const int b = atoi(e);
    if (b == 256 || b == 512 || b == 1024) c->knobs.wf_block = b;
  }
  if (const char* e = getenv("MI355RT_TREELET_MAX")) c->knobs.treelet_cap = atol(e);
  if (const char* e = getenv("MI355RT_TREELET_ORDER")) c->treelet_order = e[0] == 'w' ? 0 : (e[0] == 'i' ? 1 : 2);
  if (const char* e = getenv("MI355RT_WALK")) c->knobs.walk = (e[0] == 'n' || e[0] == '0') ? 0 : ((e[0] == 'a' || e[0] == '2') ? 2 : 1);   // node / pairs / auto
  if (const char* e = getenv("MI355RT_WF_RAYREG")) c->knobs.wf_rayreg = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("MI355RT_PRIMARY_ROUNDS")) c->knobs.primary_rounds = (uint32_t)std::max(0, std::min(64, atoi(e)));
  if (const char* e = getenv("MI355RT_WF_BLOCKS_PER_CU")) {
    const int b = atoi(e);
    if (b >= 1 && b <= 8) c->knobs.wf_blocks_per_cu = b;
  }
  // counters: 2 banks (primary kernel, path-trace kernel) x RT_COUNTER_SHARDS x 6 u64
  if (hipMalloc(&c->counters.ptr, 2 * RT_COUNTER_SHARDS * 6 * sizeof(uint64_t)) != hipSuccess) {
    g_create_error = "hipMalloc(counters) failed";
    delete c;
    return nullptr;
  }
  c->counters.capacity = c->counters.size = 2 * RT_COUNTER_SHARDS * 6 * sizeof(uint64_t);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0)
      c->num_cus = prop.multiProcessorCount;
    c->knobs.n_cus = (uint32_t)c->num_cus;
    (void)hipMalloc(&c->ticket.ptr, 256);
    c->ticket.capacity = c->ticket.size = 256;
  }
  (void)hipMemsetAsync(c->counters.ptr, 0, c->counters.size, c->stream);
  // lights buffer exists from the start with one dummy entry so that light_count == 0 scenes run
  (void)hipMalloc(&c->lights.ptr, 16);
  c->lights.capacity = 16;
  (void)hipMemsetAsync(c->lights.ptr, 0, 16, c->stream);
  (void)hipStreamSynchronize(c->stream);
  return c;
}

void rt_destroy(rt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  dist_release(c);
  delete c;   // everything else goes with its owner (device_owned.h), the streams last
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->error.c_str() : g_create_error.c_str(); }

int rt_set_pipeline(rt_ctx* c, uint32_t max_depth, uint32_t spp) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  if (spp == 0) return fail(c, RT_ERR_INVALID, "SPP must be >= 1");
  c->max_depth = max_depth;
  c->spp = spp;
  c->pipeline_built = true;
  return RT_OK;
}

int rt_resize(rt_ctx* c, uint32_t width, uint32_t height) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead) ...
  // ... and what rt_read_gbuffer remembers of them: their planes are freed / sized for the old screen below
  c->gbuf_slot = -1;
  c->spec.valid = false;
  c->spec.slots.clear();
  // 65535: the persistent kernel packs a pixel's x and y into one word (WebGPU's maxTextureDimension2D is 8192)
  if (width == 0 || height == 0 || width > 65535u || height > 65535u || (uint64_t)width * height > (1ull << 28))
    return fail(c, RT_ERR_INVALID, "invalid screen size");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)width * height;
  // updateScreenSize destroys and recreates every screen resource (ResourceManager.ts:97-142);
  // new WebGPU resources are zero-initialised.
  struct {
    DeviceBuffer* b;
    size_t bytes;
  } items[] = {{&c->accum, n * 16}, {&c->render_target, n * 4}, {&c->g_normal, n * 16},
               {&c->g_depth, n * 4}, {&c->history[0], n * 8},   {&c->history[1], n * 8}};
  for (auto& it : items) {
    it.b->reset();
    int r = ensure_buffer(c, *it.b, it.bytes, false);
    if (r < 0) return r;
    HIP_TRY(c, hipMemsetAsync(it.b->ptr, 0, it.bytes, c->stream));
  }
  c->width = width;
  c->height = height;
  // the frame denoiser's images were sized for the old screen, and the new G-buffer is empty
  for (DeviceBuffer* b : {&c->fd.col, &c->fd.guide, &c->fd.mod, &c->fd.ping, &c->fd.pong, &c->fd.out, &c->fd.albedo_keep}) b->reset();
  c->fd.cache_valid = c->fd.keep_valid = false;
  for (DeviceBuffer* b : {&c->ft.hist[0], &c->ft.hist[1], &c->ft.mom[0], &c->ft.mom[1], &c->ft.guide[0], &c->ft.guide[1], &c->ft.integ})
    b->reset();
  for (DeviceBuffer* b : {&c->fm.carry, &c->fm.pix_id[0], &c->fm.pix_id[1]}) b->reset();
  c->fm.ran = false;
  c->ft.have = false;
  c->ft.frames = 0;
  c->gbuf_gen = 0;
  c->albedo_plane_valid = false;
  // A bound accumulation / present buffer was sized for the old screen: it is dropped, and until the caller binds
  // again (rt_bind_accum / rt_bind_present_source, NULL included) compute() and present() refuse to run instead of
  // silently rendering into the internal buffer while the caller keeps reducing its stale one.
  if (c->external_accum) c->accum_stale = true;
  if (c->present_source) c->present_stale = true;
  c->external_accum = nullptr;
  c->present_source = nullptr;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->dist.active) return dist_alloc(c);   // a rank's blocks and display buffer follow the screen on their own
  return RT_OK;
}

int rt_reset_accum(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (!c->accum.ptr) return RT_OK;  // `if (!this.accumulateBuffer) return;`
  c->fd.cache_valid = false;   // the frame denoiser's colour image was made from the old accumulation
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(accum_ptr(c), 0, (size_t)c->width * c->height * 16, c->stream));
  return RT_OK;
}

int rt_upload_textures(rt_ctx* c, const uint8_t* rgba, uint32_t layers) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  HIP_TRY(c, hipSetDevice(c->device));
  if (layers == 0) {
    c->tex_layers = 0;
    return RT_OK;
  }
  if (!rgba) return fail(c, RT_ERR_INVALID, "null texture data");
  const size_t bytes = (size_t)layers * RT_TEX_SIZE * RT_TEX_SIZE * 4;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->textures.reset();
  int r = ensure_buffer(c, c->textures, bytes, false);
  if (r < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(c->textures.ptr, rgba, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tex_layers = layers;
  return RT_OK;
}

int rt_alloc_texture_layers(rt_ctx* c, uint32_t layers) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  HIP_TRY(c, hipSetDevice(c->device));
  if (layers == 0) {
    c->tex_layers = 0;
    return RT_OK;
  }
  const size_t bytes = (size_t)layers * RT_TEX_SIZE * RT_TEX_SIZE * 4;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->textures.reset();
  int r = ensure_buffer(c, c->textures, bytes, false);
  if (r < 0) return r;
  HIP_TRY(c, hipMemsetAsync(c->textures.ptr, 0xff, bytes, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tex_layers = layers;
  return RT_OK;
}

int rt_upload_texture_image(rt_ctx* c, uint32_t layer, const uint8_t* rgba, uint32_t width, uint32_t height) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  if (layer >= c->tex_layers || !c->textures.ptr) return fail(c, RT_ERR_INVALID, "texture layer out of range");
  if (rgba && (width == 0 || height == 0 || width > 32768u || height > 32768u))
    return fail(c, RT_ERR_INVALID, "texture image size out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t* dst = (uint32_t*)c->textures.ptr + (size_t)layer * RT_TEX_SIZE * RT_TEX_SIZE;
  const uint32_t* src = nullptr;
  if (rgba) {
    const size_t bytes = (size_t)width * height * 4;
    int r = ensure_buffer(c, c->tex_staging, bytes, false);
    if (r < 0) return r;
    HIP_TRY(c, hipMemcpyAsync(c->tex_staging.ptr, rgba, bytes, hipMemcpyHostToDevice, c->stream));
    src = (const uint32_t*)c->tex_staging.ptr;
  }
  hipLaunchKernelGGL(rtk::k_resize_texture, dim3(RT_TEX_SIZE / 256, RT_TEX_SIZE), dim3(256), 0, c->stream, src, width, height,
                     dst);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller may free `rgba` and the staging buffer is reused
  return RT_OK;
}

int rt_read_texture_layer(rt_ctx* c, uint32_t layer, uint8_t* out, size_t cap) {
  if (!c || !out) return RT_ERR_INVALID;
  const size_t bytes = (size_t)RT_TEX_SIZE * RT_TEX_SIZE * 4;
  if (layer >= c->tex_layers || !c->textures.ptr) return fail(c, RT_ERR_INVALID, "texture layer out of range");
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "buffer too small for a texture layer");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, (const uint8_t*)c->textures.ptr + (size_t)layer * bytes, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

// ---- binned-SAH BLAS build on the GPU (csrc/bvh_build.hip.h) ----
// Work space of one build of n triangles (shared by successive builds: they run one after the other on c->stream).
static int blas_workspace(rt_ctx* c, uint32_t n_tris, bvhb::Build& B, bvhb::BigNode*& d_big, bvhb::Chunk*& d_chunks, uint32_t*& d_cnt,
                          uint32_t*& d_base, uint32_t*& d_lb, uint32_t*& d_blk) {
  const size_t n = n_tris, max_nodes = 2 * n;  // a binary tree with >= 1 triangle per leaf has < 2n nodes
  const size_t n_blk = (n + 1023) / 1024 + 1;
  int r;
  if ((r = ensure_buffer(c, c->bv_tri, n * 48, false)) < 0) return r;
  // ord[0], ord[1], order_final, scratch_l, scratch_r, leaf_flag, small_ids, lb (n + 1), block counts; bin cache (bytes)
  if ((r = ensure_buffer(c, c->bv_order, (8 * n + 4 + n_blk) * 4 + n + 16, false)) < 0) return r;
  // node records: ids [0, 2n) of the level kernels, [2n, 4n) blocks of the in-wave subtrees; a fresh array is zeroed once
  // (records carry the stamp of the build that made them, stamps start at 1)
  if ((r = ensure_buffer(c, c->bv_nodes, 2 * max_nodes * sizeof(bvhb::BNode), false)) < 0) return r;
  if (r > 0) HIP_TRY(c, hipMemsetAsync(c->bv_nodes.ptr, 0, c->bv_nodes.capacity, c->stream));
  if ((r = ensure_buffer(c, c->bv_counters, sizeof(bvhb::Ctl), false)) < 0) return r;
  const uint32_t nb = bvhb::big_cap(n_tris), nc = bvhb::chunk_cap(n_tris);
  if ((r = ensure_buffer(c, c->bv_big, (size_t)nb * sizeof(bvhb::BigNode) + (size_t)nc * (sizeof(bvhb::Chunk) + 16), false)) < 0) return r;
  float4* tri = (float4*)c->bv_tri.ptr;
  uint32_t* ord = (uint32_t*)c->bv_order.ptr;
  B.tri_mn = tri;
  B.tri_mx = tri + n;
  B.tri_c = tri + 2 * n;
  B.ord[0] = ord;
  B.ord[1] = ord + n;
  B.order_final = ord + 2 * n;
  B.scratch_l = ord + 3 * n;
  B.scratch_r = ord + 4 * n;
  B.leaf_flag = ord + 5 * n;
  B.small_ids = ord + 6 * n;
  d_lb = ord + 7 * n;              // n + 1 entries
  d_blk = ord + 8 * n + 4;
  B.bin_cache = (uint8_t*)(d_blk + n_blk);
  B.nodes = (bvhb::BNode*)c->bv_nodes.ptr;
  B.ctl = (bvhb::Ctl*)c->bv_counters.ptr;
  B.n_tris = n_tris;
  B.gen = ++c->bv_gen;
  if (B.gen == 0u) {   // stamp wrap-around: forget every old record
    HIP_TRY(c, hipMemsetAsync(c->bv_nodes.ptr, 0, c->bv_nodes.capacity, c->stream));
    B.gen = c->bv_gen = 1u;
  }
  d_big = (bvhb::BigNode*)c->bv_big.ptr;
  d_chunks = (bvhb::Chunk*)(d_big + nb);
  d_cnt = (uint32_t*)(d_chunks + nc);
  d_base = d_cnt + 2 * (size_t)nc;
  return RT_OK;
}
static uint32_t ceil_log2(uint32_t v) {
  uint32_t l = 0;
  while (l < 32u && (1ull << l) < v) l++;
  return l;
}
// first guesses for a mesh never built before: tree depth and the levels that still hold a node above kBig triangles
static uint32_t blas_guess_levels(uint32_t n_tris) { return std::min<uint32_t>(bvhb::kMaxLevels, ceil_log2(std::max(n_tris / 4u, 1u)) + 8u); }
static uint32_t blas_guess_big_levels(uint32_t n_tris) { return n_tris > bvhb::kBig ? ceil_log2((n_tris + bvhb::kBig - 1) / bvhb::kBig) + 3u : 0u; }

// Enqueue one whole build on c->stream: `levels` tree levels (the first `big_levels` with the large-node kernels), the
// leaf prefix sum and the node array, written to out + 2 * node_base[0] (node_base, device: [1] = [0] + node count is
// written; NULL: at out).  Nothing is read back: the caller checks Ctl::cnt[levels] == 0 (the tree was not deeper)
// whenever it next synchronises.  d_pos / d_idx / out are device pointers.
static int blas_enqueue(rt_ctx* c, const float4* d_pos, const uint32_t* d_idx, uint32_t n_tris, uint32_t levels, uint32_t big_levels,
                        float4* out, uint32_t* node_base, uint32_t topo_start, bvhb::Build& B) {
  bvhb::BigNode* d_big;
  bvhb::Chunk* d_chunks;
  uint32_t *d_cnt, *d_base, *d_lb, *d_blk;
  int r = blas_workspace(c, n_tris, B, d_big, d_chunks, d_cnt, d_base, d_lb, d_blk);
  if (r < 0) return r;
  levels = std::min<uint32_t>(levels, bvhb::kMaxLevels);
  big_levels = std::min(big_levels, levels);
  hipLaunchKernelGGL(bvhb::k_tri_boxes, dim3((n_tris + 255) / 256), dim3(256), 0, c->stream, d_pos, d_idx, n_tris, B);
  const dim3 gn_thread((bvhb::big_cap(n_tris) + 63) / 64), gn_wave(bvhb::big_cap(n_tris)), gc(bvhb::chunk_cap(n_tris));
  for (uint32_t level = 0; level < levels; level++) {
    const uint32_t bound = level >= 31u ? n_tris : std::min<uint32_t>(1u << level, n_tris);   // most nodes the level can have
    if (level < big_levels) {
      hipLaunchKernelGGL(bvhb::k_big_plan, dim3(1), dim3(1024), 0, c->stream, B, level, d_big, d_chunks);
      if (level == 0)  // only the root reduces its box; children get theirs from the parent's sweep
        hipLaunchKernelGGL(bvhb::k_big_bounds, gc, dim3(256), 0, c->stream, B, level, d_big, (const bvhb::Chunk*)d_chunks);
      hipLaunchKernelGGL(bvhb::k_big_setup, gn_thread, dim3(64), 0, c->stream, B, d_big);
      hipLaunchKernelGGL(bvhb::k_big_bin, gc, dim3(256), 0, c->stream, B, level, d_big, (const bvhb::Chunk*)d_chunks);
      hipLaunchKernelGGL(bvhb::k_big_split, gn_wave, dim3(64), 0, c->stream, B, d_big);
      hipLaunchKernelGGL(bvhb::k_big_count, gc, dim3(256), 0, c->stream, B, (const bvhb::BigNode*)d_big, (const bvhb::Chunk*)d_chunks, d_cnt);
      hipLaunchKernelGGL(bvhb::k_big_scan, gn_thread, dim3(64), 0, c->stream, B, d_big, (const uint32_t*)d_cnt, d_base);
      hipLaunchKernelGGL(bvhb::k_big_scatter, gc, dim3(256), 0, c->stream, B, (const bvhb::BigNode*)d_big, (const bvhb::Chunk*)d_chunks,
                         (const uint32_t*)d_cnt, (const uint32_t*)d_base);
      hipLaunchKernelGGL(bvhb::k_big_swap, gc, dim3(256), 0, c->stream, B, level, (const bvhb::BigNode*)d_big, (const bvhb::Chunk*)d_chunks);
      hipLaunchKernelGGL(bvhb::k_big_copy, gc, dim3(256), 0, c->stream, B, level, (const bvhb::BigNode*)d_big, (const bvhb::Chunk*)d_chunks);
      hipLaunchKernelGGL((bvhb::k_level<256, true>), dim3(std::min<uint32_t>(bound, 1024u)), dim3(256), 0, c->stream, B, level);
    } else if (level < big_levels + 3u) {
      hipLaunchKernelGGL((bvhb::k_level<256, false>), dim3(std::min<uint32_t>(bound, 2048u)), dim3(256), 0, c->stream, B, level);
    } else {
      // deep levels: tens of thousands of nodes of a few dozen triangles — one wave per node keeps four times as many
      // nodes in flight per CU
      hipLaunchKernelGGL((bvhb::k_level<64, false>), dim3(std::min<uint32_t>(bound, 8192u)), dim3(64), 0, c->stream, B, level);
    }
  }
  const uint32_t n_blk = (n_tris + 1023u) / 1024u;
  hipLaunchKernelGGL(bvhb::k_scan_blocks, dim3(n_blk), dim3(1024), 0, c->stream, (const uint32_t*)B.leaf_flag, n_tris, d_blk);
  hipLaunchKernelGGL(bvhb::k_scan_top, dim3(1), dim3(1024), 0, c->stream, d_blk, n_blk, B.ctl, node_base);
  hipLaunchKernelGGL(bvhb::k_scan_apply, dim3(n_blk), dim3(1024), 0, c->stream, (const uint32_t*)B.leaf_flag, n_tris, (const uint32_t*)d_blk,
                     (const bvhb::Ctl*)B.ctl, d_lb);
  hipLaunchKernelGGL(bvhb::k_emit, dim3((4 * n_tris + 255) / 256), dim3(256), 0, c->stream, (const bvhb::BNode*)B.nodes, 4u * n_tris, B.gen,
                     (const bvhb::Ctl*)B.ctl, (const uint32_t*)d_lb, (const uint32_t*)node_base, topo_start, out);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

// The tree and the triangle order of the scene compiler's BlasBuilder, byte for byte.  Host arrays in, host arrays out
// (the scene compiler's ms_blas_builder hook; the device-resident update, rt_world_update, uses blas_enqueue directly).
int rt_build_blas(rt_ctx* c, const float* verts4, uint32_t n_verts, const uint32_t* indices, uint32_t n_tris, float* nodes_out,
                  uint32_t nodes_cap, uint32_t* n_nodes_out, uint32_t* order_out) {
  if (!c || !n_nodes_out) return RT_ERR_INVALID;
  *n_nodes_out = 0;
  if (n_tris == 0) return RT_OK;
  if (!verts4 || !indices || !nodes_out || !order_out || n_verts == 0) return fail(c, RT_ERR_INVALID, "rt_build_blas: null argument");
  if (n_tris > (1u << 28)) return fail(c, RT_ERR_INVALID, "rt_build_blas: too many triangles for the 29-bit leaf field");
  for (size_t i = 0; i < (size_t)n_tris * 3; i++)
    if (indices[i] >= n_verts) return fail(c, RT_ERR_INVALID, "rt_build_blas: vertex index out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = n_tris;
  int r;
  if ((r = ensure_buffer(c, c->bv_in, (size_t)n_verts * 16 + n * 12, false)) < 0) return r;
  if ((r = ensure_buffer(c, c->bv_out, 2 * n * 32, false)) < 0) return r;
  float4* d_pos = (float4*)c->bv_in.ptr;
  uint32_t* d_idx = (uint32_t*)((char*)c->bv_in.ptr + (size_t)n_verts * 16);
  HIP_TRY(c, hipMemcpyAsync(d_pos, verts4, (size_t)n_verts * 16, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_idx, indices, n * 12, hipMemcpyHostToDevice, c->stream));
  if (!c->bv_pinned) HIP_TRY(c, hipHostMalloc(&c->bv_pinned, 1 << 16, hipHostMallocDefault));
  bvhb::Ctl* ctl = (bvhb::Ctl*)c->bv_pinned.h;
  // as many levels as the last build of a mesh of this size needed (+ 2), else a guess; a deeper tree is built again
  uint32_t levels = (c->bv_levels && c->bv_last_tris == n_tris) ? c->bv_levels + 2u : blas_guess_levels(n_tris);
  uint32_t big_levels = (c->bv_levels && c->bv_last_tris == n_tris) ? c->bv_big_levels : blas_guess_big_levels(n_tris);
  bvhb::Build B;
  for (;;) {
    levels = std::min<uint32_t>(levels, bvhb::kMaxLevels);
    if ((r = blas_enqueue(c, d_pos, d_idx, n_tris, levels, big_levels, (float4*)c->bv_out.ptr, nullptr, 0u, B)) < 0) return r;
    HIP_TRY(c, hipMemcpyAsync(ctl, B.ctl, sizeof(bvhb::Ctl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ctl->cnt[levels] == 0u) break;
    if (levels >= bvhb::kMaxLevels) return fail(c, RT_ERR_INVALID, "rt_build_blas: the tree is deeper than 1024 levels");
    levels = levels * 2u + 8u;
  }
  const uint32_t total = ctl->n_nodes;
  if (total > 2 * n) return fail(c, RT_ERR_INTERNAL, "rt_build_blas: node bookkeeping broke");
  if (total > nodes_cap) return fail(c, RT_ERR_INVALID, "rt_build_blas: node buffer too small");
  HIP_TRY(c, hipMemcpyAsync(nodes_out, c->bv_out.ptr, (size_t)total * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(order_out, B.order_final, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_nodes_out = total;
  uint32_t depth = 0;
  while (depth < bvhb::kMaxLevels && ctl->cnt[depth]) depth++;
  c->bv_levels = depth;
  c->bv_big_levels = ctl->big_levels;
  c->bv_last_tris = n_tris;
  return RT_OK;
}

// ---- device-resident World::update(t): include/mi355rt.h rt_world_update, kernels in csrc/world_update.hip.h ----
// (Re)build the static side: the skinning input, index lists and attribute rows of every geometry and the instance list
// go to the device once per static_epoch; the scene buffers are sized for the whole world.
static int world_make_static(rt_ctx* c, const rt_world_frame* f) {
  auto& W = c->world;
  W.valid = false;
  W.static_cached = false;
  if (!f->n_instances || !f->instances || (f->n_geometries && !f->geometries))
    return fail(c, RT_ERR_INVALID, "rt_world_update: empty scene description");
  const uint32_t G = f->n_geometries, N = f->n_instances;
  if (N > RT_TLAS_MAX_INSTANCES)   // k_tlas sorts the ranges of a depth in LDS: 16 384 64-bit keys are 128 KB of the CU's 160
    return fail(c, RT_ERR_INVALID, "rt_world_update: more than 16 384 instances are not taken by the device path");
  // layout of the static buffer (256-byte aligned arrays) and the world's totals
  size_t bytes = 0;
  auto take = [&](size_t n) { size_t o = bytes; bytes += (n + 255) & ~(size_t)255; return o; };
  struct Off { size_t pos, nrm, uv, joints, weights, idx, attr; };
  std::vector<Off> off(G);
  W.geoms.assign(G, wu::Geom());
  uint64_t verts = 0, tris = 0, lights = 0;
  std::vector<uint32_t> em_count(G, 0u);
  for (uint32_t g = 0; g < G; g++) {
    const rt_world_geometry& d = f->geometries[g];
    if (d.n_verts && (!d.positions || !d.normals || !d.joints || !d.weights)) return fail(c, RT_ERR_INVALID, "rt_world_update: null vertex array");
    if (d.n_tris && (!d.indices || !d.attributes)) return fail(c, RT_ERR_INVALID, "rt_world_update: null triangle array");
    if (d.n_uvs > d.n_verts || (d.n_uvs && !d.uvs)) return fail(c, RT_ERR_INVALID, "rt_world_update: bad uv array");
    if (d.n_verts && !d.n_tris) return fail(c, RT_ERR_INVALID, "rt_world_update: a geometry with vertices and no triangles is not supported on the device");
    if (d.n_tris > (1u << 28)) return fail(c, RT_ERR_INVALID, "rt_world_update: too many triangles for the 29-bit leaf field");
    if (d.skin >= 0 && (uint32_t)d.skin >= f->n_skins) return fail(c, RT_ERR_INVALID, "rt_world_update: skin index out of range");
    for (size_t k = 0; k < (size_t)d.n_tris * 3; k++)
      if (d.indices[k] >= d.n_verts) return fail(c, RT_ERR_INVALID, "rt_world_update: vertex index out of range");
    for (uint32_t t = 0; t < d.n_tris; t++) em_count[g] += std::fabs(d.attributes[(size_t)t * 16 + 3] - 3.0f) < 1e-6f ? 1u : 0u;
    off[g].pos = take((size_t)d.n_verts * 12);
    off[g].nrm = take((size_t)d.n_verts * 12);
    off[g].uv = take((size_t)d.n_uvs * 8);
    off[g].joints = take((size_t)d.n_verts * 16);
    off[g].weights = take((size_t)d.n_verts * 16);
    off[g].idx = take((size_t)d.n_tris * 12);
    off[g].attr = take((size_t)d.n_tris * 64);
    wu::Geom& D = W.geoms[g];
    D.n_verts = d.n_verts;
    D.n_uvs = d.n_uvs;
    D.n_tris = d.n_tris;
    D.v_offset = (uint32_t)verts;
    D.topo_start = (uint32_t)tris;
    D.skinned = d.skin >= 0 ? 1u : 0u;
    D.joint_first = D.n_joints = 0u;   // per frame (skin_first)
    D.em_count = em_count[g];
    D.em_first = 0u;
    D.pad0 = (uint32_t)(d.skin >= 0 ? d.skin : 0);   // the skin's index, for the per-frame joint range
    D.pad1 = 0u;
    verts += d.n_verts;
    tris += d.n_tris;
  }
  if (!verts || !tris) return fail(c, RT_ERR_INVALID, "rt_world_update: the world has no triangles");
  if (verts > 0xfffffff0ull || tris > (1ull << 28)) return fail(c, RT_ERR_INVALID, "rt_world_update: world too large");
  W.inst_geom.assign(N, 0u);
  W.inst_scale2.assign(N, 1.0f);
  for (uint32_t i = 0; i < N; i++) {
    const rt_instance& I = f->instances[i];
    if (I.instance_id >= G || !f->geometries[I.instance_id].n_tris)
      return fail(c, RT_ERR_INVALID, "rt_world_update: an instance of a missing or empty geometry is not supported on the device");
    W.inst_geom[i] = I.instance_id;
    lights += em_count[I.instance_id];
    const float* m = I.transform;   // column-major 4x4: squared linear scale = |det(M3x3)|^(2/3), as in rt_upload
    const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[4] * ((double)m[1] * m[10] - (double)m[2] * m[9]) +
                       (double)m[8] * ((double)m[1] * m[6] - (double)m[2] * m[5]);
    double s2 = std::pow(std::fabs(det), 2.0 / 3.0);
    if (!(s2 > 0.0) || !std::isfinite(s2)) s2 = 1.0;
    W.inst_scale2[i] = (float)s2;
  }
  if (lights > 0x7fffffffull) return fail(c, RT_ERR_INVALID, "rt_world_update: too many lights");
  HIP_TRY(c, hipSetDevice(c->device));
  int r;
  if ((r = ensure_buffer(c, W.stat, std::max<size_t>(bytes, 256), false)) < 0) return r;
  char* base = (char*)W.stat.ptr;
  uint32_t em_first = 0, max_tris = 0;
  std::vector<wu::GeomRow> rows(G);
  for (uint32_t g = 0; g < G; g++) {
    const rt_world_geometry& d = f->geometries[g];
    wu::Geom& D = W.geoms[g];
    auto put = [&](size_t o, const void* src, size_t n) -> hipError_t {
      return n ? hipMemcpyAsync(base + o, src, n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIP_TRY(c, put(off[g].pos, d.positions, (size_t)d.n_verts * 12));
    HIP_TRY(c, put(off[g].nrm, d.normals, (size_t)d.n_verts * 12));
    HIP_TRY(c, put(off[g].uv, d.uvs, (size_t)d.n_uvs * 8));
    HIP_TRY(c, put(off[g].joints, d.joints, (size_t)d.n_verts * 16));
    HIP_TRY(c, put(off[g].weights, d.weights, (size_t)d.n_verts * 16));
    HIP_TRY(c, put(off[g].idx, d.indices, (size_t)d.n_tris * 12));
    HIP_TRY(c, put(off[g].attr, d.attributes, (size_t)d.n_tris * 64));
    D.pos3 = (const float*)(base + off[g].pos);
    D.nrm3 = (const float*)(base + off[g].nrm);
    D.uv2 = (const float*)(base + off[g].uv);
    D.joints = (const uint32_t*)(base + off[g].joints);
    D.weights = (const float*)(base + off[g].weights);
    D.idx = (const uint32_t*)(base + off[g].idx);
    D.attr = (const float*)(base + off[g].attr);
    D.em_first = em_first;
    em_first += D.em_count;
    max_tris = std::max(max_tris, D.n_tris);
    rows[g] = wu::GeomRow{D.n_tris, D.topo_start, D.em_count, D.em_first};
  }
  const uint32_t n_tlas = 2u * N - 1u;
  if ((r = ensure_buffer(c, W.raw_inst, (size_t)N * sizeof(rt_instance), false)) < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(W.raw_inst.ptr, f->instances, (size_t)N * sizeof(rt_instance), hipMemcpyHostToDevice, c->stream));
  if ((r = ensure_buffer(c, W.geom_rows, std::max<size_t>(16, (size_t)G * sizeof(wu::GeomRow)), false)) < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(W.geom_rows.ptr, rows.data(), (size_t)G * sizeof(wu::GeomRow), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // the sources above belong to the caller
  if ((r = ensure_buffer(c, W.node_base, ((size_t)G + 1) * 4, false)) < 0) return r;
  if ((r = ensure_buffer(c, W.stats, std::max<size_t>(64, (size_t)G * 16 + 16), false)) < 0) return r;
  if ((r = ensure_buffer(c, W.em_flag, (size_t)max_tris * 4, false)) < 0) return r;
  if ((r = ensure_buffer(c, W.em_blk, ((size_t)max_tris / 1024 + 2) * 4, false)) < 0) return r;
  if ((r = ensure_buffer(c, W.em_list, std::max<size_t>(16, (size_t)em_first * 4), false)) < 0) return r;
  // k_tlas scratch: box 6, ctr 3, ord 1, ord2 1, seg 3, skey 18, sinfo 2, light_off 1 words per instance + 4 status words
  if ((r = ensure_buffer(c, W.tlas_scratch, ((size_t)N * 35 + 4) * 4, false)) < 0) return r;
  // the renderer's scene buffers, sized for the whole world (node array: TLAS + at most 2 n - 1 nodes per geometry)
  size_t max_nodes = n_tlas;
  for (uint32_t g = 0; g < G; g++) max_nodes += W.geoms[g].n_tris ? 2 * (size_t)W.geoms[g].n_tris - 1 : 0;
  bool grew = false;
  auto scene_buffer = [&](DeviceBuffer& b, size_t n) -> int {
    int rr = ensure_buffer(c, b, n, true);
    if (rr > 0) grew = true;
    return rr;
  };
  if ((r = scene_buffer(c->pos, (size_t)verts * 16)) < 0) return r;
  if ((r = scene_buffer(c->nrm, (size_t)verts * 16)) < 0) return r;
  if ((r = scene_buffer(c->uv, (size_t)verts * 8)) < 0) return r;
  if ((r = scene_buffer(c->topology, (size_t)tris * sizeof(rt_topology))) < 0) return r;
  if ((r = scene_buffer(c->nodes, max_nodes * sizeof(rt_node))) < 0) return r;
  if ((r = scene_buffer(c->instances, (size_t)N * sizeof(rt_instance))) < 0) return r;
  if ((r = scene_buffer(c->lights, std::max<size_t>(16, (size_t)lights * sizeof(rt_light_ref)))) < 0) return r;
  if ((r = ensure_buffer(c, c->draw_commands, (size_t)N * 16, false)) < 0) return r;
  if (!W.ev0) HIP_TRY(c, hipEventCreate(&W.ev0));
  if (!W.ev1) HIP_TRY(c, hipEventCreate(&W.ev1));
  if (!W.ev_t0) HIP_TRY(c, hipEventCreate(&W.ev_t0));
  if (!W.ev_t1) HIP_TRY(c, hipEventCreate(&W.ev_t1));
  W.levels.assign(G, 0u);
  W.big_levels.assign(G, 0u);
  for (uint32_t g = 0; g < G; g++) {
    W.levels[g] = blas_guess_levels(W.geoms[g].n_tris);
    W.big_levels[g] = blas_guess_big_levels(W.geoms[g].n_tris);
  }
  W.any_skinned = false;
  for (uint32_t g = 0; g < G; g++) W.any_skinned = W.any_skinned || (W.geoms[g].n_verts && W.geoms[g].skinned);
  W.n_verts = (uint32_t)verts;
  W.n_tris = (uint32_t)tris;
  W.n_lights = (uint32_t)lights;
  W.n_tlas = n_tlas;
  W.n_inst = N;
  uint32_t* ts = (uint32_t*)W.tlas_scratch.ptr;
  wu::TlasArgs& A = W.tlas;
  A.raw = (const float4*)W.raw_inst.ptr;
  A.geoms = (const wu::GeomRow*)W.geom_rows.ptr;
  A.node_base = (const uint32_t*)W.node_base.ptr;
  A.box = (float*)ts;
  A.ctr = (float*)(ts + (size_t)N * 6);
  A.ord = ts + (size_t)N * 9;
  A.ord2 = ts + (size_t)N * 10;
  A.seg = ts + (size_t)N * 11;
  A.skey = ts + (size_t)N * 14;
  A.sinfo = ts + (size_t)N * 32;
  A.light_off = ts + (size_t)N * 34;
  A.status = ts + (size_t)N * 35;
  A.n_inst = N;
  A.n_tlas = n_tlas;
  A.n_lights = (uint32_t)lights;
  A.pad = 0;
  W.epoch = f->static_epoch;
  W.n_skins = f->n_skins;
  W.valid = true;
  return grew ? RT_REALLOCATED : RT_OK;
}

// *touched is set before the first kernel that writes into the live scene buffers is enqueued
static int world_update_body(rt_ctx* c, const rt_world_frame* f, bool* touched) {
  auto& W = c->world;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  c->fm.scene_gen++;
  c->facts = lp::SceneFacts();   // the topology records are (re)made on the device, or their buffer is resized: the host has not seen them
  walk_forget(c);                // ... nor the nodes and the instances
  HIP_TRY(c, hipSetDevice(c->device));
  int r, ret = RT_OK;
  if (!W.valid || W.epoch != f->static_epoch) {
    if ((r = world_make_static(c, f)) < 0) return r;
    ret = r;
  }
  const uint32_t G = (uint32_t)W.geoms.size(), N = W.n_inst;
  if (f->n_geometries != G || f->n_instances != N) return fail(c, RT_ERR_INVALID, "rt_world_update: the scene changed under an unchanged static_epoch");
  if (W.cache_enabled && W.static_cached && !W.any_skinned) {
    // nothing in this world moves: every array of this frame is the one the last update left in the scene buffers (and the
    // renderer's derived records are those of that scene) - World::update would rebuild all of it to the same bytes
    W.last_ms = 0.0;
    return ret;
  }
  // this frame's joint matrices: the per-frame arguments are checked against the static description on every call (a
  // direct C-ABI caller may hand anything): the skin table must be the one the geometries' skin indices were checked against
  if (f->n_skins != W.n_skins) return fail(c, RT_ERR_INVALID, "rt_world_update: the number of skins changed under an unchanged static_epoch");
  if (f->n_skins && !f->skin_first) return fail(c, RT_ERR_INVALID, "rt_world_update: null skin table");
  for (uint32_t k = 0; k < f->n_skins; k++)
    if (f->skin_first[k + 1] < f->skin_first[k]) return fail(c, RT_ERR_INVALID, "rt_world_update: the skin table is not non-decreasing");
  if (f->n_skins && f->skin_first[0] != 0u) return fail(c, RT_ERR_INVALID, "rt_world_update: the skin table does not start at joint 0");
  const uint32_t n_joints = f->n_skins ? f->skin_first[f->n_skins] : 0u;
  if (n_joints && !f->joint_mats) return fail(c, RT_ERR_INVALID, "rt_world_update: null joint matrices");
  const size_t joint_bytes = (size_t)n_joints * 64;
  if ((r = ensure_buffer(c, W.joints, std::max<size_t>(64, joint_bytes), false)) < 0) return r;
  // pinned staging: the end-of-update read-back (node_base, per-geometry stats, k_tlas status, TLAS root), then the joints
  const size_t rb_bytes = (((size_t)G + 1) * 4 + (size_t)G * 16 + 16 + 32 + 4095) & ~(size_t)4095;
  if (rb_bytes + joint_bytes > W.pinned_bytes) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    (void)W.pinned.reset();
    W.pinned_bytes = 0;
    HIP_TRY(c, hipHostMalloc(&W.pinned, (rb_bytes + joint_bytes) * 2 + 65536, hipHostMallocDefault));
    W.pinned_bytes = (rb_bytes + joint_bytes) * 2 + 65536;
  }
  char* pinned_rb = (char*)W.pinned.h;
  char* pinned_joints = (char*)W.pinned.h + rb_bytes;
  for (uint32_t g = 0; g < G; g++) {
    wu::Geom& D = W.geoms[g];
    if (D.skinned) {
      const uint32_t si = D.pad0;
      D.joint_first = f->skin_first[si];
      D.n_joints = f->skin_first[si + 1] - f->skin_first[si];
    }
  }
  uint32_t* d_node_base = (uint32_t*)W.node_base.ptr;
  uint32_t* d_stats = (uint32_t*)W.stats.ptr;
  float4* nodes = (float4*)c->nodes.ptr;
  for (int attempt = 0;; attempt++) {
    *touched = true;   // from here on the live scene buffers are being rewritten
    HIP_TRY(c, hipEventRecord(W.ev0, c->stream));
    if (joint_bytes) {
      std::memcpy(pinned_joints, f->joint_mats, joint_bytes);
      HIP_TRY(c, hipMemcpyAsync(W.joints.ptr, pinned_joints, joint_bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(d_node_base, 0, 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(W.tlas.status, 0, 16, c->stream));
    for (uint32_t g = 0; g < G; g++) {
      const wu::Geom& D = W.geoms[g];
      if (!D.n_verts) {   // an empty geometry owns no nodes: the next one starts where this one would
        HIP_TRY(c, hipMemcpyAsync(d_node_base + g + 1, d_node_base + g, 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(d_stats + 4 * (size_t)g, 0, 16, c->stream));
        continue;
      }
      if (W.cache_enabled && W.static_cached && !D.skinned) {   // same vertices as last frame: rows stay, nodes come from the cache
        const uint32_t cnt = W.static_count[g];
        hipLaunchKernelGGL(wu::k_static_nodes, dim3((2 * cnt + 255) / 256), dim3(256), 0, c->stream,
                           (const float4*)W.static_nodes.ptr + 2 * (size_t)W.static_off[g], cnt, d_node_base + g, nodes + 2 * (size_t)W.n_tlas);
        continue;
      }
      hipLaunchKernelGGL(wu::k_skin, dim3((D.n_verts + 255) / 256), dim3(256), 0, c->stream, D, (const float*)W.joints.ptr, (float4*)c->pos.ptr,
                         (float4*)c->nrm.ptr, (float2*)c->uv.ptr);
      bvhb::Build B;
      if ((r = blas_enqueue(c, (const float4*)c->pos.ptr + D.v_offset, D.idx, D.n_tris, W.levels[g], W.big_levels[g], nodes + 2 * (size_t)W.n_tlas,
                            d_node_base + g, D.topo_start, B)) < 0)
        return r;
      hipLaunchKernelGGL(wu::k_build_stats, dim3(1), dim3(1), 0, c->stream, (const bvhb::Ctl*)B.ctl, std::min<uint32_t>(W.levels[g], bvhb::kMaxLevels),
                         d_stats + 4 * (size_t)g);
      uint32_t* em_flag = D.em_count ? (uint32_t*)W.em_flag.ptr : nullptr;
      hipLaunchKernelGGL(wu::k_topology, dim3((D.n_tris + 255) / 256), dim3(256), 0, c->stream, D, g, (const uint32_t*)B.order_final,
                         (float4*)c->topology.ptr, em_flag);
      if (D.em_count) {
        const uint32_t n_blk = (D.n_tris + 1023u) / 1024u;
        hipLaunchKernelGGL(bvhb::k_scan_blocks, dim3(n_blk), dim3(1024), 0, c->stream, (const uint32_t*)em_flag, D.n_tris, (uint32_t*)W.em_blk.ptr);
        hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, (uint32_t*)W.em_blk.ptr, n_blk, (uint32_t*)nullptr);
        hipLaunchKernelGGL(wu::k_emissive_apply, dim3(n_blk), dim3(1024), 0, c->stream, D, (const uint32_t*)em_flag, (const uint32_t*)W.em_blk.ptr,
                           (uint32_t*)W.em_list.ptr);
      }
    }
    wu::TlasArgs A = W.tlas;
    A.nodes = nodes;
    A.inst_out = (float4*)c->instances.ptr;
    A.draw_out = (uint4*)c->draw_commands.ptr;
    {
      uint32_t m = 1024u;
      while (m < N) m <<= 1;
      if (!W.tlas_lds_set) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)wu::k_tlas, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(RT_TLAS_MAX_INSTANCES * 8u)));
        W.tlas_lds_set = true;
      }
      HIP_TRY(c, hipEventRecord(W.ev_t0, c->stream));
      if (N <= 1024u && !getenv("MI355RT_TLAS_GENERIC"))   // one position per lane, everything in LDS / registers (config 3: 1 001)
        hipLaunchKernelGGL(wu::k_tlas_small, dim3(1), dim3(1024), 0, c->stream, A);
      else
        hipLaunchKernelGGL(wu::k_tlas, dim3(1), dim3(1024), (size_t)m * 8, c->stream, A);
      HIP_TRY(c, hipEventRecord(W.ev_t1, c->stream));
    }
    if (W.n_lights)
      hipLaunchKernelGGL(wu::k_lights, dim3(N), dim3(256), 0, c->stream, A, (const uint32_t*)W.em_list.ptr, (uint2*)c->lights.ptr);
    HIP_TRY(c, hipGetLastError());
    // one read-back: where every BLAS starts, whether every tree was finished, the TLAS root
    uint32_t* rb_base = (uint32_t*)pinned_rb;
    uint32_t* rb_stats = rb_base + G + 1;
    uint32_t* rb_status = rb_stats + 4 * (size_t)G;
    float* rb_root = (float*)(rb_status + 4);
    HIP_TRY(c, hipMemcpyAsync(rb_base, d_node_base, ((size_t)G + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (G) HIP_TRY(c, hipMemcpyAsync(rb_stats, d_stats, (size_t)G * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rb_status, W.tlas.status, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rb_root, nodes, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(W.ev1, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bool again = false;
    const bool was_cached = W.cache_enabled && W.static_cached;
    for (uint32_t g = 0; g < G; g++) {
      if (!W.geoms[g].n_verts || (was_cached && !W.geoms[g].skinned)) continue;
      const uint32_t* st = rb_stats + 4 * (size_t)g;
      if (st[0]) {   // deeper than launched: build again with more levels
        if (W.levels[g] >= bvhb::kMaxLevels) return fail(c, RT_ERR_INVALID, "rt_world_update: a BLAS is deeper than 1024 levels");
        W.levels[g] = std::min<uint32_t>(bvhb::kMaxLevels, W.levels[g] * 2u + 8u);
        again = true;
      } else {
        W.levels[g] = std::min<uint32_t>(bvhb::kMaxLevels, st[1] + 2u);
        W.big_levels[g] = st[2];
      }
    }
    if (again) {
      if (attempt >= 8) return fail(c, RT_ERR_INTERNAL, "rt_world_update: BLAS depth did not settle");
      continue;
    }
    if (rb_status[0]) return fail(c, RT_ERR_INVALID, "rt_world_update: an instance box has a NaN centre; the host path defines this update");
    if (rb_status[1] != W.n_lights) return fail(c, RT_ERR_INTERNAL, "rt_world_update: light count mismatch");
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, W.ev0, W.ev1) == hipSuccess) W.last_ms = ms;
    if (hipEventElapsedTime(&ms, W.ev_t0, W.ev_t1) == hipSuccess) W.last_tlas_ms = ms;
    // ---- host bookkeeping, what rt_upload / rt_upload_geometry / rt_upload_bvh would have set
    const uint32_t n_blas = rb_base[G];
    c->n_verts = c->vertex_count = W.n_verts;
    c->n_tris = W.n_tris;
    c->n_instances = N;
    c->n_lights = W.n_lights;
    c->blas_offset = W.n_tlas;
    c->n_nodes = W.n_tlas + n_blas;
    c->pos.size = (size_t)W.n_verts * 16;
    c->nodes.size = (size_t)c->n_nodes * sizeof(rt_node);
    c->draw_commands_host.clear();   // made on the device (rt_world_read gives them)
    uint32_t inner = N - 1u;
    for (uint32_t g = 0; g < G; g++) {
      const uint32_t cnt = rb_base[g + 1] - rb_base[g];
      if (cnt) inner += (cnt - 1u) / 2u;
    }
    c->n_pairs = inner;
    std::memset(&c->troot, 0, sizeof(c->troot));
    for (int k = 0; k < 3; k++) {
      c->troot.lo[k] = rb_root[k];
      c->troot.hi[k] = rb_root[4 + k];
    }
    {
      uint32_t w7;
      std::memcpy(&w7, &rb_root[7], 4);
      c->troot.word = w7 == 0u ? RT_PAIR_INNER : w7;
    }
    const std::vector<uint32_t> old_roots = c->blas_roots;
    c->blas_roots.resize(N);
    for (uint32_t i = 0; i < N; i++) c->blas_roots[i] = rb_base[W.inst_geom[i]];
    std::sort(c->blas_roots.begin(), c->blas_roots.end());
    c->blas_roots.erase(std::unique(c->blas_roots.begin(), c->blas_roots.end()), c->blas_roots.end());
    c->root_w_host.assign(c->blas_roots.size(), 0.0f);
    for (uint32_t i = 0; i < N; i++) {
      const size_t k = std::lower_bound(c->blas_roots.begin(), c->blas_roots.end(), rb_base[W.inst_geom[i]]) - c->blas_roots.begin();
      c->root_w_host[k] += W.inst_scale2[i];
    }
    // the arrays were made by this library from an index-checked description: no validation pass; the derived passes
    // of prepare_scene read the sorted roots from val_roots
    if ((r = ensure_buffer(c, c->val_roots, std::max<size_t>(4, c->blas_roots.size() * 4), false)) < 0) return r;
    HIP_TRY(c, hipMemcpyAsync(c->val_roots.ptr, c->blas_roots.data(), c->blas_roots.size() * 4, hipMemcpyHostToDevice, c->stream));
    c->validate_dirty = false;
    c->scene_valid = true;
    c->nodes_from_device = true;
    c->fm.ids_from = FrameMotionState::IDS_WORLD;   // the stable id of a TLAS position is W.tlas.ord's declaration index
    c->tris_dirty = c->inst_dirty = c->lights_dirty = c->nodes_dirty = c->pairs_dirty = c->roots_dirty = c->world_rec_dirty = true;
    if (W.cache_enabled && !W.static_cached) {   // first full update of this description: keep the static geometries' node blocks
      W.static_count.assign(G, 0u);
      W.static_off.assign(G, 0u);
      size_t total = 0;
      for (uint32_t g = 0; g < G; g++)
        if (W.geoms[g].n_verts && !W.geoms[g].skinned) {
          W.static_off[g] = (uint32_t)total;
          W.static_count[g] = rb_base[g + 1] - rb_base[g];
          total += W.static_count[g];
        }
      if ((r = ensure_buffer(c, W.static_nodes, std::max<size_t>(32, total * sizeof(rt_node)), false)) < 0) return r;
      for (uint32_t g = 0; g < G; g++)
        if (W.static_count[g])
          HIP_TRY(c, hipMemcpyAsync((char*)W.static_nodes.ptr + (size_t)W.static_off[g] * sizeof(rt_node),
                                    (const char*)c->nodes.ptr + ((size_t)W.n_tlas + rb_base[g]) * sizeof(rt_node),
                                    (size_t)W.static_count[g] * sizeof(rt_node), hipMemcpyDeviceToDevice, c->stream));
      W.static_cached = true;
    }
    return ret;
  }
}

int rt_world_update(rt_ctx* c, const rt_world_frame* f) {
  if (!c || !f) return RT_ERR_INVALID;
  bool touched = false;
  const int r = world_update_body(c, f, &touched);
  if (r < 0 && touched) {
    // The update writes straight into the live scene buffers (positions, topology, nodes, instances, lights).  A failure
    // after its first kernel leaves a mix of two scenes there, with the counts and the derived records of the old one:
    // nothing may be traced from it.  compute() refuses until the scene has been uploaded again (rt_upload* re-validates);
    // the Python / Node bridges do exactly that (the scene compiler then runs this update on the host).
    const std::string why = c->error;
    c->scene_valid = false;
    c->validate_dirty = false;
    c->scene_problem = "the device-resident world update failed part-way (" + why + "): the scene buffers hold a mix of two scenes; upload the scene again";
    c->tris_dirty = c->inst_dirty = c->lights_dirty = c->nodes_dirty = c->pairs_dirty = c->roots_dirty = c->world_rec_dirty = true;
    c->facts = lp::SceneFacts();
    walk_forget(c);
    c->world.static_cached = false;
    c->world.valid = false;
    c->error = why;
  }
  return r;
}

double rt_world_last_ms(const rt_ctx* c) { return c ? c->world.last_ms : 0.0; }
double rt_world_last_tlas_ms(const rt_ctx* c) { return c ? c->world.last_tlas_ms : 0.0; }

int rt_world_set_static_cache(rt_ctx* c, int enabled) {
  if (!c) return RT_ERR_INVALID;
  c->world.cache_enabled = enabled != 0;
  c->world.static_cached = false;   // the next update builds everything (and refills the cache when enabled)
  return RT_OK;
}

// the bridge arrays as the device update left them (tests; a host that wants them back)
int rt_world_read(rt_ctx* c, int which, void* out, size_t cap_bytes, size_t* bytes_out) {
  if (!c || !bytes_out) return RT_ERR_INVALID;
  *bytes_out = 0;
  if (!c->world.valid) return fail(c, RT_ERR_NOT_READY, "rt_world_read: no device-resident world");
  HIP_TRY(c, hipSetDevice(c->device));
  const void* src = nullptr;
  size_t n = 0;
  switch (which) {
    case RT_WORLD_VERTICES: src = c->pos.ptr; n = (size_t)c->n_verts * 16; break;
    case RT_WORLD_NORMALS: src = c->nrm.ptr; n = (size_t)c->n_verts * 16; break;
    case RT_WORLD_UVS: src = c->uv.ptr; n = (size_t)c->n_verts * 8; break;
    case RT_WORLD_TOPOLOGY: src = c->topology.ptr; n = (size_t)c->n_tris * sizeof(rt_topology); break;
    case RT_WORLD_TLAS: src = c->nodes.ptr; n = (size_t)c->blas_offset * sizeof(rt_node); break;
    case RT_WORLD_BLAS: src = (const char*)c->nodes.ptr + (size_t)c->blas_offset * sizeof(rt_node); n = (size_t)(c->n_nodes - c->blas_offset) * sizeof(rt_node); break;
    case RT_WORLD_INSTANCES: src = c->instances.ptr; n = (size_t)c->n_instances * sizeof(rt_instance); break;
    case RT_WORLD_LIGHTS: src = c->lights.ptr; n = (size_t)c->n_lights * sizeof(rt_light_ref); break;
    case RT_WORLD_DRAW_COMMANDS: src = c->draw_commands.ptr; n = (size_t)c->n_instances * 16; break;
    case RT_WORLD_INSTANCE_ORDER: src = c->world.tlas.ord; n = (size_t)c->world.n_inst * 4; break;
    default: return fail(c, RT_ERR_INVALID, "rt_world_read: unknown array");
  }
  *bytes_out = n;
  if (!out) return RT_OK;
  if (cap_bytes < n) return fail(c, RT_ERR_INVALID, "rt_world_read: buffer too small");
  if (n) HIP_TRY(c, hipMemcpyAsync(out, src, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// depth of the last rt_build_blas tree (levels of the breadth-first build that held nodes) | large-node levels << 16
int rt_build_blas_levels(const rt_ctx* c) { return c ? (int)(c->bv_levels | (c->bv_big_levels << 16)) : 0; }

int rt_upload(rt_ctx* c, rt_kind kind, const void* data, size_t bytes) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;
  c->world.static_cached = false;   // host arrays replace what the device update left in the scene buffers   // drops frames traced ahead (rt_set_lookahead)
  if (kind == RT_KIND_TOPOLOGY || kind == RT_KIND_INSTANCE) c->fm.scene_gen++;
  if (kind == RT_KIND_INSTANCE) c->fm.ids_from = FrameMotionState::IDS_IDENTITY;
  if (bytes && !data) return fail(c, RT_ERR_INVALID, "null data");
  HIP_TRY(c, hipSetDevice(c->device));
  int r;
  switch (kind) {
    case RT_KIND_TOPOLOGY:
      if (bytes % sizeof(rt_topology)) return fail(c, RT_ERR_INVALID, "topology must be 80 bytes per triangle");
      c->facts = lp::SceneFacts();
      r = upload(c, c->topology, data, bytes);
      if (r < 0) return r;
      c->n_tris = (uint32_t)(bytes / sizeof(rt_topology));
      // the materials of these records, from the caller's bytes (a scene too large for a one-leaf LDS form is not scanned)
      c->facts = scene_facts::topology_facts((const rt_topology*)data, bytes / sizeof(rt_topology));
      c->validate_dirty = true;
      c->tris_dirty = true;
      c->world_rec_dirty = true;
      c->lights_dirty = true;
      return r;
    case RT_KIND_INSTANCE:
      if (bytes % sizeof(rt_instance)) return fail(c, RT_ERR_INVALID, "instances must be 144 bytes each");
      r = upload(c, c->instances, data, bytes);
      if (r < 0) return r;
      c->n_instances = (uint32_t)(bytes / sizeof(rt_instance));
      {  // BLAS roots the instances refer to (host copy of one word per instance: the validation kernel needs them sorted)
        const rt_instance* hi = (const rt_instance*)data;
        const std::vector<uint32_t> old_roots = c->blas_roots;
        c->blas_roots.resize(c->n_instances);
        for (uint32_t k = 0; k < c->n_instances; k++) c->blas_roots[k] = hi[k].blas_node_offset;
        std::sort(c->blas_roots.begin(), c->blas_roots.end());
        c->blas_roots.erase(std::unique(c->blas_roots.begin(), c->blas_roots.end()), c->blas_roots.end());
        // visit-probability weight of each BLAS for the treelet order: sum over its instances of the squared linear
        // scale, |det(M3x3)|^(2/3) (object-space box areas times this approximate world-space areas)
        c->root_w_host.assign(c->blas_roots.size(), 0.0f);
        for (uint32_t k = 0; k < c->n_instances; k++) {
          const float* m = hi[k].transform;   // column-major 4x4
          const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) -
                             (double)m[4] * ((double)m[1] * m[10] - (double)m[2] * m[9]) +
                             (double)m[8] * ((double)m[1] * m[6] - (double)m[2] * m[5]);
          double s2 = std::pow(std::fabs(det), 2.0 / 3.0);
          if (!(s2 > 0.0) || !std::isfinite(s2)) s2 = 1.0;
          const size_t r = std::lower_bound(c->blas_roots.begin(), c->blas_roots.end(), hi[k].blas_node_offset) - c->blas_roots.begin();
          c->root_w_host[r] += (float)s2;
        }
        if (old_roots != c->blas_roots) c->pairs_dirty = true;   // BLAS-local skips are resolved against the set of roots
        // the BLAS root of every instance, for the walk facts of a one-leaf scene (which has few)
        c->inst_root_host.clear();
        if (c->n_instances <= scene_facts::kMaxWalkNodes)
          for (uint32_t k = 0; k < c->n_instances; k++) c->inst_root_host.push_back(hi[k].blas_node_offset);
        c->walk_dirty = true;
      }
      c->roots_dirty = true;
      c->nodes_dirty = true;
      c->validate_dirty = true;
      c->inst_dirty = true;
      c->world_rec_dirty = true;
      c->lights_dirty = true;
      return r;
    case RT_KIND_LIGHTS:
      if (bytes % sizeof(rt_light_ref)) return fail(c, RT_ERR_INVALID, "lights must be 8 bytes each");
      r = upload(c, c->lights, data, bytes);
      if (r < 0) return r;
      c->n_lights = (uint32_t)(bytes / sizeof(rt_light_ref));
      c->validate_dirty = true;
      c->lights_dirty = true;
      return r;
    case RT_KIND_DRAW_COMMANDS: {
      // not on the 1.5x policy in the reference (ResourceManager.ts:264-278); kept on the host too
      bool grew = !c->draw_commands.ptr || c->draw_commands.capacity < bytes;
      if (grew) {
        c->draw_commands.reset();
        r = ensure_buffer(c, c->draw_commands, bytes, false);
        if (r < 0) return r;
      }
      if (bytes) {
        HIP_TRY(c, hipMemcpyAsync(c->draw_commands.ptr, data, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
      c->draw_commands.size = bytes;
      c->draw_commands_host.assign((const uint32_t*)data, (const uint32_t*)data + bytes / 4);
      return grew ? RT_REALLOCATED : RT_OK;
    }
  }
  return fail(c, RT_ERR_INVALID, "unknown buffer kind");
}

int rt_upload_geometry(rt_ctx* c, const float* pos4, const float* nrm4, const float* uv2, uint32_t vertex_count) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;
  c->world.static_cached = false;   // host arrays replace what the device update left in the scene buffers   // drops frames traced ahead (rt_set_lookahead)
  c->fm.scene_gen++;
  if (vertex_count && (!pos4 || !nrm4 || !uv2)) return fail(c, RT_ERR_INVALID, "null geometry array");
  HIP_TRY(c, hipSetDevice(c->device));
  // The reference packs the three arrays into one buffer at 256-byte aligned offsets because WebGPU
  // binds sub-ranges (ResourceManager.ts:286-323); HIP needs no such aliasing, so they stay separate.
  int r0 = upload(c, c->pos, pos4, (size_t)vertex_count * 16);
  if (r0 < 0) return r0;
  int r1 = upload(c, c->nrm, nrm4, (size_t)vertex_count * 16);
  if (r1 < 0) return r1;
  int r2 = upload(c, c->uv, uv2, (size_t)vertex_count * 8);
  if (r2 < 0) return r2;
  c->n_verts = vertex_count;
  c->vertex_count = vertex_count;
  c->validate_dirty = true;
  c->tris_dirty = true;
  c->world_rec_dirty = true;
  c->lights_dirty = true;
  return (r0 | r1 | r2) ? RT_REALLOCATED : RT_OK;
}

int rt_upload_bvh(rt_ctx* c, const float* tlas, uint32_t n_tlas, const float* blas, uint32_t n_blas) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;
  c->world.static_cached = false;   // host arrays replace what the device update left in the scene buffers   // drops frames traced ahead (rt_set_lookahead)
  c->fm.scene_gen++;
  if ((n_tlas && !tlas) || (n_blas && !blas)) return fail(c, RT_ERR_INVALID, "null BVH array");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t total = ((size_t)n_tlas + n_blas) * sizeof(rt_node);
  int r = ensure_buffer(c, c->nodes, total, true);
  if (r < 0) return r;
  if (n_tlas)
    HIP_TRY(c, hipMemcpyAsync(c->nodes.ptr, tlas, (size_t)n_tlas * 32, hipMemcpyHostToDevice, c->stream));
  if (n_blas)
    HIP_TRY(c, hipMemcpyAsync((char*)c->nodes.ptr + (size_t)n_tlas * 32, blas, (size_t)n_blas * 32,
                              hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->blas_offset = n_tlas;  // this.blasOffset = tlas.length / 8
  c->n_nodes = n_tlas + n_blas;
  {  // inner nodes (data word 0): one child-pair record each
    uint32_t inner = 0;
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(tlas);
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(blas);
    for (uint32_t k = 0; k < n_tlas; k++) inner += tw[8 * (size_t)k + 7] == 0u;
    for (uint32_t k = 0; k < n_blas; k++) inner += bw[8 * (size_t)k + 7] == 0u;
    c->n_pairs = inner;
    std::memset(&c->troot, 0, sizeof(c->troot));
    if (n_tlas) {   // node 0; an inner root is the first inner node of the array: pair record 0
      for (int k = 0; k < 3; k++) {
        c->troot.lo[k] = tlas[k];
        c->troot.hi[k] = tlas[4 + k];
      }
      c->troot.word = tw[7] == 0u ? RT_PAIR_INNER : tw[7];
    }
  }
  c->roots_dirty = true;
  c->validate_dirty = true;
  c->nodes_dirty = true;
  c->world_rec_dirty = true;
  c->pairs_dirty = true;
  c->nodes_from_device = false;
  // the caller's bytes, for the walk facts: a one-node TLAS over a BLAS small enough for a one-leaf LDS scene
  c->blas_host.clear();
  if (n_tlas == 1u && n_blas && n_blas <= scene_facts::kMaxWalkNodes) {
    c->blas_host.assign((const rt_node*)blas, (const rt_node*)blas + n_blas);
    std::memcpy(&c->tlas0_host, tlas, sizeof(rt_node));
  }
  c->walk_dirty = true;
  return r ? RT_REALLOCATED : RT_OK;
}

int rt_set_scene(rt_ctx* c, const float camera[24], uint32_t frame_count, uint32_t light_count) {
  if (!c || !camera) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  c->light_count = light_count;
  step_jitter(c, frame_count, frame_count);
  std::memcpy(&c->uniforms.camera, camera, 96);
  std::memcpy(&c->uniforms.prev_camera, c->prev_camera, 96);
  write_mixed(c, frame_count);
  std::memcpy(c->prev_camera, camera, 96);
  return RT_OK;
}

int rt_recreate_bind_group(rt_ctx* c) { return c ? RT_OK : RT_ERR_INVALID; }

// The trace kernels by [workgroup size 256 / 512 / 1024][any][detail][lds].  The node walk's RAYREG form is compiled for
// 256-thread workgroups in mixed mode only: [any][detail].
#define RT_WF_TRACE_FNS(K, B)                                                                                          \
  {{{(const void*)K<false, false, false, B>, (const void*)K<false, false, true, B>},                                 \
    {(const void*)K<false, true, false, B>, (const void*)K<false, true, true, B>}},                                  \
   {{(const void*)K<true, false, false, B>, (const void*)K<true, false, true, B>},                                   \
    {(const void*)K<true, true, false, B>, (const void*)K<true, true, true, B>}}}
static const void* const wf_node_fns[3][2][2][2] = {RT_WF_TRACE_FNS(rtk::k_wf_trace, 256), RT_WF_TRACE_FNS(rtk::k_wf_trace, 512),
                                                    RT_WF_TRACE_FNS(rtk::k_wf_trace, 1024)};
static const void* const wf_pair_fns[3][2][2][2] = {RT_WF_TRACE_FNS(rtk::k_wf_trace_pairs, 256),
                                                    RT_WF_TRACE_FNS(rtk::k_wf_trace_pairs, 512),
                                                    RT_WF_TRACE_FNS(rtk::k_wf_trace_pairs, 1024)};
#undef RT_WF_TRACE_FNS
static const void* const wf_node_rayreg_fns[2][2] = {
    {(const void*)rtk::k_wf_trace<false, false, false, 256, true>, (const void*)rtk::k_wf_trace<false, true, false, 256, true>},
    {(const void*)rtk::k_wf_trace<true, false, false, 256, true>, (const void*)rtk::k_wf_trace<true, true, false, 256, true>}};
// the shade kernel by [first depth][detail], the primary kernel by [detail][lds]
static const void* const wf_shade_fns[2][2] = {{(const void*)rtk::k_wf_shade<false, false>, (const void*)rtk::k_wf_shade<false, true>},
                                               {(const void*)rtk::k_wf_shade<true, false>, (const void*)rtk::k_wf_shade<true, true>}};
// [counting build][form]: global memory, LDS, LDS with many tiles per wave (launch_plan.h primary_shape)
static const void* const primary_fns[2][3] = {
    {(const void*)rtk::k_primary_visibility<false, false>, (const void*)rtk::k_primary_visibility<false, true>,
     (const void*)rtk::k_primary_visibility_tiles<false>},
    {(const void*)rtk::k_primary_visibility<true, false>, (const void*)rtk::k_primary_visibility<true, true>,
     (const void*)rtk::k_primary_visibility_tiles<true>}};
// Wavefront form: per depth one shade launch and two trace launches, all enqueued without host readback.
static int launch_wavefront(rt_ctx* c, const DevScene& S, const DevFrame& F, const DevFrameSlot* dslots, uint32_t n) {
  const size_t npx = (size_t)c->width * c->height;
  const size_t items = npx * n;
  if (items >= (1ull << 31)) return fail(c, RT_ERR_INVALID, "batch too large for the wavefront queues");
  int r;
  // queues are reserved in chunks of RT_WF_CHUNK per wave: room for every item plus one partial chunk per wave
  // shade kernels: persistent waves that loop over the items; every wave may leave one partly used chunk per queue
  const uint32_t shade_blocks = (uint32_t)std::min<size_t>((items + 255) / 256, (size_t)c->num_cus * (size_t)c->shade_per_cu);
  const size_t qcap = items + (size_t)shade_blocks * 4 * 256 + 1024 * 1024;
  // per item: active[2] + shadow ids + ext ids + occlusion word (5 x 4 B) + shadow rays, extension rays of even and of odd
  // depths (3 x 32 B) + hits (16 B)
  r = ensure_buffer(c, c->wf_queues, qcap * 132, false);
  if (r < 0) return r;
  r = ensure_buffer(c, c->wf_state, 2 * qcap * sizeof(WfPath), false);   // path records in list order, double-buffered by depth parity
  if (r < 0) return r;
  const uint32_t depths = c->max_depth ? c->max_depth : 1u;
  r = ensure_buffer(c, c->wf_counters, (size_t)(depths + 2) * 32, false);
  if (r < 0) return r;
  HIP_TRY(c, hipMemsetAsync(c->wf_counters.ptr, 0, (size_t)(depths + 2) * 32, c->stream));
  WfState W;
  W.p[0] = (WfPath*)c->wf_state.ptr;
  W.p[1] = W.p[0] + qcap;
  WfQueues Q;
  char* qb = (char*)c->wf_queues.ptr;
  Q.shadow_rays = (float4*)qb;
  Q.ext_rays[0] = (float4*)(qb + qcap * 32);
  Q.ext_rays[1] = (float4*)(qb + qcap * 64);
  Q.ext_hit = (float4*)(qb + qcap * 96);
  Q.active[0] = (uint32_t*)(qb + qcap * 112);
  Q.active[1] = (uint32_t*)(qb + qcap * 116);
  Q.shadow_ids = (uint32_t*)(qb + qcap * 120);
  Q.ext_ids = (uint32_t*)(qb + qcap * 124);
  Q.occluded = (uint32_t*)(qb + qcap * 128);
  Q.counters = (uint32_t*)c->wf_counters.ptr;
  const bool detail = c->detailed_counters;
  lp::TraceShape shape = lp::trace_shape(scene_size(c), c->knobs, c->knobs.wf_block);
  shape.plan.troot = c->troot;
  const int bi = shape.block == 1024 ? 2 : (shape.block == 512 ? 1 : 0);
  const void* trace_fn[2];
  for (int k = 0; k < 2; k++)   // k = 0: any hit (shadow rays), 1: closest hit (extension rays)
    trace_fn[k] = shape.pairs ? wf_pair_fns[bi][k == 0][detail][shape.trace_lds]
                  : shape.rayreg && bi == 0 && !shape.trace_lds ? wf_node_rayreg_fns[k == 0][detail]
                                                                : wf_node_fns[bi][k == 0][detail][shape.trace_lds];
  int trace_per_cu[2];
  for (int k = 0; k < 2; k++)
    if ((r = resident_blocks(c, trace_fn[k], shape.block, shape.dyn, &trace_per_cu[k])) < 0) return r;
  if (getenv("MI355RT_DEBUG_SHAPE"))
    fprintf(stderr, "[mi355rt] trace kernels: %s walk, %d threads per workgroup, %zu bytes of LDS, resident workgroups per CU: any-hit %d, closest-hit %d\n",
            shape.pairs ? "pair" : "node", shape.block, shape.dyn, trace_per_cu[0], trace_per_cu[1]);
  uint32_t nn = shape.pairs ? c->n_pairs : c->n_nodes, nt = c->n_tris, ni = c->n_instances, depth = 0;
  DevScene Sa = S;
  DevFrame Fa = F;
  rt_scene_uniforms Ua = c->uniforms;
  void* shade_args[] = {&Sa, &Fa, &Ua, &W, &Q, &dslots, &n, &depth};
  void* trace_args[] = {&Sa, &Fa, &Ua, &Q, &depth, &nn, &nt, &ni, shape.pairs ? (void*)&shape.plan : (void*)&shape.nplan};
  EventPair* ev = next_events(c, RT_TIMER_PATHTRACE);
  if (ev) HIP_TRY(c, hipEventRecord(ev->a, c->stream));
  for (; depth < depths; depth++) {
    EventPair* evs = next_events(c, RT_TIMER_WF_SHADE);
    if (evs) HIP_TRY(c, hipEventRecord(evs->a, c->stream));
    HIP_TRY(c, hipLaunchKernel(wf_shade_fns[depth == 0][detail], dim3(shade_blocks), dim3(256), shade_args, 0, c->stream));
    if (evs) HIP_TRY(c, hipEventRecord(evs->b, c->stream));
    for (int k = 0; k < 2; k++) {
      // resident workgroups: what fits (registers, LDS; since round 4 the node-walk kernels leave room for a seventh wave per
      // SIMD), or MI355RT_WF_BLOCKS_PER_CU
      const uint32_t blocks =
          grid_blocks(c, trace_per_cu[k], c->knobs.wf_blocks_per_cu, (items + (size_t)shape.block - 1) / (size_t)shape.block);
      EventPair* evt = next_events(c, k == 0 ? RT_TIMER_WF_TRACE_SHADOW : RT_TIMER_WF_TRACE_EXT);
      hipStream_t st = c->stream;
      if (k == 0 && c->wf_overlap) {   // any-hit trace: fork to the side stream behind this depth's shade kernel
        st = c->side_stream;
        HIP_TRY(c, hipEventRecord(c->side_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(st, c->side_fork, 0));
      }
      if (evt) HIP_TRY(c, hipEventRecord(evt->a, st));
      HIP_TRY(c, hipLaunchKernel(trace_fn[k], dim3(blocks), dim3(shape.block), trace_args, shape.dyn, st));
      if (evt) HIP_TRY(c, hipEventRecord(evt->b, st));
      if (k == 0 && c->wf_overlap) HIP_TRY(c, hipEventRecord(c->side_join, st));
    }
    if (c->wf_overlap) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_join, 0));   // the next shade needs both results
  }
  {
    // one more shade pass: the paths that ended at the last depth but were waiting for their shadow ray are finished
    // here (every path of this list carries the ENDED flag, so nothing is shaded or queued)
    EventPair* evs = next_events(c, RT_TIMER_WF_SHADE);
    if (evs) HIP_TRY(c, hipEventRecord(evs->a, c->stream));
    HIP_TRY(c, hipLaunchKernel(wf_shade_fns[0][detail], dim3(shade_blocks), dim3(256), shade_args, 0, c->stream));   // depth == depths
    if (evs) HIP_TRY(c, hipEventRecord(evs->b, c->stream));
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev->b, c->stream));
  hipLaunchKernelGGL(rtk::k_accumulate_frames, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, F, dslots, c->acc_frames,
                     c->width, c->height);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

// ---- ray queries: k_ray_query by [form][any][detail], form as in k_rayquery.hip.h
#define RT_RQ_FNS(F)                                                                                                  \
  {{(const void*)rtk::k_ray_query<false, false, F>, (const void*)rtk::k_ray_query<false, true, F>},                  \
   {(const void*)rtk::k_ray_query<true, false, F>, (const void*)rtk::k_ray_query<true, true, F>}}
static const void* const rq_fns[5][2][2] = {RT_RQ_FNS(rtk::RT_RQ_NODE_LDS), RT_RQ_FNS(rtk::RT_RQ_NODE_MIXED), RT_RQ_FNS(rtk::RT_RQ_NODE_RAYREG),
                                            RT_RQ_FNS(rtk::RT_RQ_PAIR_LDS), RT_RQ_FNS(rtk::RT_RQ_PAIR_GLOBAL)};
#undef RT_RQ_FNS

// Enqueue one query on the context's stream: n > 0 rays at d_rays, results to d_out (device pointers), on the state q and the
// last stats `last` of the kind that asks (`what`: the prefix of its messages).  keep_counts: a later launch of the same call,
// whose counters add to those of the launches before it.  batch_ev: the launch records into this pair, which its caller
// keeps count of, instead of the state's own.
static int launch_ray_query_on(rt_ctx* c, QueryState& q, rt_ray_stats& last, const char* what, const void* d_rays, uint32_t n,
                               int mode, float t_min, void* d_out, bool detail, bool keep_counts = false,
                               EventPair* batch_ev = nullptr) {
  int r = query_scene_ready(c, what, false);
  if (r < 0) return r;
  lp::TraceShape shape = lp::trace_shape(scene_size(c), c->knobs, 0);
  shape.plan.troot = c->troot;
  const void* fn = rq_fns[shape.rq_form][mode == RT_RAYS_ANY][detail];
  int per_cu;
  if ((r = resident_blocks(c, fn, 256, shape.dyn, &per_cu)) < 0) return r;
  const uint32_t blocks = grid_blocks(c, per_cu, c->knobs.wf_blocks_per_cu, (n + 255u) / 256u);
  rtk::RayQueryArgs A;
  A.rays = (const float4*)d_rays;
  A.out = (uint4*)d_out;
  A.n_rays = n;
  A.blas_base = c->blas_offset;
  A.t_min = t_min;
  A.n_recs = shape.pairs ? c->n_pairs : c->n_nodes;
  A.n_tris = c->n_tris;
  A.n_inst = c->n_instances;
  DevScene S = dev_scene(c);
  void* args[] = {&S, &A, &shape.nplan, &shape.plan};
  r = query_enqueue(c, q, fn, blocks, args, shape.dyn, &A.counters, &A.head, keep_counts, batch_ev, [&] {
    fprintf(stderr, "[mi355rt] %s: %s walk, form %d, %zu bytes of LDS, resident workgroups per CU %d, %u workgroups\n", what,
            shape.pairs ? "pair" : "node", shape.rq_form, shape.dyn, per_cu, blocks);
  });
  if (r < 0) return r;
  last = rt_ray_stats();
  last.walk = shape.pairs ? 1u : 0u;
  last.lds = shape.trace_lds ? 1u : 0u;
  last.rayreg = shape.rq_form == rtk::RT_RQ_NODE_RAYREG ? 1u : 0u;
  last.workgroups = blocks;
  return RT_OK;
}
static int launch_ray_query(rt_ctx* c, const void* d_rays, uint32_t n, int mode, float t_min, void* d_out, bool detail) {
  return launch_ray_query_on(c, c->rq, c->rq_last, "ray query", d_rays, n, mode, t_min, d_out, detail);
}

static int ray_query_args_ok(rt_ctx* c, uint32_t n, int mode, float t_min) {
  if (mode != RT_RAYS_CLOSEST && mode != RT_RAYS_ANY) return fail(c, RT_ERR_INVALID, "ray query: unknown mode");
  if (!(t_min >= 0.0f)) return fail(c, RT_ERR_INVALID, "ray query: t_min must be >= 0");
  if (n >= (1u << 31)) return fail(c, RT_ERR_INVALID, "ray query: too many rays for one call (n must be below 2^31)");
  return RT_OK;
}

// the stats of the last call of a kind that launches k_ray_query on the state q
static int ray_query_stats_of(rt_ctx* c, const QueryState& q, const rt_ray_stats& last, rt_ray_stats* out) {
  if (!c || !out) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  *out = last;
  uint64_t sum[6];
  const int r = query_totals(c, q, last.workgroups != 0, sum, &out->kernel_ms);
  if (r < 0) return r;
  out->rays += sum[1] + sum[2];
  out->nodes_visited += sum[3];
  out->tris_tested += sum[4];
  return RT_OK;
}
int rt_ray_query_stats(rt_ctx* c, rt_ray_stats* out) { return c ? ray_query_stats_of(c, c->rq, c->rq_last, out) : RT_ERR_INVALID; }

int rt_trace_rays_device(rt_ctx* c, const void* dev_rays, uint32_t n, int mode, float t_min, void* dev_out) {
  if (!c) return RT_ERR_INVALID;
  int r = ray_query_args_ok(c, n, mode, t_min);
  if (r < 0) return r;
  if (n == 0) {
    c->rq_last = rt_ray_stats();
    return RT_OK;
  }
  if ((r = caller_arrays_ok(c, "ray query", {dev_rays, dev_out})) < 0) return r;
  return launch_ray_query(c, dev_rays, n, mode, t_min, dev_out, c->detailed_counters);
}

int rt_trace_rays(rt_ctx* c, const rt_ray* rays, uint32_t n, int mode, float t_min, rt_ray_hit* out, rt_ray_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = ray_query_args_ok(c, n, mode, t_min);
  if (r < 0) return r;
  if (n == 0) {
    c->rq_last = rt_ray_stats();
    if (stats) *stats = c->rq_last;
    return RT_OK;
  }
  r = query_from_host(c, c->rq, "ray query", rays, n, out, sizeof(rt_ray_hit), [&](const void* d_rays, void* d_out) {
    return launch_ray_query(c, d_rays, n, mode, t_min, d_out, stats != nullptr);
  });
  if (r < 0) return r;
  if (stats) return rt_ray_query_stats(c, stats);
  return RT_OK;
}

// ---- path queries: radiance queries, irradiance gathers and the trace of probe gathers (path_query_loop, k_radiance.hip.h).
// What a kind has of its own:
struct PathQueryKind {
  const char* what;                   // prefix of its messages
  const char* items;                  // what it calls its items
  const void* fns[2][2];              // its kernel by [detail][lds]
  QueryState rt_ctx::*state;
  rt_radiance_stats rt_ctx::*last;
  size_t out_stride;                  // bytes of one result
};
#define RT_PQ_FNS(K) {{(const void*)rtk::K<false, false>, (const void*)rtk::K<false, true>}, \
                      {(const void*)rtk::K<true, false>, (const void*)rtk::K<true, true>}}
static const PathQueryKind pq_radiance = {"radiance query", "rays", RT_PQ_FNS(k_radiance_query), &rt_ctx::rd, &rt_ctx::rd_last,
                                          sizeof(rt_radiance)};
static const PathQueryKind pq_gather = {"irradiance gather", "points", RT_PQ_FNS(k_irradiance_gather), &rt_ctx::gi, &rt_ctx::gi_last,
                                        sizeof(rt_irradiance)};
// probe gathers trace with the radiance query's kernel, on a state of their own
static const PathQueryKind pq_probe = {"probe gather", "probes", RT_PQ_FNS(k_radiance_query), &rt_ctx::pr, &rt_ctx::pr_last,
                                       sizeof(rt_probe_sh9)};
// ... and so do directional gathers
static const PathQueryKind pq_directional = {"directional gather", "points", RT_PQ_FNS(k_radiance_query), &rt_ctx::dg,
                                             &rt_ctx::dg_last, sizeof(rt_directional)};
// ... and so do reflection captures
static const PathQueryKind pq_reflection = {"reflection", "texels", RT_PQ_FNS(k_radiance_query), &rt_ctx::rf, &rt_ctx::rf_last,
                                            sizeof(rt_radiance)};
#undef RT_PQ_FNS

// Enqueue one query on the context's stream: n > 0 items at d_items, results to d_out (device pointers).  keep_counts: a
// later launch of the same call, whose counters add to those of the launches before it.  batch_ev: the launch records into
// this pair, which its caller keeps count of, instead of the state's own.
static int launch_path_query(rt_ctx* c, const PathQueryKind& k, const void* d_items, uint32_t n, uint32_t max_depth, uint32_t spp,
                             uint32_t seed, void* d_out, bool detail, bool keep_counts = false, EventPair* batch_ev = nullptr) {
  int r = query_scene_ready(c, k.what, true);
  if (r < 0) return r;
  // the persistent kernel's 256-thread forms without the one-leaf one
  lp::PersistentShape shape = lp::persistent_plan(scene_size(c), c->knobs);
  const void* fn = k.fns[detail][shape.lds];
  int per_cu;
  if ((r = resident_blocks(c, fn, 256, shape.dyn, &per_cu)) < 0) return r;
  const uint32_t blocks = grid_blocks(c, per_cu, 0, (n + 255u) / 256u);
  rtk::PathQueryArgs A;
  A.items = (const float4*)d_items;
  A.out = (float4*)d_out;
  A.n_items = n;
  A.max_depth = max_depth;
  A.spp = spp;
  A.seed = seed;
  A.light_count = c->light_count;
  A.blas_base = c->blas_offset;
  A.n_nodes = c->n_nodes;
  A.n_tris = c->n_tris;
  A.n_inst = c->n_instances;
  A.n_verts = c->n_verts;
  DevScene S = dev_scene(c);
  void* args[] = {&S, &A, &shape.plan};
  r = query_enqueue(c, c->*k.state, fn, blocks, args, shape.dyn, &A.counters, &A.head, keep_counts, batch_ev, [&] {
    fprintf(stderr, "[mi355rt] %s: %s form, %zu bytes of LDS, resident workgroups per CU %d, %u workgroups\n", k.what,
            shape.lds ? "LDS" : "global", shape.dyn, per_cu, blocks);
  });
  if (r < 0) return r;
  rt_radiance_stats& last = c->*k.last;
  last = rt_radiance_stats();
  last.rays = n;
  last.samples = (uint64_t)n * spp;
  last.lds = shape.lds ? 1u : 0u;
  last.workgroups = blocks;
  return RT_OK;
}

static int path_query_args_ok(rt_ctx* c, const PathQueryKind& k, uint32_t n, uint32_t spp) {
  const std::string w(k.what);
  if (n >= (1u << 31)) return fail(c, RT_ERR_INVALID, w + ": too many " + k.items + " for one call (n must be below 2^31)");
  if (spp == 0 || spp > 65536) return fail(c, RT_ERR_INVALID, w + ": spp must be 1 .. 65536");
  return RT_OK;
}

static int path_query_stats(rt_ctx* c, const PathQueryKind& k, rt_radiance_stats* out) {
  if (!c || !out) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  *out = c->*k.last;
  uint64_t sum[6];
  const int r = query_totals(c, c->*k.state, out->workgroups != 0, sum, &out->kernel_ms);
  if (r < 0) return r;
  out->extension_rays += sum[1];
  out->shadow_rays += sum[2];
  out->nodes_visited += sum[3];
  out->tris_tested += sum[4];
  out->shaded_hits += sum[5];
  return RT_OK;
}

// detail: run the counting kernel; < 0: as rt_set_counting says
static int path_query_device(rt_ctx* c, const PathQueryKind& k, const void* dev_items, uint32_t n, uint32_t max_depth, uint32_t spp,
                             uint32_t seed, void* dev_out, int detail = -1) {
  if (!c) return RT_ERR_INVALID;
  int r = path_query_args_ok(c, k, n, spp);
  if (r < 0) return r;
  if (n == 0) {
    c->*k.last = rt_radiance_stats();
    return RT_OK;
  }
  if ((r = caller_arrays_ok(c, k.what, {dev_items, dev_out})) < 0) return r;
  return launch_path_query(c, k, dev_items, n, max_depth, spp, seed, dev_out, detail < 0 ? c->detailed_counters : detail != 0);
}

// items: rt_ray or rt_gather_point, the same 32 bytes
static int path_query_host(rt_ctx* c, const PathQueryKind& k, const rt_ray* items, uint32_t n, uint32_t max_depth, uint32_t spp,
                           uint32_t seed, void* out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = path_query_args_ok(c, k, n, spp);
  if (r < 0) return r;
  if (n == 0) {
    c->*k.last = rt_radiance_stats();
    if (stats) *stats = c->*k.last;
    return RT_OK;
  }
  r = query_from_host(c, c->*k.state, k.what, items, n, out, k.out_stride, [&](const void* d_items, void* d_out) {
    return launch_path_query(c, k, d_items, n, max_depth, spp, seed, d_out, stats != nullptr);
  });
  if (r < 0) return r;
  if (stats) return path_query_stats(c, k, stats);
  return RT_OK;
}

int rt_radiance_query_stats(rt_ctx* c, rt_radiance_stats* out) { return path_query_stats(c, pq_radiance, out); }
int rt_trace_radiance_device(rt_ctx* c, const void* dev_rays, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                             void* dev_out) {
  return path_query_device(c, pq_radiance, dev_rays, n, max_depth, spp, seed, dev_out);
}
int rt_trace_radiance(rt_ctx* c, const rt_ray* rays, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                      rt_radiance* out, rt_radiance_stats* stats) {
  return path_query_host(c, pq_radiance, rays, n, max_depth, spp, seed, out, stats);
}

int rt_irradiance_gather_stats(rt_ctx* c, rt_radiance_stats* out) { return path_query_stats(c, pq_gather, out); }
int rt_gather_irradiance_device(rt_ctx* c, const void* dev_points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                                void* dev_out) {
  return path_query_device(c, pq_gather, dev_points, n, max_depth, spp, seed, dev_out);
}
int rt_gather_irradiance(rt_ctx* c, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                         rt_irradiance* out, rt_radiance_stats* stats) {
  return path_query_host(c, pq_gather, reinterpret_cast<const rt_ray*>(points), n, max_depth, spp, seed, out, stats);
}

// ---- probe gathers: SH9 radiance per probe (mi355rt.h "probe gathers"), by composition around the radiance query's kernel:
// per batch of whole probes (run_batches) k_probe_rays -> k_radiance_query (spp = 1, seed = 0 on the pad' rays) ->
// k_probe_project (k_probe.hip.h).
// Directional gathers (mi355rt.h "directional gathers") are the same composition at surface points, with k_dir_rays and
// k_dir_project (k_directional.hip.h).  What a composed gather has of its own:
struct ComposedGather {
  const PathQueryKind& kind;                 // of its radiance launches: the state with a pair of events per batch, the last stats
  const void* rays_fn;                       // (items, rays, n_items, spp, seed), one thread per (item, sample)
  const void* project_fn;                    // (items, radiance, out, n, spp, seed), one wave per item
  uint32_t out_vec4;                         // float4 per result
};
static const ComposedGather cg_probe = {pq_probe, (const void*)rtk::k_probe_rays, (const void*)rtk::k_probe_project,
                                        sizeof(rt_probe_sh9) / 16};
static const ComposedGather cg_directional = {pq_directional, (const void*)rtk::k_dir_rays, (const void*)rtk::k_dir_project,
                                              sizeof(rt_directional) / 16};
static_assert(RT_DIRECTIONAL_BATCH_SAMPLES == RT_PROBE_BATCH_SAMPLES, "the two composed gathers share the scratch of a batch");

static int launch_composed_gather(rt_ctx* c, const ComposedGather& g, const void* d_items, uint32_t n, uint32_t max_depth,
                                  uint32_t spp, uint32_t seed, void* d_out, bool detail) {
  const PathQueryKind& k = g.kind;
  const int r = query_scene_ready(c, k.what, true);
  if (r < 0) return r;
  return run_batches(
      c, c->*k.state, c->*k.last, n, spp,
      [&](uint32_t first, uint32_t, uint32_t items) -> int {
        const float4* src = (const float4*)d_items + 2 * (size_t)first;
        float4* rays = (float4*)c->pr_rays.ptr;
        uint32_t a_items = items, a_spp = spp, a_seed = seed;
        void* args[] = {&src, &rays, &a_items, &a_spp, &a_seed};
        HIP_TRY(c, hipLaunchKernel(g.rays_fn, dim3((items + 255u) / 256u), dim3(256), args, 0, c->stream));
        return RT_OK;
      },
      [&](const void* rays, uint32_t items, void* rad, bool keep_counts, EventPair* ev) {
        return launch_path_query(c, k, rays, items, max_depth, 1u, 0u, rad, detail, keep_counts, ev);
      },
      [&](uint32_t first, uint32_t np) -> int {
        const float4* src = (const float4*)d_items + 2 * (size_t)first;
        const float4* rad = (const float4*)c->pr_rad.ptr;
        float4* out = (float4*)d_out + g.out_vec4 * (size_t)first;
        uint32_t a_np = np, a_spp = spp, a_seed = seed;
        void* args[] = {&src, &rad, &out, &a_np, &a_spp, &a_seed};
        HIP_TRY(c, hipLaunchKernel(g.project_fn, dim3((np + 3u) / 4u), dim3(256), args, 0, c->stream));
        return RT_OK;
      });
}

// the stats of a path kind whose calls trace once per batch (the composed gathers, reflection captures)
static int batched_query_stats(rt_ctx* c, const PathQueryKind& k, rt_radiance_stats* out) {
  if (!c || !out) return RT_ERR_INVALID;
  const int r = path_query_stats(c, k, out);   // fences the stream; the time is that of the batches
  if (r < 0) return r;
  return batch_time_ms(c, c->*k.state, &out->kernel_ms);
}
static int composed_gather_stats(rt_ctx* c, const ComposedGather& g, rt_radiance_stats* out) {
  return batched_query_stats(c, g.kind, out);
}
// detail: run the counting kernel; < 0: as rt_set_counting says
static int composed_gather_device(rt_ctx* c, const ComposedGather& g, const void* dev_items, uint32_t n, uint32_t max_depth,
                                  uint32_t spp, uint32_t seed, void* dev_out, int detail = -1) {
  if (!c) return RT_ERR_INVALID;
  int r = path_query_args_ok(c, g.kind, n, spp);
  if (r < 0) return r;
  if (n == 0) {
    c->*g.kind.last = rt_radiance_stats();
    (c->*g.kind.state).batches_timed = 0;
    return RT_OK;
  }
  if ((r = caller_arrays_ok(c, g.kind.what, {dev_items, dev_out})) < 0) return r;
  return launch_composed_gather(c, g, dev_items, n, max_depth, spp, seed, dev_out,
                                detail < 0 ? c->detailed_counters : detail != 0);
}
// items: rt_probe or rt_gather_point, the same 32 bytes
static int composed_gather_host(rt_ctx* c, const ComposedGather& g, const void* items, uint32_t n, uint32_t max_depth,
                                uint32_t spp, uint32_t seed, void* out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = path_query_args_ok(c, g.kind, n, spp);
  if (r < 0) return r;
  if (n == 0) {
    c->*g.kind.last = rt_radiance_stats();
    (c->*g.kind.state).batches_timed = 0;
    if (stats) *stats = c->*g.kind.last;
    return RT_OK;
  }
  r = query_from_host(c, c->*g.kind.state, g.kind.what, (const rt_ray*)items, n, out, g.kind.out_stride,
                      [&](const void* d_items, void* d_out) {
    return launch_composed_gather(c, g, d_items, n, max_depth, spp, seed, d_out, stats != nullptr);
  });
  if (r < 0) return r;
  if (stats) return composed_gather_stats(c, g, stats);
  return RT_OK;
}

int rt_probe_gather_stats(rt_ctx* c, rt_radiance_stats* out) { return composed_gather_stats(c, cg_probe, out); }
int rt_gather_probes_device(rt_ctx* c, const void* dev_probes, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                            void* dev_out) {
  return composed_gather_device(c, cg_probe, dev_probes, n, max_depth, spp, seed, dev_out);
}
int rt_gather_probes(rt_ctx* c, const rt_probe* probes, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                     rt_probe_sh9* out, rt_radiance_stats* stats) {
  return composed_gather_host(c, cg_probe, probes, n, max_depth, spp, seed, out, stats);
}

int rt_directional_gather_stats(rt_ctx* c, rt_radiance_stats* out) { return composed_gather_stats(c, cg_directional, out); }
int rt_gather_directional_device(rt_ctx* c, const void* dev_points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                                 void* dev_out) {
  return composed_gather_device(c, cg_directional, dev_points, n, max_depth, spp, seed, dev_out);
}
int rt_gather_directional(rt_ctx* c, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                          rt_directional* out, rt_radiance_stats* stats) {
  return composed_gather_host(c, cg_directional, points, n, max_depth, spp, seed, out, stats);
}

// ---- lightmap bakes: the texel rule of mi355rt.h as four launches (k_bake.hip.h), then the gather path and the scatter
// the size of an atlas, refused under the caller's name `w`
static int atlas_size_ok(rt_ctx* c, const std::string& w, uint32_t width, uint32_t height) {
  if (width == 0 || height == 0) return fail(c, RT_ERR_INVALID, w + ": width and height must be >= 1");
  if ((uint64_t)width * height > (1ull << 24)) return fail(c, RT_ERR_INVALID, w + ": width * height must be <= 2^24");
  return RT_OK;
}
// a refusal of one of the stages of a composed entry, under the entry's name: "lightmap: bake atlas: entry 3: ..."
static int refused_under(rt_ctx* c, const char* what, int code) { return fail(c, code, std::string(what) + ": " + c->error); }
// width, height and pad_base of a bake or an atlas bake
static int bake_size_ok(rt_ctx* c, const std::string& w, uint32_t width, uint32_t height, uint32_t pad_base) {
  const int r = atlas_size_ok(c, w, width, height);
  if (r < 0) return r;
  if ((uint64_t)pad_base + (uint64_t)width * height > (1ull << 31)) return fail(c, RT_ERR_INVALID, w + ": pad_base + width * height must be <= 2^31");
  return RT_OK;
}
static int bake_desc_ok(rt_ctx* c, const rt_bake_desc* d) {
  if (!d) return fail(c, RT_ERR_INVALID, "bake: NULL descriptor");
  if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return fail(c, RT_ERR_INVALID, "bake: reserved words must be 0");
  return bake_size_ok(c, "bake", d->width, d->height, d->pad_base);
}
// the scene is there and has a draw command for every instance
static int bake_scene_ready(rt_ctx* c, const char* what, bool lights) {
  const int r = query_scene_ready(c, what, lights);
  if (r < 0) return r;
  if (!c->draw_commands.ptr || c->draw_commands.size < (size_t)c->n_instances * 16)
    return fail(c, RT_ERR_NOT_READY,
                std::string(what) + ": the scene has no draw command for every instance (upload RT_KIND_DRAW_COMMANDS)");
  return RT_OK;
}
// ... and d->inst is one of them
static int bake_scene_ready(rt_ctx* c, const rt_bake_desc* d, bool lights) {
  const int r = bake_scene_ready(c, "bake", lights);
  if (r < 0) return r;
  if (d->inst >= c->n_instances) return fail(c, RT_ERR_INVALID, "bake: inst is not an instance of the scene");
  return RT_OK;
}
// the override UVs of a host entry -> the bake's staging array; *d_uv = that, or null for the scene's
static int bake_stage_uv(rt_ctx* c, const char* what, const float* atlas_uv, uint32_t n_uv_vertices, const void** d_uv) {
  *d_uv = nullptr;
  if (!atlas_uv) return RT_OK;
  if (n_uv_vertices != c->n_verts)
    return fail(c, RT_ERR_INVALID, std::string(what) + ": n_uv_vertices must be the scene's vertex count");
  const int r = ensure_buffer(c, c->bk.uv, (size_t)n_uv_vertices * 8, true);
  if (r < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(c->bk.uv.ptr, atlas_uv, (size_t)n_uv_vertices * 8, hipMemcpyHostToDevice, c->stream));
  *d_uv = c->bk.uv.ptr;
  return RT_OK;
}
// Enqueue the owner pass, the counts and their scan: afterwards d_owner (null: the bake's own map) holds the owner map,
// d_count the number of covered texels, and A everything the emit launch needs but its outputs.
static int bake_front(rt_ctx* c, const rt_bake_desc* d, const void* d_uv, void* d_owner, void* d_count, rtk::BakeArgs& A) {
  const uint32_t texels = d->width * d->height;
  int r;
  if (!d_owner) {
    if ((r = ensure_buffer(c, c->bk.owner, (size_t)texels * 4, true)) < 0) return r;
    d_owner = c->bk.owner.ptr;
  }
  A = rtk::BakeArgs();
  A.n_blocks = (texels + 255u) / 256u;
  if ((r = ensure_buffer(c, c->bk.blocks, (size_t)A.n_blocks * 4, true)) < 0) return r;
  A.auv = d_uv ? (const float2*)d_uv : (const float2*)c->uv.ptr;
  A.draw = (const uint4*)c->draw_commands.ptr;
  A.owner = (uint32_t*)d_owner;
  A.block_count = (uint32_t*)c->bk.blocks.ptr;
  A.inst = d->inst;
  A.W = d->width;
  A.H = d->height;
  A.pad_base = d->pad_base;
  A.t_max = d->t_max;
  A.n_tris = c->n_tris;
  A.tiles_x = (d->width + 7u) / 8u;
  A.tiles_y = (d->height + 7u) / 8u;
  A.bands = (A.tiles_y + RT_BAKE_BAND_TILES - 1u) / RT_BAKE_BAND_TILES;
  A.n_chunks = (c->n_tris + 63u) / 64u;
  DevScene S = dev_scene(c);
  HIP_TRY(c, hipMemsetAsync(d_owner, 0xff, (size_t)texels * 4, c->stream));   // RT_BAKE_NONE
  // one wave per (64 triangles, band) item up to what the device holds; the waves stride over the rest
  const uint64_t items = (uint64_t)A.n_chunks * A.bands;
  const uint32_t owner_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 3) / 4, (uint64_t)c->num_cus * 8));
  hipLaunchKernelGGL(rtk::k_bake_owner, dim3(owner_blocks), dim3(256), 0, c->stream, S, A);
  hipLaunchKernelGGL(rtk::k_bake_count, dim3(A.n_blocks), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, A.block_count, A.n_blocks, (uint32_t*)d_count);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}
// Enqueue the emit launch: the first min(n, cap) points and texel indices, in ascending texel order
static int bake_emit(rt_ctx* c, rtk::BakeArgs& A, void* d_points, void* d_texels, uint32_t cap) {
  if (cap == 0) return RT_OK;
  A.points = (float4*)d_points;
  A.texels = (uint32_t*)d_texels;
  A.cap = cap;
  DevScene S = dev_scene(c);
  hipLaunchKernelGGL(rtk::k_bake_emit, dim3(A.n_blocks), dim3(256), 0, c->stream, S, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

// The host entries of the point pass (rt_bake_points, rt_bake_atlas_points), around the front and the emit launch of their
// kind.  Before them: the bake's own count word and staging arrays for m records.
static int bake_points_room(rt_ctx* c, uint32_t m) {
  int r;
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.points, (size_t)m * sizeof(rt_gather_point), true)) < 0) return r;
  return ensure_buffer(c, c->bk.texels, (size_t)m * 4, true);
}
// Behind them, one fence: the count and the m staged records come back together, the first min(n, cap) of them go to the
// caller; with them owner_bytes of the owner map d_owner into owner_host (0: the caller did not ask for the map).
static int bake_points_back(rt_ctx* c, uint32_t m, rt_gather_point* points_out, uint32_t* texels_out, uint32_t* n_out,
                            const void* d_owner, void* owner_host, size_t owner_bytes) {
  uint32_t n = 0;
  std::vector<rt_gather_point> points(m);
  std::vector<uint32_t> tex(m);
  HIP_TRY(c, hipMemcpyAsync(&n, c->bk.count.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  if (m) {
    HIP_TRY(c, hipMemcpyAsync(points.data(), c->bk.points.ptr, (size_t)m * sizeof(rt_gather_point), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(tex.data(), c->bk.texels.ptr, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (owner_bytes) HIP_TRY(c, hipMemcpyAsync(owner_host, d_owner, owner_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t got = std::min(n, m);
  if (got) {
    std::memcpy(points_out, points.data(), (size_t)got * sizeof(rt_gather_point));
    std::memcpy(texels_out, tex.data(), (size_t)got * 4);
  }
  *n_out = n;
  return RT_OK;
}

// A whole bake (rt_bake_irradiance, rt_bake_atlas_irradiance) behind its front.  First the one host read of the count
// between the point pass and the gather, and the bake's arrays for *n points ...
static int bake_count_room(rt_ctx* c, uint32_t* n) {
  int r;
  *n = 0;
  HIP_TRY(c, hipMemcpyAsync(n, c->bk.count.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((r = ensure_buffer(c, c->bk.points, (size_t)*n * sizeof(rt_gather_point), true)) < 0) return r;
  return ensure_buffer(c, c->bk.texels, (size_t)*n * 4, true);
}
// ... for an irradiance bake also their results and the atlas (a directional bake has arrays of its own, below) ...
static int bake_gather_room(rt_ctx* c, uint32_t texels, uint32_t* n) {
  int r;
  if ((r = bake_count_room(c, n)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.results, (size_t)*n * sizeof(rt_irradiance), true)) < 0) return r;
  return ensure_buffer(c, c->bk.atlas, (size_t)texels * sizeof(rt_irradiance), true);
}
// ... then, behind the emit launch of the bake's kind for those n points: the gather on them and the scatter kernel of the
// bake's kind on its owner map d_owner, enqueued; the atlas stays in bk.atlas ...
static int bake_gather_scatter(rt_ctx* c, uint32_t texels, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed, bool detail,
                               void (*scatter)(rtk::BakeScatterArgs), const void* d_owner) {
  int r;
  if ((r = path_query_device(c, pq_gather, c->bk.points.ptr, n, max_depth, spp, seed, c->bk.results.ptr, detail)) < 0) return r;
  rtk::BakeScatterArgs B;
  B.owner = d_owner;
  B.texels = (const uint32_t*)c->bk.texels.ptr;
  B.results = (const float4*)c->bk.results.ptr;
  B.atlas = (float4*)c->bk.atlas.ptr;
  B.n_texels = texels;
  B.n = n;
  hipLaunchKernelGGL(scatter, dim3((texels + 255u) / 256u), dim3(256), 0, c->stream, B);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}
// ... and, for the bakes that end there, the atlas to the caller.
static int bake_gather_tail(rt_ctx* c, uint32_t texels, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                            rt_irradiance* atlas_out, uint32_t* n_covered_out, rt_radiance_stats* stats,
                            void (*scatter)(rtk::BakeScatterArgs), const void* d_owner) {
  int r;
  if ((r = bake_gather_scatter(c, texels, n, max_depth, spp, seed, stats != nullptr, scatter, d_owner)) < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(atlas_out, c->bk.atlas.ptr, (size_t)texels * sizeof(rt_irradiance), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_covered_out) *n_covered_out = n;
  if (stats) return path_query_stats(c, pq_gather, stats);
  return RT_OK;
}

int rt_bake_points_device(rt_ctx* c, const rt_bake_desc* d, const void* dev_atlas_uv, void* dev_points, void* dev_texels,
                          uint32_t cap, void* dev_count, void* dev_owner) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_desc_ok(c, d);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, "bake", {dev_count, {dev_points, cap != 0}, {dev_texels, cap != 0}, optional_array(dev_owner),
                                         optional_array(dev_atlas_uv)})) < 0)
    return r;
  if ((r = bake_scene_ready(c, d, false)) < 0) return r;
  rtk::BakeArgs A;
  if ((r = bake_front(c, d, dev_atlas_uv, dev_owner, dev_count, A)) < 0) return r;
  return bake_emit(c, A, dev_points, dev_texels, std::min(cap, d->width * d->height));
}

int rt_bake_points(rt_ctx* c, const rt_bake_desc* d, const float* atlas_uv, uint32_t n_uv_vertices, rt_gather_point* points_out,
                   uint32_t* texels_out, uint32_t cap, uint32_t* n_out, int32_t* owner_out) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_desc_ok(c, d);
  if (r < 0) return r;
  if (!n_out || (cap != 0 && (!points_out || !texels_out))) return fail(c, RT_ERR_INVALID, "bake: NULL array");
  if ((r = bake_scene_ready(c, d, false)) < 0) return r;
  const void* d_uv;
  if ((r = bake_stage_uv(c, "bake", atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  const uint32_t texels = d->width * d->height, m = std::min(cap, texels);
  rtk::BakeArgs A;
  if ((r = bake_points_room(c, m)) < 0) return r;
  if ((r = bake_front(c, d, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  if ((r = bake_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, m)) < 0) return r;
  return bake_points_back(c, m, points_out, texels_out, n_out, A.owner, owner_out, owner_out ? (size_t)texels * 4 : 0);
}

int rt_bake_irradiance(rt_ctx* c, const rt_bake_desc* d, const float* atlas_uv, uint32_t n_uv_vertices, uint32_t max_depth,
                       uint32_t spp, uint32_t seed, rt_irradiance* atlas_out, uint32_t* n_covered_out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_desc_ok(c, d);
  if (r < 0) return r;
  if (!atlas_out) return fail(c, RT_ERR_INVALID, "bake: NULL array");
  const uint32_t texels = d->width * d->height;
  if ((r = path_query_args_ok(c, pq_gather, texels, spp)) < 0) return r;
  if ((r = bake_scene_ready(c, d, true)) < 0) return r;
  const void* d_uv;
  if ((r = bake_stage_uv(c, "bake", atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  rtk::BakeArgs A;
  if ((r = bake_front(c, d, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  uint32_t n;
  if ((r = bake_gather_room(c, texels, &n)) < 0) return r;
  if ((r = bake_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, n)) < 0) return r;
  return bake_gather_tail(c, texels, n, max_depth, spp, seed, atlas_out, n_covered_out, stats, rtk::k_bake_scatter, A.owner);
}

// ---- atlas bakes: a list of (instance, rectangle) entries into one atlas (mi355rt.h "atlas bakes"; k_atlas_* of k_bake.hip.h)
static const char* const kAtlas = "bake atlas";
// everything the limits say about the descriptor and the entries that needs no scene
static int bake_atlas_desc_ok(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries) {
  const std::string w(kAtlas);
  if (!d) return fail(c, RT_ERR_INVALID, w + ": NULL descriptor");
  if (!entries) return fail(c, RT_ERR_INVALID, w + ": NULL entries");
  if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return fail(c, RT_ERR_INVALID, w + ": reserved words must be 0");
  if (d->n_entries == 0 || d->n_entries > 65536) return fail(c, RT_ERR_INVALID, w + ": n_entries must be 1 .. 65536");
  const int r = bake_size_ok(c, w, d->width, d->height, d->pad_base);
  if (r < 0) return r;
  for (uint32_t e = 0; e < d->n_entries; e++) {
    const rt_bake_rect& q = entries[e];
    const std::string at = w + ": entry " + std::to_string(e);
    if (q.reserved[0] | q.reserved[1] | q.reserved[2]) return fail(c, RT_ERR_INVALID, at + ": reserved words must be 0");
    if (q.width == 0 || q.height == 0) return fail(c, RT_ERR_INVALID, at + ": width and height must be >= 1");
    if ((uint64_t)q.x + q.width > d->width || (uint64_t)q.y + q.height > d->height)
      return fail(c, RT_ERR_INVALID, at + ": the rectangle is not inside the atlas");
  }
  return RT_OK;
}
// the scene is there, has a draw command for every instance, and every entry's inst is one of them
static int bake_atlas_scene_ready(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, bool lights) {
  const int r = bake_scene_ready(c, kAtlas, lights);
  if (r < 0) return r;
  for (uint32_t e = 0; e < d->n_entries; e++)
    if (entries[e].inst >= c->n_instances)
      return fail(c, RT_ERR_INVALID, std::string(kAtlas) + ": entry " + std::to_string(e) + ": inst is not an instance of the scene");
  return RT_OK;
}
// The entries -> the bake's device array, through a pinned staging buffer of the bake's own: the caller's array is free when
// this returns and nothing waits for the stream - unless all kEntryRing buffers are still in flight, when the oldest copy is
// waited for.
static int bake_atlas_stage_entries(rt_ctx* c, const rt_bake_rect* entries, uint32_t n) {
  BakeState& k = c->bk;
  const size_t bytes = (size_t)n * sizeof(rt_bake_rect);
  int r = ensure_buffer(c, k.entries, bytes, true);
  if (r < 0) return r;
  const int slot = k.ring_next;
  k.ring_next = (slot + 1) % BakeState::kEntryRing;
  if (!k.ring_ev[slot]) HIP_TRY(c, hipEventCreateWithFlags(&k.ring_ev[slot], hipEventDisableTiming));
  if (k.ring_used[slot]) HIP_TRY(c, hipEventSynchronize(k.ring_ev[slot]));
  if (k.ring_bytes[slot] < bytes) {
    HIP_TRY(c, k.ring[slot].reset());
    k.ring_bytes[slot] = 0;
    HIP_TRY(c, hipHostMalloc(&k.ring[slot], bytes + bytes / 2, hipHostMallocDefault));
    k.ring_bytes[slot] = bytes + bytes / 2;
  }
  std::memcpy(k.ring[slot], entries, bytes);
  HIP_TRY(c, hipMemcpyAsync(k.entries.ptr, k.ring[slot], bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(k.ring_ev[slot], c->stream));
  k.ring_used[slot] = true;
  return RT_OK;
}
// Enqueue the work list, the owner pass, the counts and their scan: afterwards d_owner (null: the bake's own map) holds the
// 64-bit owner map, d_count the number of covered texels, and A everything the emit launch needs but its outputs.
static int bake_atlas_front(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, const void* d_uv, void* d_owner,
                            void* d_count, rtk::BakeAtlasArgs& A) {
  const uint32_t texels = d->width * d->height, n = d->n_entries;
  int r;
  if (!d_owner) {
    if ((r = ensure_buffer(c, c->bk.owner64, (size_t)texels * 8, true)) < 0) return r;
    d_owner = c->bk.owner64.ptr;
  }
  A = rtk::BakeAtlasArgs();
  A.n_blocks = (texels + 255u) / 256u;
  if ((r = ensure_buffer(c, c->bk.blocks, (size_t)A.n_blocks * 4, true)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.items, ((size_t)n + 1) * 8, true)) < 0) return r;
  if ((r = bake_atlas_stage_entries(c, entries, n)) < 0) return r;
  A.auv = d_uv ? (const float2*)d_uv : (const float2*)c->uv.ptr;
  A.draw = (const uint4*)c->draw_commands.ptr;
  A.entries = (const uint4*)c->bk.entries.ptr;
  A.owner = (unsigned long long*)d_owner;
  A.items = (unsigned long long*)c->bk.items.ptr;
  A.block_count = (uint32_t*)c->bk.blocks.ptr;
  A.W = d->width;
  A.H = d->height;
  A.pad_base = d->pad_base;
  A.t_max = d->t_max;
  A.n_tris = c->n_tris;
  A.n_entries = n;
  DevScene S = dev_scene(c);
  HIP_TRY(c, hipMemsetAsync(d_owner, 0xff, (size_t)texels * 8, c->stream));   // RT_ATLAS_NONE
  // The item total stays on the device.  What the host knows is a bound, every entry with all triangles of the scene: one wave
  // per item of that up to what the device holds; the waves stride over the true list.
  uint64_t bound = 0;
  for (uint32_t e = 0; e < n; e++)
    bound += (uint64_t)((c->n_tris + 63u) / 64u) * (((entries[e].height + 7u) / 8u + RT_BAKE_BAND_TILES - 1u) / RT_BAKE_BAND_TILES);
  const uint32_t owner_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((bound + 3) / 4, (uint64_t)c->num_cus * 8));
  hipLaunchKernelGGL(rtk::k_atlas_items, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_atlas_scan, dim3(1), dim3(1024), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_atlas_owner, dim3(owner_blocks), dim3(256), 0, c->stream, S, A);
  hipLaunchKernelGGL(rtk::k_atlas_count, dim3(A.n_blocks), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, A.block_count, A.n_blocks, (uint32_t*)d_count);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}
static int bake_atlas_emit(rt_ctx* c, rtk::BakeAtlasArgs& A, void* d_points, void* d_texels, uint32_t cap) {
  if (cap == 0) return RT_OK;
  A.points = (float4*)d_points;
  A.texels = (uint32_t*)d_texels;
  A.cap = cap;
  DevScene S = dev_scene(c);
  hipLaunchKernelGGL(rtk::k_atlas_emit, dim3(A.n_blocks), dim3(256), 0, c->stream, S, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_bake_atlas_points_device(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, const void* dev_atlas_uv,
                                void* dev_points, void* dev_texels, uint32_t cap, void* dev_count, void* dev_owner) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_atlas_desc_ok(c, d, entries);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, kAtlas, {dev_count, {dev_points, cap != 0}, {dev_texels, cap != 0}, optional_array(dev_owner),
                                        optional_array(dev_atlas_uv)})) < 0)
    return r;
  if ((r = bake_atlas_scene_ready(c, d, entries, false)) < 0) return r;
  rtk::BakeAtlasArgs A;
  if ((r = bake_atlas_front(c, d, entries, dev_atlas_uv, dev_owner, dev_count, A)) < 0) return r;
  return bake_atlas_emit(c, A, dev_points, dev_texels, std::min(cap, d->width * d->height));
}

int rt_bake_atlas_points(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, const float* atlas_uv,
                         uint32_t n_uv_vertices, rt_gather_point* points_out, uint32_t* texels_out, uint32_t cap, uint32_t* n_out,
                         int32_t* owner_out) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_atlas_desc_ok(c, d, entries);
  if (r < 0) return r;
  if (!n_out || (cap != 0 && (!points_out || !texels_out))) return fail(c, RT_ERR_INVALID, std::string(kAtlas) + ": NULL array");
  if ((r = bake_atlas_scene_ready(c, d, entries, false)) < 0) return r;
  const void* d_uv;
  if ((r = bake_stage_uv(c, kAtlas, atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  const uint32_t texels = d->width * d->height, m = std::min(cap, texels);
  rtk::BakeAtlasArgs A;
  std::vector<uint64_t> map(owner_out ? texels : 0);
  if ((r = bake_points_room(c, m)) < 0) return r;
  if ((r = bake_atlas_front(c, d, entries, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  if ((r = bake_atlas_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, m)) < 0) return r;
  if ((r = bake_points_back(c, m, points_out, texels_out, n_out, A.owner, map.data(), map.size() * 8)) < 0) return r;
  for (size_t i = 0; i < map.size(); i++) {   // (entry << 32) | triangle -> {entry, triangle}; all ones -> {-1, -1}
    owner_out[2 * i] = (int32_t)(uint32_t)(map[i] >> 32);
    owner_out[2 * i + 1] = (int32_t)(uint32_t)map[i];
  }
  return RT_OK;
}

int rt_bake_atlas_irradiance(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, const float* atlas_uv,
                             uint32_t n_uv_vertices, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_irradiance* atlas_out,
                             uint32_t* n_covered_out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_atlas_desc_ok(c, d, entries);
  if (r < 0) return r;
  if (!atlas_out) return fail(c, RT_ERR_INVALID, std::string(kAtlas) + ": NULL array");
  const uint32_t texels = d->width * d->height;
  if ((r = path_query_args_ok(c, pq_gather, texels, spp)) < 0) return r;
  if ((r = bake_atlas_scene_ready(c, d, entries, true)) < 0) return r;
  const void* d_uv;
  if ((r = bake_stage_uv(c, kAtlas, atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  rtk::BakeAtlasArgs A;
  if ((r = bake_atlas_front(c, d, entries, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  uint32_t n;
  if ((r = bake_gather_room(c, texels, &n)) < 0) return r;
  if ((r = bake_atlas_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, n)) < 0) return r;
  return bake_gather_tail(c, texels, n, max_depth, spp, seed, atlas_out, n_covered_out, stats, rtk::k_atlas_scatter, A.owner);
}

// ---- atlas dilation: the nearest-texel gutter fill of mi355rt.h "atlas dilation" as three launches (k_dilate.hip.h).  No
// scene, no renderer state: only the context's device and stream.
static const char* const kDilate = "dilate atlas";
static int dilate_desc_ok(rt_ctx* c, const rt_dilate_desc* d, const void* atlas) {
  const std::string w(kDilate);
  if (!d) return fail(c, RT_ERR_INVALID, w + ": NULL descriptor");
  if (!atlas) return fail(c, RT_ERR_INVALID, w + ": NULL atlas");
  if (d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3] | d->reserved[4])
    return fail(c, RT_ERR_INVALID, w + ": reserved words must be 0");
  const int r = atlas_size_ok(c, w, d->width, d->height);
  if (r < 0) return r;
  if (d->radius > RT_DILATE_MAX_RADIUS) return fail(c, RT_ERR_INVALID, w + ": radius must be <= 24");
  return RT_OK;
}
// Enqueue mask, source and apply on the context's stream.  d_src null: the source map lives in the dilation's own scratch;
// d_filled null: nothing is counted.
static int launch_dilate(rt_ctx* c, const rt_dilate_desc* d, void* d_atlas, void* d_src, void* d_filled) {
  const uint32_t texels = d->width * d->height;
  rtk::DilateArgs A;
  A.W = d->width;
  A.H = d->height;
  A.R = d->radius;
  A.wpr = (d->width + 63u) / 64u;
  A.tiles_x = (d->width + RT_DILATE_TILE - 1u) / RT_DILATE_TILE;
  const uint32_t tiles_y = (d->height + RT_DILATE_TILE - 1u) / RT_DILATE_TILE;
  const uint32_t n_words = A.H * A.wpr;   // <= 2^24: a row of W texels has at most W words
  int r;
  if ((r = ensure_buffer(c, c->dl.bitmap, (size_t)n_words * 8, true)) < 0) return r;
  if (!d_src) {
    if ((r = ensure_buffer(c, c->dl.src, (size_t)texels * 4, true)) < 0) return r;
    d_src = c->dl.src.ptr;
  }
  A.atlas = (float4*)d_atlas;
  A.bitmap = (uint64_t*)c->dl.bitmap.ptr;
  A.src = (uint32_t*)d_src;
  A.filled = (uint32_t*)d_filled;
  if (d_filled) HIP_TRY(c, hipMemsetAsync(d_filled, 0, 4, c->stream));
  hipLaunchKernelGGL(rtk::k_dilate_mask, dim3((n_words + 3u) / 4u), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_dilate_source, dim3(A.tiles_x * tiles_y), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(rtk::k_dilate_apply, dim3((texels + 255u) / 256u), dim3(256), 0, c->stream, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_dilate_atlas_device(rt_ctx* c, const rt_dilate_desc* d, void* dev_atlas, void* dev_src, void* dev_filled) {
  if (!c) return RT_ERR_INVALID;
  int r = dilate_desc_ok(c, d, dev_atlas);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, kDilate, {dev_atlas, optional_array(dev_src), optional_array(dev_filled)})) < 0) return r;
  return launch_dilate(c, d, dev_atlas, dev_src, dev_filled);
}

int rt_dilate_atlas(rt_ctx* c, const rt_dilate_desc* d, float* atlas, uint32_t* src_out, uint32_t* filled_out) {
  if (!c) return RT_ERR_INVALID;
  int r = dilate_desc_ok(c, d, atlas);
  if (r < 0) return r;
  const size_t texels = (size_t)d->width * d->height;
  DilateState& st = c->dl;
  // the atlas goes up and comes back; the source map comes from the scratch that launch_dilate makes room for; the count has
  // its room (16 bytes, as every buffer has at least) whether or not it is asked for
  return staged_call(c,
                     {{st.atlas, atlas, texels * 16, STAGE_IN | STAGE_OUT},
                      {st.src, src_out, texels * 4, STAGE_OUT | STAGE_MADE, true, src_out != nullptr},
                      {st.filled, filled_out, 4, filled_out ? STAGE_OUT : STAGE_ROOM, false}},
                     [&] { return launch_dilate(c, d, st.atlas.ptr, nullptr, filled_out ? st.filled.ptr : nullptr); });
}

// ---- atlas denoise: the edge-stopped a-trous filter of mi355rt.h "atlas denoise" as one index build and `passes` launches
// (k_denoise.hip.h).  No scene, no renderer state: only the context's device and stream.
static const char* const kDenoise = "denoise atlas";
static int denoise_desc_ok(rt_ctx* c, const rt_denoise_desc* d, const void* in, const void* points, const void* texels,
                           uint32_t n, const void* out) {
  const std::string w(kDenoise);
  if (!d) return fail(c, RT_ERR_INVALID, w + ": NULL descriptor");
  if (!in || !out || (n != 0 && (!points || !texels))) return fail(c, RT_ERR_INVALID, w + ": NULL array");
  if (d->reserved[0]) return fail(c, RT_ERR_INVALID, w + ": reserved words must be 0");
  const int r = atlas_size_ok(c, w, d->width, d->height);
  if (r < 0) return r;
  if (d->step == 0 || d->passes == 0) return fail(c, RT_ERR_INVALID, w + ": step and passes must be >= 1");
  // step >= 1, so more than three passes always exceed the limit; below that the shift cannot overflow
  if (d->passes > 3 || d->step > RT_DENOISE_MAX_STEP || (d->step << (d->passes - 1)) > RT_DENOISE_MAX_STEP)
    return fail(c, RT_ERR_INVALID, w + ": step << (passes - 1) must be <= 4");
  if (n > d->width * d->height) return fail(c, RT_ERR_INVALID, w + ": more points than texels");
  return RT_OK;
}
// Enqueue the index build and the passes on the context's stream.  Pass p reads the atlas the pass before it wrote (the
// first one `d_in`) and writes `d_out` when an even number of passes follows it, else the scratch atlas: the last pass lands
// in `d_out` and `d_in` is only read.
static int launch_denoise(rt_ctx* c, const rt_denoise_desc* d, const void* d_in, const void* d_points, const void* d_texels,
                          uint32_t n, void* d_out) {
  const uint32_t texels = d->width * d->height;
  int r;
  if ((r = ensure_buffer(c, c->dn.index, (size_t)texels * 4, true)) < 0) return r;
  if (d->passes > 1 && (r = ensure_buffer(c, c->dn.scratch, (size_t)texels * 16, true)) < 0) return r;
  rtk::DenoiseArgs A;
  A.points = (const float4*)d_points;
  A.texels = (const uint32_t*)d_texels;
  A.index = (uint32_t*)c->dn.index.ptr;
  A.W = d->width;
  A.H = d->height;
  A.n = n;
  A.tiles_x = (d->width + RT_DENOISE_TILE_W - 1u) / RT_DENOISE_TILE_W;
  const uint32_t tiles_y = (d->height + RT_DENOISE_TILE_H - 1u) / RT_DENOISE_TILE_H;
  A.normal_cos = d->normal_cos;
  A.plane_eps = d->plane_eps;
  A.md2 = d->max_dist * d->max_dist;
  A.in = (const uint4*)d_in;
  A.out = nullptr;
  A.step = d->step;
  HIP_TRY(c, hipMemsetAsync(c->dn.index.ptr, 0xff, (size_t)texels * 4, c->stream));
  if (n) hipLaunchKernelGGL(rtk::k_denoise_index, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, A);
  for (uint32_t p = 0; p < d->passes; p++) {
    A.out = (uint4*)(((d->passes - 1u - p) & 1u) ? c->dn.scratch.ptr : d_out);
    A.step = d->step << p;
    hipLaunchKernelGGL(rtk::k_denoise_pass, dim3(A.tiles_x * tiles_y), dim3(256), 0, c->stream, A);
    A.in = A.out;
  }
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_denoise_atlas_device(rt_ctx* c, const rt_denoise_desc* d, const void* dev_in, const void* dev_points,
                            const void* dev_texels, uint32_t n, void* dev_out) {
  if (!c) return RT_ERR_INVALID;
  int r = denoise_desc_ok(c, d, dev_in, dev_points, dev_texels, n, dev_out);
  if (r < 0) return r;
  if (dev_in == dev_out) return fail(c, RT_ERR_INVALID, std::string(kDenoise) + ": the output must not be the input");
  if ((r = caller_arrays_ok(c, kDenoise, {dev_in, dev_out, {dev_points, n != 0}, {dev_texels, n != 0}})) < 0) return r;
  return launch_denoise(c, d, dev_in, dev_points, dev_texels, n, dev_out);
}

int rt_denoise_atlas(rt_ctx* c, const rt_denoise_desc* d, const float* atlas_in, const rt_gather_point* points,
                     const uint32_t* texels, uint32_t n, float* atlas_out) {
  if (!c) return RT_ERR_INVALID;
  int r = denoise_desc_ok(c, d, atlas_in, points, texels, n, atlas_out);
  if (r < 0) return r;
  const size_t bytes = (size_t)d->width * d->height * 16;
  DenoiseState& st = c->dn;
  return staged_call(c,
                     {{st.in, atlas_in, bytes, STAGE_IN},
                      {st.out, atlas_out, bytes, STAGE_OUT},
                      {st.points, points, (size_t)n * sizeof(rt_gather_point), STAGE_IN, true, n != 0},
                      {st.texels, texels, (size_t)n * 4, STAGE_IN, true, n != 0}},
                     [&] {
                       return launch_denoise(c, d, st.in.ptr, n ? st.points.ptr : nullptr, n ? st.texels.ptr : nullptr, n,
                                             st.out.ptr);
                     });
}

// ---- frame denoise: the G-buffer-guided a-trous filter of mi355rt.h "frame denoise" as one prepare launch (or its cached
// outputs), `passes` launches in the form picked per pass, and the finish (k_frame_denoise.hip.h).
static const char* const kFrameDenoise = "frame denoise";
static int frame_denoise_desc_ok(rt_ctx* c, const rt_frame_denoise_desc* d) {
  if (!d) return refuse(c, kFrameDenoise, "NULL descriptor");
  if (d->reserved[0] | d->reserved[1]) return refuse(c, kFrameDenoise, "reserved words must be 0");
  if (d->flags & ~(RT_FRAME_DENOISE_DEMODULATE | RT_FRAME_DENOISE_SAME_INSTANCE)) return refuse(c, kFrameDenoise, "unknown flag bit");
  if (d->passes == 0 || d->passes > RT_FRAME_DENOISE_MAX_PASSES) return refuse(c, kFrameDenoise, "passes must be 1 .. 5");
  if (d->step == 0) return refuse(c, kFrameDenoise, "step must be >= 1");
  // step <= 16 and passes <= 5: the shift cannot overflow
  if (d->step > RT_FRAME_DENOISE_MAX_STEP || (d->step << (d->passes - 1)) > RT_FRAME_DENOISE_MAX_STEP)
    return refuse(c, kFrameDenoise, "step << (passes - 1) must be <= 16");
  return RT_OK;
}
// what a call needs of the context, checked before anything is enqueued
static int frame_denoise_ctx_ok(rt_ctx* c, const rt_frame_denoise_desc* d) {
  const std::string w(kFrameDenoise);
  if (c->fd.form == 1 && (d->step << (d->passes - 1)) > RT_FRAME_LDS_MAX_STEP)
    return refuse(c, kFrameDenoise, "the LDS form is forced (rt_set_frame_denoise_form) and a spacing above 4 has no LDS window");
  if (c->dist.active) return refuse(c, kFrameDenoise, "the context is a rank of a sharded image: its G-buffer covers only its own rows");
  if (c->stripe_count > 1) return refuse(c, kFrameDenoise, "stripes are on: the G-buffer covers only this context's rows");
  if (!c->width || !c->render_target.ptr || !c->accum.ptr) return fail(c, RT_ERR_NOT_READY, w + ": no screen (rt_resize first)");
  if (c->accum_stale)
    return fail(c, RT_ERR_INVALID, w + ": the bound accumulation buffer was dropped by rt_resize: call rt_bind_accum again");
  if (c->gbuf_gen == 0) return fail(c, RT_ERR_NOT_READY, w + ": no G-buffer yet; call compute first");
  // frame motion follows the G-buffer's indices into the scene arrays: they must be the arrays that G-buffer was traced in
  if (c->ft.on && (c->ft.desc.flags & RT_FRAME_TEMPORAL_MOTION) && c->fm.gbuf_scene_gen != c->fm.scene_gen)
    return fail(c, RT_ERR_NOT_READY, "frame motion: the scene changed since the last compute()");
  return RT_OK;
}
static const void* const frame_lds_fns[RT_FRAME_LDS_MAX_STEP] = {
    (const void*)rtk::k_frame_pass_lds<1>, (const void*)rtk::k_frame_pass_lds<2>, (const void*)rtk::k_frame_pass_lds<3>,
    (const void*)rtk::k_frame_pass_lds<4>};
// The form of a pass at spacing s: the forced one, else what was measured faster at 1920 x 1080 (the staged
// form at spacings 1 and 2, 77 against 139 us and 87 against 134 us; the direct form at 4, 131 against 165 us).  Spacing 3 was
// not timed and keeps the staged form.
static int frame_pass_form(const rt_ctx* c, uint32_t s) {
  if (s > RT_FRAME_LDS_MAX_STEP) return 2;
  if (c->fd.form) return c->fd.form;
  return s >= 4 ? 2 : 1;
}
// Enqueue a whole call on the context's stream: `d` and the context have been checked.  dev_out: W * H float4.
static int frame_denoise_run(rt_ctx* c, const rt_frame_denoise_desc* d, void* dev_out) {
  DenoiseFrameState& fd = c->fd;
  fd.wanted = true;
  const size_t npx = (size_t)c->width * c->height;
  // the G-buffer of the last compute(), as rt_read_gbuffer finds it
  const void *pa = c->render_target.ptr, *pn = c->g_normal.ptr, *pd = c->g_depth.ptr;
  bool plane_ok = c->albedo_plane_valid;
  if (c->gbuf_slot >= 0 && (size_t)c->gbuf_slot < c->spec.slots.size()) {
    const DevFrameSlot& sl = c->spec.slots[c->gbuf_slot];
    pn = sl.normal_id;
    pd = sl.depth;
    if (sl.albedo != (uint32_t*)c->render_target.ptr) {
      pa = sl.albedo;   // a plane of the batch: present() does not write there
      plane_ok = true;
    } else if (fd.keep_valid) {
      pa = fd.albedo_keep.ptr;
      plane_ok = true;
    }
  }
  const uint32_t demod = d->flags & RT_FRAME_DENOISE_DEMODULATE;
  const bool hit = fd.cache_valid && fd.cache_gen == c->gbuf_gen && fd.cache_epoch == c->epoch && fd.cache_flags == demod;
  if (!hit && !plane_ok)
    return fail(c, RT_ERR_NOT_READY, std::string(kFrameDenoise) + ": the albedo plane was overwritten by present(); call compute first");
  int r;
  if ((r = ensure_buffer(c, fd.col, npx * 16, false)) < 0) return r;
  FrameTemporalState& ft = c->ft;
  FrameMotionState& fm = c->fm;
  const bool motion = ft.on && (ft.desc.flags & RT_FRAME_TEMPORAL_MOTION) != 0u;
  if (ft.on) {
    for (int k = 0; k < 2; k++) {
      if ((r = ensure_buffer(c, ft.hist[k], npx * 16, false)) < 0) return r;
      if ((r = ensure_buffer(c, ft.mom[k], npx * 8, false)) < 0) return r;
      if ((r = ensure_buffer(c, ft.guide[k], npx * 32, false)) < 0) return r;
    }
    if ((r = ensure_buffer(c, ft.integ, npx * 16, false)) < 0) return r;
    if (motion) {
      if ((r = ensure_buffer(c, fm.carry, npx * 32, false)) < 0) return r;
      for (int k = 0; k < 2; k++)
        if ((r = ensure_buffer(c, fm.pix_id[k], npx * 4, false)) < 0) return r;
      if ((r = ensure_buffer(c, fm.snap_pos, std::max<size_t>(16, (size_t)c->n_verts * 16), false)) < 0) return r;
      if ((r = ensure_buffer(c, fm.snap_xf, std::max<size_t>(64, (size_t)c->n_instances * 64), false)) < 0) return r;
    }
  } else if ((r = ensure_buffer(c, fd.guide, npx * 32, false)) < 0) {
    return r;
  }
  if ((r = ensure_buffer(c, fd.mod, npx * 16, false)) < 0) return r;
  if ((r = ensure_buffer(c, fd.ping, npx * 16, false)) < 0) return r;
  if (d->passes > 1 && (r = ensure_buffer(c, fd.pong, npx * 16, false)) < 0) return r;
  if (!fd.ev_ready) {
    for (EventPair& p : fd.ev) {
      HIP_TRY(c, hipEventCreate(&p.a));
      HIP_TRY(c, hipEventCreate(&p.b));
    }
    HIP_TRY(c, hipEventCreate(&ft.ev.a));
    HIP_TRY(c, hipEventCreate(&ft.ev.b));
    HIP_TRY(c, hipEventCreate(&fm.ev.a));
    HIP_TRY(c, hipEventCreate(&fm.ev.b));
    fd.ev_ready = true;
  }
  fd.timed = false;
  fd.last = {};
  fd.last.passes = d->passes;
  fd.last.cache_hit = hit ? 1 : 0;
  fd.last.temporal = ft.on ? (hit ? 2 : 1) : 0;
  if (!hit) {
    fd.cache_valid = false;
    const int next = ft.cur ^ 1;
    rtk::FramePrepareArgs A;
    A.accum = accum_ptr(c);
    A.albedo = (const uint32_t*)pa;
    A.normal_id = (const float4*)pn;
    A.depth = (const float*)pd;
    A.col = (float4*)fd.col.ptr;
    A.guide = (float4*)(ft.on ? ft.guide[next].ptr : fd.guide.ptr);
    A.mod = (float4*)fd.mod.ptr;
    A.flags = d->flags;
    HIP_TRY(c, hipEventRecord(fd.ev[0].a, c->stream));
    hipLaunchKernelGGL(rtk::k_frame_prepare, dim3((c->width + 255u) / 256u, c->height), dim3(256), 0, c->stream, A, c->uniforms);
    HIP_TRY(c, hipEventRecord(fd.ev[0].b, c->stream));
    if (ft.on) {   // one run of prepare is one frame of history
      if (ft.have && ft.hist_flags != demod) ft.have = false, ft.frames = 0;   // the stored quantity changes: dropped
      // frame motion: a snapshot of other counts is of another scene - dropped, as by rt_reset_frame_history
      if (motion && ft.have && (fm.snap_verts != c->n_verts || fm.snap_inst != c->n_instances)) ft.have = false, ft.frames = 0;
      const uint32_t* ids = fm.ids_from == FrameMotionState::IDS_WORLD      ? (const uint32_t*)c->world.tlas.ord
                            : fm.ids_from == FrameMotionState::IDS_DECLARED ? (const uint32_t*)fm.ids.ptr
                                                                            : nullptr;
      if (motion) {
        rtk::FrameMotionArgs M;
        M.normal_id = (const float4*)pn;
        M.guide = (const float4*)ft.guide[next].ptr;
        M.topo = (const float4*)c->topology.ptr;
        M.pos = (const float4*)c->pos.ptr;
        M.inst = (const float4*)c->instances.ptr;
        M.ids = ids;
        M.snap_pos = (const float4*)fm.snap_pos.ptr;
        M.snap_xf = (const float4*)fm.snap_xf.ptr;
        M.carry = (float4*)fm.carry.ptr;
        M.pix_id = (uint32_t*)fm.pix_id[next].ptr;
        M.W = c->width;
        M.H = c->height;
        // a count is the count of ITS array: nothing is followed into an array that is not on the device
        M.n_tris = c->topology.ptr ? c->n_tris : 0u;
        M.n_verts = c->pos.ptr ? c->n_verts : 0u;
        M.n_inst = c->instances.ptr ? c->n_instances : 0u;
        M.have = ft.have ? 1u : 0u;
        HIP_TRY(c, hipEventRecord(fm.ev.a, c->stream));
        hipLaunchKernelGGL(rtk::k_frame_motion, dim3((c->width + 255u) / 256u, c->height), dim3(256), 0, c->stream, M);
        HIP_TRY(c, hipEventRecord(fm.ev.b, c->stream));
        fm.ran = true;
        fd.last.motion = 1;
      }
      const rt_scene_uniforms& V = ft.prev_uniforms;
      rtk::FrameTemporalArgs T;
      T.col = (const float4*)fd.col.ptr;
      T.guide = (const float4*)ft.guide[next].ptr;
      T.prev_hist = (const float4*)ft.hist[ft.cur].ptr;
      T.prev_mom = (const float2*)ft.mom[ft.cur].ptr;
      T.prev_guide = (const float4*)ft.guide[ft.cur].ptr;
      T.integ = (float4*)ft.integ.ptr;
      T.hist = (float4*)ft.hist[next].ptr;
      T.mom = (float2*)ft.mom[next].ptr;
      T.W = c->width;
      T.H = c->height;
      T.flags = ft.desc.flags;
      T.have = ft.have ? 1u : 0u;
      T.max_history = (float)ft.desc.max_history;
      T.var_history = (float)ft.desc.var_history;
      T.normal_cos = ft.desc.normal_cos;
      T.plane_eps = ft.desc.plane_eps;
      for (int k = 0; k < 3; k++) {
        T.eye[k] = V.camera.origin[k];
        T.ll[k] = V.camera.lower_left[k];
        T.hor[k] = V.camera.horizontal[k];
        T.ver[k] = V.camera.vertical[k];
      }
      T.jit[0] = V.jitter[0];
      T.jit[1] = V.jitter[1];
      HIP_TRY(c, hipEventRecord(ft.ev.a, c->stream));
      if (motion)
        hipLaunchKernelGGL(rtk::k_frame_temporal_motion, dim3((c->width + 255u) / 256u, c->height), dim3(256), 0, c->stream, T,
                           (const float4*)fm.carry.ptr, (const uint32_t*)fm.pix_id[ft.cur].ptr);
      else
        hipLaunchKernelGGL(rtk::k_frame_temporal, dim3((c->width + 255u) / 256u, c->height), dim3(256), 0, c->stream, T);
      HIP_TRY(c, hipEventRecord(ft.ev.b, c->stream));
      if (motion) {   // the snapshot of this frame, behind its last reader on the stream
        if (c->n_verts && c->pos.ptr)
          HIP_TRY(c, hipMemcpyAsync(fm.snap_pos.ptr, c->pos.ptr, (size_t)c->n_verts * 16, hipMemcpyDeviceToDevice, c->stream));
        if (c->n_instances && c->instances.ptr)
          hipLaunchKernelGGL(rtk::k_frame_motion_scatter, dim3((c->n_instances + 255u) / 256u), dim3(256), 0, c->stream,
                             (const float4*)c->instances.ptr, ids, (float4*)fm.snap_xf.ptr, c->n_instances);
        fm.snap_verts = c->n_verts;
        fm.snap_inst = c->n_instances;
      }
      ft.cur = next;
      ft.have = true;
      ft.hist_flags = demod;
      ft.frames++;
      ft.prev_uniforms = c->uniforms;
    }
    fd.cache_gen = c->gbuf_gen;
    fd.cache_epoch = c->epoch;
    fd.cache_flags = demod;
    fd.cache_valid = true;
  }
  rtk::FramePassArgs P;
  P.guide = (const float4*)(ft.on ? ft.guide[ft.cur].ptr : fd.guide.ptr);
  P.W = c->width;
  P.H = c->height;
  P.tiles_x = (c->width + RT_FRAME_TILE_W - 1u) / RT_FRAME_TILE_W;
  const uint32_t tiles_y = (c->height + RT_FRAME_TILE_H - 1u) / RT_FRAME_TILE_H;
  P.flags = d->flags;
  P.normal_cos = d->normal_cos;
  P.plane_eps = d->plane_eps;
  P.sigma_lum = d->sigma_lum;
  P.in = (const float4*)(ft.on ? ft.integ.ptr : fd.col.ptr);
  for (uint32_t p = 0; p < d->passes; p++) {
    P.out = (float4*)((p & 1u) ? fd.pong.ptr : fd.ping.ptr);
    P.step = d->step << p;
    const int form = frame_pass_form(c, P.step);
    fd.last.form[p] = (uint8_t)form;
    HIP_TRY(c, hipEventRecord(fd.ev[2 + p].a, c->stream));
    if (form == 1) {
      void* args[] = {&P};
      HIP_TRY(c, hipLaunchKernel(frame_lds_fns[P.step - 1u], dim3(P.tiles_x * tiles_y), dim3(256), args, 0, c->stream));
    } else {
      hipLaunchKernelGGL(rtk::k_frame_pass_direct, dim3((c->width + 255u) / 256u, c->height), dim3(256), 0, c->stream, P);
    }
    HIP_TRY(c, hipEventRecord(fd.ev[2 + p].b, c->stream));
    P.in = P.out;
  }
  HIP_TRY(c, hipEventRecord(fd.ev[1].a, c->stream));
  hipLaunchKernelGGL(rtk::k_frame_finish, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, P.in,
                     (const float4*)fd.mod.ptr, (float4*)dev_out, (uint32_t)npx);
  HIP_TRY(c, hipEventRecord(fd.ev[1].b, c->stream));
  HIP_TRY(c, hipGetLastError());
  fd.timed = true;
  return RT_OK;
}

int rt_denoise_frame_device(rt_ctx* c, const rt_frame_denoise_desc* d, void* dev_out) {
  int r = frame_denoise_desc_ok(c, d);
  if (r < 0) return r;
  if (!c) return RT_ERR_INVALID;
  if (!dev_out) return refuse(c, kFrameDenoise, "NULL output");
  if ((r = frame_denoise_ctx_ok(c, d)) < 0) return r;
  if (dev_out == (void*)accum_ptr(c) || dev_out == c->accum.ptr)
    return refuse(c, kFrameDenoise, "the output must not be the accumulation buffer");
  if ((r = caller_arrays_ok(c, kFrameDenoise, {dev_out})) < 0) return r;
  return frame_denoise_run(c, d, dev_out);
}

int rt_denoise_frame(rt_ctx* c, const rt_frame_denoise_desc* d, float* out, size_t cap_bytes) {
  int r = frame_denoise_desc_ok(c, d);
  if (r < 0) return r;
  if (!c) return RT_ERR_INVALID;
  if (!out) return refuse(c, kFrameDenoise, "NULL output");
  if ((r = frame_denoise_ctx_ok(c, d)) < 0) return r;
  const size_t bytes = (size_t)c->width * c->height * 16;
  if (cap_bytes < bytes) return refuse(c, kFrameDenoise, "output buffer too small");
  return staged_call(c, {{c->fd.out, out, bytes, STAGE_OUT, false}}, [&] { return frame_denoise_run(c, d, c->fd.out.ptr); });
}

int rt_set_present_denoise(rt_ctx* c, const rt_frame_denoise_desc* d) {
  if (!d) {
    if (!c) return RT_ERR_INVALID;
    c->fd.present_on = false;
    return RT_OK;
  }
  int r = frame_denoise_desc_ok(c, d);
  if (r < 0) return r;
  if (!c) return RT_ERR_INVALID;
  if (c->present_source || c->present_stale)
    return refuse(c, kFrameDenoise, "a present source is bound (rt_bind_present_source(NULL) first): present() cannot read both");
  if (c->dist.active)
    return refuse(c, kFrameDenoise, "the context is a rank of a sharded image (rt_dist_init): its G-buffer covers only its own rows");
  if (c->stripe_count > 1) return refuse(c, kFrameDenoise, "stripes are on (rt_set_stripes): the G-buffer covers only this context's rows");
  if (c->fd.form == 1 && (d->step << (d->passes - 1)) > RT_FRAME_LDS_MAX_STEP)
    return refuse(c, kFrameDenoise, "the LDS form is forced (rt_set_frame_denoise_form) and a spacing above 4 has no LDS window");
  c->fd.present_desc = *d;
  c->fd.present_on = true;
  c->fd.wanted = true;
  return RT_OK;
}

int rt_set_frame_denoise_form(rt_ctx* c, int form) {
  if (form < 0 || form > 2) return refuse(c, kFrameDenoise, "form must be 0 (auto), 1 (LDS) or 2 (direct)");
  if (!c) return RT_ERR_INVALID;
  if (form == 1 && c->fd.present_on &&
      (c->fd.present_desc.step << (c->fd.present_desc.passes - 1)) > RT_FRAME_LDS_MAX_STEP)
    return refuse(c, kFrameDenoise, "present() filters at a spacing above 4, which has no LDS window");
  c->fd.form = form;
  return RT_OK;
}

int rt_frame_denoise_stats(rt_ctx* c, rt_frame_denoise_report* out) {
  if (!c || !out) return RT_ERR_INVALID;
  DenoiseFrameState& fd = c->fd;
  if (fd.timed) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!fd.last.cache_hit) HIP_TRY(c, hipEventElapsedTime(&fd.last.prepare_ms, fd.ev[0].a, fd.ev[0].b));
    if (fd.last.temporal == 1) HIP_TRY(c, hipEventElapsedTime(&fd.last.temporal_ms, c->ft.ev.a, c->ft.ev.b));
    if (fd.last.motion == 1) HIP_TRY(c, hipEventElapsedTime(&fd.last.motion_ms, c->fm.ev.a, c->fm.ev.b));
    HIP_TRY(c, hipEventElapsedTime(&fd.last.finish_ms, fd.ev[1].a, fd.ev[1].b));
    for (uint32_t p = 0; p < fd.last.passes; p++) HIP_TRY(c, hipEventElapsedTime(&fd.last.pass_ms[p], fd.ev[2 + p].a, fd.ev[2 + p].b));
    fd.timed = false;
  }
  *out = fd.last;
  return RT_OK;
}

// ---- frame temporal: the stage between the prepare stage and the first pass (mi355rt.h "THE FRAME TEMPORAL RULE";
// k_frame_temporal.hip.h).  It runs inside frame_denoise_run, exactly when the prepare stage does.
static const char* const kFrameTemporal = "frame temporal";
// the history, and the prepare outputs that were made beside it: the next call runs both stages again
static void frame_history_drop(rt_ctx* c) {
  c->ft.have = false;
  c->ft.frames = 0;
  c->fd.cache_valid = false;
}

int rt_set_frame_temporal(rt_ctx* c, const rt_frame_temporal_desc* d) {
  if (d) {
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return refuse(c, kFrameTemporal, "reserved words must be 0");
    if (d->flags & ~(RT_FRAME_TEMPORAL_SAME_INSTANCE | RT_FRAME_TEMPORAL_MOTION)) return refuse(c, kFrameTemporal, "unknown flag bit");
    if (d->max_history == 0 || d->max_history > RT_FRAME_TEMPORAL_MAX_HISTORY)
      return refuse(c, kFrameTemporal, "max_history must be 1 .. 256");
    if (d->var_history == 0) return refuse(c, kFrameTemporal, "var_history must be >= 1");
    // the motion stage follows G-buffer indices into the scene arrays: there is nothing to follow them into before a scene
    if ((d->flags & RT_FRAME_TEMPORAL_MOTION) && !(c && c->n_tris && c->n_verts && c->n_instances))
      return refuse(c, kFrameTemporal, "RT_FRAME_TEMPORAL_MOTION needs an uploaded scene: set it after the first upload or rt_world_update");
  }
  if (!c) return RT_ERR_INVALID;
  frame_history_drop(c);
  c->fm.ran = false;
  c->ft.on = d != nullptr;
  if (d) c->ft.desc = *d;
  return RT_OK;
}

int rt_reset_frame_history(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  frame_history_drop(c);
  return RT_OK;
}

int rt_read_frame_history(rt_ctx* c, float* colour, float* moments, size_t cap_pixels, uint32_t* frames_out) {
  if (!c) return RT_ERR_INVALID;
  const FrameTemporalState& ft = c->ft;
  if (frames_out) *frames_out = ft.frames;
  if (!colour && !moments) return RT_OK;
  if (!ft.on) return refuse(c, kFrameTemporal, "the stage is off (rt_set_frame_temporal)");
  if (!ft.have || !ft.hist[ft.cur].ptr) return fail(c, RT_ERR_NOT_READY, "frame temporal: no history yet");
  const size_t npx = (size_t)c->width * c->height;
  if (cap_pixels < npx) return refuse(c, kFrameTemporal, "output buffers too small");
  HIP_TRY(c, hipSetDevice(c->device));
  if (colour) HIP_TRY(c, hipMemcpyAsync(colour, ft.hist[ft.cur].ptr, npx * 16, hipMemcpyDeviceToHost, c->stream));
  if (moments) HIP_TRY(c, hipMemcpyAsync(moments, ft.mom[ft.cur].ptr, npx * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---- frame motion (mi355rt.h "THE FRAME MOTION RULE"; k_frame_motion.hip.h): the stage itself runs inside frame_denoise_run
static const char* const kFrameMotion = "frame motion";
int rt_set_frame_motion_ids(rt_ctx* c, const uint32_t* ids, uint32_t n) {
  if (!ids) return refuse(c, kFrameMotion, "NULL ids");
  if (!c) return RT_ERR_INVALID;
  if (n != c->n_instances || !n) return refuse(c, kFrameMotion, "n must be the instance count of the uploaded instance array");
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t p = 0; p < n; p++) {
    if (ids[p] >= n || seen[ids[p]]) return refuse(c, kFrameMotion, "the ids must be a permutation of 0 .. n - 1");
    seen[ids[p]] = 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // no kernel in flight may still read the old ids: the buffer is rewritten in place
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int r = ensure_buffer(c, c->fm.ids, (size_t)n * 4, false);
  if (r < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(c->fm.ids.ptr, ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->fm.ids_from = FrameMotionState::IDS_DECLARED;
  return RT_OK;
}

int rt_read_frame_motion(rt_ctx* c, float* carry, size_t cap_pixels) {
  if (!c) return RT_ERR_INVALID;
  if (!carry) return refuse(c, kFrameMotion, "NULL output");
  const FrameMotionState& fm = c->fm;
  if (!fm.ran || !fm.carry.ptr) return fail(c, RT_ERR_NOT_READY, "frame motion: the stage has not run yet");
  const size_t npx = (size_t)c->width * c->height;
  if (cap_pixels < npx) return refuse(c, kFrameMotion, "output buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(carry, fm.carry.ptr, npx * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---- lightmaps: the stages above back to back on the context's stream, and the encode stage (mi355rt.h "lightmaps";
// k_encode.hip.h).  Bytes per texel of a format; 0 = not a format.
static const char* const kLightmap = "lightmap";
static const char* const kEncode = "encode atlas";
static size_t lightmap_texel_bytes(uint32_t format) {
  return format == RT_LIGHTMAP_F32 ? 16 : format == RT_LIGHTMAP_F16 ? 8 : format == RT_LIGHTMAP_RGBE8 ? 4 : 0;
}
// Enqueue the encode of `texels` texels at d_in into d_out, which is another array: a copy for RT_LIGHTMAP_F32, else the kernel
static int launch_encode(rt_ctx* c, uint32_t texels, uint32_t format, const void* d_in, void* d_out) {
  if (format == RT_LIGHTMAP_F32) {
    HIP_TRY(c, hipMemcpyAsync(d_out, d_in, (size_t)texels * 16, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
  }
  rtk::EncodeArgs A;
  A.in = (const uint4*)d_in;
  A.out = d_out;
  A.n = texels;
  A.format = format;
  hipLaunchKernelGGL(rtk::k_encode_atlas, dim3((texels + 255u) / 256u), dim3(256), 0, c->stream, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}
// everything the limits say that needs neither a scene nor the output
static int lightmap_desc_ok(rt_ctx* c, const rt_lightmap_desc* d, const rt_bake_rect* entries, rt_bake_atlas_desc* bake) {
  const std::string w(kLightmap);
  if (!d) return fail(c, RT_ERR_INVALID, w + ": NULL descriptor");
  if (d->reserved[0]) return fail(c, RT_ERR_INVALID, w + ": reserved words must be 0");
  if (!lightmap_texel_bytes(d->format)) return fail(c, RT_ERR_INVALID, w + ": format must be RT_LIGHTMAP_F32, _F16 or _RGBE8");
  if (d->passes > 3) return fail(c, RT_ERR_INVALID, w + ": passes must be <= 3");
  if (d->passes && (d->step == 0 || d->step > RT_DENOISE_MAX_STEP || (d->step << (d->passes - 1)) > RT_DENOISE_MAX_STEP))
    return fail(c, RT_ERR_INVALID, w + ": step must be >= 1 and step << (passes - 1) <= 4");
  if (d->dilate_radius > RT_DILATE_MAX_RADIUS) return fail(c, RT_ERR_INVALID, w + ": dilate_radius must be <= 24");
  *bake = rt_bake_atlas_desc();
  bake->width = d->width;
  bake->height = d->height;
  bake->pad_base = d->pad_base;
  bake->t_max = d->t_max;
  bake->n_entries = d->n_entries;
  int r = bake_atlas_desc_ok(c, bake, entries);
  if (r < 0) return refused_under(c, kLightmap, r);
  if ((r = path_query_args_ok(c, pq_gather, d->width * d->height, d->spp)) < 0) return refused_under(c, kLightmap, r);
  return RT_OK;
}
// The finishing chain of both lightmap forms, filter then gutter fill.  Its atlas-sized arrays, asked for before the first
// launch: growing one later would wait for the stream (ensure_buffer).  The stages ask again for what is theirs, and find it.
static int lightmap_finish_room(rt_ctx* c, const rt_lightmap_desc* d) {
  const size_t texels = (size_t)d->width * d->height;
  int r;
  if (d->passes) {
    if ((r = ensure_buffer(c, c->lm.filtered, texels * 16, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->dn.index, texels * 4, true)) < 0) return r;
    if (d->passes > 1 && (r = ensure_buffer(c, c->dn.scratch, texels * 16, true)) < 0) return r;
  }
  if (d->dilate_radius) {
    if ((r = ensure_buffer(c, c->dl.bitmap, (size_t)d->height * ((d->width + 63u) / 64u) * 8, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->dl.src, texels * 4, true)) < 0) return r;
    if ((r = ensure_buffer(c, c->lm.filled, 16, false)) < 0) return r;
  }
  return RT_OK;
}
// Enqueue the chain on one f32 layer with the bake's n points: the filter into lm.filtered when passes != 0, then the gutter
// fill in place when dilate_radius != 0, counting into d_filled unless that is null.  *finished: where the layer then lies,
// `layer` itself or lm.filtered.
static int lightmap_finish_layer(rt_ctx* c, const rt_lightmap_desc* d, void* layer, uint32_t n, void* d_filled, void** finished) {
  int r;
  if (d->passes) {
    const rt_denoise_desc f = {d->width, d->height, d->step, d->passes, d->normal_cos, d->plane_eps, d->max_dist, {0}};
    if ((r = launch_denoise(c, &f, layer, c->bk.points.ptr, c->bk.texels.ptr, n, c->lm.filtered.ptr)) < 0) return r;
    layer = c->lm.filtered.ptr;
  }
  if (d->dilate_radius) {
    const rt_dilate_desc g = {d->width, d->height, d->dilate_radius, {0}};
    if ((r = launch_dilate(c, &g, layer, nullptr, d_filled)) < 0) return r;
  }
  *finished = layer;
  return RT_OK;
}
// the output of a scalar lightmap holds width * height texels of the format
static int lightmap_out_bytes_ok(rt_ctx* c, const rt_lightmap_desc* d, size_t out_bytes) {
  if (out_bytes < (size_t)d->width * d->height * lightmap_texel_bytes(d->format))
    return fail(c, RT_ERR_INVALID, std::string(kLightmap) + ": out_bytes is below width * height texels of the format");
  return RT_OK;
}
// The whole bake behind its checks.  d_out null: the host form, `out` receives the encoded atlas; else the device form.
static int lightmap_bake(rt_ctx* c, const rt_lightmap_desc* d, const rt_bake_atlas_desc* bake, const rt_bake_rect* entries,
                         const void* d_uv, void* out, void* d_out, uint32_t* n_covered_out, uint32_t* n_filled_out,
                         rt_radiance_stats* stats) {
  const uint32_t texels = d->width * d->height;
  const size_t atlas_bytes = (size_t)texels * 16, out_bytes = (size_t)texels * lightmap_texel_bytes(d->format);
  const bool count_filled = n_filled_out && d->dilate_radius;
  int r;
  // every atlas-sized array before the first launch (lightmap_finish_room)
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.atlas, atlas_bytes, true)) < 0) return r;
  if ((r = lightmap_finish_room(c, d)) < 0) return r;
  if (!d_out && d->format != RT_LIGHTMAP_F32 && (r = ensure_buffer(c, c->lm.encoded, out_bytes, true)) < 0) return r;
  // the point pass, once: its points and texels stay in the bake's arrays for the filter
  rtk::BakeAtlasArgs A;
  if ((r = bake_atlas_front(c, bake, entries, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  uint32_t n;
  if ((r = bake_gather_room(c, texels, &n)) < 0) return r;
  if ((r = bake_atlas_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, n)) < 0) return r;
  if ((r = bake_gather_scatter(c, texels, n, d->max_depth, d->spp, d->seed, stats != nullptr, rtk::k_atlas_scatter, A.owner)) < 0)
    return r;
  void* current;
  if ((r = lightmap_finish_layer(c, d, c->bk.atlas.ptr, n, count_filled ? c->lm.filled.ptr : nullptr, &current)) < 0) return r;
  uint32_t filled = 0;
  if (d_out) {
    if ((r = launch_encode(c, texels, d->format, current, d_out)) < 0) return r;
  } else {
    const void* from = current;
    if (d->format != RT_LIGHTMAP_F32) {
      if ((r = launch_encode(c, texels, d->format, current, c->lm.encoded.ptr)) < 0) return r;
      from = c->lm.encoded.ptr;
    }
    HIP_TRY(c, hipMemcpyAsync(out, from, out_bytes, hipMemcpyDeviceToHost, c->stream));
  }
  if (count_filled) HIP_TRY(c, hipMemcpyAsync(&filled, c->lm.filled.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  if (!d_out || count_filled) HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_covered_out) *n_covered_out = n;
  if (n_filled_out) *n_filled_out = filled;
  if (stats) return path_query_stats(c, pq_gather, stats);
  return RT_OK;
}

int rt_bake_atlas_lightmap(rt_ctx* c, const rt_lightmap_desc* d, const rt_bake_rect* entries, const float* atlas_uv,
                           uint32_t n_uv_vertices, void* out, size_t out_bytes, uint32_t* n_covered_out, uint32_t* n_filled_out,
                           rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  rt_bake_atlas_desc bake;
  int r = lightmap_desc_ok(c, d, entries, &bake);
  if (r < 0) return r;
  if (!out) return fail(c, RT_ERR_INVALID, std::string(kLightmap) + ": NULL array");
  if ((r = lightmap_out_bytes_ok(c, d, out_bytes)) < 0) return r;
  if ((r = bake_atlas_scene_ready(c, &bake, entries, true)) < 0) return refused_under(c, kLightmap, r);
  const void* d_uv;
  if ((r = bake_stage_uv(c, kLightmap, atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  return lightmap_bake(c, d, &bake, entries, d_uv, out, nullptr, n_covered_out, n_filled_out, stats);
}

int rt_bake_atlas_lightmap_device(rt_ctx* c, const rt_lightmap_desc* d, const rt_bake_rect* entries, const void* dev_atlas_uv,
                                  void* dev_out, size_t out_bytes, uint32_t* n_covered_out, uint32_t* n_filled_out,
                                  rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  rt_bake_atlas_desc bake;
  int r = lightmap_desc_ok(c, d, entries, &bake);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, kLightmap, {dev_out, optional_array(dev_atlas_uv)})) < 0) return r;
  if ((r = lightmap_out_bytes_ok(c, d, out_bytes)) < 0) return r;
  if ((r = bake_atlas_scene_ready(c, &bake, entries, true)) < 0) return refused_under(c, kLightmap, r);
  return lightmap_bake(c, d, &bake, entries, dev_atlas_uv, nullptr, dev_out, n_covered_out, n_filled_out, stats);
}

// ---- directional lightmaps: the atlas bake and the finished lightmap around the directional gather (mi355rt.h "directional
// lightmaps"; k_dir_scatter of k_directional.hip.h).  Four layers of an atlas, layer-major, in db_layers.
static const char* const kBakeDirectional = "bake directional";
static const char* const kDirLightmap = "directional lightmap";
// Behind the front of an atlas bake: the one host read of the count, the arrays for *n points, their results and the four
// layers, the emit launch, the directional gather on the points and the scatter, enqueued; the layers stay in db_layers.
static int directional_bake(rt_ctx* c, const char* what, uint32_t texels, rtk::BakeAtlasArgs& A, uint32_t max_depth, uint32_t spp,
                            uint32_t seed, bool detail, uint32_t* n_out) {
  int r;
  uint32_t n;
  if ((r = bake_count_room(c, &n)) < 0) return r;
  *n_out = n;
  if ((r = ensure_buffer(c, c->db_results, (size_t)n * sizeof(rt_directional), true)) < 0) return r;
  if ((r = ensure_buffer(c, c->db_layers, (size_t)texels * 4 * sizeof(rt_irradiance), true)) < 0) return r;
  if ((r = bake_atlas_emit(c, A, c->bk.points.ptr, c->bk.texels.ptr, n)) < 0) return r;
  if ((r = composed_gather_device(c, cg_directional, c->bk.points.ptr, n, max_depth, spp, seed, c->db_results.ptr, detail)) < 0)
    return refused_under(c, what, r);
  rtk::DirScatterArgs B;
  B.owner = A.owner;
  B.texels = (const uint32_t*)c->bk.texels.ptr;
  B.results = (const float4*)c->db_results.ptr;
  B.layers = (float4*)c->db_layers.ptr;
  B.n_texels = texels;
  B.n = n;
  hipLaunchKernelGGL(rtk::k_dir_scatter, dim3((texels + 255u) / 256u), dim3(256), 0, c->stream, B);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_bake_atlas_directional(rt_ctx* c, const rt_bake_atlas_desc* d, const rt_bake_rect* entries, const float* atlas_uv,
                              uint32_t n_uv_vertices, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_irradiance* layers_out,
                              uint32_t* n_covered_out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  int r = bake_atlas_desc_ok(c, d, entries);
  if (r < 0) return refused_under(c, kBakeDirectional, r);
  if (!layers_out) return fail(c, RT_ERR_INVALID, std::string(kBakeDirectional) + ": NULL array");
  const uint32_t texels = d->width * d->height;
  if ((r = path_query_args_ok(c, pq_directional, texels, spp)) < 0) return refused_under(c, kBakeDirectional, r);
  if ((r = bake_atlas_scene_ready(c, d, entries, true)) < 0) return refused_under(c, kBakeDirectional, r);
  const void* d_uv;
  if ((r = bake_stage_uv(c, kBakeDirectional, atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  rtk::BakeAtlasArgs A;
  if ((r = bake_atlas_front(c, d, entries, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  uint32_t n;
  if ((r = directional_bake(c, kBakeDirectional, texels, A, max_depth, spp, seed, stats != nullptr, &n)) < 0) return r;
  HIP_TRY(c, hipMemcpyAsync(layers_out, c->db_layers.ptr, (size_t)texels * 4 * sizeof(rt_irradiance), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_covered_out) *n_covered_out = n;
  if (stats) return rt_directional_gather_stats(c, stats);
  return RT_OK;
}

int rt_bake_atlas_directional_lightmap(rt_ctx* c, const rt_lightmap_desc* d, const rt_bake_rect* entries, const float* atlas_uv,
                                       uint32_t n_uv_vertices, void* out, size_t out_bytes, uint32_t* n_covered_out,
                                       uint32_t* n_filled_out, rt_radiance_stats* stats) {
  if (!c) return RT_ERR_INVALID;
  const std::string w(kDirLightmap);
  rt_bake_atlas_desc bake;
  int r = lightmap_desc_ok(c, d, entries, &bake);
  if (r < 0) return refused_under(c, kDirLightmap, r);
  if (d->format == RT_LIGHTMAP_RGBE8)
    return fail(c, RT_ERR_INVALID, w + ": format must be RT_LIGHTMAP_F32 or _F16 (band-1 coefficients are signed; RGBE8 zeroes negatives)");
  if (!out) return fail(c, RT_ERR_INVALID, w + ": NULL array");
  const uint32_t texels = d->width * d->height;
  const size_t atlas_bytes = (size_t)texels * 16, layer_bytes = (size_t)texels * lightmap_texel_bytes(d->format);
  if (out_bytes < 4 * layer_bytes)
    return fail(c, RT_ERR_INVALID, w + ": out_bytes is below four layers of width * height texels of the format");
  if ((r = bake_atlas_scene_ready(c, &bake, entries, true)) < 0) return refused_under(c, kDirLightmap, r);
  const void* d_uv;
  if ((r = bake_stage_uv(c, kDirLightmap, atlas_uv, n_uv_vertices, &d_uv)) < 0) return r;
  const bool count_filled = n_filled_out && d->dilate_radius;
  // every atlas-sized array before the first launch, as lightmap_bake does; the point-sized ones follow the read of the count
  if ((r = ensure_buffer(c, c->bk.count, 16, false)) < 0) return r;
  if ((r = ensure_buffer(c, c->db_layers, 4 * atlas_bytes, true)) < 0) return r;
  if ((r = ensure_buffer(c, c->db_encoded, 4 * layer_bytes, true)) < 0) return r;
  if ((r = lightmap_finish_room(c, d)) < 0) return r;
  rtk::BakeAtlasArgs A;
  if ((r = bake_atlas_front(c, &bake, entries, d_uv, nullptr, c->bk.count.ptr, A)) < 0) return r;
  uint32_t n;
  if ((r = directional_bake(c, kDirLightmap, texels, A, d->max_depth, d->spp, d->seed, stats != nullptr, &n)) < 0) return r;
  // filter, gutter and encode layer by layer, with the stages as they stand: the filtered layer is lm.filtered for each in
  // turn (the stream orders the layers), the gutter fill is in place, the encoded layers lie side by side in db_encoded
  for (uint32_t k = 0; k < 4u; k++) {
    void* current;
    if ((r = lightmap_finish_layer(c, d, (char*)c->db_layers.ptr + k * atlas_bytes, n,
                                   (count_filled && k == 0) ? c->lm.filled.ptr : nullptr, &current)) < 0)
      return r;
    if ((r = launch_encode(c, texels, d->format, current, (char*)c->db_encoded.ptr + k * layer_bytes)) < 0) return r;
  }
  uint32_t filled = 0;
  HIP_TRY(c, hipMemcpyAsync(out, c->db_encoded.ptr, 4 * layer_bytes, hipMemcpyDeviceToHost, c->stream));
  if (count_filled) HIP_TRY(c, hipMemcpyAsync(&filled, c->lm.filled.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_covered_out) *n_covered_out = n;
  if (n_filled_out) *n_filled_out = filled;
  if (stats) return rt_directional_gather_stats(c, stats);
  return RT_OK;
}

static int encode_args_ok(rt_ctx* c, uint32_t width, uint32_t height, uint32_t format, const void* in, const void* out,
                          size_t out_bytes) {
  const std::string w(kEncode);
  const int r = atlas_size_ok(c, w, width, height);
  if (r < 0) return r;
  if (!lightmap_texel_bytes(format)) return fail(c, RT_ERR_INVALID, w + ": format must be RT_LIGHTMAP_F32, _F16 or _RGBE8");
  if (!in || !out) return fail(c, RT_ERR_INVALID, w + ": NULL array");
  if (out_bytes < (size_t)width * height * lightmap_texel_bytes(format))
    return fail(c, RT_ERR_INVALID, w + ": out_bytes is below width * height texels of the format");
  return RT_OK;
}

int rt_encode_atlas_device(rt_ctx* c, uint32_t width, uint32_t height, uint32_t format, const void* dev_in, void* dev_out,
                           size_t out_bytes) {
  if (!c) return RT_ERR_INVALID;
  int r = encode_args_ok(c, width, height, format, dev_in, dev_out, out_bytes);
  if (r < 0) return r;
  if (dev_in == dev_out) return fail(c, RT_ERR_INVALID, std::string(kEncode) + ": the output must not be the input");
  if ((r = caller_arrays_ok(c, kEncode, {dev_in, dev_out})) < 0) return r;
  return launch_encode(c, width * height, format, dev_in, dev_out);
}

int rt_encode_atlas(rt_ctx* c, uint32_t width, uint32_t height, uint32_t format, const float* atlas_in, void* out,
                    size_t out_bytes) {
  if (!c) return RT_ERR_INVALID;
  int r = encode_args_ok(c, width, height, format, atlas_in, out, out_bytes);
  if (r < 0) return r;
  const uint32_t texels = width * height;
  const size_t bytes = (size_t)texels * lightmap_texel_bytes(format);
  if (format == RT_LIGHTMAP_F32) {   // the 16 bytes unchanged: nothing for the device to do
    if (out != (const void*)atlas_in) std::memmove(out, atlas_in, bytes);
    return RT_OK;
  }
  return staged_call(c, {{c->lm.in, atlas_in, (size_t)texels * 16, STAGE_IN}, {c->lm.encoded, out, bytes, STAGE_OUT}},
                     [&] { return launch_encode(c, texels, format, c->lm.in.ptr, c->lm.encoded.ptr); });
}

// ---- irradiance volumes (mi355rt.h "THE VOLUME RULE"; k_volume.hip.h): a grid of probes baked through the probe gather's
// device path, finished into windowed irradiance coefficients, sampled trilinearly, exported as texel layers.
static const char* const kVolume = "volume";
// everything the limits say about a descriptor; *n_out = nx * ny * nz
static int volume_desc_ok(rt_ctx* c, const rt_volume_desc* d, uint32_t* n_out) {
  if (!d) return refuse(c, kVolume, "NULL descriptor");
  if (d->nx == 0 || d->ny == 0 || d->nz == 0 || d->nx > 1024 || d->ny > 1024 || d->nz > 1024)
    return refuse(c, kVolume, "nx, ny and nz must be 1 .. 1024");
  const uint64_t n = (uint64_t)d->nx * d->ny * d->nz;
  if (n > (1ull << 24)) return refuse(c, kVolume, "nx * ny * nz must be <= 2^24");
  if ((uint64_t)d->pad_first + n > (1ull << 31)) return refuse(c, kVolume, "pad_first + nx * ny * nz must be <= 2^31");
  for (int a = 0; a < 3; a++) {
    if (!(std::isfinite(d->step[a]) && d->step[a] > 0.0f)) return refuse(c, kVolume, "step must be finite and > 0");
    if (!(std::isfinite(d->window[a]) && d->window[a] >= 0.0f)) return refuse(c, kVolume, "window must be finite and >= 0");
  }
  if (d->max_hit_fraction != d->max_hit_fraction) return refuse(c, kVolume, "max_hit_fraction must not be NaN");
  if (d->reserved) return refuse(c, kVolume, "reserved must be 0");
  *n_out = (uint32_t)n;
  return RT_OK;
}

// Enqueue a bake: the grid's probes into the probe gather's staging, its device path with its batching into d_out, the
// finish in place.
static int launch_bake_volume(rt_ctx* c, const rt_volume_desc& D, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                              void* d_out, bool detail) {
  int r = query_scene_ready(c, kVolume, true);
  if (r < 0) return r;
  if ((r = ensure_buffer(c, c->pr.in, (size_t)n * sizeof(rt_probe), true)) < 0) return r;
  hipLaunchKernelGGL(rtk::k_volume_probes, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, D, (float4*)c->pr.in.ptr, n);
  HIP_TRY(c, hipGetLastError());
  if ((r = launch_composed_gather(c, cg_probe, c->pr.in.ptr, n, max_depth, spp, seed, d_out, detail)) < 0)
    return refused_under(c, kVolume, r);
  const uint32_t n_vec = n * (uint32_t)(sizeof(rt_probe_sh9) / 16);
  hipLaunchKernelGGL(rtk::k_volume_finish, dim3((n_vec + 255u) / 256u), dim3(256), 0, c->stream, D, (float4*)d_out, n_vec);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_bake_volume_device(rt_ctx* c, const rt_volume_desc* desc, uint32_t max_depth, uint32_t spp, uint32_t seed, void* dev_out) {
  uint32_t n = 0;
  int r = volume_desc_ok(c, desc, &n);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if ((r = path_query_args_ok(c, pq_probe, n, spp)) < 0) return refused_under(c, kVolume, r);
  if ((r = caller_arrays_ok(c, kVolume, {dev_out})) < 0) return r;
  return launch_bake_volume(c, *desc, n, max_depth, spp, seed, dev_out, c->detailed_counters);
}

int rt_bake_volume(rt_ctx* c, const rt_volume_desc* desc, uint32_t max_depth, uint32_t spp, uint32_t seed, rt_probe_sh9* out,
                   rt_radiance_stats* stats) {
  uint32_t n = 0;
  int r = volume_desc_ok(c, desc, &n);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if ((r = path_query_args_ok(c, pq_probe, n, spp)) < 0) return refused_under(c, kVolume, r);
  if (!out) return fail(c, RT_ERR_INVALID, std::string(kVolume) + ": NULL array");
  r = staged_call(c, {{c->pr.out, out, (size_t)n * sizeof(rt_probe_sh9), STAGE_OUT}},
                  [&] { return launch_bake_volume(c, *desc, n, max_depth, spp, seed, c->pr.out.ptr, stats != nullptr); });
  if (r < 0) return r;
  if (stats) return composed_gather_stats(c, cg_probe, stats);
  return RT_OK;
}

// the arguments of a sample beside the descriptor; 1: nothing to do
static int volume_sample_args_ok(rt_ctx* c, uint32_t n, const void* volume, const void* points, const void* out) {
  const std::string w(kVolume);
  if (n >= (1u << 31)) return fail(c, RT_ERR_INVALID, w + ": too many points for one call (n must be below 2^31)");
  if (n == 0) return 1;
  if (!volume || !points || !out) return fail(c, RT_ERR_INVALID, w + ": NULL array");
  return RT_OK;
}
static int launch_sample_volume(rt_ctx* c, const rt_volume_desc& D, const void* d_volume, const void* d_points, uint32_t n,
                                void* d_out) {
  rtk::VolumeSampleArgs A;
  A.D = D;
  A.volume = (const float4*)d_volume;
  A.points = (const float4*)d_points;
  A.out = (float4*)d_out;
  A.n = n;
  hipLaunchKernelGGL(rtk::k_volume_sample, dim3((n + 31u) / 32u), dim3(256), 0, c->stream, A);   // 8 lanes per point
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_sample_volume_device(rt_ctx* c, const rt_volume_desc* desc, const void* dev_volume, const void* dev_points, uint32_t n,
                            void* dev_out) {
  uint32_t probes = 0;
  int r = volume_desc_ok(c, desc, &probes);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if ((r = volume_sample_args_ok(c, n, dev_volume, dev_points, dev_out)) != RT_OK) return r < 0 ? r : RT_OK;
  if ((r = caller_arrays_ok(c, kVolume, {dev_volume, dev_points, dev_out})) < 0) return r;
  return launch_sample_volume(c, *desc, dev_volume, dev_points, n, dev_out);
}

int rt_sample_volume(rt_ctx* c, const rt_volume_desc* desc, const rt_probe_sh9* volume, const rt_gather_point* points, uint32_t n,
                     rt_irradiance* out) {
  uint32_t probes = 0;
  int r = volume_desc_ok(c, desc, &probes);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if ((r = volume_sample_args_ok(c, n, volume, points, out)) != RT_OK) return r < 0 ? r : RT_OK;
  VolumeState& st = c->vol;
  return staged_call(c,
                     {{st.volume, volume, (size_t)probes * sizeof(rt_probe_sh9), STAGE_IN},
                      {st.points, points, (size_t)n * sizeof(rt_gather_point), STAGE_IN},
                      {st.out, out, (size_t)n * sizeof(rt_irradiance), STAGE_OUT}},
                     [&] { return launch_sample_volume(c, *desc, st.volume.ptr, st.points.ptr, n, st.out.ptr); });
}

// the arguments of an export beside the descriptor: the format is f32 or f16, the capacity holds seven layers
static int volume_encode_args_ok(rt_ctx* c, uint32_t probes, uint32_t format, const void* volume, const void* out, size_t cap) {
  const std::string w(kVolume);
  if (format == RT_LIGHTMAP_RGBE8) return refuse(c, kVolume, "RT_LIGHTMAP_RGBE8 cannot hold signed coefficients");
  if (format != RT_LIGHTMAP_F32 && format != RT_LIGHTMAP_F16) return refuse(c, kVolume, "format must be RT_LIGHTMAP_F32 or _F16");
  if (!c) return RT_ERR_INVALID;
  if (!volume || !out) return fail(c, RT_ERR_INVALID, w + ": NULL array");
  if (cap < 7 * (size_t)probes * lightmap_texel_bytes(format))
    return fail(c, RT_ERR_INVALID, w + ": the capacity is below seven layers of nx * ny * nz texels of the format");
  return RT_OK;
}
static int launch_volume_layers(rt_ctx* c, uint32_t probes, uint32_t format, const void* d_volume, void* d_out) {
  rtk::VolumeLayersArgs A;
  A.volume = (const uint4*)d_volume;
  A.out = d_out;
  A.n = probes;
  A.format = format;
  hipLaunchKernelGGL(rtk::k_volume_layers, dim3((7u * probes + 255u) / 256u), dim3(256), 0, c->stream, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_encode_volume_device(rt_ctx* c, const rt_volume_desc* desc, uint32_t format, const void* dev_volume, void* dev_out,
                            size_t cap) {
  uint32_t probes = 0;
  int r = volume_desc_ok(c, desc, &probes);
  if (r < 0) return r;
  if ((r = volume_encode_args_ok(c, probes, format, dev_volume, dev_out, cap)) < 0) return r;
  if (dev_volume == dev_out) return fail(c, RT_ERR_INVALID, std::string(kVolume) + ": the output must not be the input");
  if ((r = caller_arrays_ok(c, kVolume, {dev_volume, dev_out})) < 0) return r;
  return launch_volume_layers(c, probes, format, dev_volume, dev_out);
}

int rt_encode_volume(rt_ctx* c, const rt_volume_desc* desc, uint32_t format, const rt_probe_sh9* volume, void* out, size_t cap) {
  uint32_t probes = 0;
  int r = volume_desc_ok(c, desc, &probes);
  if (r < 0) return r;
  if ((r = volume_encode_args_ok(c, probes, format, volume, out, cap)) < 0) return r;
  const size_t in_bytes = (size_t)probes * sizeof(rt_probe_sh9), out_bytes = 7 * (size_t)probes * lightmap_texel_bytes(format);
  return staged_call(c, {{c->vol.volume, volume, in_bytes, STAGE_IN}, {c->vol.encoded, out, out_bytes, STAGE_OUT}},
                     [&] { return launch_volume_layers(c, probes, format, c->vol.volume.ptr, c->vol.encoded.ptr); });
}

// ---- reflection probes (mi355rt.h "THE REFLECTION RULE"; k_reflection.hip.h): octahedral radiance maps captured through the
// radiance query's kernel, one path item per (texel, sample), and their GGX-filtered chains.
static const char* const kReflection = "reflection";
struct ReflectionShape {
  uint32_t size_log2;
  uint32_t map, chain;   // texels of level 0, of a whole chain
};
enum { RF_CAPTURE = 1, RF_FILTER = 2 };
// everything the limits say about a descriptor and n, for the parts (RF_*) an entry runs
static int reflection_desc_ok(rt_ctx* c, const rt_reflection_desc* d, uint32_t n, int parts, ReflectionShape* sh) {
  if (!d) return refuse(c, kReflection, "NULL descriptor");
  if (d->size < 8 || d->size > 512 || (d->size & (d->size - 1u))) return refuse(c, kReflection, "size must be a power of two in 8 .. 512");
  if (d->levels < 2) return refuse(c, kReflection, "levels must be >= 2");
  if (d->levels > 32 || (d->size >> (d->levels - 1u)) < 4) return refuse(c, kReflection, "size >> (levels - 1) must be >= 4");
  if ((parts & RF_CAPTURE) && (d->spt == 0 || d->spt > 65536)) return refuse(c, kReflection, "spt must be 1 .. 65536");
  if ((parts & RF_FILTER) && (d->filter_samples < 64 || d->filter_samples > 4096 || (d->filter_samples & 63u)))
    return refuse(c, kReflection, "filter_samples must be a multiple of 64 in 64 .. 4096");
  for (int k = 0; k < 4; k++)
    if (d->reserved[k]) return refuse(c, kReflection, "reserved must be 0");
  sh->size_log2 = (uint32_t)__builtin_ctz(d->size);
  sh->map = d->size * d->size;
  sh->chain = 0;
  for (uint32_t m = 0; m < d->levels; m++) sh->chain += (d->size >> m) * (d->size >> m);
  if ((uint64_t)n * sh->chain >= (1ull << 31)) return refuse(c, kReflection, "n * texels of a chain must be below 2^31");
  return RT_OK;
}
// the host entries of capture and bake: every probe's pads stay below 2^31
static int reflection_pads_ok(rt_ctx* c, const rt_probe* probes, uint32_t n, const ReflectionShape& sh) {
  for (uint32_t i = 0; i < n; i++)
    if ((uint64_t)probes[i].pad + sh.map > (1ull << 31))
      return fail(c, RT_ERR_INVALID, std::string(kReflection) + ": probe " + std::to_string(i) + ": pad + size * size must be <= 2^31");
  return RT_OK;
}
static void reflection_no_work(rt_ctx* c) {
  c->rf_last = rt_radiance_stats();
  c->rf.batches_timed = 0;
}

// Enqueue a capture: the n * size^2 texels of the call in batches of whole texels, each k_reflection_rays -> the radiance
// query's kernel (spp = 1, seed = 0 on the pad' rays) -> k_reflection_texels, map p to d_out + p * out_stride texels.  The
// items of run_batches are the texels, under a global index: a probe may span batches and a batch probes.
static int launch_reflection_capture(rt_ctx* c, const rt_reflection_desc& D, const ReflectionShape& sh, const void* d_probes,
                                     uint32_t n, uint32_t max_depth, uint32_t seed, void* d_out, uint32_t out_stride, bool detail) {
  const PathQueryKind& k = pq_reflection;
  const int r = query_scene_ready(c, k.what, true);
  if (r < 0) return r;
  const uint32_t spt = D.spt;
  return run_batches(
      c, c->*k.state, c->*k.last, n * sh.map, spt,
      [&](uint32_t first, uint32_t, uint32_t items) -> int {
        hipLaunchKernelGGL(rtk::k_reflection_rays, dim3((items + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)d_probes,
                           (float4*)c->pr_rays.ptr, items, spt, seed, first, sh.size_log2);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
      },
      [&](const void* rays, uint32_t items, void* rad, bool keep_counts, EventPair* ev) {
        return launch_path_query(c, k, rays, items, max_depth, 1u, 0u, rad, detail, keep_counts, ev);
      },
      [&](uint32_t first, uint32_t nt) -> int {
        hipLaunchKernelGGL(rtk::k_reflection_texels, dim3((nt + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)d_probes,
                           (const float4*)c->pr_rad.ptr, (float4*)d_out, nt, spt, first, sh.size_log2, out_stride);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
      });
}

// Enqueue a filter: level 0 of chain p is read at d_src + p * src_stride texels; where that is not the chain itself the maps
// are copied into level 0 first; then one launch per level >= 1 over all n probes.
static int launch_reflection_filter(rt_ctx* c, const rt_reflection_desc& D, const ReflectionShape& sh, const void* d_src,
                                    uint32_t src_stride, void* d_out, uint32_t n) {
  if (d_src != (const void*)d_out) {
    const uint32_t texels = n * sh.map;
    hipLaunchKernelGGL(rtk::k_reflection_copy, dim3((texels + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)d_src,
                       (float4*)d_out, texels, sh.size_log2, sh.chain);
    HIP_TRY(c, hipGetLastError());
  }
  rtk::ReflectionFilterArgs A;
  A.src = (const float4*)d_src;
  A.out = (float4*)d_out;
  A.src_stride = src_stride;
  A.chain = sh.chain;
  A.n = n;
  A.size_log2 = sh.size_log2;
  A.levels = D.levels;
  A.K = D.filter_samples;
  const uint32_t ns = D.filter_samples / 64u;
  uint32_t offset = sh.map;
  for (uint32_t m = 1; m < D.levels; m++) {
    const uint32_t S = D.size >> m, texels = n * S * S;
    A.level = m;
    A.offset = offset;
    offset += S * S;
    // one wave per texel at a time, four per workgroup, persistent: at most eight workgroups per CU
    const uint32_t blocks = std::min((texels + 3u) / 4u, (uint32_t)c->num_cus * 8u);
    if (ns <= 4)
      hipLaunchKernelGGL(rtk::k_reflection_filter<4>, dim3(blocks), dim3(256), 0, c->stream, A);
    else if (ns <= 16)
      hipLaunchKernelGGL(rtk::k_reflection_filter<16>, dim3(blocks), dim3(256), 0, c->stream, A);
    else
      hipLaunchKernelGGL(rtk::k_reflection_filter<64>, dim3(blocks), dim3(256), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
  }
  return RT_OK;
}

int rt_reflection_stats(rt_ctx* c, rt_radiance_stats* out) { return batched_query_stats(c, pq_reflection, out); }

int rt_capture_reflection_device(rt_ctx* c, const rt_reflection_desc* desc, const void* dev_probes, uint32_t n, uint32_t max_depth,
                                 uint32_t seed, void* dev_maps) {
  ReflectionShape sh;
  int r = reflection_desc_ok(c, desc, n, RF_CAPTURE, &sh);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if (n == 0) return reflection_no_work(c), RT_OK;
  if ((r = caller_arrays_ok(c, kReflection, {dev_probes, dev_maps})) < 0) return r;
  return launch_reflection_capture(c, *desc, sh, dev_probes, n, max_depth, seed, dev_maps, sh.map, c->detailed_counters);
}

int rt_bake_reflection_device(rt_ctx* c, const rt_reflection_desc* desc, const void* dev_probes, uint32_t n, uint32_t max_depth,
                              uint32_t seed, void* dev_chains) {
  ReflectionShape sh;
  int r = reflection_desc_ok(c, desc, n, RF_CAPTURE | RF_FILTER, &sh);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if (n == 0) return reflection_no_work(c), RT_OK;
  if ((r = caller_arrays_ok(c, kReflection, {dev_probes, dev_chains})) < 0) return r;
  if ((r = launch_reflection_capture(c, *desc, sh, dev_probes, n, max_depth, seed, dev_chains, sh.chain, c->detailed_counters)) < 0)
    return r;
  return launch_reflection_filter(c, *desc, sh, dev_chains, sh.chain, dev_chains, n);
}

int rt_filter_reflection_device(rt_ctx* c, const rt_reflection_desc* desc, const void* dev_maps, uint32_t n, void* dev_chains) {
  ReflectionShape sh;
  int r = reflection_desc_ok(c, desc, n, RF_FILTER, &sh);
  if (r < 0 || !c) return RT_ERR_INVALID;
  if (n == 0) return RT_OK;
  if ((r = caller_arrays_ok(c, kReflection, {dev_maps, dev_chains})) < 0) return r;
  return launch_reflection_filter(c, *desc, sh, dev_maps, dev_maps == (const void*)dev_chains ? sh.chain : sh.map, dev_chains, n);
}

// the blocking entries: probes or maps up into the reflection staging, the chains or maps back; the stream is idle on return
static int reflection_from_host(rt_ctx* c, const rt_reflection_desc* desc, int parts, const rt_probe* probes, const float* maps,
                                uint32_t n, uint32_t max_depth, uint32_t seed, float* out, rt_radiance_stats* stats) {
  ReflectionShape sh;
  int r = reflection_desc_ok(c, desc, n, parts, &sh);
  if (r < 0 || !c) return RT_ERR_INVALID;
  const bool capture = (parts & RF_CAPTURE) != 0, filter = (parts & RF_FILTER) != 0;
  if (n == 0) {
    if (capture) {
      reflection_no_work(c);
      if (stats) *stats = c->rf_last;
    }
    return RT_OK;
  }
  if (!(capture ? (const void*)probes : (const void*)maps) || !out) return fail(c, RT_ERR_INVALID, std::string(kReflection) + ": NULL array");
  if (capture && (r = reflection_pads_ok(c, probes, n, sh)) < 0) return r;
  ReflectionState& st = c->rfl;
  const size_t map_bytes = (size_t)n * sh.map * 16, chain_bytes = (size_t)n * sh.chain * 16;
  DeviceBuffer& result = filter ? st.chains : st.maps;   // (a filter alone reads st.maps and writes st.chains)
  r = staged_call(c,
                  {{result, out, filter ? chain_bytes : map_bytes, STAGE_OUT},
                   {st.probes, probes, (size_t)n * sizeof(rt_probe), STAGE_IN, true, capture},
                   {st.maps, maps, map_bytes, STAGE_IN, true, !capture}},
                  [&] {
                    if (!capture) return launch_reflection_filter(c, *desc, sh, st.maps.ptr, sh.map, result.ptr, n);
                    const int e = launch_reflection_capture(c, *desc, sh, st.probes.ptr, n, max_depth, seed, result.ptr,
                                                            filter ? sh.chain : sh.map, stats != nullptr);
                    if (e < 0 || !filter) return e;
                    return launch_reflection_filter(c, *desc, sh, result.ptr, sh.chain, result.ptr, n);
                  });
  if (r < 0) return r;
  if (capture && stats) return rt_reflection_stats(c, stats);
  return RT_OK;
}

int rt_capture_reflection(rt_ctx* c, const rt_reflection_desc* desc, const rt_probe* probes, uint32_t n, uint32_t max_depth,
                          uint32_t seed, float* out_maps, rt_radiance_stats* stats) {
  return reflection_from_host(c, desc, RF_CAPTURE, probes, nullptr, n, max_depth, seed, out_maps, stats);
}
int rt_filter_reflection(rt_ctx* c, const rt_reflection_desc* desc, const float* maps, uint32_t n, float* out_chains) {
  return reflection_from_host(c, desc, RF_FILTER, nullptr, maps, n, 0, 0, out_chains, nullptr);
}
int rt_bake_reflection(rt_ctx* c, const rt_reflection_desc* desc, const rt_probe* probes, uint32_t n, uint32_t max_depth,
                       uint32_t seed, float* out_chains, rt_radiance_stats* stats) {
  return reflection_from_host(c, desc, RF_CAPTURE | RF_FILTER, probes, nullptr, n, max_depth, seed, out_chains, stats);
}

// ---- the reflection sampler (mi355rt.h "THE REFLECTION SAMPLE RULE"; k_reflection_sample.hip.h): baked chains read at the
// caller's queries, one thread per query.  Needs no scene; the kernel and its launcher are reflection_sample.hip.
// everything the limits say about the descriptor and the two counts; *chain = texels of a chain
static int reflection_sample_desc_ok(rt_ctx* c, const rt_reflection_sample_desc* d, uint32_t n_probes, uint32_t n, uint32_t* chain) {
  if (!d) return refuse(c, kReflection, "NULL descriptor");
  if (d->size < 8 || d->size > 512 || (d->size & (d->size - 1u))) return refuse(c, kReflection, "size must be a power of two in 8 .. 512");
  if (d->levels < 2) return refuse(c, kReflection, "levels must be >= 2");
  if (d->levels > 32 || (d->size >> (d->levels - 1u)) < 4) return refuse(c, kReflection, "size >> (levels - 1) must be >= 4");
  if (d->flags & ~RT_REFLECTION_SAMPLE_PARALLAX) return refuse(c, kReflection, "unknown flags");
  for (int k = 0; k < 5; k++)
    if (d->reserved[k]) return refuse(c, kReflection, "reserved must be 0");
  *chain = 0;
  for (uint32_t m = 0; m < d->levels; m++) *chain += (d->size >> m) * (d->size >> m);
  if (n_probes == 0 && n > 0) return refuse(c, kReflection, "n_probes must be > 0");
  if ((uint64_t)n_probes * *chain >= (1ull << 31)) return refuse(c, kReflection, "n_probes * texels of a chain must be below 2^31");
  if (n >= (1u << 31)) return refuse(c, kReflection, "too many queries for one call (n must be below 2^31)");
  return RT_OK;
}
static int launch_sample_reflection(rt_ctx* c, const rt_reflection_sample_desc& D, uint32_t chain, const void* d_chains,
                                    uint32_t n_probes, const void* d_probes, const void* d_boxes, const void* d_queries, uint32_t n,
                                    void* d_out) {
  rtk::ReflectionSampleArgs A;
  A.chains = (const float4*)d_chains;
  A.probes = (const float4*)d_probes;
  A.boxes = (const float4*)d_boxes;
  A.queries = (const float4*)d_queries;
  A.out = (float4*)d_out;
  A.n = n;
  A.n_probes = n_probes;
  A.chain = chain;
  A.size_log2 = (uint32_t)__builtin_ctz(D.size);
  A.levels = D.levels;
  HIP_TRY(c, rtk::launch_reflection_sample(A, (D.flags & RT_REFLECTION_SAMPLE_PARALLAX) != 0, c->stream));
  return RT_OK;
}

int rt_sample_reflection_device(rt_ctx* c, const rt_reflection_sample_desc* desc, const void* dev_chains, uint32_t n_probes,
                                const void* dev_probes, const void* dev_boxes, const void* dev_queries, uint32_t n, void* dev_out) {
  uint32_t chain = 0;
  int r = reflection_sample_desc_ok(c, desc, n_probes, n, &chain);
  if (r < 0) return r;
  if (n == 0) return c ? RT_OK : RT_ERR_INVALID;
  const bool parallax = (desc->flags & RT_REFLECTION_SAMPLE_PARALLAX) != 0;
  if ((r = caller_arrays_ok(c, kReflection, {dev_chains, {dev_probes, parallax}, {dev_boxes, parallax}, dev_queries, dev_out})) < 0)
    return r;
  if (!c) return RT_ERR_INVALID;
  return launch_sample_reflection(c, *desc, chain, dev_chains, n_probes, dev_probes, dev_boxes, dev_queries, n, dev_out);
}

int rt_sample_reflection(rt_ctx* c, const rt_reflection_sample_desc* desc, const float* chains, uint32_t n_probes,
                         const rt_probe* probes, const rt_reflection_box* boxes, const rt_reflection_query* queries, uint32_t n,
                         float* out) {
  uint32_t chain = 0;
  int r = reflection_sample_desc_ok(c, desc, n_probes, n, &chain);
  if (r < 0) return r;
  if (n == 0) return c ? RT_OK : RT_ERR_INVALID;
  const bool parallax = (desc->flags & RT_REFLECTION_SAMPLE_PARALLAX) != 0;
  if ((r = caller_arrays_ok(c, kReflection, {chains, {probes, parallax}, {boxes, parallax}, queries, out}, false)) < 0 || !c)
    return RT_ERR_INVALID;
  ReflectionSampleState& st = c->rfs;
  return staged_call(c,
                     {{st.chains, chains, (size_t)n_probes * chain * 16, STAGE_IN},
                      {st.probes, probes, (size_t)n_probes * sizeof(rt_probe), STAGE_IN, true, parallax},
                      {st.boxes, boxes, (size_t)n_probes * sizeof(rt_reflection_box), STAGE_IN, true, parallax},
                      {st.queries, queries, (size_t)n * sizeof(rt_reflection_query), STAGE_IN},
                      {st.out, out, (size_t)n * 16, STAGE_OUT}},
                     [&] {
                       return launch_sample_reflection(c, *desc, chain, st.chains.ptr, n_probes, st.probes.ptr, st.boxes.ptr,
                                                       st.queries.ptr, n, st.out.ptr);
                     });
}

// ---- probe visibility maps (mi355rt.h "THE VISIBILITY RULE"; k_volume_visibility.hip.h): per probe of an irradiance volume an
// octahedral map of distance moments, captured through the ray query's kernel, one ray per (texel, sample); a sampler that
// weights each corner by a Chebyshev bound from them; the export into bordered tiles.
static const char* const kVisibility = "volume visibility";
enum { VV_BAKE = 1 };
// everything the limits say about the two descriptors, for the parts (VV_*) an entry runs; *n_out = nx * ny * nz
static int visibility_desc_ok(rt_ctx* c, const rt_volume_desc* d, const rt_volume_visibility_desc* v, int parts, uint32_t* n_out) {
  int r = volume_desc_ok(c, d, n_out);
  if (r < 0) return r;
  if (!v) return refuse(c, kVisibility, "NULL descriptor");
  if (v->size < 4 || v->size > 32 || (v->size & (v->size - 1u))) return refuse(c, kVisibility, "size must be a power of two in 4 .. 32");
  if ((parts & VV_BAKE) && (v->spt == 0 || v->spt > 65536)) return refuse(c, kVisibility, "spt must be 1 .. 65536");
  if (!(std::isfinite(v->max_distance) && v->max_distance > 0.0f)) return refuse(c, kVisibility, "max_distance must be finite and > 0");
  if (!(std::isfinite(v->normal_bias) && v->normal_bias >= 0.0f)) return refuse(c, kVisibility, "normal_bias must be finite and >= 0");
  if (!(v->min_visibility >= 0.0f && v->min_visibility <= 1.0f)) return refuse(c, kVisibility, "min_visibility must be in [0, 1]");
  if (!(v->crush_threshold >= 0.0f && v->crush_threshold <= 1.0f)) return refuse(c, kVisibility, "crush_threshold must be in [0, 1]");
  if (v->flags & ~RT_VOLUME_VIS_BACKFACE) return refuse(c, kVisibility, "unknown flags");
  if (v->reserved) return refuse(c, kVisibility, "reserved must be 0");
  const uint64_t texels = (uint64_t)*n_out * v->size * v->size;
  if (texels >= (1ull << 31)) return refuse(c, kVisibility, "nx * ny * nz * size * size must be below 2^31");
  if ((parts & VV_BAKE) && (uint64_t)d->pad_first + texels > (1ull << 31))
    return refuse(c, kVisibility, "pad_first + nx * ny * nz * size * size must be <= 2^31");
  return RT_OK;
}

// Enqueue a bake: the n * size^2 texels of the grid in batches of whole texels, each k_visibility_rays -> the ray query's
// closest-hit kernel -> k_visibility_texels.  The items of run_batches are the texels, as in a reflection capture: a probe may
// span batches and a batch probes.
static int launch_visibility_bake(rt_ctx* c, const rt_volume_desc& D, const rt_volume_visibility_desc& V, uint32_t n, uint32_t seed,
                                  void* d_out, bool detail) {
  const int r = query_scene_ready(c, kVisibility, false);
  if (r < 0) return r;
  const uint32_t size_log2 = (uint32_t)__builtin_ctz(V.size), spt = V.spt;
  return run_batches(
      c, c->vv, c->vv_last, n * V.size * V.size, spt,
      [&](uint32_t first, uint32_t, uint32_t items) -> int {
        hipLaunchKernelGGL(rtk::k_visibility_rays, dim3((items + 255u) / 256u), dim3(256), 0, c->stream, D, (float4*)c->pr_rays.ptr,
                           items, spt, seed, first, size_log2, V.max_distance);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
      },
      [&](const void* rays, uint32_t items, void* hits, bool keep_counts, EventPair* ev) {
        return launch_ray_query_on(c, c->vv, c->vv_last, kVisibility, rays, items, RT_RAYS_CLOSEST, 0.001f, hits, detail,
                                   keep_counts, ev);
      },
      [&](uint32_t first, uint32_t nt) -> int {
        hipLaunchKernelGGL(rtk::k_visibility_texels, dim3((nt + 255u) / 256u), dim3(256), 0, c->stream,
                           (const uint4*)c->pr_rad.ptr, (float2*)d_out, nt, spt, first, V.max_distance);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
      });
}

int rt_volume_visibility_stats(rt_ctx* c, rt_ray_stats* out) {
  if (!c || !out) return RT_ERR_INVALID;
  const int r = ray_query_stats_of(c, c->vv, c->vv_last, out);   // fences the stream; the time is that of the batches
  if (r < 0) return r;
  return batch_time_ms(c, c->vv, &out->kernel_ms);
}

int rt_bake_volume_visibility_device(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t seed,
                                     void* dev_out) {
  uint32_t n = 0;
  int r = visibility_desc_ok(c, desc, vis, VV_BAKE, &n);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, kVisibility, {dev_out})) < 0) return r;
  if (!c) return RT_ERR_INVALID;
  return launch_visibility_bake(c, *desc, *vis, n, seed, dev_out, c->detailed_counters);
}

int rt_bake_volume_visibility(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t seed, float* out,
                              rt_ray_stats* stats) {
  uint32_t n = 0;
  int r = visibility_desc_ok(c, desc, vis, VV_BAKE, &n);
  if (r < 0) return r;
  if ((r = caller_arrays_ok(c, kVisibility, {out}, false)) < 0 || !c) return RT_ERR_INVALID;
  r = staged_call(c, {{c->vis.maps, out, (size_t)n * vis->size * vis->size * 8, STAGE_OUT}},
                  [&] { return launch_visibility_bake(c, *desc, *vis, n, seed, c->vis.maps.ptr, stats != nullptr); });
  if (r < 0) return r;
  if (stats) return rt_volume_visibility_stats(c, stats);
  return RT_OK;
}

static int launch_sample_volume_visible(rt_ctx* c, const rt_volume_desc& D, const rt_volume_visibility_desc& V, const void* d_volume,
                                        const void* d_vis, const void* d_points, uint32_t n, void* d_out) {
  rtk::VolumeSampleVisibleArgs A;
  A.D = D;
  A.V = V;
  A.volume = (const float4*)d_volume;
  A.visibility = (const float2*)d_vis;
  A.points = (const float4*)d_points;
  A.out = (float4*)d_out;
  A.n = n;
  hipLaunchKernelGGL(rtk::k_volume_sample_visible, dim3((n + 31u) / 32u), dim3(256), 0, c->stream, A);   // 8 lanes per point
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_sample_volume_visible_device(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, const void* dev_volume,
                                    const void* dev_visibility, const void* dev_points, uint32_t n, void* dev_out) {
  uint32_t probes = 0;
  int r = visibility_desc_ok(c, desc, vis, 0, &probes);
  if (r < 0) return r;
  if (n >= (1u << 31)) return refuse(c, kVisibility, "too many points for one call (n must be below 2^31)");
  if (n == 0) return c ? RT_OK : RT_ERR_INVALID;
  if ((r = caller_arrays_ok(c, kVisibility, {dev_volume, dev_visibility, dev_points, dev_out})) < 0) return r;
  if (!c) return RT_ERR_INVALID;
  return launch_sample_volume_visible(c, *desc, *vis, dev_volume, dev_visibility, dev_points, n, dev_out);
}

int rt_sample_volume_visible(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, const rt_probe_sh9* volume,
                             const float* visibility, const rt_gather_point* points, uint32_t n, rt_irradiance* out) {
  uint32_t probes = 0;
  int r = visibility_desc_ok(c, desc, vis, 0, &probes);
  if (r < 0) return r;
  if (n >= (1u << 31)) return refuse(c, kVisibility, "too many points for one call (n must be below 2^31)");
  if (n == 0) return c ? RT_OK : RT_ERR_INVALID;
  if ((r = caller_arrays_ok(c, kVisibility, {volume, visibility, points, out}, false)) < 0 || !c) return RT_ERR_INVALID;
  VisibilityState& st = c->vis;
  return staged_call(c,
                     {{st.volume, volume, (size_t)probes * sizeof(rt_probe_sh9), STAGE_IN},
                      {st.maps, visibility, (size_t)probes * vis->size * vis->size * 8, STAGE_IN},
                      {st.points, points, (size_t)n * sizeof(rt_gather_point), STAGE_IN},
                      {st.out, out, (size_t)n * sizeof(rt_irradiance), STAGE_OUT}},
                     [&] {
                       return launch_sample_volume_visible(c, *desc, *vis, st.volume.ptr, st.maps.ptr, st.points.ptr, n, st.out.ptr);
                     });
}

// bytes of the tiled image of an export
static size_t visibility_tiles_bytes(uint32_t probes, uint32_t size, uint32_t format) {
  return (size_t)probes * (size + 2u) * (size + 2u) * (format == RT_LIGHTMAP_F16 ? 4 : 8);
}
// the arguments of an export beside the descriptors: the format is f32 or f16, the capacity holds the image
static int visibility_encode_args_ok(rt_ctx* c, uint32_t probes, uint32_t size, uint32_t format, const void* in, const void* out,
                                     size_t cap, bool device) {
  if (format == RT_LIGHTMAP_RGBE8) return refuse(c, kVisibility, "RT_LIGHTMAP_RGBE8 cannot hold two distance moments");
  if (format != RT_LIGHTMAP_F32 && format != RT_LIGHTMAP_F16) return refuse(c, kVisibility, "format must be RT_LIGHTMAP_F32 or _F16");
  const int r = caller_arrays_ok(c, kVisibility, {in, out}, device);
  if (r < 0) return r;
  if (device && in == out) return refuse(c, kVisibility, "the output must not be the input");
  if (cap < visibility_tiles_bytes(probes, size, format))
    return refuse(c, kVisibility, "the capacity is below nx * ny * nz tiles of (size + 2)^2 texels of the format");
  return c ? RT_OK : RT_ERR_INVALID;
}
static int launch_visibility_tiles(rt_ctx* c, const rt_volume_desc& D, const rt_volume_visibility_desc& V, uint32_t format,
                                   const void* d_vis, void* d_out) {
  rtk::VisibilityTilesArgs A;
  A.visibility = (const float2*)d_vis;
  A.out = d_out;
  A.nx = D.nx;
  A.rows = D.ny * D.nz;
  A.size = V.size;
  A.format = format;
  const uint64_t texels = (uint64_t)D.nx * A.rows * (V.size + 2u) * (V.size + 2u);   // < 2^31 * 2.25
  hipLaunchKernelGGL(rtk::k_visibility_tiles, dim3((uint32_t)((texels + 255u) / 256u)), dim3(256), 0, c->stream, A);
  HIP_TRY(c, hipGetLastError());
  return RT_OK;
}

int rt_encode_volume_visibility_device(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t format,
                                       const void* dev_visibility, void* dev_out, size_t cap) {
  uint32_t probes = 0;
  int r = visibility_desc_ok(c, desc, vis, 0, &probes);
  if (r < 0) return r;
  if ((r = visibility_encode_args_ok(c, probes, vis->size, format, dev_visibility, dev_out, cap, true)) < 0) return r;
  return launch_visibility_tiles(c, *desc, *vis, format, dev_visibility, dev_out);
}

int rt_encode_volume_visibility(rt_ctx* c, const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t format,
                                const float* visibility, void* out, size_t cap) {
  uint32_t probes = 0;
  int r = visibility_desc_ok(c, desc, vis, 0, &probes);
  if (r < 0) return r;
  if ((r = visibility_encode_args_ok(c, probes, vis->size, format, visibility, out, cap, false)) < 0) return r;
  const size_t in_bytes = (size_t)probes * vis->size * vis->size * 8, out_bytes = visibility_tiles_bytes(probes, vis->size, format);
  return staged_call(c, {{c->vis.maps, visibility, in_bytes, STAGE_IN}, {c->vis.encoded, out, out_bytes, STAGE_OUT}},
                     [&] { return launch_visibility_tiles(c, *desc, *vis, format, c->vis.maps.ptr, c->vis.encoded.ptr); });
}

// ---- the kernels of compute().  Variant 0, the one-pixel-per-lane megakernel: one tile per workgroup, no dynamic LDS.
static int launch_megakernel(rt_ctx* c, const DevScene& S, const DevFrame& F, const DevFrameSlot* dslots, uint32_t tiles) {
  EventPair* ev = next_events(c, RT_TIMER_PATHTRACE);
  if (ev) HIP_TRY(c, hipEventRecord(ev->a, c->stream));
  if (c->detailed_counters)
    hipLaunchKernelGGL(rtk::k_pathtrace<true>, dim3(tiles), dim3(64), 0, c->stream, S, F, c->uniforms, dslots);
  else
    hipLaunchKernelGGL(rtk::k_pathtrace<false>, dim3(tiles), dim3(64), 0, c->stream, S, F, c->uniforms, dslots);
  if (ev) HIP_TRY(c, hipEventRecord(ev->b, c->stream));
  return RT_OK;
}
// The persistent kernel by [detail][lds] of its lp::PersistentShape, its one-leaf LDS form by [detail], and that form's
// product build in 512-thread workgroups (wide)
static const void* const pt_fns[2][2] = {
    {(const void*)rtk::k_pathtrace_persistent<false, false>, (const void*)rtk::k_pathtrace_persistent<false, true>},
    {(const void*)rtk::k_pathtrace_persistent<true, false>, (const void*)rtk::k_pathtrace_persistent<true, true>}};
static const void* const pt_one_leaf_fns[2] = {(const void*)rtk::k_pathtrace_persistent<false, true, true>,
                                               (const void*)rtk::k_pathtrace_persistent<true, true, true>};
static const void* const pt_wide_fn = (const void*)rtk::k_pathtrace_persistent_wide<false, true, true>;
// ... and the wide form of a scene whose materials the host knows to be plain (lp::PersistentShape::plain)
static const void* const pt_plain_fn = (const void*)rtk::k_pathtrace_persistent_plain<false, true, true>;
// ... and the two of them with the leaf sweep for walks (lp::PersistentShape::sweep), by [plain]
static const void* const pt_sweep_fns[2] = {(const void*)rtk::k_pathtrace_sweep_wide<false, true, true>,
                                            (const void*)rtk::k_pathtrace_sweep_plain<false, true, true>};

// compute() for n consecutive frame counts in ONE dispatch of each kernel (n == 1: the plain compute()).
// n_commit < n: frames n_commit .. n-1 are traced AHEAD (speculative lookahead): their host state is not committed and their
// colours are not accumulated yet — consume_ahead() does both when the matching compute() call arrives.
static int compute_frames(rt_ctx* c, const uint32_t* frame_counts, uint32_t n, uint32_t n_commit) {
  if (!c || !frame_counts || n == 0 || n_commit == 0 || n_commit > n) return RT_ERR_INVALID;
  c->spec.valid = false;   // whatever was traced ahead is dropped: its buffers are about to be reused
  c->gbuf_slot = -1;
  // host state advances exactly as n successive compute() calls would (WebGPURenderer.ts:88-91)
  std::vector<DevFrameSlot> slots(n);
  const uint32_t tf_first = c->total_frames + 1;
  struct HostState {
    uint32_t total_frames;
    double jx, jy, acc_jx, acc_jy, avg_jx, avg_jy;
    rt_scene_uniforms uniforms;
  } committed = {};
  for (uint32_t i = 0; i < n; i++) {
    c->total_frames++;
    step_jitter(c, c->total_frames, frame_counts[i]);  // updateFrameUniforms(frameCount, totalFrames)
    write_mixed(c, frame_counts[i]);
    slots[i].frame_count = frame_counts[i];
    slots[i].jitter_x = c->uniforms.jitter[0];
    slots[i].jitter_y = c->uniforms.jitter[1];
    slots[i].pad = 0;
    slots[i].pad2 = 0;
    if (i + 1 == n_commit) committed = {c->total_frames, c->jx, c->jy, c->acc_jx, c->acc_jy, c->avg_jx, c->avg_jy, c->uniforms};
  }
  // the renderer's host state is that of the committed frames only
  c->total_frames = committed.total_frames;
  c->jx = committed.jx; c->jy = committed.jy;
  c->acc_jx = committed.acc_jx; c->acc_jy = committed.acc_jy;
  c->avg_jx = committed.avg_jx; c->avg_jy = committed.avg_jy;
  c->uniforms = committed.uniforms;
  c->acc_frames = n_commit;
  if (!scene_ready(c)) return RT_SKIPPED;
  if (c->accum_stale)
    return fail(c, RT_ERR_INVALID, "the bound accumulation buffer was dropped by rt_resize: call rt_bind_accum again");
  HIP_TRY(c, hipSetDevice(c->device));
  // Host-side shape checks before any kernel indexes these buffers.
  if (c->uniforms.light_count > c->n_lights)
    return fail(c, RT_ERR_INVALID, "light_count exceeds the uploaded lights buffer");
  if (c->blas_offset > c->n_nodes) return fail(c, RT_ERR_INVALID, "blas_base_idx exceeds the node buffer");
  if (c->variant == 0 && n > 1) return fail(c, RT_ERR_INVALID, "batched dispatch needs the persistent or wavefront kernel form");
  int r = prepare_scene(c);
  if (r < 0) return r;

  const size_t npx = (size_t)c->width * c->height;
  const lp::SceneSize size = scene_size(c);
  // auto: the wavefront form pays from 4 frames per dispatch (measured: 1 frame 11.9 vs 8.7 ms persistent, 2: 17.0 vs
  // 15.7, 4: 27.8 vs 29.5, 8: 47.9 vs 57.0 on sponza-like) — a single frame leaves its deeper stages too few rays
  const bool wavefront = c->spp == 1 && (c->variant == 2 || (c->variant == 3 && !lp::scene_fits_lds(size, c->knobs) && n >= 4));
  if (n > 1) {
    r = ensure_buffer(c, c->gbuf_batch, (size_t)(n - 1) * npx * 24, false);
    if (r < 0) return r;
  }
  if (n > 1 || wavefront) {
    r = ensure_buffer(c, c->frame_col, (size_t)n * npx * 16, false);
    if (r < 0) return r;
  }
  for (uint32_t i = 0; i < n; i++) {
    if (i + 1 == n) {  // the last frame lands in the main G-buffer, like a plain compute()
      slots[i].albedo = (uint32_t*)c->render_target.ptr;
      slots[i].normal_id = (float4*)c->g_normal.ptr;
      slots[i].depth = (float*)c->g_depth.ptr;
    } else {
      char* base = (char*)c->gbuf_batch.ptr + (size_t)i * npx * 24;
      slots[i].normal_id = (float4*)base;
      slots[i].albedo = (uint32_t*)(base + npx * 16);
      slots[i].depth = (float*)(base + npx * 20);
    }
  }
  // The table goes through a pinned ring, one device table per ring entry: the copy is asynchronous, its source
  // outlives it, and a dispatch still in flight keeps reading its own table while the next one is being written.
  if (!c->slot_ring) {
    HIP_TRY(c, hipHostMalloc(&c->slot_ring, (size_t)rt_ctx::kSlotRing * 64 * sizeof(DevFrameSlot), hipHostMallocDefault));
    for (int k = 0; k < rt_ctx::kSlotRing; k++) HIP_TRY(c, hipEventCreateWithFlags(&c->slot_ring_ev[k], hipEventDisableTiming));
  }
  r = ensure_buffer(c, c->slots, (size_t)rt_ctx::kSlotRing * 64 * sizeof(DevFrameSlot), false);
  if (r < 0) return r;
  const int ring = c->slot_ring_next;
  c->slot_ring_next = (ring + 1) % rt_ctx::kSlotRing;
  if (c->slot_ring_used[ring]) HIP_TRY(c, hipEventSynchronize(c->slot_ring_ev[ring]));  // the dispatch that used this entry is done
  DevFrameSlot* host_slots = (DevFrameSlot*)c->slot_ring.h + (size_t)ring * 64;
  std::memcpy(host_slots, slots.data(), (size_t)n * sizeof(DevFrameSlot));
  DevFrameSlot* dev_slots = (DevFrameSlot*)c->slots.ptr + (size_t)ring * 64;
  HIP_TRY(c, hipMemcpyAsync(dev_slots, host_slots, (size_t)n * sizeof(DevFrameSlot), hipMemcpyHostToDevice, c->stream));
  const DevFrameSlot* dslots = dev_slots;

  DevScene S = dev_scene(c);
  DevFrame F;
  F.accum = accum_ptr(c);
  F.frame_col = (n > 1 || wavefront) ? (float4*)c->frame_col.ptr : nullptr;
  F.albedo = (uint32_t*)c->render_target.ptr;
  F.normal_id = (float4*)c->g_normal.ptr;
  F.depth = (float*)c->g_depth.ptr;
  F.counters = (uint64_t*)c->counters.ptr;
  F.max_depth = c->max_depth;
  F.spp = c->spp;
  F.stripe_rows = c->stripe_rows;
  F.stripe_rank = c->stripe_rank;
  F.stripe_count = c->stripe_count;
  F.own_run = F.own_period = F.own_first = F.own_tile_rows = 0;
  if (c->stripe_count > 1 && c->stripe_rows && c->stripe_rows % 8 == 0) {
    const uint32_t tile_rows = (c->height + 7) / 8;
    F.own_run = c->stripe_rows / 8;
    F.own_period = F.own_run * c->stripe_count;
    F.own_first = F.own_run * c->stripe_rank;
    uint32_t owned = 0;
    for (uint32_t ty = 0; ty < tile_rows; ty++)
      if ((ty / F.own_run) % c->stripe_count == c->stripe_rank) owned++;
    F.own_tile_rows = owned;
  }
  DevFrame Fp = F;  // the primary kernel counts into bank 0, the path tracer into bank 1
  F.counters = (uint64_t*)c->counters.ptr + (size_t)RT_COUNTER_SHARDS * 6;
  const uint32_t tiles = ((c->width + 7) / 8) * ((c->height + 7) / 8);
  const uint32_t own_tiles = F.own_period ? ((c->width + 7) / 8) * F.own_tile_rows : tiles;  // this rank's: what both kernels cover

  // 1. primary visibility (the reference clears + rasterises the G-buffer every compute()); frame = blockIdx.y
  EventPair* ev = next_events(c, RT_TIMER_PRIMARY);
  if (ev) HIP_TRY(c, hipEventRecord(ev->a, c->stream));
  // own_tiles == 0: tile-aligned stripes and a rank that owns no tile row (fewer tile rows than ranks) - nothing to cast, and
  // a grid of x-size 0 is an invalid launch configuration
  if (own_tiles) {
    const lp::PrimaryShape shape = lp::primary_shape(size, c->knobs, (uint64_t)own_tiles * n, c->stripe_count > 1 && c->stripe_rows);
    uint32_t nn = c->n_nodes, nt = c->n_tris, ni = c->n_instances, nv = c->n_verts, n_ptiles = own_tiles;
    // one-leaf scenes: the LDS form stages the shading records with world-space vertex normals
    const bool one_leaf = lp::one_leaf_lds(size, c->knobs);
    const float4* tsw = (one_leaf && !c->world_rec_dirty) ? (const float4*)c->tri_shade_w.ptr : nullptr;
    uint32_t rounds = shape.rounds;   // LDS form: tiles per wave behind one staging (lds_sizes.h primary_tile)
    if (getenv("MI355RT_DEBUG_SHAPE"))
      fprintf(stderr, "[mi355rt] primary kernel: %s form, %u rounds, grid %u x %u, %zu bytes of LDS\n",
              shape.lds ? (shape.tiles ? "LDS many-tiles" : "LDS") : "global", rounds, lp::primary_grid_x(shape, own_tiles), (unsigned)n, shape.dyn);
    void* args[] = {&S, &Fp, &c->uniforms, &dslots, &n_ptiles, &nn, &nt, &ni, &nv, &tsw, &rounds};
    HIP_TRY(c, hipLaunchKernel(primary_fns[c->detailed_counters][shape.lds ? (shape.tiles ? 2 : 1) : 0], dim3(lp::primary_grid_x(shape, own_tiles), n),
                               dim3(shape.block), args, shape.dyn, c->stream));
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev->b, c->stream));
  // the frame denoiser's key: a new G-buffer is current, and the render target holds its last frame's albedo again.  A last
  // frame that is traced AHEAD is consumed after present() calls that overwrite the plane: a context that denoises frames
  // keeps a copy (4 B / px, only then)
  c->gbuf_gen++;
  c->fm.gbuf_scene_gen = c->fm.scene_gen;   // frame motion: the scene arrays are those this G-buffer's indices point into
  c->albedo_plane_valid = true;
  c->fd.keep_valid = false;
  if (c->fd.wanted && n_commit < n) {
    if ((r = ensure_buffer(c, c->fd.albedo_keep, npx * 4, false)) < 0) return r;
    HIP_TRY(c, hipMemcpyAsync(c->fd.albedo_keep.ptr, c->render_target.ptr, npx * 4, hipMemcpyDeviceToDevice, c->stream));
    c->fd.keep_valid = true;
  }

  // 2. path trace
  c->pt_form = RT_PT_FORM_NONE;   // until the persistent kernel is launched below
  if (wavefront) {
    r = launch_wavefront(c, S, F, dslots, n);
    if (r < 0) return r;
  } else if (c->variant == 0) {
    r = launch_megakernel(c, S, F, dslots, tiles);
    if (r < 0) return r;
  } else {
    // persistent kernel: grid = resident workgroups, tiles handed out through a ticket counter
    HIP_TRY(c, hipMemsetAsync(c->ticket.ptr, 0, 4, c->stream));
    lp::PersistentShape shape = lp::persistent_shape(size, c->knobs, n, c->detailed_counters, c->facts, c->walk);
    if (shape.one_inst && c->world_rec_dirty) return fail(c, RT_ERR_INTERNAL, "one-leaf form without its world records");
    if (shape.sweep && (c->walk_dirty || !c->leaf_recs.ptr)) return fail(c, RT_ERR_INTERNAL, "sweep form without its leaf records");
    if (shape.sweep && (c->walk_nodes < c->walk.n_leaves || c->walk_nodes > scene_facts::kMaxNodeRecords))
      return fail(c, RT_ERR_INTERNAL, "sweep form without its node records");
    const void* fn = shape.sweep      ? pt_sweep_fns[shape.plain]
                     : shape.plain    ? pt_plain_fn
                     : shape.wide     ? pt_wide_fn
                     : shape.one_inst ? pt_one_leaf_fns[c->detailed_counters]
                                      : pt_fns[c->detailed_counters][shape.lds];
    int per_cu;
    if ((r = resident_blocks(c, fn, (int)(64 * shape.waves), shape.dyn, &per_cu)) < 0) return r;
    // as many waves as there are tickets (tiles x frames), up to the resident limit; fewer, longer-lived waves measured worse
    const uint32_t blocks = grid_blocks(c, per_cu, 0, (own_tiles * n + shape.waves - 1) / shape.waves);
    uint32_t* ticket = (uint32_t*)c->ticket.ptr;
    uint32_t nn = c->n_nodes, nt = c->n_tris, ni = c->n_instances, nv = c->n_verts, ns = n;
    // (the two sweep forms read two parameters more; the others have no such parameters and are not handed them)
    const float4* leaf_recs = (const float4*)c->leaf_recs.ptr;
    uint32_t leaf_info = c->walk.n_leaves | (c->walk_nodes << 16) | (c->knobs.leaf_sweep_guard ? 0x80000000u : 0u);
    void* args[] = {&S, &F, &c->uniforms, &ticket, &nn, &nt, &ni, &nv, &dslots, &ns, &shape.plan, &leaf_recs, &leaf_info};
    ev = next_events(c, RT_TIMER_PATHTRACE);
    if (ev) HIP_TRY(c, hipEventRecord(ev->a, c->stream));
    HIP_TRY(c, hipLaunchKernel(fn, dim3(blocks), dim3(64 * shape.waves), args, shape.dyn, c->stream));
    c->pt_launch[0] = 64 * shape.waves;
    c->pt_launch[1] = blocks;
    c->pt_launch[2] = (uint32_t)shape.dyn;
    c->pt_launch[3] = (uint32_t)per_cu;
    c->pt_form = shape.sweep ? (shape.plain ? RT_PT_FORM_PLAIN_SWEEP : RT_PT_FORM_GENERIC_SWEEP)
                             : (shape.plain ? RT_PT_FORM_PLAIN : RT_PT_FORM_GENERIC);
    if (ev) HIP_TRY(c, hipEventRecord(ev->b, c->stream));
    if (n > 1)  // ordered accumulation of the batch's frame colours
      hipLaunchKernelGGL(rtk::k_accumulate_frames, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, F, dslots,
                         c->acc_frames, c->width, c->height);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->slot_ring_ev[ring], c->stream));
  c->slot_ring_used[ring] = true;
  if (n_commit < n) {   // frames traced ahead: remember where their colours and G-buffers are
    c->spec.valid = true;
    c->spec.epoch = c->epoch;
    c->spec.n = n;
    c->spec.k = n_commit;
    c->spec.fc0 = frame_counts[0];
    c->spec.tf0 = tf_first;
    c->spec.dslots = dslots;
    c->spec.slots = slots;
    c->spec.frame = F;
    c->gbuf_slot = (int)n_commit - 1;
  }
  return RT_OK;
}

// compute(frame_count) when that frame has been traced ahead: commit its host state, add its colours.
static int consume_ahead(rt_ctx* c, uint32_t frame_count) {
  auto& sp = c->spec;
  const uint32_t k = sp.k;
  c->total_frames++;
  step_jitter(c, c->total_frames, frame_count);
  write_mixed(c, frame_count);
  if (c->uniforms.jitter[0] != sp.slots[k].jitter_x || c->uniforms.jitter[1] != sp.slots[k].jitter_y)
    return fail(c, RT_ERR_INTERNAL, "lookahead: the frame traced ahead does not match the frame asked for");
  HIP_TRY(c, hipSetDevice(c->device));
  DevFrame F = sp.frame;
  const size_t npx = (size_t)c->width * c->height;
  F.accum = accum_ptr(c);
  F.frame_col = sp.frame.frame_col + (size_t)k * npx;
  hipLaunchKernelGGL(rtk::k_accumulate_frames, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, F, sp.dslots + k, 1u,
                     c->width, c->height);
  HIP_TRY(c, hipGetLastError());
  c->gbuf_slot = (int)k;
  c->gbuf_gen++;   // another frame's G-buffer is current (the frame denoiser's key)
  c->fm.gbuf_scene_gen = c->fm.scene_gen;   // whatever rewrites the scene drops the frames traced ahead: it is still their scene
  sp.k++;
  if (sp.k >= sp.n) sp.valid = false;
  return RT_OK;
}

int rt_compute(rt_ctx* c, uint32_t frame_count) {
  if (!c) return RT_ERR_INVALID;
  if (c->lookahead_max <= 1 || c->detailed_counters || c->variant == 0 || c->accum_stale) return compute_frames(c, &frame_count, 1, 1);
  // a frame traced ahead by an earlier call of this run?
  if (c->spec.valid && c->spec.epoch == c->epoch && frame_count == c->spec.fc0 + c->spec.k &&
      c->total_frames + 1 == c->spec.tf0 + c->spec.k && scene_ready(c)) {
    const int r = consume_ahead(c, frame_count);
    c->run_last_fc = frame_count;
    c->run_last_tf = c->total_frames;
    return r;
  }
  // does this call continue a run of consecutive frames?  Then trace ahead, twice as far as last time.
  const bool continues = c->run_epoch == c->epoch && frame_count == c->run_last_fc + 1 && c->total_frames == c->run_last_tf;
  c->look = continues ? std::min<uint32_t>(std::min<uint32_t>(c->look * 2u, c->lookahead_max), 64u) : 1u;
  if (c->look_limit) c->look = std::max<uint32_t>(1u, std::min(c->look, c->look_limit));   // rt_set_lookahead_limit: the caller knows when the run ends
  c->run_epoch = c->epoch;
  uint32_t fcs[64];
  for (uint32_t i = 0; i < c->look; i++) fcs[i] = frame_count + i;
  const int r = compute_frames(c, fcs, c->look, 1);
  c->run_last_fc = frame_count;
  c->run_last_tf = c->total_frames;
  return r;
}

int rt_compute_batch(rt_ctx* c, const uint32_t* frame_counts, uint32_t n) {
  if (!c) return RT_ERR_INVALID;
  if (n > 64) return fail(c, RT_ERR_INVALID, "at most 64 frames per batch");
  c->epoch++;   // an explicit batch ends a run
  return compute_frames(c, frame_counts, n, n);
}

int rt_set_lookahead(rt_ctx* c, uint32_t max_frames) {
  if (!c) return RT_ERR_INVALID;
  if (max_frames > 64) return fail(c, RT_ERR_INVALID, "at most 64 frames of lookahead");
  c->lookahead_max = max_frames;
  c->epoch++;
  return RT_OK;
}

int rt_set_lookahead_limit(rt_ctx* c, uint32_t frames_left) {
  if (!c) return RT_ERR_INVALID;
  c->look_limit = frames_left;   // changes no result and drops nothing: only how far the next dispatches trace ahead
  return RT_OK;
}

int rt_present(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (!c->width || !c->render_target.ptr || !c->accum.ptr) return RT_SKIPPED;  // PostProcessPass.ts:32-38
  if (c->accum_stale)
    return fail(c, RT_ERR_INVALID, "the bound accumulation buffer was dropped by rt_resize: call rt_bind_accum again");
  if (c->present_stale)
    return fail(c, RT_ERR_INVALID, "the bound present source was dropped by rt_resize: call rt_bind_present_source again");
  if (c->dist.active && c->dist.rank == 0 && !c->dist.display.ptr)
    return fail(c, RT_ERR_NOT_READY, "rank 0 has no display buffer (its allocation failed at the last rt_resize)");
  HIP_TRY(c, hipSetDevice(c->device));
  DevPost P;
  P.accum = c->present_source ? (const float4*)c->present_source : accum_ptr(c);
  if (c->dist.active && c->dist.rank == 0) P.accum = (const float4*)c->dist.display.ptr;   // the assembled image
  if (c->fd.present_on) {   // rt_set_present_denoise: the post pass reads the filtered frame (no source bound, no rank: refused there)
    const size_t bytes = (size_t)c->width * c->height * 16;
    int r = frame_denoise_ctx_ok(c, &c->fd.present_desc);
    if (r < 0) return r;
    if ((r = ensure_buffer(c, c->fd.out, bytes, false)) < 0) return r;
    if ((r = frame_denoise_run(c, &c->fd.present_desc, c->fd.out.ptr)) < 0) return r;
    P.accum = (const float4*)c->fd.out.ptr;
  }
  c->albedo_plane_valid = false;   // the post pass writes the render target, which is the albedo plane
  P.history_in = (const ushort4*)c->history[1 - c->history_index].ptr;  // previous frame (read)
  P.history_out = (ushort4*)c->history[c->history_index].ptr;           // current frame (write)
  P.out_rgba8 = (uint32_t*)c->render_target.ptr;
  dim3 grid((c->width + 15) / 16, (c->height + 15) / 16);
  EventPair* ev = next_events(c, RT_TIMER_POST);
  if (ev) HIP_TRY(c, hipEventRecord(ev->a, c->stream));
  hipLaunchKernelGGL(rtk::k_postprocess, grid, dim3(256), 0, c->stream, P, c->uniforms);
  if (ev) HIP_TRY(c, hipEventRecord(ev->b, c->stream));
  HIP_TRY(c, hipGetLastError());
  c->history_index = 1 - c->history_index;  // swap history index for TAA
  return RT_OK;
}

int rt_capture(rt_ctx* c, uint8_t* out_rgba, size_t cap) {
  if (!c || !out_rgba) return RT_ERR_INVALID;
  if (!c->render_target.ptr) return fail(c, RT_ERR_NOT_READY, "No render target");  // WebGPUContext.ts:43
  const size_t bytes = (size_t)c->width * c->height * 4;
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "capture buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(out_rgba, c->render_target.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_sync(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---------------------------------------------------------------- additions
int rt_read_accum(rt_ctx* c, float* out, size_t cap) {
  if (!c || !out) return RT_ERR_INVALID;
  const size_t bytes = (size_t)c->width * c->height * 16;
  if (!c->accum.ptr) return fail(c, RT_ERR_NOT_READY, "no accumulation buffer");
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(out, accum_ptr(c), bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
int rt_write_accum(rt_ctx* c, const float* in, size_t bytes) {
  if (!c || !in) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  if (!c->accum.ptr || bytes != (size_t)c->width * c->height * 16)
    return fail(c, RT_ERR_INVALID, "accumulation size mismatch");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(accum_ptr(c), in, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
int rt_read_gbuffer(rt_ctx* c, uint8_t* albedo, float* normal_id, float* depth) {
  if (!c) return RT_ERR_INVALID;
  if (!c->render_target.ptr) return fail(c, RT_ERR_NOT_READY, "no G-buffer");
  const size_t n = (size_t)c->width * c->height;
  HIP_TRY(c, hipSetDevice(c->device));
  const void *pa = c->render_target.ptr, *pn = c->g_normal.ptr, *pd = c->g_depth.ptr;
  // the frame of the last compute() was traced as part of a batch; rt_resize and the next dispatch (the only calls that free
  // or reuse the batch's planes) reset gbuf_slot
  if (c->gbuf_slot >= 0 && (size_t)c->gbuf_slot < c->spec.slots.size()) {
    const DevFrameSlot& sl = c->spec.slots[c->gbuf_slot];
    pa = sl.albedo;
    pn = sl.normal_id;
    pd = sl.depth;
  }
  if (albedo) HIP_TRY(c, hipMemcpyAsync(albedo, pa, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (normal_id) HIP_TRY(c, hipMemcpyAsync(normal_id, pn, n * 16, hipMemcpyDeviceToHost, c->stream));
  if (depth) HIP_TRY(c, hipMemcpyAsync(depth, pd, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
int rt_read_history(rt_ctx* c, uint16_t* out, size_t cap) {
  if (!c || !out) return RT_ERR_INVALID;
  const size_t bytes = (size_t)c->width * c->height * 8;
  if (!c->history[0].ptr) return fail(c, RT_ERR_NOT_READY, "no history");
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(out, c->history[1 - c->history_index].ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
int rt_read_uniforms(rt_ctx* c, void* out256) {
  if (!c || !out256) return RT_ERR_INVALID;
  std::memcpy(out256, &c->uniforms, 256);
  return RT_OK;
}
static int read_counters(rt_ctx* c, int bank_lo, int bank_hi, rt_counters* out) {
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<uint64_t> host((size_t)2 * RT_COUNTER_SHARDS * 6);
  HIP_TRY(c, hipMemcpyAsync(host.data(), c->counters.ptr, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t sum[6] = {0, 0, 0, 0, 0, 0};
  for (int b = bank_lo; b <= bank_hi; b++)
    for (size_t s = 0; s < RT_COUNTER_SHARDS; s++)
      for (int k = 0; k < 6; k++) sum[k] += host[((size_t)b * RT_COUNTER_SHARDS + s) * 6 + k];
  out->primary_rays = sum[0];
  out->extension_rays = sum[1];
  out->shadow_rays = sum[2];
  out->nodes_visited = sum[3];
  out->tris_tested = sum[4];
  out->shaded_hits = sum[5];
  return RT_OK;
}
int rt_get_counters(rt_ctx* c, rt_counters* out) {
  if (!c || !out) return RT_ERR_INVALID;
  return read_counters(c, 0, 1, out);
}
int rt_get_kernel_counters(rt_ctx* c, int kernel, rt_counters* out) {
  if (!c || !out || kernel < 0 || kernel > 1) return RT_ERR_INVALID;
  return read_counters(c, kernel, kernel, out);
}
int rt_reset_counters(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(c->counters.ptr, 0, c->counters.size, c->stream));
  return RT_OK;
}
int rt_set_counting(rt_ctx* c, int detailed) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  c->detailed_counters = detailed != 0;
  return RT_OK;
}
int rt_set_stripes(rt_ctx* c, uint32_t stripe_rows, uint32_t rank, uint32_t count) {
  if (!c) return RT_ERR_INVALID;
  if (count > 1 && (stripe_rows == 0 || rank >= count)) return fail(c, RT_ERR_INVALID, "invalid stripe spec");
  if (c->dist.active) {
    if (stripe_rows != c->dist.stripe_rows || rank != c->dist.rank || (count ? count : 1) != c->dist.world)
      return fail(c, RT_ERR_INVALID, "rt_set_stripes contradicts the rank rt_dist_init made this context (rt_dist_shutdown first)");
    return RT_OK;
  }
  if (count > 1 && c->fd.present_on)
    return fail(c, RT_ERR_INVALID, "rt_set_stripes: present() filters the frame, and a striped G-buffer covers only its own rows (rt_set_present_denoise(NULL) first)");
  c->epoch++;
  c->stripe_rows = stripe_rows;
  c->stripe_rank = rank;
  c->stripe_count = count ? count : 1;
  return RT_OK;
}
void* rt_accum_device_ptr(rt_ctx* c) { return c ? (void*)accum_ptr(c) : nullptr; }
int rt_bind_accum(rt_ctx* c, void* device_ptr) {
  if (!c) return RT_ERR_INVALID;
  if (c->dist.active)
    return fail(c, RT_ERR_INVALID, "rt_bind_accum: the context is a rank of a sharded image and packs its own accumulator (rt_dist_shutdown first)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->external_accum = device_ptr;
  c->accum_stale = false;
  c->fd.cache_valid = false;   // the frame denoiser's colour image was made from the other accumulation buffer
  return RT_OK;
}
int rt_bind_present_source(rt_ctx* c, void* device_ptr) {
  if (!c) return RT_ERR_INVALID;
  if (c->dist.active)
    return fail(c, RT_ERR_INVALID, "rt_bind_present_source: the context is a rank of a sharded image and presents its own display buffer (rt_dist_shutdown first)");
  if (device_ptr && c->fd.present_on)
    return fail(c, RT_ERR_INVALID, "rt_bind_present_source: present() filters the frame into its own source (rt_set_present_denoise(NULL) first)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->present_source = device_ptr;
  c->present_stale = false;
  return RT_OK;
}
int rt_set_stream(rt_ctx* c, void* hip_stream) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return RT_OK;
}
int rt_set_kernel_variant(rt_ctx* c, int variant) {
  if (!c || variant < 0 || variant > 3) return RT_ERR_INVALID;
  c->variant = variant;
  c->epoch++;
  return RT_OK;
}
int rt_set_walk(rt_ctx* c, int walk) {
  if (!c || walk < 0 || walk > 2) return RT_ERR_INVALID;
  c->knobs.walk = walk;
  c->epoch++;
  return RT_OK;
}
int rt_set_kernel_timing(rt_ctx* c, int enabled) {
  if (!c) return RT_ERR_INVALID;
  c->epoch++;   // drops frames traced ahead (rt_set_lookahead)
  c->timing = enabled != 0;
  return RT_OK;
}
int rt_debug_read_traversal_nodes(rt_ctx* c, float* tnodes_out, uint32_t* new_index_out, uint32_t* inst_root_out, uint32_t cap_nodes) {
  if (!c) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  int r = prepare_scene(c);
  if (r < 0) return r;
  if (cap_nodes < c->n_nodes || !c->tnodes.ptr) return fail(c, RT_ERR_INVALID, "rt_debug_read_traversal_nodes: no nodes or buffer too small");
  if (tnodes_out) HIP_TRY(c, hipMemcpyAsync(tnodes_out, c->tnodes.ptr, (size_t)c->n_nodes * 32, hipMemcpyDeviceToHost, c->stream));
  if (new_index_out) HIP_TRY(c, hipMemcpyAsync(new_index_out, c->node_newidx.ptr, (size_t)c->n_nodes * 4, hipMemcpyDeviceToHost, c->stream));
  if (inst_root_out) HIP_TRY(c, hipMemcpyAsync(inst_root_out, c->inst_root.ptr, (size_t)c->n_instances * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return (int)c->n_nodes;
}
int rt_debug_read_pairs(rt_ctx* c, float* pairs_out, float* root_rec_out, uint32_t cap_pairs) {
  if (!c) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  c->pairs_wanted = true;
  int r = prepare_scene(c);
  c->pairs_wanted = false;
  if (r < 0) return r;
  if (cap_pairs < c->n_pairs || !c->pairs.ptr || !c->root_rec.ptr) return fail(c, RT_ERR_INVALID, "rt_debug_read_pairs: no records or buffer too small");
  if (pairs_out && c->n_pairs) HIP_TRY(c, hipMemcpyAsync(pairs_out, c->pairs.ptr, (size_t)c->n_pairs * 64, hipMemcpyDeviceToHost, c->stream));
  if (root_rec_out) HIP_TRY(c, hipMemcpyAsync(root_rec_out, c->root_rec.ptr, ((size_t)c->n_instances + 1) * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return (int)c->n_pairs;
}
int rt_debug_trace_sections(rt_ctx* c, uint64_t* out16, int reset) {
  if (!c || !out16) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(rtk::g_trace_sections), 128, 0, hipMemcpyDeviceToHost));
  if (reset) {
    uint64_t zero[16] = {0};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_trace_sections), zero, 128, 0, hipMemcpyHostToDevice));
  }
#ifdef RT_TRACE_STAMPS
  return 1;
#else
  return 0;
#endif
}
int rt_debug_pt_sections(rt_ctx* c, uint64_t* out8, int reset) {
  if (!c || !out8) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpyFromSymbol(out8, HIP_SYMBOL(rtk::g_pt_sections), 64, 0, hipMemcpyDeviceToHost));
  if (reset) {
    uint64_t zero[8] = {0};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_pt_sections), zero, 64, 0, hipMemcpyHostToDevice));
  }
#ifdef RT_PT_STAMPS
  return 1;
#else
  return 0;
#endif
}
int rt_debug_pt_launch(rt_ctx* c, uint32_t* out4) {
  if (!c || !out4) return RT_ERR_INVALID;
  for (int k = 0; k < 4; k++) out4[k] = c->pt_launch[k];
  return RT_OK;
}
int rt_debug_pt_form(const rt_ctx* c) { return c ? c->pt_form : RT_ERR_INVALID; }
int rt_debug_lane_stats(rt_ctx* c, uint64_t* out32, int reset) {
  if (!c || !out32) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpyFromSymbol(out32, HIP_SYMBOL(rtk::g_lane_stats), 256, 0, hipMemcpyDeviceToHost));
  if (reset) {
    uint64_t zero[32] = {0};
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_lane_stats), zero, 256, 0, hipMemcpyHostToDevice));
  }
#ifdef RT_LANE_STATS
  return 1;
#else
  return 0;
#endif
}
int rt_debug_clock_stamps(rt_ctx* c, uint64_t* out_pairs, uint32_t cap_pairs) {
  if (!c || !out_pairs) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t n = cap_pairs < RT_CLOCK_STAMP_SLOTS ? cap_pairs : RT_CLOCK_STAMP_SLOTS;
  HIP_TRY(c, hipMemcpyFromSymbol(out_pairs, HIP_SYMBOL(rtk::g_clock_stamps), (size_t)n * 16, 0, hipMemcpyDeviceToHost));
#ifdef RT_CLOCK_STAMP
  return (int)n;
#else
  return 0;  // product build: the kernels execute no stamp
#endif
}
int rt_debug_ieee_check(rt_ctx* c, int op, uint64_t first, uint64_t count, rt_ieee_report* out) {
  if (!c || !out) return RT_ERR_INVALID;
  static_assert(sizeof(rt_ieee_report) == sizeof(rtk::IeeeReport), "report layouts differ");
  std::memset(out, 0, sizeof(*out));
#ifdef RT_IEEE_PLAIN
  return fail(c, RT_ERR_INVALID, "rt_debug_ieee_check: built with RT_IEEE_PLAIN, the kernels use the plain operators");
#else
  if (op < 0 || op >= RT_IEEE_OP_COUNT) return fail(c, RT_ERR_INVALID, "rt_debug_ieee_check: unknown op");
  if (count == 0) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  DeviceBuffer report;   // freed on every way out
  HIP_TRY(c, hipMalloc(&report.ptr, sizeof(rtk::IeeeReport)));
  rtk::IeeeReport* d = (rtk::IeeeReport*)report.ptr;
  hipError_t e = hipMemsetAsync(d, 0, sizeof(rtk::IeeeReport), c->stream);
  const uint64_t want = (count + 255) / 256;
  const dim3 grid((uint32_t)std::min<uint64_t>(want, (uint64_t)c->num_cus * 32u)), block(256);
  if (e == hipSuccess) {
    switch (op) {
      case RT_IEEE_OP_RCP: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_RCP>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_SQRT: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_SQRT>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_RSQRT: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_RSQRT>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_DIV: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_DIV>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_DIV3: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_DIV3>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_DIV3Z: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_DIV3Z>, grid, block, 0, c->stream, first, count, d); break;
      case RT_IEEE_OP_DIV_PI: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_DIV_PI>, grid, block, 0, c->stream, first, count, d); break;
      default: hipLaunchKernelGGL(rtk::k_ieee_check<RT_IEEE_OP_UNORM8>, grid, block, 0, c->stream, first, count, d); break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(*out), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "rt_debug_ieee_check");
  out->n = count;
  return RT_OK;
#endif
}
int rt_kernel_times(rt_ctx* c, double* sum_ms, uint32_t* launches, uint32_t n) {
  if (!c || !sum_ms || !launches) return RT_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < n; k++) {
    sum_ms[k] = 0.0;
    launches[k] = 0;
  }
  for (auto& t : c->ev_tags) {
    float ms = 0;
    if ((uint32_t)t.second < n && hipEventElapsedTime(&ms, c->ev_pool[t.first].a, c->ev_pool[t.first].b) == hipSuccess) {
      sum_ms[t.second] += ms;
      launches[t.second]++;
    }
  }
  c->ev_tags.clear();
  c->ev_used = 0;
  return RT_OK;
}
int rt_kernel_time_ms(rt_ctx* c, double* avg_pt, double* avg_pv, uint32_t* launches) {
  double sum[RT_TIMER_COUNT];
  uint32_t cnt[RT_TIMER_COUNT];
  int r = rt_kernel_times(c, sum, cnt, RT_TIMER_COUNT);
  if (r < 0) return r;
  if (avg_pv) *avg_pv = cnt[RT_TIMER_PRIMARY] ? sum[RT_TIMER_PRIMARY] / cnt[RT_TIMER_PRIMARY] : 0.0;
  if (avg_pt) *avg_pt = cnt[RT_TIMER_PATHTRACE] ? sum[RT_TIMER_PATHTRACE] / cnt[RT_TIMER_PATHTRACE] : 0.0;
  if (launches) *launches = cnt[RT_TIMER_PATHTRACE];
  return RT_OK;
}

// ---------------------------------------------------------------- the sharded image
int rt_dist_unique_id(uint8_t out[128]) {
  if (!out) return RT_ERR_INVALID;
  Rccl& R = rccl();
  if (!R.error.empty()) {
    g_create_error = R.error;
    return RT_ERR_RCCL;
  }
  RcclUniqueId id;
  std::memset(&id, 0, sizeof(id));
  const int rc = R.GetUniqueId(&id);
  if (rc != 0) {
    g_create_error = rccl_what("ncclGetUniqueId", rc);
    return RT_ERR_RCCL;
  }
  std::memcpy(out, id.internal, 128);
  return RT_OK;
}
int rt_dist_init(rt_ctx* c, uint32_t rank, uint32_t world, uint32_t stripe_rows, const uint8_t* unique_id128) {
  if (!c) return RT_ERR_INVALID;
  if (world == 0 || world > 65535u) return fail(c, RT_ERR_INVALID, "rt_dist_init: world must be 1 .. 65535");
  if (rank >= world) return fail(c, RT_ERR_INVALID, "rt_dist_init: rank >= world");
  if (stripe_rows == 0) return fail(c, RT_ERR_INVALID, "rt_dist_init: stripe_rows must be >= 1");
  if (c->dist.active) return fail(c, RT_ERR_INVALID, "rt_dist_init: the context is a rank already (rt_dist_shutdown first)");
  if (c->external_accum || c->present_source || c->accum_stale || c->present_stale)
    return fail(c, RT_ERR_INVALID, "rt_dist_init: unbind rt_bind_accum / rt_bind_present_source first (a rank uses the context's own buffers)");
  if (c->fd.present_on)
    return fail(c, RT_ERR_INVALID, "rt_dist_init: present() filters the frame, and a rank's G-buffer covers only its own rows (rt_set_present_denoise(NULL) first)");
  HIP_TRY(c, hipSetDevice(c->device));
  void* comm = nullptr;
  if (unique_id128) {
    Rccl& R = rccl();
    if (!R.error.empty()) return fail(c, RT_ERR_RCCL, "rt_dist_init: " + R.error);
    RcclUniqueId id;
    std::memcpy(id.internal, unique_id128, 128);
    const int rc = R.CommInitRank(&comm, (int)world, id, (int)rank);
    if (rc != 0 || !comm) return fail(c, RT_ERR_RCCL, "rt_dist_init: " + rccl_what("ncclCommInitRank", rc));
  }
  c->dist.active = true;
  c->dist.rank = rank;
  c->dist.world = world;
  c->dist.stripe_rows = stripe_rows;
  c->dist.comm = comm;
  c->stripe_rows = stripe_rows;
  c->stripe_rank = rank;
  c->stripe_count = world;
  c->epoch++;   // drops frames traced ahead for other stripes (rt_set_lookahead)
  const int r = dist_alloc(c);
  if (r < 0) {
    const std::string why = c->error;
    (void)hipStreamSynchronize(c->stream);
    dist_release(c);
    return fail(c, r, "rt_dist_init: " + why);
  }
  return RT_OK;
}
int rt_dist_shutdown(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (!c->dist.active) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dist_release(c);
  return RT_OK;
}
size_t rt_dist_block_bytes(const rt_ctx* c) { return (c && c->dist.active) ? dist_block_bytes(c) : 0; }
int rt_pack_stripes(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_pack_stripes", false)) return r;
  HIP_TRY(c, hipSetDevice(c->device));
  return dist_launch_pack(c);
}
int rt_dist_read_block(rt_ctx* c, void* host_out, size_t cap) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_dist_read_block", false)) return r;
  if (!host_out) return fail(c, RT_ERR_INVALID, "rt_dist_read_block: null buffer");
  const size_t bytes = dist_block_bytes(c);
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "rt_dist_read_block: buffer smaller than rt_dist_block_bytes");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(host_out, c->dist.send.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}
int rt_dist_write_block(rt_ctx* c, uint32_t from_rank, const void* host_in, size_t bytes) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_dist_write_block", true)) return r;
  if (!host_in) return fail(c, RT_ERR_INVALID, "rt_dist_write_block: null buffer");
  if (from_rank >= c->dist.world) return fail(c, RT_ERR_INVALID, "rt_dist_write_block: from_rank >= world");
  const size_t block = dist_block_bytes(c);
  if (bytes != block) return fail(c, RT_ERR_INVALID, "rt_dist_write_block: byte count is not rt_dist_block_bytes");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync((char*)c->dist.recv.ptr + (size_t)from_rank * block, host_in, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // queue.writeBuffer semantics: the source may be reused on return
  return RT_OK;
}
int rt_unpack_stripes(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_unpack_stripes", true)) return r;
  HIP_TRY(c, hipSetDevice(c->device));
  return dist_launch_unpack(c);
}
int rt_gather_stripes(rt_ctx* c) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_gather_stripes", false)) return r;
  if (!c->dist.comm)
    return fail(c, RT_ERR_INVALID, "rt_gather_stripes: no communicator (rt_dist_init was given no unique id): move the blocks with "
                                   "rt_dist_read_block / rt_dist_write_block and call rt_pack_stripes / rt_unpack_stripes");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int r = dist_launch_pack(c)) return r;
  Rccl& R = rccl();
  const size_t block = dist_block_bytes(c), count = block / 4;
  int rc = R.GroupStart();
  if (rc != 0) return fail(c, RT_ERR_RCCL, rccl_what("ncclGroupStart", rc));
  int rc_op = R.Send(c->dist.send.ptr, count, kNcclFloat32, 0, c->dist.comm, c->stream);
  if (c->dist.rank == 0)
    for (uint32_t k = 0; k < c->dist.world && rc_op == 0; k++)
      rc_op = R.Recv((char*)c->dist.recv.ptr + (size_t)k * block, count, kNcclFloat32, (int)k, c->dist.comm, c->stream);
  rc = R.GroupEnd();   // always closed, also after a failed call inside the group
  if (rc_op != 0) return fail(c, RT_ERR_RCCL, rccl_what("ncclSend / ncclRecv", rc_op));
  if (rc != 0) return fail(c, RT_ERR_RCCL, rccl_what("ncclGroupEnd", rc));
  if (c->dist.rank == 0) return dist_launch_unpack(c);
  return RT_OK;
}
int rt_read_display(rt_ctx* c, float* out, size_t cap) {
  if (!c) return RT_ERR_INVALID;
  if (int r = dist_ready(c, "rt_read_display", true)) return r;
  if (!out) return fail(c, RT_ERR_INVALID, "rt_read_display: null buffer");
  const size_t bytes = (size_t)c->width * c->height * 16;
  if (cap < bytes) return fail(c, RT_ERR_INVALID, "rt_read_display: buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(out, c->dist.display.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

}  // extern "C"
