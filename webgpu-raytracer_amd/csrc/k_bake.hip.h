// k_bake.hip.h — lightmap bakes: the UV-space rasteriser that turns the texels of one instance's atlas into gather points
// (rt_bake_points, mi355rt.h "lightmap bakes": the texel rule is stated there, once) and the scatter that puts gathered
// values back into the atlas (rt_bake_irradiance); behind them the same for a list of (instance, rectangle) entries in one
// atlas (rt_bake_atlas_points, "atlas bakes"), on the same device functions.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_BAKE_HIP_H
#define MI355RT_K_BAKE_HIP_H

namespace rtk {

// Four launches on one stream; the kernel boundary is the only synchronisation between them, and no workgroup reads what
// another workgroup of the same launch wrote:
//   k_bake_owner   (triangle, tile) items.  A work item is 64 consecutive triangles of the instance x one band of
//                  RT_BAKE_BAND_TILES tile rows: every lane loads ONE triangle (its texel-space vertices, area and box:
//                  the vertex data is read once per wave), the wave then takes the triangles whose box meets the band
//                  one by one, their values broadcast from the lane that loaded them, and tests one 8 x 8 texel tile
//                  per step - 64 lanes, 64 centres - over the tiles of the box inside the band.  Ownership is an integer
//                  atomicMin of the global triangle index on the u32 owner map: the minimum does not depend on the order
//                  in which the waves arrive, so the map is the same in every run.  A triangle that spans the atlas is
//                  thereby split over tiles_y / RT_BAKE_BAND_TILES items instead of being one wave's loop; the item list
//                  is a function of W, H and the scene's triangle count alone.
//   k_bake_count   256 texels per workgroup: covered texels (block_count, k_block_scan.hip.h), one total per workgroup
//   k_scan_counts  one workgroup: exclusive prefix sums of those totals in place, the grand total to the device count
//   k_bake_emit    256 texels per workgroup again: rank of a covered texel = prefix of its workgroup + covered texels
//                  before it in the workgroup (block_rank), which is ascending texel order; its point is computed and
//                  stored there (two 16-byte stores) with its texel index, when the rank is below cap
// and k_bake_scatter, the way back: atlas[texels[j]] = results[j], every uncovered texel {+0, +0, +0, -1}.
#define RT_BAKE_NONE 0xffffffffu     // owner map: no triangle covers the texel (-1 as the i32 the host reads)
#define RT_BAKE_BAND_TILES 4u        // tile rows of one owner-pass item

struct BakeArgs {
  const float2* auv;       // atlas UV of every global vertex: the caller's override array, or the scene's uv
  const uint4* draw;       // draw commands, one per TLAS-order instance: {3 n_tris, 1, 3 first_tri, i}
  uint32_t* owner;         // W * H
  uint32_t* block_count;   // n_blocks: covered texels of each 256-texel block, then (k_scan_counts) their exclusive prefix
  float4* points;          // 2 per covered texel (rt_gather_point)
  uint32_t* texels;
  uint32_t inst, W, H, pad_base;
  float t_max;
  uint32_t n_tris;         // triangles of the topology array (robust-access clamp)
  uint32_t cap;            // records points / texels hold
  uint32_t n_blocks;       // ceil(W * H / 256)
  uint32_t tiles_x, tiles_y, bands, n_chunks;   // ceil(W / 8), ceil(H / 8), ceil(tiles_y / BAND), ceil(n_tris / 64)
};

struct BakeTri {   // texel-space vertices and E(a, b, c)
  float ax, ay, bx, by, cx, cy, A;
};

__device__ __forceinline__ uint32_t rt_min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t rt_max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ bool bake_finite(float x) { return (rt_f2u(x) & 0x7fffffffu) < 0x7f800000u; }
__device__ __forceinline__ float bake_edge(float qx, float qy, float rx, float ry, float sx, float sy) {
  return (rx - qx) * (sy - qy) - (ry - qy) * (sx - qx);
}
// texel-space triangle of global triangle k in a W x H atlas with the atlas UVs auv; false: a coordinate or the area is not
// finite, or the area is 0
__device__ __forceinline__ bool bake_load_tri(const DevScene& S, const float2* auv, uint32_t W, uint32_t H, uint32_t k, BakeTri& T) {
  const float4 idx = S.topo[5 * (size_t)k];
  const float2 u0 = auv[rt_f2u(idx.x)], u1 = auv[rt_f2u(idx.y)], u2 = auv[rt_f2u(idx.z)];
  const float fw = (float)W, fh = (float)H;
  T.ax = u0.x * fw;
  T.ay = u0.y * fh;
  T.bx = u1.x * fw;
  T.by = u1.y * fh;
  T.cx = u2.x * fw;
  T.cy = u2.y * fh;
  T.A = bake_edge(T.ax, T.ay, T.bx, T.by, T.cx, T.cy);
  return bake_finite(T.ax) && bake_finite(T.ay) && bake_finite(T.bx) && bake_finite(T.by) && bake_finite(T.cx) &&
         bake_finite(T.cy) && bake_finite(T.A) && T.A != 0.0f;
}
// the coverage rule for a triangle bake_load_tri accepted
__device__ __forceinline__ bool bake_covers(const BakeTri& T, float px, float py) {
  const float min_x = rt_min(rt_min(T.ax, T.bx), T.cx), max_x = rt_max(rt_max(T.ax, T.bx), T.cx);
  const float min_y = rt_min(rt_min(T.ay, T.by), T.cy), max_y = rt_max(rt_max(T.ay, T.by), T.cy);
  if (!(min_x <= px && px <= max_x && min_y <= py && py <= max_y)) return false;
  const float sg = T.A > 0.0f ? 1.0f : -1.0f;
  return sg * bake_edge(T.ax, T.ay, T.bx, T.by, px, py) >= 0.0f && sg * bake_edge(T.bx, T.by, T.cx, T.cy, px, py) >= 0.0f &&
         sg * bake_edge(T.cx, T.cy, T.ax, T.ay, px, py) >= 0.0f;
}
// The texels i of 0 .. n-1 whose centre (float)i + 0.5f can lie in [min_v, max_v] (finite): a superset, floor(min_v) - 1 ..
// floor(max_v), clamped IN FLOAT before the conversion.  false: none.
__device__ __forceinline__ bool bake_range(float min_v, float max_v, uint32_t n, uint32_t& lo, uint32_t& hi) {
  const float fn = (float)n;
  if (!(max_v >= 0.5f) || !(min_v <= fn)) return false;
  lo = (uint32_t)(rt_floor(rt_max(min_v, 1.0f)) - 1.0f);   // 0 .. n - 1
  hi = (uint32_t)rt_floor(rt_min(max_v, fn));              // 0 .. n
  if (hi > n - 1u) hi = n - 1u;
  return lo <= hi;
}
__device__ __forceinline__ float bake_bcast(float v, uint32_t src) {   // src: wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)src));
}
__device__ __forceinline__ uint32_t bake_bcast(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}

// One owner-pass item: triangles first + 64 chunk .. of the n_own triangles from `first`, against band `band` of the W x H
// atlas.  own(x, y, k) is called by the lane of texel (x, y) for every global triangle k of the item that covers it.
template <class Own>
__device__ __forceinline__ void bake_owner_item(const DevScene& S, const float2* auv, uint32_t W, uint32_t H, uint32_t first,
                                                uint32_t n_own, uint32_t chunk, uint32_t band, uint32_t lane, Own own) {
  const uint32_t tiles_y = (H + 7u) / 8u;
  const uint32_t band_y0 = band * RT_BAKE_BAND_TILES;
  const uint32_t band_y1 = rt_min_u32(band_y0 + RT_BAKE_BAND_TILES, tiles_y) - 1u;
  // one triangle per lane
  const uint32_t t = chunk * 64u + lane;
  BakeTri T = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t tx0 = 0u, tx1 = 0u, ty0 = 0u, ty1 = 0u;
  bool live = t < n_own;
  if (live) live = bake_load_tri(S, auv, W, H, first + t, T);
  if (live) {
    uint32_t x0, x1, y0, y1;
    live = bake_range(rt_min(rt_min(T.ax, T.bx), T.cx), rt_max(rt_max(T.ax, T.bx), T.cx), W, x0, x1) &&
           bake_range(rt_min(rt_min(T.ay, T.by), T.cy), rt_max(rt_max(T.ay, T.by), T.cy), H, y0, y1);
    if (live) {
      tx0 = x0 >> 3;
      tx1 = x1 >> 3;
      ty0 = rt_max_u32(y0 >> 3, band_y0);
      ty1 = rt_min_u32(y1 >> 3, band_y1);
      live = ty0 <= ty1;
    }
  }
  uint64_t todo = __ballot(live);
  while (todo) {
    const uint32_t src = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
    todo &= todo - 1ull;
    BakeTri U;
    U.ax = bake_bcast(T.ax, src);
    U.ay = bake_bcast(T.ay, src);
    U.bx = bake_bcast(T.bx, src);
    U.by = bake_bcast(T.by, src);
    U.cx = bake_bcast(T.cx, src);
    U.cy = bake_bcast(T.cy, src);
    U.A = bake_bcast(T.A, src);
    const uint32_t ux0 = bake_bcast(tx0, src), ux1 = bake_bcast(tx1, src);
    const uint32_t uy0 = bake_bcast(ty0, src), uy1 = bake_bcast(ty1, src);
    const uint32_t k = first + chunk * 64u + src;
    for (uint32_t ty = uy0; ty <= uy1; ty++) {
      const uint32_t y = ty * 8u + (lane >> 3);
      for (uint32_t tx = ux0; tx <= ux1; tx++) {
        const uint32_t x = tx * 8u + (lane & 7u);
        if (x < W && y < H && bake_covers(U, (float)x + 0.5f, (float)y + 0.5f)) own(x, y, k);
      }
    }
  }
}
// triangles of a draw command that exist in a topology array of n_tris: the first, and how many
__device__ __forceinline__ uint32_t bake_own_tris(const uint4 dc, uint32_t n_tris, uint32_t& first) {
  first = dc.z / 3u;
  const uint32_t cnt = dc.x / 3u;
  return first < n_tris ? (cnt < n_tris - first ? cnt : n_tris - first) : 0u;
}

__global__ __launch_bounds__(256) void k_bake_owner(DevScene S, BakeArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * 4u;
  uint32_t first;
  const uint32_t n_own = bake_own_tris(A.draw[A.inst], A.n_tris, first);
  const uint64_t n_items = (uint64_t)A.n_chunks * A.bands;
  for (uint64_t item = wave; item < n_items; item += n_waves) {
    const uint32_t chunk = (uint32_t)(item / A.bands), band = (uint32_t)(item - (uint64_t)chunk * A.bands);
    if (chunk * 64u >= n_own) break;   // items are chunk-major: nothing of this wave's later items has a triangle either
    bake_owner_item(S, A.auv, A.W, A.H, first, n_own, chunk, band, lane,
                    [&](uint32_t x, uint32_t y, uint32_t k) { atomicMin(&A.owner[(size_t)y * A.W + x], k); });
  }
}

__global__ __launch_bounds__(256) void k_bake_count(BakeArgs A) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = block_count<256>(i < A.W * A.H && A.owner[i] != RT_BAKE_NONE, s_wave);
  if (threadIdx.x == 0u) A.block_count[blockIdx.x] = n;
}

// the point of texel (x, y) of instance inst's W x H atlas, owned by global triangle k
__device__ __forceinline__ void bake_point(const DevScene& S, const float2* auv, uint32_t W, uint32_t H, uint32_t inst, float t_max,
                                           uint32_t pad, uint32_t k, uint32_t x, uint32_t y, float4& r0, float4& r1) {
  BakeTri T;
  (void)bake_load_tri(S, auv, W, H, k, T);
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float bu = rt_div(bake_edge(T.cx, T.cy, T.ax, T.ay, px, py), T.A);
  const float bv = rt_div(bake_edge(T.ax, T.ay, T.bx, T.by, px, py), T.A);
  const float bw = 1.0f - bu - bv;
  const WorldTri w = world_triangle(S, k, inst);
  const rt3 pos = bw * w.v0 + bu * w.v1 + bv * w.v2;
  const float4 idx = S.topo[5 * (size_t)k];
  const rt3 n0 = xyz(S.nrm[rt_f2u(idx.x)]), n1 = xyz(S.nrm[rt_f2u(idx.y)]), n2 = xyz(S.nrm[rt_f2u(idx.z)]);
  const InvRows m = load_inv_rows(S, inst);
  const rt3 ln = rt_normalize(n0 * bw + n1 * bu + n2 * bv);   // setup_surface, without the normal map
  const rt3 n = rt_normalize(normal_to_world(m, ln));
  r0 = make_float4(pos.x, pos.y, pos.z, t_max);
  r1 = make_float4(n.x, n.y, n.z, rt_u2f(pad));
}
// The rank of a covered texel in ascending texel order: the exclusive prefix of its workgroup + the covered texels before it
// in the workgroup.
__global__ __launch_bounds__(256) void k_bake_emit(DevScene S, BakeArgs A) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t k = i < A.W * A.H ? A.owner[i] : RT_BAKE_NONE;
  uint32_t in_block;
  const uint32_t rank = A.block_count[blockIdx.x] + block_rank<256>(k != RT_BAKE_NONE, s_wave, in_block);
  if (k == RT_BAKE_NONE || rank >= A.cap) return;
  float4 r0, r1;
  bake_point(S, A.auv, A.W, A.H, A.inst, A.t_max, A.pad_base + i, k, i % A.W, i / A.W, r0, r1);
  A.points[2 * (size_t)rank] = r0;
  A.points[2 * (size_t)rank + 1] = r1;
  A.texels[rank] = i;
}

struct BakeScatterArgs {
  const void* owner;        // n_texels: u32 (k_bake_scatter) or u64 (k_atlas_scatter)
  const uint32_t* texels;   // n, each below n_texels and covered
  const float4* results;    // n rt_irradiance
  float4* atlas;            // n_texels
  uint32_t n_texels, n;
};
// The two stores of a thread go to different kinds of texel (an uncovered one, the covered texels[i]), and every texel is
// written by exactly one thread.
template <class T>
__device__ __forceinline__ void bake_scatter(const BakeScatterArgs& A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < A.n_texels && ((const T*)A.owner)[i] == (T)~(T)0) A.atlas[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if (i < A.n) A.atlas[A.texels[i]] = A.results[i];
}
__global__ __launch_bounds__(256) void k_bake_scatter(BakeScatterArgs A) { bake_scatter<uint32_t>(A); }

// ---- atlas bakes (rt_bake_atlas_points, mi355rt.h "atlas bakes"): a list of (instance, rectangle) entries into one atlas.
// The same launches on a 64-bit owner map, (entry << 32) | triangle, behind a work list made on the device:
//   k_atlas_items   one thread per entry: the owner-pass items of its local bake, ceil(n_own / 64) chunks of its draw
//                   command's triangles x the bands of its rectangle (tiles are local to the rectangle)
//   k_atlas_scan    one workgroup: exclusive prefix sums of those in place, the total behind them (it stays on the device)
//   k_atlas_owner   a persistent grid: the waves stride over item < total, find the entry by a wave-uniform binary search in
//                   the prefix array and run bake_owner_item on the entry's local atlas; ownership is an atomicMin of
//                   (entry << 32) | triangle on the u64 map at the atlas texel, the lexicographic minimum of (entry, triangle)
//   k_atlas_count, k_scan_counts, k_atlas_emit, k_atlas_scatter   as in the instance bake, on the u64 map; emit decodes
//                   (entry, triangle), loads the entry and computes the point of its local texel
struct BakeAtlasArgs {
  const float2* auv;
  const uint4* draw;
  const uint4* entries;          // rt_bake_rect: {inst, x, y, w} {h, 0, 0, 0}
  unsigned long long* owner;     // W * H
  unsigned long long* items;     // n_entries + 1: items per entry, then (k_atlas_scan) their exclusive prefix and the total
  uint32_t* block_count;         // n_blocks
  float4* points;
  uint32_t* texels;
  uint32_t W, H, pad_base;
  float t_max;
  uint32_t n_tris, cap, n_blocks, n_entries;
};
#define RT_ATLAS_NONE 0xffffffffffffffffull

__device__ __forceinline__ uint32_t atlas_bands(uint32_t h) {
  return ((h + 7u) / 8u + RT_BAKE_BAND_TILES - 1u) / RT_BAKE_BAND_TILES;
}

__global__ __launch_bounds__(256) void k_atlas_items(BakeAtlasArgs A) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= A.n_entries) return;
  const uint4 e0 = A.entries[2 * (size_t)e], e1 = A.entries[2 * (size_t)e + 1];
  uint32_t first;
  const uint32_t n_own = bake_own_tris(A.draw[e0.x], A.n_tris, first);
  A.items[e] = (unsigned long long)((n_own + 63u) / 64u) * atlas_bands(e1.x);
}

__global__ __launch_bounds__(1024) void k_atlas_scan(BakeAtlasArgs A) {
  __shared__ unsigned long long s[1024];
  array_scan_exclusive<1024>(A.items, A.n_entries, A.items + A.n_entries, s);
}

__global__ __launch_bounds__(256) void k_atlas_owner(DevScene S, BakeAtlasArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * 4u;
  const unsigned long long total = A.items[A.n_entries];
  for (unsigned long long item = wave; item < total; item += n_waves) {
    // the last entry whose prefix is <= item: entries without items share their prefix with the next one and are passed over
    uint32_t lo = 0u, hi = A.n_entries;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (A.items[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const unsigned long long local = item - A.items[e];
    const uint4 e0 = A.entries[2 * (size_t)e], e1 = A.entries[2 * (size_t)e + 1];
    uint32_t first;
    const uint32_t n_own = bake_own_tris(A.draw[e0.x], A.n_tris, first);
    const uint32_t bands = atlas_bands(e1.x);
    const uint32_t chunk = (uint32_t)(local / bands), band = (uint32_t)(local - (unsigned long long)chunk * bands);
    const unsigned long long tag = (unsigned long long)e << 32;
    bake_owner_item(S, A.auv, e0.w, e1.x, first, n_own, chunk, band, lane, [&](uint32_t x, uint32_t y, uint32_t k) {
      atomicMin(&A.owner[(size_t)(e0.z + y) * A.W + (e0.y + x)], tag | k);
    });
  }
}

__global__ __launch_bounds__(256) void k_atlas_count(BakeAtlasArgs A) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = block_count<256>(i < A.W * A.H && A.owner[i] != RT_ATLAS_NONE, s_wave);
  if (threadIdx.x == 0u) A.block_count[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void k_atlas_emit(DevScene S, BakeAtlasArgs A) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long o = i < A.W * A.H ? A.owner[i] : RT_ATLAS_NONE;
  uint32_t in_block;
  const uint32_t rank = A.block_count[blockIdx.x] + block_rank<256>(o != RT_ATLAS_NONE, s_wave, in_block);
  if (o == RT_ATLAS_NONE || rank >= A.cap) return;
  const uint32_t e = (uint32_t)(o >> 32), k = (uint32_t)o;
  const uint4 e0 = A.entries[2 * (size_t)e], e1 = A.entries[2 * (size_t)e + 1];
  float4 r0, r1;
  bake_point(S, A.auv, e0.w, e1.x, e0.x, A.t_max, A.pad_base + i, k, i % A.W - e0.y, i / A.W - e0.z, r0, r1);
  A.points[2 * (size_t)rank] = r0;
  A.points[2 * (size_t)rank + 1] = r1;
  A.texels[rank] = i;
}

__global__ __launch_bounds__(256) void k_atlas_scatter(BakeScatterArgs A) { bake_scatter<unsigned long long>(A); }

}  // namespace rtk
#endif
