// k_volume_visibility.hip.h — the kernels of probe visibility maps (rt_bake_volume_visibility / rt_sample_volume_visible /
// rt_encode_volume_visibility, mi355rt.h "THE VISIBILITY RULE"): k_visibility_rays and k_visibility_texels go around
// k_ray_query as k_reflection_rays and k_reflection_texels go around k_radiance_query, with the (texel, sample) pair as the
// unit of ray work; k_volume_sample_visible is k_volume_sample's body with a Chebyshev weight per corner; k_visibility_tiles is
// the export into bordered tiles.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_VOLUME_VISIBILITY_HIP_H
#define MI355RT_K_VOLUME_VISIBILITY_HIP_H

namespace rtk {

// A map is size * size texels of 8 bytes {mean distance, mean squared distance}, size = 1 << size_log2; the texels of the n
// probes of a grid are numbered T = p * size^2 + t, below 2^31 (the host refuses more).  A batch is the texels [first, first +
// n_texels) of that numbering: item g = tl * spt + s of a batch is sample s of texel first + tl.

// One thread per (texel, sample) of the batch: the ray {position of probe p, max_distance} {d, pad_t} as two 16-byte stores,
// pad_t = pad_first + T and d the reflection capture's jittered octahedral direction.  n_items = n_texels * spt <=
// RT_PROBE_BATCH_SAMPLES.
__global__ __launch_bounds__(256)
void k_visibility_rays(rt_volume_desc D, float4* __restrict__ rays, uint32_t n_items, uint32_t spt, uint32_t seed, uint32_t first,
                       uint32_t size_log2, float max_distance) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_items) return;
  const uint32_t tl = g / spt, s = g - tl * spt;
  const uint32_t T = first + tl;
  const uint32_t p = T >> (2u * size_log2), t = T & ((1u << (2u * size_log2)) - 1u);
  const uint32_t i = t & ((1u << size_log2) - 1u), j = t >> size_log2;
  const uint32_t f = seed * spt + s;
  const uint32_t x = p % D.nx, yz = p / D.nx;
  const uint32_t y = yz % D.ny, z = yz / D.ny;
  const float px = D.origin[0] + (float)x * D.step[0];
  const float py = D.origin[1] + (float)y * D.step[1];
  const float pz = D.origin[2] + (float)z * D.step[2];
  const uint32_t pad_t = D.pad_first + T;
  const rt3 d = reflection_direction(pad_t, f, i, j, (float)(1u << size_log2));
  rays[2 * (size_t)g] = make_float4(px, py, pz, max_distance);
  rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, rt_u2f(pad_t));
}

// One thread per texel of the batch: its spt hits {bits(t), tri, inst, hit} in sample order, x = rt_min(t, max_distance) - a
// miss hands the ray's t_max back, which is max_distance - summed from +0 beside x * x, both divided by spt; one 8-byte store.
__global__ __launch_bounds__(256)
void k_visibility_texels(const uint4* __restrict__ hits, float2* __restrict__ out, uint32_t n_texels, uint32_t spt, uint32_t first,
                         float max_distance) {
  const uint32_t tl = blockIdx.x * 256u + threadIdx.x;
  if (tl >= n_texels) return;
  const uint4* h = hits + (size_t)tl * spt;
  float m1 = 0.0f, m2 = 0.0f;
  for (uint32_t s = 0u; s < spt; s++) {
    const float x = rt_min(rt_u2f(h[s].x), max_distance);
    m1 = m1 + x;
    m2 = m2 + x * x;
  }
  if (spt != 1u) {
    m1 = rt_div(m1, (float)spt);
    m2 = rt_div(m2, (float)spt);
  }
  out[(size_t)first + tl] = make_float2(m1, m2);
}

// the wrap of a tap (i, j) in -1 .. size across the octahedral edge, x first, then y; -> texel index j * size + i
__device__ __forceinline__ uint32_t visibility_wrap(int i, int j, int size) {
  if (i < 0) {
    i = -1 - i;
    j = size - 1 - j;
  } else if (i >= size) {
    i = 2 * size - 1 - i;
    j = size - 1 - j;
  }
  if (j < 0) {
    j = -1 - j;
    i = size - 1 - i;
  } else if (j >= size) {
    j = 2 * size - 1 - j;
    i = size - 1 - i;
  }
  return (uint32_t)(j * size + i);
}

// one axis of the fetch: the left tap in -1 .. size - 1 and the weight of its neighbour.  A NaN u, or one below -1, takes tap
// -1; one above takes size - 1; the weight is u - (float)i0 whatever u is.
__device__ __forceinline__ int visibility_axis(float q, float fsize, float* fx) {
  const float u = (q * 0.5f + 0.5f) * fsize - 0.5f;
  float fl = rt_floor(u);
  if (!(fl >= -1.0f)) fl = -1.0f;   // NaN too
  fl = rt_min(fl, fsize - 1.0f);
  *fx = u - fl;
  return (int)fl;
}

// The visible sampler: k_volume_sample's body (volume_sample_body, k_volume.hip.h) - eight lanes per point, 32 points per
// 256-thread workgroup - with a weight hook.  Behind the eight record loads lane c of a group works out vis_c of corner c: the
// direction from the probe to the biased point, pack, the four 8-byte taps of the probe's map, all issued before one is used,
// and the Chebyshev arithmetic.  Eight shuffles inside the group hand the eight weights to all lanes: w_c = vis_c * tri_c.
// Everything behind that is k_volume_sample's own sequence.  No LDS, no atomics; a result depends on (volume, visibility,
// descs, point) alone.
struct VolumeSampleVisibleArgs {
  rt_volume_desc D;
  rt_volume_visibility_desc V;
  const float4* volume;     // nx * ny * nz records, 7 float4 each
  const float2* visibility; // nx * ny * nz maps of size * size texels
  const float4* points;     // n rt_gather_point, 2 float4 each
  float4* out;              // n rt_irradiance
  uint32_t n;               // < 2^31
};

struct VolumeVisibleWeight {
  const rt_volume_visibility_desc& V;
  const float2* visibility;
  __device__ __forceinline__ void operator()(const rt_volume_desc& D, VolumeAxis ax, VolumeAxis ay,
                                             VolumeAxis az, const float4& p0, const float4& p1, uint32_t j,
                                             float (&w)[8]) const {
    // this lane's corner
    const uint32_t cx = (j & 1u) ? ax.i1 : ax.i0, cy = (j & 2u) ? ay.i1 : ay.i0, cz = (j & 4u) ? az.i1 : az.i0;
    const rt3 P = rt3_make(D.origin[0] + (float)cx * D.step[0], D.origin[1] + (float)cy * D.step[1],
                           D.origin[2] + (float)cz * D.step[2]);
    const rt3 pos = rt3_make(p0.x, p0.y, p0.z);
    const rt3 nrm = rt_normalize(rt3_make(p1.x, p1.y, p1.z));
    const rt3 e = (pos + nrm * V.normal_bias) - P;
    const float len = rt_sqrt(rt_dot(e, e));
    float vis = 1.0f;
    if (len > 0.0f) {
      const int size = (int)V.size;
      const float fsize = (float)V.size;
      const rt2 q = pack_normal(e * rt_rcp(len));
      float fx, fy;
      const int i0 = visibility_axis(q.x, fsize, &fx), j0 = visibility_axis(q.y, fsize, &fy);
      // probe < 2^24 and every tap inside its map: the index stays below n * size^2 < 2^31 texels
      const float2* map = visibility + (size_t)((cz * D.ny + cy) * D.nx + cx) * (size_t)(V.size * V.size);
      const float2 t00 = map[visibility_wrap(i0, j0, size)];
      const float2 t10 = map[visibility_wrap(i0 + 1, j0, size)];
      const float2 t01 = map[visibility_wrap(i0, j0 + 1, size)];
      const float2 t11 = map[visibility_wrap(i0 + 1, j0 + 1, size)];
      const float a1 = t00.x + fx * (t10.x - t00.x), b1 = t01.x + fx * (t11.x - t01.x);
      const float a2 = t00.y + fx * (t10.y - t00.y), b2 = t01.y + fx * (t11.y - t01.y);
      const float m1 = a1 + fy * (b1 - a1), m2 = a2 + fy * (b2 - a2);
      if (!(len <= m1)) {
        const float var = rt_abs(m1 * m1 - m2);
        const float g = len - m1;
        float ch = rt_div(var, var + g * g);
        if (!(ch > 0.0f)) ch = 0.0f;   // NaN too
        ch = (ch * ch) * ch;
        vis = rt_max(ch, V.min_visibility);
      }
    }
    if (V.flags & RT_VOLUME_VIS_BACKFACE) {
      const rt3 h = rt_normalize(P - pos);
      const float b = (rt_dot(h, nrm) + 1.0f) * 0.5f;
      vis = vis * (b * b + 0.2f);
    }
    if (V.crush_threshold > 0.0f && vis < V.crush_threshold)
      vis = rt_div((vis * vis) * vis, V.crush_threshold * V.crush_threshold);
#pragma unroll
    for (int c = 0; c < 8; c++) w[c] = __shfl(vis, c, 8) * w[c];
  }
};

__global__ __launch_bounds__(256)
void k_volume_sample_visible(VolumeSampleVisibleArgs A) { volume_sample_body(A, VolumeVisibleWeight{A.V, A.visibility}); }

// The export for consumers that sample with a texture unit: map p becomes the tile (p % nx, p / nx) of (size + 2)^2 texels of an
// image nx tiles wide and ny * nz tiles high, its one-texel border the wrapped neighbour.  One thread per output texel in
// image order: 8 bytes (RT_LIGHTMAP_F32, the words unchanged) or 4 (RT_LIGHTMAP_F16, two rt_f32_to_f16).  The format is a
// kernel argument, hence wave-uniform.
struct VisibilityTilesArgs {
  const float2* visibility; // n maps
  void* out;                // width * height uint2 (F32) or uint32_t (F16); not `visibility`
  uint32_t nx, rows;        // tiles per row, rows of tiles (ny * nz)
  uint32_t size;
  uint32_t format;          // RT_LIGHTMAP_F32 or RT_LIGHTMAP_F16
};

__global__ __launch_bounds__(256)
void k_visibility_tiles(VisibilityTilesArgs A) {
  const uint32_t tile = A.size + 2u;
  const uint32_t width = A.nx * tile;                                  // <= 1024 * 34
  const uint64_t total = (uint64_t)width * (A.rows * tile);            // n * tile^2 < 2^31 * 2.25
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= total) return;
  const uint32_t Y = (uint32_t)(g / width), X = (uint32_t)(g - (uint64_t)Y * width);
  const uint32_t tx = X / tile, ty = Y / tile;
  const int i = (int)(X - tx * tile) - 1, j = (int)(Y - ty * tile) - 1;
  const size_t p = (size_t)ty * A.nx + tx;
  const float2 t = A.visibility[p * (A.size * A.size) + visibility_wrap(i, j, (int)A.size)];
  if (A.format == RT_LIGHTMAP_F16)
    ((uint32_t*)A.out)[g] = (uint32_t)rt_f32_to_f16(t.x) | ((uint32_t)rt_f32_to_f16(t.y) << 16);
  else
    ((float2*)A.out)[g] = t;
}

}  // namespace rtk
#endif
