// k_volume.hip.h — the kernels of irradiance volumes (rt_bake_volume / rt_sample_volume / rt_encode_volume, mi355rt.h "THE
// VOLUME RULE"): k_volume_probes makes the rt_probe records of a grid, k_volume_finish turns gathered SH9 radiance into
// windowed irradiance coefficients in place, k_volume_sample is the trilinear sampler and k_volume_layers the export into
// seven texel layers.  The path work between the first two is the probe gather's launch sequence as it stands.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_VOLUME_HIP_H
#define MI355RT_K_VOLUME_HIP_H

namespace rtk {

#define RT_VOLUME_VEC4 7u   // float4 per rt_probe_sh9

// One thread per probe p = (z * ny + y) * nx + x: position[a] = origin[a] + (float)idx_a * step[a] (the product rounded
// first), t_max of the desc, unused +0, pad = pad_first + p.  The 32 bytes leave as two 16-byte stores.
__global__ __launch_bounds__(256)
void k_volume_probes(rt_volume_desc D, float4* __restrict__ probes, uint32_t n) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  const uint32_t x = p % D.nx, yz = p / D.nx;
  const uint32_t y = yz % D.ny, z = yz / D.ny;
  const float px = D.origin[0] + (float)x * D.step[0];
  const float py = D.origin[1] + (float)y * D.step[1];
  const float pz = D.origin[2] + (float)z * D.step[2];
  probes[2 * (size_t)p] = make_float4(px, py, pz, D.t_max);
  probes[2 * (size_t)p + 1] = make_float4(0.0f, 0.0f, 0.0f, rt_u2f(D.pad_first + p));
}

// band factor of word w = 3 k + c of a record (w < 27): the cosine-lobe constant of k's band, and which window entry
__device__ __forceinline__ float volume_band_A(uint32_t w) { return w < 3u ? 3.141592654f : w < 12u ? 2.094395102f : 0.785398163f; }
__device__ __forceinline__ float volume_band_window(const rt_volume_desc& D, uint32_t w) {
  return w < 3u ? D.window[0] : w < 12u ? D.window[1] : D.window[2];
}

// One thread per (probe, 16-byte vector): sh' = (sh * A_band) * window[band], in place; the 28th word, hit_fraction, keeps
// its bits (the seventh vector carries it through untouched).
__global__ __launch_bounds__(256)
void k_volume_finish(rt_volume_desc D, float4* __restrict__ volume, uint32_t n_vec) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;   // n_vec = 7 n <= 7 * 2^24
  if (g >= n_vec) return;
  const uint32_t w0 = 4u * (g % RT_VOLUME_VEC4);
  float4 v = volume[g];
  v.x = (v.x * volume_band_A(w0)) * volume_band_window(D, w0);
  v.y = (v.y * volume_band_A(w0 + 1u)) * volume_band_window(D, w0 + 1u);
  v.z = (v.z * volume_band_A(w0 + 2u)) * volume_band_window(D, w0 + 2u);
  if (w0 + 3u < 27u) v.w = (v.w * volume_band_A(w0 + 3u)) * volume_band_window(D, w0 + 3u);
  volume[g] = v;
}

// the cell of one axis: the two probe indices and their weights
struct VolumeAxis {
  uint32_t i0, i1;
  float w0, w1;
};
__device__ __forceinline__ VolumeAxis volume_axis(float position, float origin, float step, uint32_t N) {
  float g = rt_div(position - origin, step);
  if (!(g > 0.0f)) g = 0.0f;   // NaN too
  g = rt_min(g, (float)(N - 1u));
  VolumeAxis a;
  a.i0 = (uint32_t)g;
  if (N > 1u && a.i0 > N - 2u) a.i0 = N - 2u;
  a.i1 = N > 1u ? a.i0 + 1u : a.i0;
  const float f = N > 1u ? g - (float)a.i0 : 0.0f;
  a.w0 = 1.0f - f;
  a.w1 = f;
  return a;
}

// The sampler: EIGHT lanes per point, 32 points per 256-thread workgroup.  Lane j = 0 .. 6 of a point's group owns the j-th
// 16-byte vector of a record (words 4 j .. 4 j + 3); lane 7 rides along on vector 6 and contributes nothing.  Every lane
// works out the cell and the eight weights of its point (the same arithmetic on the same two broadcast loads), then issues
// its eight 16-byte loads, one per corner, before anything uses one: the seven working lanes of a group read one corner's
// 112 bytes as one run, and a corner's x-neighbour is the next 112.  Lane 6's fourth word is a corner's hit_fraction: eight
// shuffles inside the group hand the validity to all.  A lane then sums ITS four words over the corners in corner order,
// skipping corners of weight zero - the rule's order, no cross-lane sum - and divides them by W.  27 group shuffles give every
// lane the 27 coefficients; the evaluation at the normal is in k order; lane 0 of the group stores the 16 bytes.  No LDS, no
// atomics; a result depends on (volume, desc, point) alone.
struct VolumeSampleArgs {
  rt_volume_desc D;
  const float4* volume;     // nx * ny * nz records, 7 float4 each
  const float4* points;     // n rt_gather_point, 2 float4 each
  float4* out;              // n rt_irradiance
  uint32_t n;               // < 2^31
};

// no weight beside the trilinear one: k_volume_sample's.  k_volume_sample_visible (k_volume_visibility.hip.h) has another.
struct VolumeNoWeight {
  __device__ __forceinline__ void operator()(const rt_volume_desc&, VolumeAxis, VolumeAxis, VolumeAxis,
                                             const float4&, const float4&, uint32_t, float (&)[8]) const {}
};

// the sampler's body for the arguments A (VolumeSampleArgs, or a record with the same members); corner_weights(D, ax, ay, az,
// p0, p1, j, w) may scale the eight trilinear weights of lane j's point, the same in all eight lanes, after the loads are issued
// (the three axis records go by value: handed over by reference they stayed in memory, which the compiler then put into LDS)
template <class Args, class CornerWeights>
__device__ __forceinline__ void volume_sample_body(const Args& A, const CornerWeights& corner_weights) {
  const uint32_t i = blockIdx.x * 32u + (threadIdx.x >> 3);
  if (i >= A.n) return;                                  // whole groups leave together
  const uint32_t j = threadIdx.x & 7u;
  const uint32_t vec = j < RT_VOLUME_VEC4 ? j : RT_VOLUME_VEC4 - 1u;
  const rt_volume_desc& D = A.D;
  const float4 p0 = A.points[2 * (size_t)i];
  const float4 p1 = A.points[2 * (size_t)i + 1];
  const VolumeAxis ax = volume_axis(p0.x, D.origin[0], D.step[0], D.nx);
  const VolumeAxis ay = volume_axis(p0.y, D.origin[1], D.step[1], D.ny);
  const VolumeAxis az = volume_axis(p0.z, D.origin[2], D.step[2], D.nz);
  float4 v[8];
  float w[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const uint32_t x = (c & 1) ? ax.i1 : ax.i0, y = (c & 2) ? ay.i1 : ay.i0, z = (c & 4) ? az.i1 : az.i0;
    const uint32_t p = (z * D.ny + y) * D.nx + x;        // < n <= 2^24: every index is clamped into the grid
    v[c] = A.volume[RT_VOLUME_VEC4 * (size_t)p + vec];
    w[c] = (((c & 1) ? ax.w1 : ax.w0) * ((c & 2) ? ay.w1 : ay.w0)) * ((c & 4) ? az.w1 : az.w0);
  }
  corner_weights(D, ax, ay, az, p0, p1, j, w);
  float W = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const float hit_fraction = __shfl(v[c].w, 6, 8);
    if (!(hit_fraction <= D.max_hit_fraction)) w[c] = 0.0f;
    W = W + w[c];
  }
  float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int c = 0; c < 8; c++)
    if (w[c] != 0.0f) {
      S.x = S.x + w[c] * v[c].x;
      S.y = S.y + w[c] * v[c].y;
      S.z = S.z + w[c] * v[c].z;
      S.w = S.w + w[c] * v[c].w;
    }
  const bool any = W > 0.0f;                             // the same in all eight lanes of the group
  const float den = any ? W : 1.0f;
  const float q[4] = {rt_div(S.x, den), rt_div(S.y, den), rt_div(S.z, den), rt_div(S.w, den)};
  float coef[27];
#pragma unroll
  for (int k = 0; k < 27; k++) coef[k] = __shfl(q[k & 3], k >> 2, 8);
  const rt3 d = rt_normalize(rt3_make(p1.x, p1.y, p1.z));
  float Y[9];
  Y[0] = 0.282094792f;
  Y[1] = 0.488602512f * d.y;
  Y[2] = 0.488602512f * d.z;
  Y[3] = 0.488602512f * d.x;
  Y[4] = 1.092548431f * (d.x * d.y);
  Y[5] = 1.092548431f * (d.y * d.z);
  Y[6] = 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
  Y[7] = 1.092548431f * (d.x * d.z);
  Y[8] = 0.546274215f * (d.x * d.x - d.y * d.y);
  float E[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 9; k++)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) E[ch] = E[ch] + coef[3 * k + ch] * Y[k];
  if (j == 0u)
    A.out[i] = any ? make_float4(rt_max(0.0f, E[0]), rt_max(0.0f, E[1]), rt_max(0.0f, E[2]), W)
                   : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(256)
void k_volume_sample(VolumeSampleArgs A) { volume_sample_body(A, VolumeNoWeight()); }

// The export for consumers that upload 3D textures: n probe-major records into 7 layers of n texels, layer j holding the
// floats 4 j .. 4 j + 3 of each record.  One thread per (probe, vector), the probe fastest, so a wave writes one run of a
// layer: 16 bytes per texel (RT_LIGHTMAP_F32, the words unchanged) or 8 (RT_LIGHTMAP_F16: four rt_f32_to_f16, as
// k_encode_atlas does it).  The format is a kernel argument, hence wave-uniform.
struct VolumeLayersArgs {
  const uint4* volume;      // n records, 7 uint4 each
  void* out;                // 7 * n uint4 (F32) or uint2 (F16); not `volume`
  uint32_t n;               // <= 2^24
  uint32_t format;          // RT_LIGHTMAP_F32 or RT_LIGHTMAP_F16
};

__global__ __launch_bounds__(256)
void k_volume_layers(VolumeLayersArgs A) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;    // = layer * n + probe < 7 * 2^24
  if (g >= RT_VOLUME_VEC4 * A.n) return;
  const uint32_t layer = g / A.n, p = g - layer * A.n;
  const uint4 t = A.volume[RT_VOLUME_VEC4 * (size_t)p + layer];
  if (A.format == RT_LIGHTMAP_F16) {
    uint2 h;
    h.x = (uint32_t)rt_f32_to_f16(__uint_as_float(t.x)) | ((uint32_t)rt_f32_to_f16(__uint_as_float(t.y)) << 16);
    h.y = (uint32_t)rt_f32_to_f16(__uint_as_float(t.z)) | ((uint32_t)rt_f32_to_f16(__uint_as_float(t.w)) << 16);
    ((uint2*)A.out)[g] = h;
  } else {
    ((uint4*)A.out)[g] = t;
  }
}

}  // namespace rtk
#endif
