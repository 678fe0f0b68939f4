// k_stripes.hip.h — the two copies of the sharded image's gather (rt_pack_stripes / rt_unpack_stripes, mi355rt.h).
//
// Layout (the one distributed.py uses, so the two paths are interchangeable): rank k owns the image rows y with
// (y / stripe_rows) % world == k; its COMPACT BLOCK holds those rows in ascending y, `width` float4 each, padded to
// max_rows rows (the largest share: blocks are equal-sized so that one collective moves them).  Row j of block k is
// image row
//     y(k, j) = ((j / stripe_rows) * world + k) * stripe_rows + j % stripe_rows
// which rises with j and runs through exactly the rows k owns: j is a row of the image while y < height and a padding
// row from there on.  Both kernels compute y arithmetically (no index table in memory), never move a padding row, and do
// no floating-point arithmetic: one 16-byte load and one 16-byte store per lane per float4, consecutive lanes on
// consecutive float4 of one row.
//
// Work item = (block row, 256-float4 chunk of the row): which row a workgroup copies is uniform over the workgroup, so the
// divisions run once per item on scalar values, not per lane.  The grid is capped and strides over the items.
#ifndef MI355RT_K_STRIPES_HIP_H
#define MI355RT_K_STRIPES_HIP_H

namespace rtk {

struct StripePlan {
  uint32_t width, height;      // image size in pixels (float4)
  uint32_t stripe_rows, world;
  uint32_t max_rows;           // rows of a compact block
  uint32_t chunks;             // ceil(width / 256)
};

// image row of row j of rank k's block; >= height: a padding row (64-bit: (j / stripe_rows) * world may pass 2^32)
__device__ __forceinline__ uint64_t stripe_image_row(const StripePlan& p, uint32_t k, uint32_t j) {
  return ((uint64_t)(j / p.stripe_rows) * p.world + k) * p.stripe_rows + j % p.stripe_rows;
}

// accumulator (full size; only the rows this rank owns are read) -> this rank's compact block
__global__ __launch_bounds__(256) void k_pack_stripes(const float4* __restrict__ accum, float4* __restrict__ block,
                                                      StripePlan p, uint32_t rank) {
  const uint32_t items = p.max_rows * p.chunks;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item / p.chunks, x = (item % p.chunks) * 256u + threadIdx.x;
    const uint64_t y = stripe_image_row(p, rank, j);
    if (y >= p.height) break;   // rows rise with j, and so do the items of this workgroup: only padding follows
    if (x < p.width) block[(size_t)j * p.width + x] = accum[(size_t)y * p.width + x];
  }
}

// rank 0: the `world` received blocks (block k at blocks + k * max_rows * width) -> the display image, one launch
__global__ __launch_bounds__(256) void k_unpack_stripes(const float4* __restrict__ blocks, float4* __restrict__ display,
                                                        StripePlan p) {
  const uint64_t per_block = (uint64_t)p.max_rows * p.chunks, items = per_block * p.world;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t k = (uint32_t)(item / per_block), r = (uint32_t)(item % per_block);
    const uint32_t j = r / p.chunks, x = (r % p.chunks) * 256u + threadIdx.x;
    const uint64_t y = stripe_image_row(p, k, j);
    if (y >= p.height) continue;   // a padding row of block k; the next item may belong to another block
    if (x < p.width) display[(size_t)y * p.width + x] = blocks[((size_t)k * p.max_rows + j) * p.width + x];
  }
}

}  // namespace rtk
#endif
