// Batch assembly from a device-resident dataset cache (dataset.py:DeviceCachedLoader).
//
// The host preprocessing of src/dataset.py:55-84 (PIL open, bilinear resize, polygon fill, NEAREST
// resize) runs once per sample; what it yields is kept on the device in its smallest exact form:
//   image  u8   the resized grey image as PIL returns it, + (lo, den) per sample, or
//          f32  the float image verbatim (any dataset without raw pixels);
//   mask   bits one bit per pixel (little bit order: pixel p is bit p & 31 of word p >> 5), or
//          f32  verbatim (a mask with values other than 0 and 1).
// One launch turns B cache rows, picked by a device index list, into the (B, 1, H, W) fp32 image
// and mask batches the step consumes:
//   img = (float(v) - lo) / den   correctly rounded, uncontracted: the bits of the host's
//                                 (img - img.min()) / (img.max() - img.min() + 1e-8)
//   mask = bit ? 1.0f : 0.0f
// optionally under one of the 8 symmetries of the grid per sample (flip W, flip H, transpose).
//
// A block works on one sample. A u8 pixel has 256 possible values, so the block's 256 threads
// divide once each — lut[v] = (float(v) - lo) / den in LDS — and every pixel is a lookup: the
// same correctly rounded quotient without a division sequence per pixel (a launch this short is
// bound by what its waves issue as much as by its bytes: DESIGN.md). Each thread then produces a
// run of 4 consecutive output pixels: the writes are coalesced float4 when W % 4 == 0, and the
// flipped / transposed reads pay the gather. A row-flipped run is still one aligned 4-pixel read
// (W % 4 == 0), reversed in registers; only the transpose gathers per pixel.
#include "common.h"

namespace pis {

constexpr int CB_PIX = 1024;  // pixels per block: 256 threads x one run of 4

struct CacheArgs {
  const uint8_t* img;
  const uint8_t* mask;
  size_t img_stride, mask_stride;  // bytes between samples, multiples of 16
  const float* norm;               // [N][2] (lo, den), u8 images only
  const int64_t* idx;              // [B]
  const uint8_t* sym;              // [B] or NULL
  int64_t N;
  float* img_out;
  float* mask_out;
  int img_fmt, mask_fmt, H, W;
};

// source pixel offset of output pixel (y, x) under symmetry s: out = T(F_H(F_W(sample)))
__device__ __forceinline__ int cache_src(int y, int x, int s, int H, int W) {
  int r = (s & 4) ? x : y, c = (s & 4) ? y : x;
  if (s & 2) r = H - 1 - r;
  if (s & 1) c = W - 1 - c;
  return r * W + c;
}

__device__ __forceinline__ float cache_img_at(const uint8_t* row, int fmt, int q, const float* lut) {
  return fmt == PIS_CACHE_IMG_U8 ? lut[row[q]] : ((const float*)row)[q];
}

__device__ __forceinline__ float cache_mask_at(const uint8_t* row, int fmt, int q) {
  if (fmt == PIS_CACHE_MASK_BITS) return (((const uint32_t*)row)[q >> 5] >> (q & 31)) & 1u ? 1.f : 0.f;
  return ((const float*)row)[q];
}

// The sample of block row blockIdx.y: its rows, its symmetry code and (u8) its value table in
// lut[256]; ok = false when the index or the code is illegal (nothing of the cache is read then).
// Block-uniform; ends in a barrier when ok.
struct CacheSample {
  const uint8_t* img;
  const uint8_t* mask;
  int s;
  bool ok;
};
__device__ __forceinline__ CacheSample cache_sample(const CacheArgs& a, int b, float* lut) {
  CacheSample r{};
  const int64_t i = a.idx[b];
  r.s = a.sym ? a.sym[b] : 0;
  r.ok = i >= 0 && i < a.N && r.s < 8 && (!(r.s & 4) || a.H == a.W);
  if (!r.ok) return r;
  r.img = a.img + (size_t)i * a.img_stride;
  r.mask = a.mask + (size_t)i * a.mask_stride;
  if (a.img_fmt == PIS_CACHE_IMG_U8) {
    lut[threadIdx.x] = __fdiv_rn(__fsub_rn((float)threadIdx.x, a.norm[2 * i]), a.norm[2 * i + 1]);
    __syncthreads();
  }
  return r;
}

// W % 4 == 0: every run of 4 output pixels lies in one row, and both outputs are 16-B aligned.
// One run per thread: the launch is short (about 10 us at 8 x 512^2), and more, smaller threads
// measured faster than 2 or 4 runs per thread.
__global__ __launch_bounds__(256) void cache_batch_vec_kernel(CacheArgs a) {
  __shared__ float lut[256];
  const int b = blockIdx.y, H = a.H, W = a.W, npx = H * W;
  const CacheSample sm = cache_sample(a, b, lut);
  const int p = blockIdx.x * CB_PIX + threadIdx.x * 4;
  if (p >= npx) return;
  f32x4* __restrict__ io = (f32x4*)(a.img_out + (size_t)b * npx) + (p >> 2);
  f32x4* __restrict__ mo = (f32x4*)(a.mask_out + (size_t)b * npx) + (p >> 2);
  if (!sm.ok) {
    const float qn = __int_as_float(0x7fc00000);
    *io = *mo = f32x4{qn, qn, qn, qn};
    return;
  }
  const int s = sm.s;
  f32x4 vi, vm;
  if (!(s & 4)) {
    // one aligned 4-pixel read at q, reversed when the row is flipped; no symmetry: q = p
    const bool rev = s & 1;
    int q = p;
    if (s) {
      const int y = p / W, x = p - y * W;
      q = ((s & 2) ? H - 1 - y : y) * W + (rev ? W - 4 - x : x);
    }
    if (a.img_fmt == PIS_CACHE_IMG_U8) {
      uint32_t w = *(const uint32_t*)(sm.img + q);
      if (rev) w = __builtin_bswap32(w);
#pragma unroll
      for (int j = 0; j < 4; ++j) vi[j] = lut[(w >> (8 * j)) & 255u];
    } else {
      const f32x4 t = *(const f32x4*)(sm.img + (size_t)q * 4);
      vi = rev ? f32x4{t[3], t[2], t[1], t[0]} : t;
    }
    if (a.mask_fmt == PIS_CACHE_MASK_BITS) {
      const uint32_t nib = ((const uint32_t*)sm.mask)[q >> 5] >> (q & 31);  // q % 4 == 0: one word
#pragma unroll
      for (int j = 0; j < 4; ++j) vm[j] = (nib >> (rev ? 3 - j : j)) & 1u ? 1.f : 0.f;
    } else {
      const f32x4 t = *(const f32x4*)(sm.mask + (size_t)q * 4);
      vm = rev ? f32x4{t[3], t[2], t[1], t[0]} : t;
    }
  } else {
    const int y = p / W, x = p - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = cache_src(y, x + j, s, H, W);
      vi[j] = cache_img_at(sm.img, a.img_fmt, q, lut);
      vm[j] = cache_mask_at(sm.mask, a.mask_fmt, q);
    }
  }
  *io = vi;
  *mo = vm;
}

// any W: one pixel per thread and step, scalar coalesced stores
__global__ __launch_bounds__(256) void cache_batch_px_kernel(CacheArgs a) {
  __shared__ float lut[256];
  const int b = blockIdx.y, H = a.H, W = a.W, npx = H * W;
  const CacheSample sm = cache_sample(a, b, lut);
  float* __restrict__ io = a.img_out + (size_t)b * npx;
  float* __restrict__ mo = a.mask_out + (size_t)b * npx;
  const int p0 = blockIdx.x * CB_PIX + threadIdx.x;
#pragma unroll
  for (int g = 0; g < CB_PIX / 256; ++g) {
    const int p = p0 + g * 256;
    if (p >= npx) break;
    if (!sm.ok) {
      io[p] = mo[p] = __int_as_float(0x7fc00000);
      continue;
    }
    const int y = p / W, x = p - y * W;
    const int q = cache_src(y, x, sm.s, H, W);
    io[p] = cache_img_at(sm.img, a.img_fmt, q, lut);
    mo[p] = cache_mask_at(sm.mask, a.mask_fmt, q);
  }
}

}  // namespace pis

using namespace pis;

extern "C" int pis_cache_batch(const void* img, int img_fmt, size_t img_stride, const void* mask, int mask_fmt,
                               size_t mask_stride, const float* norm, const int64_t* idx, const uint8_t* sym,
                               int64_t N, float* img_out, float* mask_out, int B, int H, int W,
                               pis_stream_t stream) {
  PIS_CHECK_ARG(img && mask && idx && img_out && mask_out && N > 0 && B > 0 && H > 0 && W > 0,
                "pis_cache_batch: bad arguments");
  PIS_CHECK_ARG(B <= 65535 && (int64_t)H * W <= (1 << 30), "pis_cache_batch: B > 65535 or H * W > 2^30");
  PIS_CHECK_ARG(img_fmt == PIS_CACHE_IMG_U8 || img_fmt == PIS_CACHE_IMG_F32, "pis_cache_batch: unknown image format %d",
                img_fmt);
  PIS_CHECK_ARG(mask_fmt == PIS_CACHE_MASK_BITS || mask_fmt == PIS_CACHE_MASK_F32,
                "pis_cache_batch: unknown mask format %d", mask_fmt);
  PIS_CHECK_ARG(img_fmt != PIS_CACHE_IMG_U8 || norm, "pis_cache_batch: u8 images need the norm table");
  const size_t npx = (size_t)H * W;
  const size_t img_row = img_fmt == PIS_CACHE_IMG_U8 ? npx : npx * 4;
  const size_t mask_row = mask_fmt == PIS_CACHE_MASK_BITS ? (npx + 7) / 8 : npx * 4;
  PIS_CHECK_ARG(img_stride % 16 == 0 && mask_stride % 16 == 0 && img_stride >= img_row && mask_stride >= mask_row,
                "pis_cache_batch: a stride is no multiple of 16 bytes or shorter than a sample");
  PIS_CHECK_ARG(((uintptr_t)img | (uintptr_t)mask | (uintptr_t)img_out | (uintptr_t)mask_out) % 16 == 0,
                "pis_cache_batch: img, mask, img_out, mask_out must be 16-byte aligned");
  CacheArgs a{};
  a.img = (const uint8_t*)img; a.mask = (const uint8_t*)mask;
  a.img_stride = img_stride; a.mask_stride = mask_stride;
  a.norm = norm; a.idx = idx; a.sym = sym; a.N = N;
  a.img_out = img_out; a.mask_out = mask_out;
  a.img_fmt = img_fmt; a.mask_fmt = mask_fmt; a.H = H; a.W = W;
  const dim3 grid((unsigned)cdiv((int64_t)npx, CB_PIX), B);
  if (W % 4 == 0)
    hipLaunchKernelGGL(cache_batch_vec_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cache_batch_px_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("cache_batch");
}
