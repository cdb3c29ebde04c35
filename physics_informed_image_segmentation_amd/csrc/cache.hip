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

struct AffineRec;

struct CacheArgs {
  const uint8_t* img;
  const uint8_t* mask;
  size_t img_stride, mask_stride;  // bytes between samples, multiples of 16
  const float* norm;               // [N][2] (lo, den), u8 images only
  const int64_t* idx;              // [B]
  const uint8_t* sym;              // [B] or NULL
  const AffineRec* aff;            // [B], pis_cache_batch_affine only
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

// ---- random affine + tone augmentation (pis_cache_batch_affine) ---------------------------------
// The definition is include/pis_capi.h's and dataset.py:PackedSamples.warp's: source coordinates in
// 16.16 fixed point from six int32 coefficients, 8-bit bilinear fractions, reflection without a
// repeated edge pixel, nearest mask. All geometry is integer arithmetic and every float operation is
// rounded on its own (this file is built with contraction on), so the host restatement agrees on
// every pixel.
//
// A block owns a 32 x 32 tile of output pixels of one batch entry, a thread 4 consecutive pixels of
// one tile row: under rotation the tile's source footprint stays a compact patch of the sample
// (a linear run of 1024 pixels would spread it over whole rows), the gathers go through L1 / L2, and
// with W % 4 == 0 both outputs leave as coalesced float4 stores.
constexpr int AF_TILE = 32;

struct alignas(16) AffineRec {
  int32_t a[6];
  float gain, bias;
};
static_assert(sizeof(AffineRec) == 32, "pis_cache_batch_affine: 32-byte records");

// One correctly rounded multiply / add that no neighbour fuses with: the file is built with
// contraction on, under which __fmul_rn and __fadd_rn are plain operators and a product feeding a sum
// becomes one fma. The pragma takes the contract flag off these two operations.
__device__ __forceinline__ float af_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float af_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

// index i reflected into [0, n) about the edge pixels (period 2n - 2), any number of periods out.
// One fold covers [-(n - 1), 2n - 2]; only an index further out pays the modulo.
__device__ __forceinline__ int af_reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  if ((unsigned)(i + (n - 1)) > (unsigned)(3 * n - 3)) {
    i %= p;
    if (i < 0) i += p;
  }
  i = i < 0 ? -i : i;
  return i >= n ? p - i : i;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cache_batch_affine_kernel(CacheArgs a) {
  const int b = blockIdx.y, H = a.H, W = a.W, npx = H * W;
  const int tiles_x = (W + AF_TILE - 1) / AF_TILE;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y = ty * AF_TILE + (threadIdx.x >> 3), x = tx * AF_TILE + (threadIdx.x & 7) * 4;
  if (y >= H || x >= W) return;
  float* __restrict__ io = a.img_out + (size_t)b * npx + (size_t)y * W + x;
  float* __restrict__ mo = a.mask_out + (size_t)b * npx + (size_t)y * W + x;
  const int nrun = VEC ? 4 : min(4, W - x);  // VEC: W % 4 == 0, the run never crosses the row's end
  const float qn = __int_as_float(0x7fc00000);
  f32x4 vi{qn, qn, qn, qn}, vm{qn, qn, qn, qn};
  // block-uniform: the index, the record (one aligned 32-byte read) and (lo, den)
  const int64_t i = a.idx[b];
  if (i >= 0 && i < a.N) {
    const AffineRec r = a.aff[b];
    const uint8_t* __restrict__ img = a.img + (size_t)i * a.img_stride;
    const uint8_t* __restrict__ mask = a.mask + (size_t)i * a.mask_stride;
    const bool u8 = a.img_fmt == PIS_CACHE_IMG_U8;
    const float lo = u8 ? a.norm[2 * i] : 0.f, den = u8 ? a.norm[2 * i + 1] : 1.f;
    // 64-bit sums; |SX >> 16| < 2^29 for H, W <= 4096
    int64_t SX = (int64_t)r.a[0] * x + (int64_t)r.a[1] * y + r.a[2];
    int64_t SY = (int64_t)r.a[3] * x + (int64_t)r.a[4] * y + r.a[5];
#pragma unroll
    for (int j = 0; j < 4; ++j, SX += r.a[0], SY += r.a[3]) {
      if (!VEC && j >= nrun) break;
      const int x0 = (int)(SX >> 16), y0 = (int)(SY >> 16);
      const int fx = (int)(SX >> 8) & 255, fy = (int)(SY >> 8) & 255;
      const int c0 = af_reflect(x0, W), c1 = af_reflect(x0 + 1, W);
      const int r0 = af_reflect(y0, H) * W, r1 = af_reflect(y0 + 1, H) * W;
      float v;
      if (u8) {
        const uint32_t top = (256 - fx) * img[r0 + c0] + fx * img[r0 + c1];
        const uint32_t bot = (256 - fx) * img[r1 + c0] + fx * img[r1 + c1];
        const float t = af_mul((float)((256 - fy) * top + fy * bot), 0x1p-16f);  // < 2^24: exact
        v = __fdiv_rn(__fsub_rn(t, lo), den);
      } else {
        const float* f = (const float*)img;
        const float w00 = (float)((256 - fy) * (256 - fx)), w01 = (float)((256 - fy) * fx);
        const float w10 = (float)(fy * (256 - fx)), w11 = (float)(fy * fx);
        const float top = af_add(af_mul(w00, f[r0 + c0]), af_mul(w01, f[r0 + c1]));
        const float bot = af_add(af_mul(w10, f[r1 + c0]), af_mul(w11, f[r1 + c1]));
        v = af_mul(af_add(top, bot), 0x1p-16f);
      }
      vi[j] = af_add(af_mul(r.gain, v), r.bias);
      const int q = af_reflect((int)((SY + 32768) >> 16), H) * W + af_reflect((int)((SX + 32768) >> 16), W);
      vm[j] = cache_mask_at(mask, a.mask_fmt, q);
    }
  }
  if (VEC) {
    *(f32x4*)io = vi;
    *(f32x4*)mo = vm;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nrun) {
        io[j] = vi[j];
        mo[j] = vm[j];
      }
  }
}

}  // namespace pis

using namespace pis;

// the checks pis_cache_batch and pis_cache_batch_affine share, and the launch arguments
static int cache_args(const char* who, CacheArgs& a, const void* img, int img_fmt, size_t img_stride, const void* mask,
                      int mask_fmt, size_t mask_stride, const float* norm, const int64_t* idx, int64_t N,
                      float* img_out, float* mask_out, int B, int H, int W) {
  PIS_CHECK_ARG(img && mask && idx && img_out && mask_out && N > 0 && B > 0 && H > 0 && W > 0, "%s: bad arguments", who);
  PIS_CHECK_ARG(B <= 65535 && (int64_t)H * W <= (1 << 30), "%s: B > 65535 or H * W > 2^30", who);
  PIS_CHECK_ARG(img_fmt == PIS_CACHE_IMG_U8 || img_fmt == PIS_CACHE_IMG_F32, "%s: unknown image format %d", who, img_fmt);
  PIS_CHECK_ARG(mask_fmt == PIS_CACHE_MASK_BITS || mask_fmt == PIS_CACHE_MASK_F32, "%s: unknown mask format %d", who,
                mask_fmt);
  PIS_CHECK_ARG(img_fmt != PIS_CACHE_IMG_U8 || norm, "%s: u8 images need the norm table", who);
  const size_t npx = (size_t)H * W;
  const size_t img_row = img_fmt == PIS_CACHE_IMG_U8 ? npx : npx * 4;
  const size_t mask_row = mask_fmt == PIS_CACHE_MASK_BITS ? (npx + 7) / 8 : npx * 4;
  PIS_CHECK_ARG(img_stride % 16 == 0 && mask_stride % 16 == 0 && img_stride >= img_row && mask_stride >= mask_row,
                "%s: a stride is no multiple of 16 bytes or shorter than a sample", who);
  PIS_CHECK_ARG(((uintptr_t)img | (uintptr_t)mask | (uintptr_t)img_out | (uintptr_t)mask_out) % 16 == 0,
                "%s: img, mask, img_out, mask_out must be 16-byte aligned", who);
  a = CacheArgs{};
  a.img = (const uint8_t*)img; a.mask = (const uint8_t*)mask;
  a.img_stride = img_stride; a.mask_stride = mask_stride;
  a.norm = norm; a.idx = idx; a.N = N;
  a.img_out = img_out; a.mask_out = mask_out;
  a.img_fmt = img_fmt; a.mask_fmt = mask_fmt; a.H = H; a.W = W;
  return PIS_OK;
}

extern "C" int pis_cache_batch_affine(const void* img, int img_fmt, size_t img_stride, const void* mask, int mask_fmt,
                                      size_t mask_stride, const float* norm, const int64_t* idx, const void* params,
                                      int64_t N, float* img_out, float* mask_out, int B, int H, int W,
                                      pis_stream_t stream) {
  CacheArgs a;
  if (int rc = cache_args("pis_cache_batch_affine", a, img, img_fmt, img_stride, mask, mask_fmt, mask_stride, norm, idx,
                          N, img_out, mask_out, B, H, W))
    return rc;
  PIS_CHECK_ARG(params && (uintptr_t)params % 16 == 0,
                "pis_cache_batch_affine: params must be B records, 16-byte aligned");
  PIS_CHECK_ARG(H <= 4096 && W <= 4096, "pis_cache_batch_affine: H or W > 4096");
  a.aff = (const AffineRec*)params;
  const dim3 grid((unsigned)(cdiv(W, AF_TILE) * cdiv(H, AF_TILE)), B);
  if (W % 4 == 0)
    hipLaunchKernelGGL(cache_batch_affine_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cache_batch_affine_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("cache_batch_affine");
}

extern "C" int pis_cache_batch(const void* img, int img_fmt, size_t img_stride, const void* mask, int mask_fmt,
                               size_t mask_stride, const float* norm, const int64_t* idx, const uint8_t* sym,
                               int64_t N, float* img_out, float* mask_out, int B, int H, int W,
                               pis_stream_t stream) {
  CacheArgs a;
  if (int rc = cache_args("pis_cache_batch", a, img, img_fmt, img_stride, mask, mask_fmt, mask_stride, norm, idx, N,
                          img_out, mask_out, B, H, W))
    return rc;
  a.sym = sym;
  const dim3 grid((unsigned)cdiv((int64_t)H * W, CB_PIX), B);
  if (W % 4 == 0)
    hipLaunchKernelGGL(cache_batch_vec_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cache_batch_px_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("cache_batch");
}
