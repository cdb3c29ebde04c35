// Whole-image inference: the data movement around the forwards (predict.py:Predictor).
//
// An image of any size is cut into overlapping th x tw tiles, reflected past its edges, each tile
// presented under a set of the 8 symmetries of the grid (the codes of pis_cache_batch: bit 0 flips
// W, bit 1 flips H, then bit 2 transposes); the tile probabilities the network returns are blended
// back into one map. Two launches:
//   pis_tile_gather   sources -> (n_jobs, 1, th, tw) network inputs of a chunk of jobs
//   pis_tile_blend    (J, 1, th, tw) tile outputs -> (S, H, W) probabilities and the 0 / 1 mask
// The tiling is a pure function of by-value arguments (include/pis_capi.h): the host validates every
// call in full, no job list lives in device memory, and predict.py:gather_tiles_np / blend_tiles_np
// restate both kernels in float32 numpy bit for bit.
//
// Both kernels: a thread owns 4 consecutive output pixels of one row and stores them as one float4
// (and, in the blend, four packed mask bytes); stores are coalesced along the output row, the reads
// pay the reflection, the flips and (codes >= 4) the transpose's stride. The blend is in gather
// form: one thread computes a pixel from every tile that covers it, found from the closed-form
// origins; no atomics, so the sum's order is fixed. Its blocks own 32 x 32 patches of the image, so
// that the strided reads of a transposing code use their cache lines in full inside one block; no
// LDS staging (profiles/predict.txt: with all eight symmetries 3.2 x / 2.1 x faster than blocks of
// 1024 consecutive pixels at 8 x 512^2 / 2048^2, the same without symmetries).
#include "common.h"

namespace pis {

// tile k of an axis of length n starts here: stride t - o, the last tile pulled back to end at the
// image's edge; a single tile on an axis shorter than t starts at 0
__host__ __device__ __forceinline__ int tile_origin(int k, int n, int t, int o) {
  const int a = k * (t - o), b = n > t ? n - t : 0;
  return a < b ? a : b;
}

static int tile_axis_count(int n, int t, int o) { return n <= t ? 1 : (int)cdiv(n - o, t - o); }

struct TileGeom {
  int S, H, W, th, tw, ov, Ky, Kx, Ns;
  uint32_t codes;  // code of symmetry qi in bits 4 qi .. 4 qi + 3, ascending
};

// index i reflected into [0, n) about the edge pixels (period 2n - 2), any number of periods out:
// the header's reflect(i, n)
__device__ __forceinline__ int tile_reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  if ((unsigned)(i + (n - 1)) > (unsigned)(3 * n - 3)) {
    i %= p;
    if (i < 0) i += p;
  }
  i = i < 0 ? -i : i;
  return i >= n ? p - i : i;
}

// One correctly rounded multiply / add that no neighbour fuses with (this file is built with
// contraction on: see cache.hip)
__device__ __forceinline__ float tb_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float tb_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

// ---- gather -------------------------------------------------------------------------------------
struct GatherArgs {
  const uint8_t* src;
  size_t stride;  // bytes between sources
  const float* norm;
  float* out;
  int64_t first_job;
  int fmt, bpj;  // blocks per job
  TileGeom g;
};

// A block works on one job, so on one source: its 256 threads divide once each for the u8 value
// table (as cache_batch_vec_kernel), and every pixel is a lookup.
__global__ __launch_bounds__(256) void tile_gather_kernel(GatherArgs a) {
  __shared__ float lut[256];
  const TileGeom& g = a.g;
  const int64_t jl = blockIdx.x / a.bpj;
  const int blk = (int)(blockIdx.x - jl * a.bpj);
  int64_t t = a.first_job + jl;
  const int qi = (int)(t % g.Ns);
  t /= g.Ns;
  const int kx = (int)(t % g.Kx);
  t /= g.Kx;
  const int ky = (int)(t % g.Ky), s = (int)(t / g.Ky);
  const int q = (g.codes >> (4 * qi)) & 15;
  const uint8_t* __restrict__ img = a.src + (size_t)s * a.stride;
  const bool u8 = a.fmt == PIS_CACHE_IMG_U8;
  if (u8) {
    lut[threadIdx.x] = __fdiv_rn(__fsub_rn((float)threadIdx.x, a.norm[2 * s]), a.norm[2 * s + 1]);
    __syncthreads();
  }
  const int th = g.th, tw = g.tw;
  const int p = (blk * 256 + (int)threadIdx.x) * 4;
  if (p >= th * tw) return;
  const int oy = p / tw, ox = p - oy * tw;  // tw % 4 == 0: the run stays in one row
  const int y0 = tile_origin(ky, g.H, th, g.ov), x0 = tile_origin(kx, g.W, tw, g.ov);
  f32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // out = T(F_H(F_W(tile))): output (oy, ox + i) reads the tile at (r, c)
    int r = (q & 4) ? ox + i : oy, c = (q & 4) ? oy : ox + i;
    if (q & 2) r = th - 1 - r;
    if (q & 1) c = tw - 1 - c;
    const int64_t at = (int64_t)tile_reflect(y0 + r, g.H) * g.W + tile_reflect(x0 + c, g.W);
    v[i] = u8 ? lut[img[at]] : ((const float*)img)[at];
  }
  *(f32x4*)(a.out + jl * ((int64_t)th * tw) + p) = v;
}

// ---- blend --------------------------------------------------------------------------------------
constexpr int BL_TILE = 32;  // 256 threads x one run of 4

struct BlendArgs {
  const float* u;
  float* prob;
  uint8_t* mask;
  float thr;
  int nbx, nby;  // patches per image row and column
  TileGeom g;
};

// the tiles of one axis that cover coordinate y, ascending: tile index, offset inside the tile and
// the integer ramp weight w1(l, t, o) = min(l + 1, t - l, o), 1 for o == 0. With o <= t / 2 two
// unclamped tiles at most cover a coordinate, and the pulled-back last tile makes three.
struct Cover {
  int n;
  int k[3], l[3], w[3];
};
__device__ __forceinline__ Cover tile_cover(int y, int n, int t, int o, int K) {
  Cover c;
  c.n = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) c.k[i] = c.l[i] = c.w[i] = 0;
  const int st = t - o;
  const int k0 = y >= t ? (y - t) / st + 1 : 0;  // the smallest k with k (t - o) + t > y
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // k0, k0 + 1 and the last tile at most: the 4th step only ends the scan
    const int k = k0 + i;
    if (k >= K) break;
    const int org = tile_origin(k, n, t, o);
    if (org > y) break;
    const int l = y - org;
    if (l >= t || c.n >= 3) continue;
    const int up = l + 1, dn = t - l;
    const int w = o ? min(min(up, dn), o) : 1;
#pragma unroll
    for (int m = 0; m < 3; ++m)
      if (m == c.n) {
        c.k[m] = k;
        c.l[m] = l;
        c.w[m] = w;
      }
    ++c.n;
  }
  return c;
}

template <bool VEC>
__global__ __launch_bounds__(256) void tile_blend_kernel(BlendArgs a) {
  const TileGeom& g = a.g;
  const int H = g.H, W = g.W, th = g.th, tw = g.tw, Ns = g.Ns;
  // a block owns a BL_TILE x BL_TILE patch of one image, a thread 4 consecutive pixels of one patch
  // row: under a transposing code the patch reads a BL_TILE x BL_TILE patch of the tile output, whose
  // cache lines the block uses in full (a linear run of 1024 pixels would touch one element per line)
  const int bx = blockIdx.x % a.nbx, by = (blockIdx.x / a.nbx) % a.nby, s = blockIdx.x / (a.nbx * a.nby);
  const int y = by * BL_TILE + (int)(threadIdx.x >> 3), x = bx * BL_TILE + (int)(threadIdx.x & 7) * 4;
  if (y >= H || x >= W) return;
  const int64_t row = (int64_t)s * H + y;
  const int nrun = VEC ? 4 : min(4, W - x);
  const int64_t tt = (int64_t)th * tw;
  const Cover cy = tile_cover(y, H, th, g.ov, g.Ky);
  f32x4 pr{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!VEC && i >= nrun) break;
    const Cover cx = tile_cover(x + i, W, tw, g.ov, g.Kx);
    float acc = 0.f;
    int wsum = 0;
#pragma unroll
    for (int iy = 0; iy < 3; ++iy) {
      if (iy >= cy.n) break;
#pragma unroll
      for (int ix = 0; ix < 3; ++ix) {
        if (ix >= cx.n) break;
        const int w = cy.w[iy] * cx.w[ix];
        const float wf = (float)w;
        const float* __restrict__ uj = a.u + (((int64_t)s * g.Ky + cy.k[iy]) * g.Kx + cx.k[ix]) * Ns * tt;
        const int ly = cy.l[iy], lx = cx.l[ix];
        for (int qi = 0; qi < Ns; ++qi, uj += tt) {
          const int q = (g.codes >> (4 * qi)) & 15;
          // where apply_symmetry sends tile element (ly, lx): the inverse of the gather
          const int r = (q & 2) ? th - 1 - ly : ly, c = (q & 1) ? tw - 1 - lx : lx;
          const int at = (q & 4) ? c * tw + r : r * tw + c;  // th == tw under a transpose
          acc = tb_add(acc, tb_mul(wf, uj[at]));
          wsum += w;
        }
      }
    }
    pr[i] = __fdiv_rn(acc, (float)wsum);
  }
  const int64_t at = row * W + x;
  if (VEC) {
    *(f32x4*)(a.prob + at) = pr;
    if (a.mask) {
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) m |= (pr[i] > a.thr ? 1u : 0u) << (8 * i);
      *(uint32_t*)(a.mask + at) = m;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nrun) {
        a.prob[at + i] = pr[i];
        if (a.mask) a.mask[at + i] = pr[i] > a.thr ? 1 : 0;
      }
  }
}

}  // namespace pis

using namespace pis;

// the checks the three entry points share, and the geometry
static int tile_geom(const char* who, TileGeom& g, int S, int H, int W, int th, int tw, int ov, int sym_mask) {
  PIS_CHECK_ARG(th >= 16 && th <= 2048 && th % 16 == 0 && tw >= 16 && tw <= 2048 && tw % 16 == 0,
                "%s: tile %d x %d: multiples of 16 in [16, 2048] are needed", who, th, tw);
  PIS_CHECK_ARG(ov >= 0 && ov <= std::min(th, tw) / 2 && ov <= 256,
                "%s: overlap %d: 0 <= overlap <= min(th, tw) / 2 and <= 256 is needed", who, ov);
  PIS_CHECK_ARG(H >= 1 && H <= 32768 && W >= 1 && W <= 32768, "%s: H = %d, W = %d: [1, 32768] is needed", who, H, W);
  PIS_CHECK_ARG(S >= 1, "%s: S = %d sources", who, S);
  PIS_CHECK_ARG(sym_mask >= 1 && sym_mask <= 255, "%s: sym_mask 0x%x: a non-empty set of the codes 0..7 is needed", who,
                sym_mask);
  PIS_CHECK_ARG(!(sym_mask & 0xF0) || th == tw, "%s: a symmetry code >= 4 transposes: th == tw is needed (%d x %d)", who,
                th, tw);
  g = TileGeom{};
  g.S = S; g.H = H; g.W = W; g.th = th; g.tw = tw; g.ov = ov;
  g.Ky = tile_axis_count(H, th, ov);
  g.Kx = tile_axis_count(W, tw, ov);
  for (int q = 0; q < 8; ++q)
    if (sym_mask >> q & 1) g.codes |= (uint32_t)q << (4 * g.Ns++);
  return PIS_OK;
}

extern "C" int pis_tile_count(int H, int W, int th, int tw, int ov, int* Ky, int* Kx) {
  TileGeom g;
  if (int rc = tile_geom("pis_tile_count", g, 1, H, W, th, tw, ov, 1)) return rc;
  PIS_CHECK_ARG(Ky && Kx, "pis_tile_count: Ky or Kx is NULL");
  *Ky = g.Ky;
  *Kx = g.Kx;
  return PIS_OK;
}

extern "C" int pis_tile_gather(const void* src, int src_fmt, size_t src_stride, const float* norm, int S, int H, int W,
                               int th, int tw, int ov, int sym_mask, int64_t first_job, int64_t n_jobs, float* out,
                               pis_stream_t stream) {
  GatherArgs a{};
  if (int rc = tile_geom("pis_tile_gather", a.g, S, H, W, th, tw, ov, sym_mask)) return rc;
  PIS_CHECK_ARG(src && out, "pis_tile_gather: src or out is NULL");
  PIS_CHECK_ARG(src_fmt == PIS_CACHE_IMG_U8 || src_fmt == PIS_CACHE_IMG_F32, "pis_tile_gather: unknown image format %d",
                src_fmt);
  PIS_CHECK_ARG(src_fmt != PIS_CACHE_IMG_U8 || norm, "pis_tile_gather: u8 images need the norm table");
  const size_t row = (size_t)H * W * (src_fmt == PIS_CACHE_IMG_U8 ? 1 : 4);
  PIS_CHECK_ARG(src_stride % 16 == 0 && src_stride >= row,
                "pis_tile_gather: the stride is no multiple of 16 bytes or shorter than a source");
  PIS_CHECK_ARG(((uintptr_t)src | (uintptr_t)out) % 16 == 0, "pis_tile_gather: src and out must be 16-byte aligned");
  const int64_t J = (int64_t)S * a.g.Ky * a.g.Kx * a.g.Ns;
  PIS_CHECK_ARG(first_job >= 0 && n_jobs >= 1 && first_job <= J - n_jobs,
                "pis_tile_gather: %lld jobs from job %lld on are not within [0, %lld)", (long long)n_jobs,
                (long long)first_job, (long long)J);
  a.bpj = (int)cdiv(th * tw / 4, 256);
  PIS_CHECK_ARG(n_jobs * a.bpj <= 0x7fffffffLL, "pis_tile_gather: %lld jobs are too many for one launch",
                (long long)n_jobs);
  a.src = (const uint8_t*)src; a.stride = src_stride; a.norm = norm; a.out = out;
  a.first_job = first_job; a.fmt = src_fmt;
  hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)(n_jobs * a.bpj)), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("tile_gather");
}

extern "C" int pis_tile_blend(const float* u, int S, int H, int W, int th, int tw, int ov, int sym_mask, float thr,
                              float* prob, uint8_t* mask, pis_stream_t stream) {
  BlendArgs a{};
  if (int rc = tile_geom("pis_tile_blend", a.g, S, H, W, th, tw, ov, sym_mask)) return rc;
  PIS_CHECK_ARG(u && prob, "pis_tile_blend: u or prob is NULL");
  PIS_CHECK_ARG(((uintptr_t)u | (uintptr_t)prob) % 16 == 0 && (uintptr_t)mask % 4 == 0,
                "pis_tile_blend: u and prob must be 16-byte aligned, mask 4-byte aligned");
  a.nbx = (int)cdiv(W, BL_TILE);
  a.nby = (int)cdiv(H, BL_TILE);
  const int64_t blocks = (int64_t)S * a.nbx * a.nby;
  PIS_CHECK_ARG(blocks <= 0x7fffffffLL, "pis_tile_blend: S * H * W is too large for one launch");
  a.u = u; a.prob = prob; a.mask = mask; a.thr = thr;
  if (W % 4 == 0)
    hipLaunchKernelGGL(tile_blend_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(tile_blend_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("tile_blend");
}
