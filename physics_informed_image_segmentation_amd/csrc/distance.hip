// Exact squared Euclidean distance transform of a batch of binary images (pis_edt_sq) and the
// per-pixel surface distances between two boundary maps (pis_surface_distances), integer geometry,
// three launches whatever the data (evaluate.py: distance_transform_sq_np, surface_distances).
//
//   1. edt_colmask  the set flags of each (32-row segment, column) packed into 32 bits
//   2. edt_coldist  g[n][y][x] = vertical distance to the nearest set pixel of column x (uint16,
//                   0xFFFF = none), one thread per (segment, column), coalesced across x
//                   (both as bnd_colmask / bnd_coldist of boundary.hip, on uint8 sets)
//   3. edt_row      one wave per (image, row): the g row in LDS, clamped to GV_NONE, with the minimum
//                   of every 64 columns beside it. Lane l owns the pixels x = l + 64 k and computes
//                   d^2 = min_x' (x - x')^2 + g[x']^2 outwards from x: radii in blocks of 64, a block
//                   skipped when (its nearest radius)^2 + (the minimum of g over the segments it
//                   touches)^2 is no better than the best so far, a block searched 8 columns a side
//                   per step and left once radius^2 >= best; a step is skipped in the same way by
//                   the minima of the aligned 8-column groups it touches. The search ends once the
//                   next block's nearest radius alone is no better. One set pixel in a corner costs
//                   W / 64 block tests, 16 step tests and two steps per pixel, not W columns.
//                   pis_tune key PIS_TUNE_EDT_PRUNE switches the two prunings off (same integers).
//
// A row whose g is all none belongs to an image with an empty set: PIS_EDT_NONE, no flag needed.
// For the surface distances the 2B maps are the images (i < B: bnd_p[i], else bnd_t[i - B]); the row
// pass of image i reads the g of its opposite map and computes only where image i's own flag is set.
#include "common.h"

namespace pis {

constexpr int EDT_MAX = 4096;          // H, W limit (uint16 column distances)
constexpr unsigned EDT_G_NONE = 0xFFFFu;
constexpr int EDT_CSEG = 32;           // rows per segment of the column pass (one mask word)
// "none" in the LDS row: its square 2^30 is above every real distance (< 2^26), and
// 2^30 + 4096^2 still fits an int
constexpr int GV_NONE = 0x8000;
constexpr int D2_NONE = GV_NONE * GV_NONE;
constexpr int ESTEP = 8;               // columns per side and step of the search

struct EdtArgs {
  const uint8_t* set0;  // images [0, B0)
  const uint8_t* set1;  // images [B0, N)
  int N, B0, H, W, nseg;
  int surf;             // 0: the transform of image n everywhere; 1: surface distances (B0 = B, N = 2B)
  uint16_t* g;          // [N][H*W]
  unsigned* cmask;      // [N][nseg][W]
  int32_t* out0;        // images [0, B0)
  int32_t* out1;        // images [B0, N)
};

__device__ __forceinline__ const uint8_t* edt_src(const EdtArgs& a, int img, size_t npx) {
  return img < a.B0 ? a.set0 + (size_t)img * npx : a.set1 + (size_t)(img - a.B0) * npx;
}

__global__ __launch_bounds__(256) void edt_colmask_kernel(EdtArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), seg = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.W || seg >= a.nseg) return;
  const size_t npx = (size_t)a.H * a.W;
  const int y0 = seg * EDT_CSEG;
  for (int img = blockIdx.z; img < a.N; img += gridDim.z) {
    const uint8_t* __restrict__ b = edt_src(a, img, npx) + (size_t)y0 * a.W + x;
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < EDT_CSEG; ++r)
      if (y0 + r < a.H && b[(size_t)r * a.W]) m |= 1u << r;
    a.cmask[((size_t)img * a.nseg + seg) * a.W + x] = m;
  }
}

// the nearest set row above and below the segment from the other segments' masks, then the 32
// distances of the segment from its own mask, in registers
__global__ __launch_bounds__(256) void edt_coldist_kernel(EdtArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), seg = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.W || seg >= a.nseg) return;
  const size_t npx = (size_t)a.H * a.W;
  const int y0 = seg * EDT_CSEG;
  for (int img = blockIdx.z; img < a.N; img += gridDim.z) {
    const unsigned* __restrict__ cm = a.cmask + (size_t)img * a.nseg * a.W + x;
    uint16_t* __restrict__ g = a.g + (size_t)img * npx + (size_t)y0 * a.W + x;
    const unsigned m = cm[(size_t)seg * a.W];
    int above = -1, below = -1;  // rows of the nearest set pixels outside the segment
    for (int s = seg - 1; s >= 0; --s) {
      const unsigned o = cm[(size_t)s * a.W];
      if (o) {
        above = s * EDT_CSEG + 31 - __clz(o);
        break;
      }
    }
    for (int s = seg + 1; s < a.nseg; ++s) {
      const unsigned o = cm[(size_t)s * a.W];
      if (o) {
        below = s * EDT_CSEG + __ffs(o) - 1;
        break;
      }
    }
#pragma unroll
    for (int r = 0; r < EDT_CSEG; ++r) {
      if (y0 + r >= a.H) break;
      const unsigned lo = m & (0xFFFFFFFFu >> (31 - r)), hi = m >> r;  // flags of rows <= r, >= r
      const unsigned up = lo ? (unsigned)(r - (31 - __clz(lo))) : above >= 0 ? (unsigned)(y0 + r - above) : EDT_G_NONE;
      const unsigned dn = hi ? (unsigned)(__ffs(hi) - 1) : below >= 0 ? (unsigned)(below - y0 - r) : EDT_G_NONE;
      g[(size_t)r * a.W] = (uint16_t)min(up, dn);
    }
  }
}

// squared distance from column x to the set whose clamped column distances of this row are
// g[0..W), smin[s] = min g[64 s .. 64 s + 63], s8[j] = min g[8 j .. 8 j + 7]; D2_NONE or more when
// the row has none. PRUNE bit 0: skip blocks by smin, bit 1: skip steps by s8.
template <int PRUNE>
__device__ __forceinline__ int edt_nearest2(const uint16_t* g, const uint16_t* smin, const uint16_t* s8, int x,
                                            int W) {
  const int g0 = g[x];
  int best = g0 * g0;
  const int reach = max(x, W - 1 - x);
  for (int r0 = 0; r0 < reach && (r0 + 1) * (r0 + 1) < best; r0 += 64) {
    if (PRUNE & 1) {
      // the block of radii r0 + 1 .. r0 + 64: columns l0 .. l1 on the left, r1 .. r2 on the right
      // (the parts inside the row), each within two segments
      const int l1 = x - r0 - 1, l0 = max(l1 - 63, 0), r1 = x + r0 + 1, r2 = min(r1 + 63, W - 1);
      int m = GV_NONE;
      if (l1 >= 0) m = min((int)smin[l0 >> 6], (int)smin[l1 >> 6]);
      if (r1 < W) m = min(m, min((int)smin[r1 >> 6], (int)smin[r2 >> 6]));
      if ((r0 + 1) * (r0 + 1) + m * m >= best) continue;
    }
    // (a step may run up to ESTEP - 1 radii past the block or the reach: those columns are
    // bounds-checked and are candidates like any other)
    const int rend = min(r0 + 64, reach);
    for (int d0 = r0 + 1; d0 <= rend && d0 * d0 < best; d0 += ESTEP) {
      if (PRUNE & 2) {
        // the step's columns x - d0 - 7 .. x - d0 and x + d0 .. x + d0 + 7 lie in two aligned groups
        // a side; an index clamped into the row names a group that can only lower the bound
        const int m = min(min((int)s8[max(x - d0 - 7, 0) >> 3], (int)s8[max(x - d0, 0) >> 3]),
                          min((int)s8[min(x + d0, W - 1) >> 3], (int)s8[min(x + d0 + 7, W - 1) >> 3]));
        if (d0 * d0 + m * m >= best) continue;
      }
#pragma unroll
      for (int k = 0; k < ESTEP; ++k) {
        const int dx = d0 + k, xl = x - dx, xr = x + dx;
        int vl = g[max(xl, 0)], vr = g[min(xr, W - 1)];
        vl = xl >= 0 ? vl : GV_NONE;
        vr = xr < W ? vr : GV_NONE;
        const int v = min(vl, vr);
        best = min(best, v * v + dx * dx);
      }
    }
  }
  return best;
}

// LDS of edt_row in uint16: the g row, the 8-column minima, the 64-column minima, each 16-byte aligned
__host__ __device__ inline int edt_lds_s8(int W) { return (W + 7) & ~7; }
__host__ __device__ inline int edt_lds_smin(int W) { return edt_lds_s8(W) + ((((W + 7) >> 3) + 7) & ~7); }

template <int PRUNE>
__global__ __launch_bounds__(64) void edt_row_kernel(EdtArgs a) {
  extern __shared__ uint16_t edt_lds[];
  uint16_t* grow = edt_lds;
  uint16_t* s8 = edt_lds + edt_lds_s8(a.W);
  uint16_t* smin = edt_lds + edt_lds_smin(a.W);
  const size_t npx = (size_t)a.H * a.W;
  const int y = blockIdx.x, lane = threadIdx.x;
  const int nsx = (a.W + 63) >> 6;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    // the image whose transform is read: itself, or the opposite boundary map of the same sample
    const int src = !a.surf ? img : img < a.B0 ? img + a.B0 : img - a.B0;
    const uint16_t* __restrict__ gsrc = a.g + (size_t)src * npx + (size_t)y * a.W;
    const uint8_t* __restrict__ flag = a.surf ? edt_src(a, img, npx) + (size_t)y * a.W : nullptr;
    int32_t* __restrict__ out =
        (img < a.B0 ? a.out0 + (size_t)img * npx : a.out1 + (size_t)(img - a.B0) * npx) + (size_t)y * a.W;
    int rowmin = GV_NONE;  // uniform
    for (int k = 0; k < nsx; ++k) {
      const int x = 64 * k + lane;
      int v = GV_NONE;
      if (x < a.W) {
        v = min((int)gsrc[x], GV_NONE);
        grow[x] = (uint16_t)v;
      }
      // the minimum of each aligned group of 8 lanes, then of the wave (lanes past W hold none)
      int m = v;
      m = min(m, __shfl_xor(m, 1, 64));
      m = min(m, __shfl_xor(m, 2, 64));
      m = min(m, __shfl_xor(m, 4, 64));
      if ((lane & 7) == 0 && x < a.W) s8[x >> 3] = (uint16_t)m;
      m = min(m, __shfl_xor(m, 8, 64));
      m = min(m, __shfl_xor(m, 16, 64));
      m = min(m, __shfl_xor(m, 32, 64));
      if (lane == 0) smin[k] = (uint16_t)m;
      rowmin = min(rowmin, m);
    }
    __syncthreads();
    for (int k = 0; k < nsx; ++k) {
      const int x = 64 * k + lane;
      if (x >= a.W) break;
      int d2 = -1;
      if (!flag || flag[x]) {
        d2 = rowmin < GV_NONE ? edt_nearest2<PRUNE>(grow, smin, s8, x, a.W) : D2_NONE;
        if (d2 >= D2_NONE) d2 = PIS_EDT_NONE;
      }
      out[x] = d2;
    }
    __syncthreads();  // the row buffers are restaged for the next image
  }
}

static size_t edt_align256(size_t n) { return (n + 255) & ~(size_t)255; }

static size_t edt_ws_bytes(int64_t N, int H, int W) {
  return edt_align256((size_t)N * H * W * 2) + edt_align256((size_t)N * cdiv(H, EDT_CSEG) * W * 4);
}

static int edt_launch(EdtArgs a, void* ws, hipStream_t s) {
  a.nseg = (int)cdiv(a.H, EDT_CSEG);
  a.g = (uint16_t*)ws;
  a.cmask = (unsigned*)((char*)ws + edt_align256((size_t)a.N * a.H * a.W * 2));
  const unsigned gn = (unsigned)std::min(a.N, 65535);
  const double px = (double)a.N * a.H * a.W;
  int rc;
#define PIS_EDT(NAME, KERNEL, GRID, BLOCK, SMEM)            \
  launch_hook(NAME, 0, s, px);                              \
  hipLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), SMEM, s, a); \
  launch_hook(NAME, 1, s, px);                              \
  rc = launch_status(NAME);                                 \
  if (rc) return rc;
  const dim3 gcol((unsigned)cdiv(a.W, 64), (unsigned)cdiv(a.nseg, 4), gn);
  PIS_EDT("edt_colmask", edt_colmask_kernel, gcol, 256, 0)
  PIS_EDT("edt_coldist", edt_coldist_kernel, gcol, 256, 0)
  const size_t smem = (size_t)2 * (edt_lds_smin(a.W) + cdiv(a.W, 64));
  const dim3 grow(a.H, gn);
  switch (tune_get(PIS_TUNE_EDT_PRUNE)) {
    case 0: PIS_EDT("edt_row", edt_row_kernel<0>, grow, 64, smem) break;
    case 1: PIS_EDT("edt_row", edt_row_kernel<1>, grow, 64, smem) break;
    default: PIS_EDT("edt_row", edt_row_kernel<3>, grow, 64, smem) break;
  }
#undef PIS_EDT
  return PIS_OK;
}

static bool edt_overlap(const void* p, size_t n, const void* q, size_t m) {
  return (const char*)p < (const char*)q + m && (const char*)q < (const char*)p + n;
}

}  // namespace pis

using namespace pis;

extern "C" size_t pis_edt_ws(int N, int H, int W) {
  if (N <= 0 || N > (1 << 25) || H <= 0 || W <= 0 || H > EDT_MAX || W > EDT_MAX) return 0;
  return edt_ws_bytes(N, H, W);
}

extern "C" size_t pis_surface_distances_ws(int B, int H, int W) {
  if (B <= 0 || B > (1 << 24)) return 0;
  return pis_edt_ws(2 * B, H, W);
}

extern "C" int pis_edt_sq(const uint8_t* set, int N, int H, int W, int32_t* d2, void* ws, size_t ws_bytes,
                          pis_stream_t stream) {
  PIS_CHECK_ARG(set && d2, "pis_edt_sq: set or d2 is NULL");
  PIS_CHECK_ARG(N >= 1 && N <= (1 << 25) && H >= 1 && W >= 1 && H <= EDT_MAX && W <= EDT_MAX,
                "pis_edt_sq: bad shape N=%d H=%d W=%d (1 <= N <= 2^25, 1 <= H, W <= %d)", N, H, W, EDT_MAX);
  PIS_CHECK_ARG(ws != nullptr, "pis_edt_sq: ws is NULL");
  const size_t need = pis_edt_ws(N, H, W);
  if (ws_bytes < need) {
    set_error("pis_edt_sq: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    return PIS_ERR_WORKSPACE;
  }
  PIS_CHECK_ARG(!edt_overlap(d2, (size_t)N * H * W * 4, ws, need), "pis_edt_sq: d2 overlaps ws");
  EdtArgs a{};
  a.set0 = set; a.set1 = set; a.N = N; a.B0 = N; a.H = H; a.W = W; a.surf = 0;
  a.out0 = d2; a.out1 = d2;
  return edt_launch(a, ws, (hipStream_t)stream);
}

extern "C" int pis_surface_distances(const uint8_t* bnd_p, const uint8_t* bnd_t, int B, int H, int W,
                                     int32_t* d2_pt, int32_t* d2_tp, void* ws, size_t ws_bytes,
                                     pis_stream_t stream) {
  PIS_CHECK_ARG(bnd_p && bnd_t && d2_pt && d2_tp, "pis_surface_distances: bnd_p, bnd_t, d2_pt or d2_tp is NULL");
  PIS_CHECK_ARG(B >= 1 && B <= (1 << 24) && H >= 1 && W >= 1 && H <= EDT_MAX && W <= EDT_MAX,
                "pis_surface_distances: bad shape B=%d H=%d W=%d (1 <= B <= 2^24, 1 <= H, W <= %d)", B, H, W,
                EDT_MAX);
  PIS_CHECK_ARG(ws != nullptr, "pis_surface_distances: ws is NULL");
  const size_t need = pis_surface_distances_ws(B, H, W);
  if (ws_bytes < need) {
    set_error("pis_surface_distances: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    return PIS_ERR_WORKSPACE;
  }
  const size_t nb = (size_t)B * H * W * 4;
  PIS_CHECK_ARG(!edt_overlap(d2_pt, nb, ws, need) && !edt_overlap(d2_tp, nb, ws, need) &&
                    !edt_overlap(d2_pt, nb, d2_tp, nb),
                "pis_surface_distances: d2_pt, d2_tp and ws overlap");
  EdtArgs a{};
  a.set0 = bnd_p; a.set1 = bnd_t; a.N = 2 * B; a.B0 = B; a.H = H; a.W = W; a.surf = 1;
  a.out0 = d2_pt; a.out1 = d2_tp;
  return edt_launch(a, ws, (hipStream_t)stream);
}
