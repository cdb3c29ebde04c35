// Boundary F1 and Hausdorff counters of a batch on the device (evaluate.py: extract_boundaries,
// _boundary_f1_np, compute_hausdorff_distance), exact integer geometry, fixed launch count.
//
// All 2B images (B predictions thresholded at p > thr, B targets at t > 0) go through one set of
// launches; image i < B is prediction i, image B + i is target i.
//
//   1. bnd_init     counts = {0, 0, 0, 0, -1, -1}
//   2. bnd_label    per 32x32 tile: union-find over the tile's background pixels in LDS (parent =
//                   up neighbour, else left neighbour; compress; union(left, self) where both
//                   neighbours are background; compress), written to the global label array as
//                   "tile root pixel + 1". Foreground is -1, the value 0 is the virtual frame.
//   3. bnd_merge    unions across tile edges and with the frame (image border pixels) by atomic-min
//                   on the global labels: a parent is always smaller than its child, so 0 (the
//                   frame) ends as the root of exactly the outer background.
//   4. bnd_flatten  label = root
//   5. bnd_extract  boundary = foreground with a 4-neighbour that is out of the image or labelled 0;
//                   writes the uint8 maps, counts n_p / n_t
//   6. bnd_colmask  the boundary flags of each (32-row segment, column) packed into 32 bits
//   7. bnd_coldist  g[y][x] = vertical distance to the nearest boundary pixel of column x (uint16,
//                   0xFFFF = none), one thread per (segment, column), coalesced across x
//   8. bnd_query    one wave per (sample, row): for each pixel of Bp the exact squared distance to Bt,
//                   d^2 = min_x' (x - x')^2 + g_Bt[y][x']^2, with the g rows and the columns of the
//                   row's boundary pixels in LDS, one lane per pixel, searched outwards from x eight
//                   columns a side per step and stopped once (x - x')^2 >= best. The same for Bt
//                   against Bp.
//                   Per row: m_* = #[d^2 <= tol^2], h2_* = max d^2
//   9. bnd_reduce   the rows' partials summed / maximised per sample (integers: order-independent)
//
// Union-find under concurrency: links only ever move to a smaller label of the same component, so
// a stale or racing read still names a member of the component and every loop ends at the atomic
// that decides; the result is the set of components, independent of ordering.
#include "common.h"

namespace pis {

constexpr int BT = 32;               // label tile edge
constexpr int BND_MAX = 4096;        // H, W limit (uint16 distances, H^2 + W^2 < 2^31)
constexpr unsigned G_NONE = 0xFFFFu;  // no boundary pixel in this column
constexpr int CSEG = 32;             // rows per segment of the column pass (one mask word)
constexpr int EXT_PER = 8;           // pixels per thread in bnd_extract (fewer counter atomics)

struct BndArgs {
  const float* p;
  const float* t;
  int B, H, W, N;  // N = 2B images
  int tiles_x, tiles_y, nseg;
  float thr;
  int tol2;
  int* counts;       // [B][6]
  int* label;        // [N][H*W]
  uint8_t* bnd;      // [N][H*W]
  uint16_t* g;       // [N][H*W]
  unsigned* cmask;   // [N][nseg][W]
  int* part;         // [B][H][4] per-row (m_p, m_t, h2_pt, h2_tp)
  uint8_t* out_p;    // [B][H*W] or NULL
  uint8_t* out_t;    // [B][H*W] or NULL
};

__global__ __launch_bounds__(256) void bnd_init_kernel(BndArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.B * 6) a.counts[i] = (i % 6) < 4 ? 0 : -1;
}

__device__ __forceinline__ int lds_find(volatile int* lab, int i) {
  for (;;) {
    const int n = lab[i];
    if (n == i) return i;
    i = n;
  }
}

__global__ __launch_bounds__(256) void bnd_label_kernel(BndArgs a) {
  __shared__ int lab[BT * BT];
  __shared__ uint8_t bg[BT * BT];
  const int x0 = (blockIdx.x % a.tiles_x) * BT, y0 = (blockIdx.x / a.tiles_x) * BT;
  const size_t npx = (size_t)a.H * a.W;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    const float* src = img < a.B ? a.p + (size_t)img * npx : a.t + (size_t)(img - a.B) * npx;
    const float thr = img < a.B ? a.thr : 0.f;
    int* L = a.label + (size_t)img * npx;
    for (int i = threadIdx.x; i < BT * BT; i += 256) {
      const int y = y0 + (i >> 5), x = x0 + (i & 31);
      // strict '>' : NaN is background; slots past the image edge are not background (the frame
      // is joined through the image border pixels in bnd_merge)
      bg[i] = (y < a.H && x < a.W) ? !(src[(size_t)y * a.W + x] > thr) : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BT * BT; i += 256) {
      const bool up = (i >> 5) > 0 && bg[i - BT], left = (i & 31) > 0 && bg[i - 1];
      lab[i] = up ? i - BT : left ? i - 1 : i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BT * BT; i += 256)
      if (bg[i]) {
        const int r = lds_find(lab, i);
        lab[i] = r;
      }
    __syncthreads();
    for (int i = threadIdx.x; i < BT * BT; i += 256) {
      if (!(bg[i] && (i >> 5) > 0 && bg[i - BT] && (i & 31) > 0 && bg[i - 1])) continue;
      int u = lds_find(lab, i), v = lds_find(lab, i - 1);
      while (u != v) {
        if (u < v) {
          const int s = u;
          u = v;
          v = s;
        }
        const int old = atomicMin(&lab[u], v);
        if (old == u) break;
        u = old;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BT * BT; i += 256) {
      const int y = y0 + (i >> 5), x = x0 + (i & 31);
      if (y >= a.H || x >= a.W) continue;
      int v = -1;
      if (bg[i]) {
        const int r = lds_find(lab, i);
        v = (y0 + (r >> 5)) * a.W + x0 + (r & 31) + 1;
      }
      L[(size_t)y * a.W + x] = v;
    }
    __syncthreads();
  }
}

// labels: -1 foreground, 0 the frame, v > 0 the pixel v - 1 (a root holds its own v)
__device__ __forceinline__ int g_find(int* L, int v) {
  while (v > 0) {
    const int n = __hip_atomic_load(&L[v - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == v) break;
    v = n;
  }
  return v;
}

__device__ __forceinline__ void g_union(int* L, int u, int v) {
  u = g_find(L, u);
  v = g_find(L, v);
  while (u != v) {
    if (u < v) {
      const int s = u;
      u = v;
      v = s;
    }
    // u > v >= 0: u names a pixel
    const int old = atomicMin(&L[u - 1], v);
    if (old == u) break;
    u = old;
  }
}

__global__ __launch_bounds__(256) void bnd_merge_kernel(BndArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= npx) return;
  const int y = (int)(q / a.W), x = (int)(q - (size_t)y * a.W);
  const bool edge_x = x > 0 && (x % BT) == 0, edge_y = y > 0 && (y % BT) == 0;
  const bool on_h = y == 0 || y == a.H - 1, on_v = x == 0 || x == a.W - 1;
  if (!(edge_x || edge_y || on_h || on_v)) return;
  // Only the first of a run does the union: a background pair across a tile edge whose
  // predecessor along the edge (same tiles) is a background pair too joins the same two tile
  // components, and a border pixel whose predecessor along the border (same tile) is background
  // shares its component. Every run starts at a pixel that does not skip.
  const bool in_x = (x % BT) != 0, in_y = (y % BT) != 0;  // the predecessor is in the same tile
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    int* L = a.label + (size_t)img * npx;
    if (L[q] < 0) continue;  // (the sign of a label never changes: plain reads of it are safe)
    const int self = (int)q + 1;
    if (edge_x && L[q - 1] >= 0 && !(in_y && L[q - a.W] >= 0 && L[q - a.W - 1] >= 0)) g_union(L, self, self - 1);
    if (edge_y && L[q - a.W] >= 0 && !(in_x && L[q - 1] >= 0 && L[q - 1 - a.W] >= 0)) g_union(L, self, self - a.W);
    if ((on_h || on_v) && !((on_h && in_x && L[q - 1] >= 0) || (on_v && in_y && L[q - a.W] >= 0))) g_union(L, self, 0);
  }
}

__global__ __launch_bounds__(256) void bnd_flatten_kernel(BndArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= npx) return;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    int* L = a.label + (size_t)img * npx;
    const int v = L[q];
    if (v > 0) L[q] = g_find(L, v);
  }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(256) void bnd_extract_kernel(BndArgs a) {
  __shared__ int red[4];
  const size_t npx = (size_t)a.H * a.W;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    const int* L = a.label + (size_t)img * npx;
    uint8_t* o = img < a.B ? a.out_p : a.out_t;
    if (o) o += (size_t)(img < a.B ? img : img - a.B) * npx;
    int nb = 0;
#pragma unroll
    for (int j = 0; j < EXT_PER; ++j) {
      const size_t q = ((size_t)blockIdx.x * EXT_PER + j) * 256 + threadIdx.x;
      if (q >= npx) break;
      const int y = (int)(q / a.W), x = (int)(q - (size_t)y * a.W);
      int b = 0;
      if (L[q] < 0)
        b = x == 0 || y == 0 || x == a.W - 1 || y == a.H - 1 || L[q - 1] == 0 || L[q + 1] == 0 ||
            L[q - a.W] == 0 || L[q + a.W] == 0;
      a.bnd[(size_t)img * npx + q] = (uint8_t)b;
      if (o) o[q] = (uint8_t)b;
      nb += b;
    }
    const int s = wave_sum_i(nb);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = red[0] + red[1] + red[2] + red[3];
      if (n) atomicAdd(&a.counts[(img < a.B ? img : img - a.B) * 6 + (img < a.B ? 0 : 1)], n);
    }
    __syncthreads();
  }
}

// Column pass, in segments of CSEG = 32 rows so that no thread walks a whole column.
// bnd_colmask: one thread per (segment, column) packs the segment's boundary flags into 32 bits.
__global__ __launch_bounds__(256) void bnd_colmask_kernel(BndArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), seg = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.W || seg >= a.nseg) return;
  const size_t npx = (size_t)a.H * a.W;
  const int y0 = seg * CSEG;
  for (int img = blockIdx.z; img < a.N; img += gridDim.z) {
    const uint8_t* __restrict__ b = a.bnd + (size_t)img * npx + (size_t)y0 * a.W + x;
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < CSEG; ++r)
      if (y0 + r < a.H && b[(size_t)r * a.W]) m |= 1u << r;
    a.cmask[((size_t)img * a.nseg + seg) * a.W + x] = m;
  }
}

// bnd_coldist: the nearest boundary row above and below the segment from the other segments'
// masks, then the 32 distances of the segment from its own mask, in registers.
__global__ __launch_bounds__(256) void bnd_coldist_kernel(BndArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), seg = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.W || seg >= a.nseg) return;
  const size_t npx = (size_t)a.H * a.W;
  const int y0 = seg * CSEG;
  for (int img = blockIdx.z; img < a.N; img += gridDim.z) {
    const unsigned* __restrict__ cm = a.cmask + (size_t)img * a.nseg * a.W + x;
    uint16_t* __restrict__ g = a.g + (size_t)img * npx + (size_t)y0 * a.W + x;
    const unsigned m = cm[(size_t)seg * a.W];
    int above = -1, below = -1;  // rows of the nearest boundary pixels outside the segment
    for (int s = seg - 1; s >= 0; --s) {
      const unsigned o = cm[(size_t)s * a.W];
      if (o) {
        above = s * CSEG + 31 - __clz(o);
        break;
      }
    }
    for (int s = seg + 1; s < a.nseg; ++s) {
      const unsigned o = cm[(size_t)s * a.W];
      if (o) {
        below = s * CSEG + __ffs(o) - 1;
        break;
      }
    }
#pragma unroll
    for (int r = 0; r < CSEG; ++r) {
      if (y0 + r >= a.H) break;
      const unsigned lo = m & (0xFFFFFFFFu >> (31 - r)), hi = m >> r;  // flags of rows <= r, >= r
      const unsigned up = lo ? (unsigned)(r - (31 - __clz(lo))) : above >= 0 ? (unsigned)(y0 + r - above) : G_NONE;
      const unsigned dn = hi ? (unsigned)(__ffs(hi) - 1) : below >= 0 ? (unsigned)(below - y0 - r) : G_NONE;
      g[(size_t)r * a.W] = (uint16_t)min(up, dn);
    }
  }
}

constexpr int QSTEP = 8;  // columns per side and step of the search (their LDS reads are in flight together)

// squared distance from (y, x) to the set whose column distances of row y are g[0..W): outwards
// from x, QSTEP columns on each side per step, until the step's nearest column is no nearer than
// the best so far
__device__ __forceinline__ int nearest2(const uint16_t* g, int x, int W) {
  const unsigned g0 = g[x];
  int best = g0 != G_NONE ? (int)(g0 * g0) : INT32_MAX;
  const int reach = max(x, W - 1 - x);
  for (int d0 = 1; d0 <= reach && d0 * d0 < best; d0 += QSTEP) {
#pragma unroll
    for (int k = 0; k < QSTEP; ++k) {
      const int dx = d0 + k, xl = x - dx, xr = x + dx;
      const unsigned vl = g[max(xl, 0)], vr = g[min(xr, W - 1)];
      if (xl >= 0 && vl != G_NONE) best = min(best, (int)(vl * vl) + dx * dx);
      if (xr < W && vr != G_NONE) best = min(best, (int)(vr * vr) + dx * dx);
    }
  }
  return best;
}

// m = #[d^2 <= tol2], h = max d^2 over the n pixels of the row listed in xs against g
__device__ __forceinline__ void query_row(const uint16_t* xs, int n, const uint16_t* g, int W, int tol2, int lane,
                                          int& m, int& h) {
  for (int i = lane; i < n; i += 64) {
    const int d2 = nearest2(g, xs[i], W);
    m += d2 <= tol2;
    h = max(h, d2);
  }
}

__global__ __launch_bounds__(64) void bnd_query_kernel(BndArgs a) {
  // row y of g_Bt, then of g_Bp; then the columns of the row's Bp pixels, then of its Bt pixels
  // (boundary pixels are few per row: compacted, every lane of the search has one)
  extern __shared__ uint16_t grow[];  // [4][W]
  uint16_t* xs = grow + 2 * a.W;
  const size_t npx = (size_t)a.H * a.W;
  const int y = blockIdx.x, lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1;  // the lanes before this one
  for (int s = blockIdx.y; s < a.B; s += gridDim.y) {
    const int* c = a.counts + s * 6;
    const size_t row_p = (size_t)s * npx + (size_t)y * a.W, row_t = (size_t)(a.B + s) * npx + (size_t)y * a.W;
    // everything the row needs in one round of independent loads; all later reads are LDS
    const int n_p = c[0], n_t = c[1];
    int k_p = 0, k_t = 0;  // pixels of Bp, Bt in this row (uniform)
    for (int x0 = 0; x0 < a.W; x0 += 64) {
      const int x = x0 + lane;
      bool fp = false, ft = false;
      if (x < a.W) {
        fp = a.bnd[row_p + x] != 0;
        ft = a.bnd[row_t + x] != 0;
        grow[x] = a.g[row_t + x];
        grow[a.W + x] = a.g[row_p + x];
      }
      const unsigned long long mp = __ballot(fp), mt = __ballot(ft);
      if (fp) xs[k_p + __popcll(mp & below)] = (uint16_t)x;
      if (ft) xs[a.W + k_t + __popcll(mt & below)] = (uint16_t)x;
      k_p += __popcll(mp);
      k_t += __popcll(mt);
    }
    __syncthreads();
    // an empty set: m_* = 0, h2_* = -1 (all of this is block-uniform)
    int m_p = 0, m_t = 0, h_p = -1, h_t = -1;
    if (n_p != 0 && n_t != 0) {
      query_row(xs, k_p, grow, a.W, a.tol2, lane, m_p, h_p);
      query_row(xs + a.W, k_t, grow + a.W, a.W, a.tol2, lane, m_t, h_t);
      m_p = wave_sum_i(m_p);
      m_t = wave_sum_i(m_t);
      h_p = wave_max_i(h_p);
      h_t = wave_max_i(h_t);
    }
    // per-row partials, reduced per sample by bnd_reduce: plain stores instead of thousands of
    // rows' atomics on the same four counters
    if (lane == 0) *(int4*)(a.part + ((size_t)s * a.H + y) * 4) = make_int4(m_p, m_t, h_p, h_t);
    __syncthreads();  // the row buffers are restaged for the next sample
  }
}

// counts[s][2..5] = (sum m_p, sum m_t, max h_p, max h_t) over the rows of sample s
__global__ __launch_bounds__(256) void bnd_reduce_kernel(BndArgs a) {
  __shared__ int red[4][4];
  for (int s = blockIdx.x; s < a.B; s += gridDim.x) {
    int m_p = 0, m_t = 0, h_p = -1, h_t = -1;
    for (int y = threadIdx.x; y < a.H; y += 256) {
      const int4 v = *(const int4*)(a.part + ((size_t)s * a.H + y) * 4);
      m_p += v.x;
      m_t += v.y;
      h_p = max(h_p, v.z);
      h_t = max(h_t, v.w);
    }
    m_p = wave_sum_i(m_p);
    m_t = wave_sum_i(m_t);
    h_p = wave_max_i(h_p);
    h_t = wave_max_i(h_t);
    if ((threadIdx.x & 63) == 0) {
      int* r = red[threadIdx.x >> 6];
      r[0] = m_p;
      r[1] = m_t;
      r[2] = h_p;
      r[3] = h_t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int* c = a.counts + s * 6;
      c[2] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
      c[3] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
      c[4] = max(max(red[0][2], red[1][2]), max(red[2][2], red[3][2]));
      c[5] = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
    }
    __syncthreads();
  }
}

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace pis

using namespace pis;

// labels (int32) + boundary maps (uint8) + column distances (uint16) + segment masks for the 2B images,
// per-row partials
extern "C" size_t pis_boundary_ws(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > BND_MAX || W > BND_MAX) return 0;
  const size_t n = (size_t)2 * B * H * W;
  return align256(n * 4) + align256(n) + align256(n * 2) + align256((size_t)2 * B * cdiv(H, CSEG) * W * 4) +
         align256((size_t)B * H * 16);
}

extern "C" int pis_boundary_metrics(const float* p, const float* t, int B, int H, int W, float thr, int tolerance,
                                    int* counts, uint8_t* bnd_p, uint8_t* bnd_t, void* ws, size_t ws_bytes,
                                    pis_stream_t stream) {
  PIS_CHECK_ARG(p && t && counts, "pis_boundary_metrics: p, t or counts is NULL");
  PIS_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= BND_MAX && W <= BND_MAX,
                "pis_boundary_metrics: bad shape B=%d H=%d W=%d (B >= 1, 1 <= H, W <= %d)", B, H, W, BND_MAX);
  PIS_CHECK_ARG(B <= (1 << 24), "pis_boundary_metrics: B=%d > 2^24", B);
  PIS_CHECK_ARG(tolerance >= 0, "pis_boundary_metrics: tolerance=%d < 0", tolerance);
  PIS_CHECK_ARG(ws != nullptr, "pis_boundary_metrics: ws is NULL");
  if (ws_bytes < pis_boundary_ws(B, H, W)) {
    set_error("pis_boundary_metrics: workspace too small (%zu < %zu bytes)", ws_bytes, pis_boundary_ws(B, H, W));
    return PIS_ERR_WORKSPACE;
  }
  BndArgs a{};
  a.p = p; a.t = t; a.B = B; a.H = H; a.W = W; a.N = 2 * B;
  a.tiles_x = (int)cdiv(W, BT); a.tiles_y = (int)cdiv(H, BT); a.nseg = (int)cdiv(H, CSEG);
  a.thr = thr;
  a.tol2 = tolerance > 46340 ? INT32_MAX : tolerance * tolerance;
  a.counts = counts;
  const size_t n = (size_t)a.N * H * W;
  char* w = (char*)ws;
  a.label = (int*)w;
  a.bnd = (uint8_t*)(w + align256(n * 4));
  a.g = (uint16_t*)(w + align256(n * 4) + align256(n));
  a.cmask = (unsigned*)(w + align256(n * 4) + align256(n) + align256(n * 2));
  a.part = (int*)((char*)a.cmask + align256((size_t)a.N * a.nseg * W * 4));
  a.out_p = bnd_p; a.out_t = bnd_t;
  hipStream_t s = (hipStream_t)stream;
  const unsigned gy = (unsigned)std::min(a.N, 65535), gb = (unsigned)std::min(B, 65535);
  const unsigned npb = (unsigned)cdiv((int64_t)H * W, 256);
  const double px = (double)n;
  int rc;
#define PIS_BND(NAME, KERNEL, GRID, BLOCK, SMEM)            \
  launch_hook(NAME, 0, s, px);                              \
  hipLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), SMEM, s, a); \
  launch_hook(NAME, 1, s, px);                              \
  rc = launch_status(NAME);                                 \
  if (rc) return rc;
  PIS_BND("bnd_init", bnd_init_kernel, dim3((unsigned)cdiv((int64_t)B * 6, 256)), 256, 0)
  PIS_BND("bnd_label", bnd_label_kernel, dim3(a.tiles_x * a.tiles_y, gy), 256, 0)
  PIS_BND("bnd_merge", bnd_merge_kernel, dim3(npb, gy), 256, 0)
  PIS_BND("bnd_flatten", bnd_flatten_kernel, dim3(npb, gy), 256, 0)
  PIS_BND("bnd_extract", bnd_extract_kernel, dim3((unsigned)cdiv(npb, EXT_PER), gy), 256, 0)
  const dim3 gcol((unsigned)cdiv(W, 64), (unsigned)cdiv(a.nseg, 4), gy);
  PIS_BND("bnd_colmask", bnd_colmask_kernel, gcol, 256, 0)
  PIS_BND("bnd_coldist", bnd_coldist_kernel, gcol, 256, 0)
  PIS_BND("bnd_query", bnd_query_kernel, dim3(H, gb), 64, (size_t)8 * W)
  PIS_BND("bnd_reduce", bnd_reduce_kernel, dim3(gb), 256, 0)
#undef PIS_BND
  return PIS_OK;
}
