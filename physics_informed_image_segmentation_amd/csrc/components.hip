// Object-level counters of a batch on the device (evaluate.py: object_counts, label_components):
// connected components of the foreground, detection matches at IoU 0.5 / 0.75 and the Aggregated
// Jaccard Index, exact integers, fixed launch count. Definitions: include/pis_capi.h.
//
// All 2B images (B predictions thresholded at p > thr, B targets at t > 0) go through one set of
// launches; image i < B is prediction i, image B + i is target i. Per image and pixel the
// workspace holds a label, an area slot and an auxiliary slot (int32 each).
//
//   1. obj_init     counts = 0, overflow flags = 0, pair table emptied
//   2. obj_label    per 32x32 tile: union-find over the tile's foreground pixels in LDS (parent =
//                   up, else left, else up-left, else up-right neighbour, the diagonals for
//                   8-connectivity only; compress; the unions the parent choice leaves out;
//                   compress), written to the global label array as "tile root pixel + 1".
//                   Background is 0. area = 0; aux = 0 (predictions) / -1 (targets).
//   3. obj_merge    unions across tile edges by atomic-min on the global labels, for
//                   8-connectivity with both diagonals across an edge (and so across a corner)
//   4. obj_flatten  label = root, area[root] += pixels (one add per horizontal run and wave)
//   5. obj_overlap  per horizontal run of P n T (one predicted and one true object by
//                   construction) table[(root_p, root_t)] += length; predicted objects below
//                   min_area take no part
//   6. obj_pairs    per table entry: tp50 / tp75, and the entry competes for "best match of its
//                   true object" (aux of the true root = slot of the best entry)
//   7. obj_targets  per true root: n_t, the AJI terms of its best match, which is marked used
//                   (aux of the predicted root = 1)
//   8. obj_preds    per predicted root: n_p, area_p, removed, unused kept objects into aji_union
//   9. obj_final    a sample whose table gave up on an insert gets -1 in all counters
//  and, when a label map is asked for, the object numbers as a prefix sum over the root flags in
//  row-major order, in separate launches (no block waits for another one):
//  10. obj_rank_sums   flags per block of 256 pixels
//  11. obj_rank_scan   exclusive scan of each image's block sums, one block per image
//  12. obj_rank_write  aux[root] = number
//  13. obj_rank_gather label map = number of the pixel's root (0: background, removed)
//
// The root of a component is its smallest pixel index: tile roots are the smallest tile-local
// index, which orders pixels of a tile as the image does, and merging keeps the minimum. So "the
// smaller object number" of the tie rule is the smaller root.
//
// Union-find under concurrency (as csrc/boundary.hip): links only ever move to a smaller label of
// the same component, so a stale or racing read still names a member of the component and every
// loop ends at the atomic that decides; the result is the set of components, independent of
// ordering. The best-match loop of obj_pairs ends the same way: the slot only ever moves to an
// entry that is strictly better in a total order (larger I / U, then smaller root_p; the entries
// of one true object have distinct root_p), so a failed compare-and-swap means progress elsewhere.
//
// The pair table is open addressing with linear probing, 64-bit keys claimed by compare-and-swap,
// int32 sums by atomic add (integers: order-independent). Its entries are the distinct pairs,
// and distinct pairs <= horizontal runs of P n T <= H * ceil(W / 2) per image; the capacity is the
// next power of two >= twice that, so it is never more than half full and cannot overflow. The
// probe loop is bounded by the capacity all the same and raises the sample's overflow flag
// instead of spinning.
#include "common.h"

namespace pis {

constexpr int OT = 32;          // label tile edge
constexpr int OBJ_MAX = 4096;   // H, W limit (roots and areas in int32, I * U below 2^50)

struct ObjArgs {
  const float* p;
  const float* t;
  int B, H, W, N;  // N = 2B images
  int tiles_x, tiles_y;
  float thr;
  int conn8, min_area;
  unsigned cap;               // table slots per sample, a power of two
  int nblk;                   // blocks of 256 pixels per image
  unsigned long long* counts; // [B][8] (int64 bit patterns)
  int* label;                 // [N][H*W]
  int* area;                  // [N][H*W]
  int* aux;                   // [N][H*W]
  unsigned long long* keys;   // [B][cap]  (root_p << 32) | root_t, 0 = empty
  int* vals;                  // [B][cap]
  int* ovf;                   // [B]
  int* bsum;                  // [N][nblk]
  int* out_p;                 // [B][H*W] or NULL
  int* out_t;                 // [B][H*W] or NULL
};

__device__ __forceinline__ long long obj_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// counts[idx] += the wave's sum of v (one atomic per wave that has something to add)
__device__ __forceinline__ void obj_count(unsigned long long* c, long long v) {
  v = obj_wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(c, (unsigned long long)v);
}

__global__ __launch_bounds__(256) void obj_init_kernel(ObjArgs a) {
  const size_t total = (size_t)a.B * a.cap, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    a.keys[i] = 0;
    a.vals[i] = 0;
    if (i < (size_t)a.B * 8) a.counts[i] = 0;
    if (i < (size_t)a.B) a.ovf[i] = 0;
  }
}

__device__ __forceinline__ int obj_lds_find(volatile int* lab, int i) {
  for (;;) {
    const int n = lab[i];
    if (n == i) return i;
    i = n;
  }
}

__device__ __forceinline__ void obj_lds_union(int* lab, int i, int j) {
  int u = obj_lds_find(lab, i), v = obj_lds_find(lab, j);
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

__global__ __launch_bounds__(256) void obj_label_kernel(ObjArgs a) {
  __shared__ int lab[OT * OT];
  __shared__ uint8_t fg[OT * OT];
  const int x0 = (blockIdx.x % a.tiles_x) * OT, y0 = (blockIdx.x / a.tiles_x) * OT;
  const size_t npx = (size_t)a.H * a.W;
  const bool c8 = a.conn8 != 0;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    const float* src = img < a.B ? a.p + (size_t)img * npx : a.t + (size_t)(img - a.B) * npx;
    const float thr = img < a.B ? a.thr : 0.f;
    for (int i = threadIdx.x; i < OT * OT; i += 256) {
      const int y = y0 + (i >> 5), x = x0 + (i & 31);
      // strict '>' : NaN is background; so are the slots past the image edge
      fg[i] = (y < a.H && x < a.W) ? (src[(size_t)y * a.W + x] > thr) : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OT * OT; i += 256) {
      const int ty = i >> 5, tx = i & 31;
      const bool up = ty > 0 && fg[i - OT], left = tx > 0 && fg[i - 1];
      const bool ul = c8 && ty > 0 && tx > 0 && fg[i - OT - 1], ur = c8 && ty > 0 && tx < OT - 1 && fg[i - OT + 1];
      lab[i] = up ? i - OT : left ? i - 1 : ul ? i - OT - 1 : ur ? i - OT + 1 : i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OT * OT; i += 256)
      if (fg[i]) {
        const int r = obj_lds_find(lab, i);
        lab[i] = r;
      }
    __syncthreads();
    // After the parent choice every pixel is joined to its up and to its left neighbour except
    // where both exist (the parent is up: join left here). That already joins up-left (the left of
    // up, the up of left) and, next to a foreground up, up-right (whose left is up). What is left
    // for 8-connectivity is up-right without up, when the parent was left or up-left.
    for (int i = threadIdx.x; i < OT * OT; i += 256) {
      if (!fg[i]) continue;
      const int ty = i >> 5, tx = i & 31;
      const bool up = ty > 0 && fg[i - OT], left = tx > 0 && fg[i - 1];
      if (up && left) obj_lds_union(lab, i, i - 1);
      if (c8 && !up && ty > 0 && tx < OT - 1 && fg[i - OT + 1] && (left || (tx > 0 && fg[i - OT - 1])))
        obj_lds_union(lab, i, i - OT + 1);
    }
    __syncthreads();
    int* L = a.label + (size_t)img * npx;
    int* A = a.area + (size_t)img * npx;
    int* X = a.aux + (size_t)img * npx;
    for (int i = threadIdx.x; i < OT * OT; i += 256) {
      const int y = y0 + (i >> 5), x = x0 + (i & 31);
      if (y >= a.H || x >= a.W) continue;
      int v = 0;
      if (fg[i]) {
        const int r = obj_lds_find(lab, i);
        v = (y0 + (r >> 5)) * a.W + x0 + (r & 31) + 1;
      }
      const size_t q = (size_t)y * a.W + x;
      L[q] = v;
      A[q] = 0;
      X[q] = img < a.B ? 0 : -1;
    }
    __syncthreads();
  }
}

// labels: 0 background, v > 0 the pixel v - 1 (a root holds its own v)
__device__ __forceinline__ int obj_find(int* L, int v) {
  for (;;) {
    const int n = __hip_atomic_load(&L[v - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n == v) return v;
    v = n;
  }
}

// u, v > 0: foreground pixels
__device__ __forceinline__ void obj_union(int* L, int u, int v) {
  u = obj_find(L, u);
  v = obj_find(L, v);
  while (u != v) {
    if (u < v) {
      const int s = u;
      u = v;
      v = s;
    }
    const int old = atomicMin(&L[u - 1], v);
    if (old == u) break;
    u = old;
  }
}

__global__ __launch_bounds__(256) void obj_merge_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= npx) return;
  const int W = a.W, y = (int)(q / W), x = (int)(q - (size_t)y * W);
  const bool edge_x = x > 0 && (x % OT) == 0, edge_y = y > 0 && (y % OT) == 0;
  if (!(edge_x || edge_y)) return;
  const bool c8 = a.conn8 != 0;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    int* L = a.label + (size_t)img * npx;
    if (L[q] == 0) continue;  // (whether a label is 0 never changes: plain reads of that are safe)
    const int self = (int)q + 1;
    if (edge_x) {  // the tile to the left: (y, x-1), and for 8-connectivity (y-1, x-1), (y+1, x-1)
      if (L[q - 1] != 0) obj_union(L, self, self - 1);
      if (c8 && y > 0 && L[q - W - 1] != 0) obj_union(L, self, self - W - 1);
      if (c8 && y < a.H - 1 && L[q + W - 1] != 0) obj_union(L, self, self + W - 1);
    }
    if (edge_y) {  // the tile above: (y-1, x), and for 8-connectivity (y-1, x-1), (y-1, x+1)
      if (L[q - W] != 0) obj_union(L, self, self - W);
      if (c8 && x > 0 && L[q - W - 1] != 0) obj_union(L, self, self - W - 1);
      if (c8 && x < W - 1 && L[q - W + 1] != 0) obj_union(L, self, self - W + 1);
    }
  }
}

// Horizontal runs inside a wave: lanes are consecutive pixels, f marks the pixels of interest.
// Returns the length of the run that starts at this lane (cut at the end of the image row and of
// the wave), 0 for every other lane. All 64 lanes must call it.
__device__ __forceinline__ int obj_run_start(bool f, int x, int W) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(f);
  if (!f) return 0;
  if (!(lane == 0 || x == 0 || !((m >> (lane - 1)) & 1))) return 0;
  const unsigned long long inv = ~(m >> lane);
  const int n = inv ? __ffsll((long long)inv) - 1 : 64;
  return min(n, W - x);
}

__global__ __launch_bounds__(256) void obj_flatten_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = q < npx;
  const int x = valid ? (int)(q % a.W) : 0;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    int* L = a.label + (size_t)img * npx;
    int r = 0;
    if (valid) {
      const int v = L[q];
      if (v > 0) {
        r = obj_find(L, v);
        L[q] = r;
      }
    }
    // the pixels of a horizontal run are 4-connected: one root
    const int n = obj_run_start(r > 0, x, a.W);
    if (n) atomicAdd(&a.area[(size_t)img * npx + r - 1], n);
  }
}

__device__ __forceinline__ unsigned long long obj_mix(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// table[key] += n; false if no slot could be had within cap probes
__device__ __forceinline__ bool obj_table_add(unsigned long long* keys, int* vals, unsigned cap,
                                              unsigned long long key, int n) {
  unsigned slot = (unsigned)obj_mix(key) & (cap - 1);
  for (unsigned probe = 0; probe < cap; ++probe) {
    unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) k = atomicCAS(&keys[slot], 0ull, key);  // the old value: 0 = this call claimed the slot
    if (k == 0 || k == key) {
      atomicAdd(&vals[slot], n);
      return true;
    }
    slot = (slot + 1) & (cap - 1);
  }
  return false;
}

__global__ __launch_bounds__(256) void obj_overlap_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = q < npx;
  const int x = valid ? (int)(q % a.W) : 0;
  for (int s = blockIdx.y; s < a.B; s += gridDim.y) {
    const int rp = valid ? a.label[(size_t)s * npx + q] : 0;
    const int rt = valid ? a.label[(size_t)(a.B + s) * npx + q] : 0;
    const bool f = rp > 0 && rt > 0 && a.area[(size_t)s * npx + rp - 1] >= a.min_area;
    const int n = obj_run_start(f, x, a.W);
    if (n && !obj_table_add(a.keys + (size_t)s * a.cap, a.vals + (size_t)s * a.cap, a.cap,
                            ((unsigned long long)(unsigned)rp << 32) | (unsigned)rt, n))
      a.ovf[s] = 1;
  }
}

__global__ __launch_bounds__(256) void obj_pairs_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const unsigned e = blockIdx.x * 256 + threadIdx.x;
  for (int s = blockIdx.y; s < a.B; s += gridDim.y) {
    const unsigned long long* keys = a.keys + (size_t)s * a.cap;
    const int* vals = a.vals + (size_t)s * a.cap;
    const int* Ap = a.area + (size_t)s * npx;
    const int* At = a.area + (size_t)(a.B + s) * npx;
    const unsigned long long key = e < a.cap ? keys[e] : 0;
    long long tp50 = 0, tp75 = 0;
    if (key) {
      const int rp = (int)(key >> 32), rt = (int)(key & 0xffffffffu);
      const long long I = vals[e], at = At[rt - 1], S = Ap[rp - 1] + at, U = S - I;
      tp50 = 3 * I > S;
      tp75 = 7 * I > 3 * S;
      int* best = a.aux + (size_t)(a.B + s) * npx + rt - 1;
      int cur = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        if (cur >= 0) {
          const int rc = (int)(keys[cur] >> 32);
          const long long Ic = vals[cur], Uc = Ap[rc - 1] + at - Ic;
          const long long l = I * Uc, r = Ic * U;  // I / U against Ic / Uc, both below 2^50
          if (!(l > r || (l == r && rp < rc))) break;
        }
        const int old = atomicCAS(best, cur, (int)e);
        if (old == cur) break;
        cur = old;
      }
    }
    obj_count(a.counts + (size_t)s * 8 + 2, tp50);
    obj_count(a.counts + (size_t)s * 8 + 3, tp75);
  }
}

__global__ __launch_bounds__(256) void obj_targets_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int s = blockIdx.y; s < a.B; s += gridDim.y) {
    long long n_t = 0, inter = 0, uni = 0;
    if (q < npx && a.label[(size_t)(a.B + s) * npx + q] == (int)q + 1) {
      n_t = 1;
      const long long at = a.area[(size_t)(a.B + s) * npx + q];
      const int b = a.aux[(size_t)(a.B + s) * npx + q];
      if (b < 0) {
        uni = at;
      } else {
        const int rp = (int)(a.keys[(size_t)s * a.cap + b] >> 32);
        inter = a.vals[(size_t)s * a.cap + b];
        uni = a.area[(size_t)s * npx + rp - 1] + at - inter;
        a.aux[(size_t)s * npx + rp - 1] = 1;  // used (every writer stores the same 1)
      }
    }
    obj_count(a.counts + (size_t)s * 8 + 1, n_t);
    obj_count(a.counts + (size_t)s * 8 + 4, inter);
    obj_count(a.counts + (size_t)s * 8 + 5, uni);
  }
}

__global__ __launch_bounds__(256) void obj_preds_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int s = blockIdx.y; s < a.B; s += gridDim.y) {
    long long n_p = 0, uni = 0, area_p = 0, removed = 0;
    if (q < npx && a.label[(size_t)s * npx + q] == (int)q + 1) {
      const int ap = a.area[(size_t)s * npx + q];
      if (ap >= a.min_area) {
        n_p = 1;
        area_p = ap;
        if (!a.aux[(size_t)s * npx + q]) uni = ap;
      } else {
        removed = 1;
      }
    }
    obj_count(a.counts + (size_t)s * 8 + 0, n_p);
    obj_count(a.counts + (size_t)s * 8 + 5, uni);
    obj_count(a.counts + (size_t)s * 8 + 6, area_p);
    obj_count(a.counts + (size_t)s * 8 + 7, removed);
  }
}

__global__ __launch_bounds__(256) void obj_final_kernel(ObjArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.B * 8 && a.ovf[i >> 3]) a.counts[i] = ~0ull;  // -1
}

// ---- object numbers: prefix sum over the root flags of each image, row-major ----

// the kept roots; an image whose label map is not asked for has none (its launches do nothing)
__device__ __forceinline__ bool obj_wanted(const ObjArgs& a, int img) { return (img < a.B ? a.out_p : a.out_t) != nullptr; }

__device__ __forceinline__ bool obj_flag(const ObjArgs& a, int img, size_t q, size_t npx) {
  if (q >= npx || a.label[(size_t)img * npx + q] != (int)q + 1) return false;
  return img >= a.B || a.area[(size_t)img * npx + q] >= a.min_area;
}

__global__ __launch_bounds__(256) void obj_rank_sums_kernel(ObjArgs a) {
  __shared__ int red[4];
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    if (!obj_wanted(a, img)) continue;
    const unsigned long long m = __ballot(obj_flag(a, img, q, npx));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) a.bsum[(size_t)img * a.nblk + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
}

// bsum[img][0..nblk) -> its exclusive prefix sums; one block per image walks the row in chunks
__global__ __launch_bounds__(256) void obj_rank_scan_kernel(ObjArgs a) {
  __shared__ int sc[256];
  for (int img = blockIdx.x; img < a.N; img += gridDim.x) {
    if (!obj_wanted(a, img)) continue;
    int* b = a.bsum + (size_t)img * a.nblk;
    int carry = 0;
    for (int c0 = 0; c0 < a.nblk; c0 += 256) {
      const int i = c0 + threadIdx.x;
      const int v = i < a.nblk ? b[i] : 0;
      sc[threadIdx.x] = v;
      __syncthreads();
      for (int off = 1; off < 256; off <<= 1) {
        const int add = threadIdx.x >= off ? sc[threadIdx.x - off] : 0;
        __syncthreads();
        sc[threadIdx.x] += add;
        __syncthreads();
      }
      if (i < a.nblk) b[i] = carry + sc[threadIdx.x] - v;
      carry += sc[255];
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void obj_rank_write_kernel(ObjArgs a) {
  __shared__ int red[4];
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    if (!obj_wanted(a, img)) continue;
    const bool f = obj_flag(a, img, q, npx);
    const unsigned long long m = __ballot(f);
    if (lane == 0) red[wv] = __popcll(m);
    __syncthreads();
    int before = a.bsum[(size_t)img * a.nblk + blockIdx.x];
    for (int w = 0; w < wv; ++w) before += red[w];
    if (f) a.aux[(size_t)img * npx + q] = before + __popcll(m & ((1ull << lane) - 1)) + 1;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void obj_rank_gather_kernel(ObjArgs a) {
  const size_t npx = (size_t)a.H * a.W;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= npx) return;
  for (int img = blockIdx.y; img < a.N; img += gridDim.y) {
    if (!obj_wanted(a, img)) continue;
    int* o = img < a.B ? a.out_p + (size_t)img * npx : a.out_t + (size_t)(img - a.B) * npx;
    const int r = a.label[(size_t)img * npx + q];
    const bool kept = r > 0 && (img >= a.B || a.area[(size_t)img * npx + r - 1] >= a.min_area);
    o[q] = kept ? a.aux[(size_t)img * npx + r - 1] : 0;
  }
}

static size_t obj_align(size_t n) { return (n + 255) & ~(size_t)255; }

// slots per sample: the next power of two >= 2 * H * ceil(W / 2) (at least 16)
static unsigned obj_cap(int H, int W) {
  const uint64_t runs = (uint64_t)H * (uint64_t)((W + 1) / 2);
  uint64_t c = 16;
  while (c < 2 * runs) c <<= 1;
  return (unsigned)c;  // <= 2^24
}

}  // namespace pis

using namespace pis;

// label, area and auxiliary slot (int32 each) per pixel of the 2B images; per sample the pair
// table (8-byte keys, 4-byte sums) and an overflow flag; per image one int per 256 pixels
extern "C" size_t pis_objects_ws(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > OBJ_MAX || W > OBJ_MAX) return 0;
  const size_t n = (size_t)2 * B * H * W, cap = obj_cap(H, W);
  return 3 * obj_align(n * 4) + obj_align((size_t)B * cap * 8) + obj_align((size_t)B * cap * 4) +
         obj_align((size_t)B * 4) + obj_align((size_t)2 * B * cdiv((int64_t)H * W, 256) * 4);
}

extern "C" int pis_object_metrics(const float* p, const float* t, int B, int H, int W, float thr, int connectivity,
                                  int min_area, int64_t* counts, int32_t* labels_p, int32_t* labels_t, void* ws,
                                  size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(p && t && counts, "pis_object_metrics: p, t or counts is NULL");
  PIS_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= OBJ_MAX && W <= OBJ_MAX,
                "pis_object_metrics: bad shape B=%d H=%d W=%d (B >= 1, 1 <= H, W <= %d)", B, H, W, OBJ_MAX);
  PIS_CHECK_ARG(B <= (1 << 24), "pis_object_metrics: B=%d > 2^24", B);
  PIS_CHECK_ARG(connectivity == 4 || connectivity == 8, "pis_object_metrics: connectivity=%d (4 or 8)", connectivity);
  PIS_CHECK_ARG(min_area >= 0, "pis_object_metrics: min_area=%d < 0", min_area);
  PIS_CHECK_ARG(ws != nullptr, "pis_object_metrics: ws is NULL");
  if (ws_bytes < pis_objects_ws(B, H, W)) {
    set_error("pis_object_metrics: workspace too small (%zu < %zu bytes)", ws_bytes, pis_objects_ws(B, H, W));
    return PIS_ERR_WORKSPACE;
  }
  ObjArgs a{};
  a.p = p; a.t = t; a.B = B; a.H = H; a.W = W; a.N = 2 * B;
  a.tiles_x = (int)cdiv(W, OT); a.tiles_y = (int)cdiv(H, OT);
  a.thr = thr;
  a.conn8 = connectivity == 8;
  a.min_area = min_area;
  a.cap = obj_cap(H, W);
  a.nblk = (int)cdiv((int64_t)H * W, 256);
  a.counts = (unsigned long long*)counts;
  const size_t n = (size_t)a.N * H * W;
  char* w = (char*)ws;
  a.label = (int*)w;  w += obj_align(n * 4);
  a.area = (int*)w;   w += obj_align(n * 4);
  a.aux = (int*)w;    w += obj_align(n * 4);
  a.keys = (unsigned long long*)w;  w += obj_align((size_t)B * a.cap * 8);
  a.vals = (int*)w;   w += obj_align((size_t)B * a.cap * 4);
  a.ovf = (int*)w;    w += obj_align((size_t)B * 4);
  a.bsum = (int*)w;
  a.out_p = labels_p; a.out_t = labels_t;
  hipStream_t s = (hipStream_t)stream;
  const unsigned gy = (unsigned)std::min(a.N, 65535), gb = (unsigned)std::min(B, 65535);
  const unsigned npb = (unsigned)a.nblk;
  const double px = (double)n;
  int rc;
#define PIS_OBJ(NAME, KERNEL, GRID)                       \
  launch_hook(NAME, 0, s, px);                            \
  hipLaunchKernelGGL(KERNEL, GRID, dim3(256), 0, s, a);   \
  launch_hook(NAME, 1, s, px);                            \
  rc = launch_status(NAME);                               \
  if (rc) return rc;
  PIS_OBJ("obj_init", obj_init_kernel, dim3((unsigned)std::min<int64_t>(cdiv((int64_t)B * a.cap, 256), 1 << 20)))  // grid-stride beyond
  PIS_OBJ("obj_label", obj_label_kernel, dim3(a.tiles_x * a.tiles_y, gy))
  PIS_OBJ("obj_merge", obj_merge_kernel, dim3(npb, gy))
  PIS_OBJ("obj_flatten", obj_flatten_kernel, dim3(npb, gy))
  PIS_OBJ("obj_overlap", obj_overlap_kernel, dim3(npb, gb))
  PIS_OBJ("obj_pairs", obj_pairs_kernel, dim3(a.cap / 256 ? a.cap / 256 : 1, gb))
  PIS_OBJ("obj_targets", obj_targets_kernel, dim3(npb, gb))
  PIS_OBJ("obj_preds", obj_preds_kernel, dim3(npb, gb))
  PIS_OBJ("obj_final", obj_final_kernel, dim3((unsigned)cdiv((int64_t)B * 8, 256)))
  if (labels_p || labels_t) {
    PIS_OBJ("obj_rank_sums", obj_rank_sums_kernel, dim3(npb, gy))
    PIS_OBJ("obj_rank_scan", obj_rank_scan_kernel, dim3(gy))
    PIS_OBJ("obj_rank_write", obj_rank_write_kernel, dim3(npb, gy))
    PIS_OBJ("obj_rank_gather", obj_rank_gather_kernel, dim3(npb, gy))
  }
#undef PIS_OBJ
  return PIS_OK;
}
