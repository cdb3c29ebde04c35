// Probability-level table of a batch on the device (evaluate.py: probability_table): per sample and
// target class a 1025-bin histogram of the predictions quantised UP to 16 fractional bits, with the
// sum of the quantised values per bin and the sums of their squares per class. Exact integers; the
// threshold sweep, AUROC, average precision, ECE and the Brier score are torch arithmetic on it.
// Definitions: include/pis_capi.h, DESIGN.md §12.
//
//   1. prob_hist  one block of 1024 threads per PB_PIX consecutive pixels of ONE sample (a block never
//                 straddles two samples): one pass over p and t, float4 loads where the sample's base
//                 allows (a scalar head up to the first 16-byte boundary and a scalar tail; all
//                 scalar when p and t are misaligned against each other), the second float4 pair in
//                 flight while the first is counted. Per pixel q, bin, class as the header defines
//                 them, then
//                   - one LDS integer atomic into one of the block's two histograms (waves alternate).
//                     Inside bin i >= 1, q = 64 (i - 1) + 1 + r' with r' in 0..63, so one 32-bit word
//                     per (class, bin) carries both the count (bits 18..31) and the sum of r' (bits
//                     0..17): a histogram sees at most PB_PIX / 2 + 6 pixels, so the count stays
//                     below 2^14 and the sum of r' below 2^18. 8.2 KB per copy;
//                   - a lane merges equal (class, bin) keys of the pixels it meets one after the
//                     other in a register and adds once per run: on a constant or a saturated field
//                     (every lane of a wave on one address) one add per lane and block instead of
//                     eight;
//                   - the squares: (uint64) q * q into two per-lane accumulators, reduced through the
//                     wave and the block; NaNs counted by ballot + popcount.
//                 The block widens its merged histogram to { count, count (64 (i - 1) + 1) + sum r' }
//                 (both below 2^30 for PB_PIX pixels: uint32) and stores it with its three extra
//                 sums into the workspace with plain stores.
//   2. prob_sum   per sample and entry: the sum of the blocks' partials in int64, written to table
//                 and extra. Integers: any order gives the same bits.
// Nothing in ws is read before it is written in the same call.
//
// Forms kept behind pis_tune key 52 for the A/B (tools/bench_probability.py; all give the same
// integers; profiles/probability_metrics.txt has the numbers, 8 x 512^2 / 64 x 128^2 per call):
//   bit 0  the two END bins (q = 0, and bin 1024) never reach a per-lane atomic: counts per class
//          from three wave ballots + popcounts in wave-uniform registers, the top bin's sum of r' in a
//          per-lane register reduced across the wave once, lane 0 adds. Costs 10 % on every input,
//          saturated fields included: with the merging above a lane's end-bin pixels are one add.
//   bit 1  four histograms per block instead of two: within 2 % either way.
//   bit 2  no merging, one atomic per pixel: +15-25 % on constant and saturated fields.
#include "common.h"

namespace pis {

constexpr int PROB_MAX = 4096;        // H, W limit: count <= 2^24, sum q <= 2^40, sum q^2 <= 2^56
constexpr int PB_PIX = 8192;          // pixels per block
constexpr int PB_THREADS = 1024;     // 16 waves: two float4 of p and of t per thread
constexpr int PB_ENT = 2 * (PIS_PROB_BINS + 1);  // (class, bin) entries of one histogram
constexpr int PB_TOPQ = 64 * (PIS_PROB_BINS - 1) + 1;  // the smallest q of bin 1024
static_assert(PIS_PROB_QBITS == 16 && PIS_PROB_BINS == 1024, "bin = (q + 63) >> 6");
// packed words: (pixels a copy can see) * 63 below 2^18 for the two-copy form, counts below 2^14
static_assert((PB_PIX / 2 + 6) * 63 < (1 << 18) && PB_PIX / 2 + 6 < (1 << 14), "packed histogram word overflows");
static_assert((long long)PB_PIX * 65536 < (1ll << 32), "a block's sum of q must fit uint32");

struct ProbArgs {
  const float* p;
  const float* t;
  int B, nblk;
  long long npx;
  uint2* part;                  // [B][nblk][PB_ENT] { count, sum q }
  unsigned long long* bex;      // [B][nblk][4] { sum q^2 class 0, class 1, n_nan, 0 }
  unsigned long long* table;    // [B][PB_ENT][2] (int64 bit patterns)
  unsigned long long* extra;    // [B][4]
};

struct ProbLane {
  unsigned long long s2_0, s2_1;            // per lane: sum of q^2 by class
  unsigned rt0, rt1;                        // per lane: sum of r' over the top bin by class
  unsigned c00, c01, ct0, ct1, nnan;        // wave-uniform: end-bin counts by class, NaN count
  int cur_key;                              // per lane: the open run, -1 none
  unsigned cur_val;
};

__device__ __forceinline__ unsigned long long prob_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
  return v;
}

// All 64 lanes of a wave call this together (ballots); `active` masks the lanes without a pixel.
template <bool ENDS, bool MERGE>
__device__ __forceinline__ void prob_pixel(ProbLane& s, unsigned* h, bool active, float pv, float tv) {
  // on the bit pattern, so that a denormal p is positive whatever the denormal mode: positive
  // and not NaN is 0 < bits <= +Inf
  const int bi = __float_as_int(pv);
  const bool pos = active && bi > 0 && bi <= 0x7f800000;
  const float x = pv * 65536.0f;
  int q = 0;
  if (pos) q = x >= 65536.0f ? 65536 : max((int)ceilf(x), 1);
  const bool cls = tv > 0.5f;  // NaN: class 0
  const int bin = (q + 63) >> 6;
  const unsigned long long qq = (unsigned long long)(unsigned)q * (unsigned)q;
  s.s2_0 += cls ? 0ull : qq;
  s.s2_1 += cls ? qq : 0ull;
  s.nnan += __popcll(__ballot(active && (bi & 0x7fffffff) > 0x7f800000));
  bool interior = active;
  if (ENDS) {
    const bool z = active && bin == 0, top = active && bin == PIS_PROB_BINS;
    const unsigned long long mz = __ballot(z), mt = __ballot(top), mc = __ballot(cls);
    s.c00 += __popcll(mz & ~mc);
    s.c01 += __popcll(mz & mc);
    s.ct0 += __popcll(mt & ~mc);
    s.ct1 += __popcll(mt & mc);
    const unsigned r1 = (unsigned)(q - PB_TOPQ);
    s.rt0 += (top && !cls) ? r1 : 0u;
    s.rt1 += (top && cls) ? r1 : 0u;
    interior = active && !z && !top;
  }
  if (interior) {
    const int key = (cls ? PIS_PROB_BINS + 1 : 0) + bin;
    const unsigned v = (1u << 18) + (bin ? (unsigned)(q - ((bin - 1) << 6) - 1) : 0u);
    if (MERGE) {
      if (key == s.cur_key) {
        s.cur_val += v;
      } else {
        if (s.cur_key >= 0) atomicAdd(&h[s.cur_key], s.cur_val);
        s.cur_key = key;
        s.cur_val = v;
      }
    } else {
      atomicAdd(&h[key], v);
    }
  }
}

template <bool ENDS, int NCOPY, bool MERGE>
__global__ __launch_bounds__(PB_THREADS) void prob_hist_kernel(ProbArgs a) {
  __shared__ unsigned hist[NCOPY * PB_ENT];
  __shared__ unsigned long long red[PB_THREADS / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned* h = hist + (wv & (NCOPY - 1)) * PB_ENT;
  const long long start = (long long)blockIdx.x * PB_PIX;
  const int n = (int)min((long long)PB_PIX, a.npx - start);  // >= 1: the grid has cdiv(npx, PB_PIX) blocks
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    for (int i = tid; i < NCOPY * PB_ENT; i += PB_THREADS) hist[i] = 0;
    __syncthreads();
    const float* ps = a.p + (size_t)b * a.npx + start;
    const float* ts = a.t + (size_t)b * a.npx + start;
    // float4 loads need p and t at the same offset from a 16-byte boundary; else everything is "head"
    const bool vec_ok = (((uintptr_t)ps ^ (uintptr_t)ts) & 15) == 0;
    const int head = vec_ok ? min(n, (int)(((16 - ((uintptr_t)ps & 15)) & 15) >> 2)) : n;
    const int nvec = (n - head) >> 2;  // <= PB_PIX / 4: at most two float4 of p and of t per thread
    const int tail0 = head + 4 * nvec, nsc = head + (n - tail0);
    ProbLane s{};
    s.cur_key = -1;
    // the next float4 pair is loaded while this one is counted (a rolled loop: unrolled, the ballot
    // form kept every pixel's masks live at once and spilled SGPRs)
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 pc = zero4, tc = zero4;
    if (tid < nvec) {
      pc = *(const f32x4*)(ps + head + 4 * tid);
      tc = *(const f32x4*)(ts + head + 4 * tid);
    }
#pragma unroll 1
    for (int i0 = 0; i0 < nvec; i0 += PB_THREADS) {  // nvec is block-uniform: whole waves take every trip
      const int in = i0 + PB_THREADS + tid;
      f32x4 pn = zero4, tn = zero4;
      if (in < nvec) {
        pn = *(const f32x4*)(ps + head + 4 * in);
        tn = *(const f32x4*)(ts + head + 4 * in);
      }
      const bool act = i0 + tid < nvec;
#pragma unroll
      for (int e = 0; e < 4; ++e) prob_pixel<ENDS, MERGE>(s, h, act, pc[e], tc[e]);
      pc = pn;
      tc = tn;
    }
    for (int j0 = 0; j0 < nsc; j0 += PB_THREADS) {  // nsc is block-uniform: whole waves take every trip
      const int j = j0 + tid;
      const bool act = j < nsc;
      const int idx = j < head ? j : tail0 + (j - head);
      prob_pixel<ENDS, MERGE>(s, h, act, act ? ps[idx] : 0.f, act ? ts[idx] : 0.f);
    }
    if (MERGE && s.cur_key >= 0) atomicAdd(&h[s.cur_key], s.cur_val);
    if (ENDS) {
      const unsigned r0 = (unsigned)prob_wave_sum(s.rt0), r1 = (unsigned)prob_wave_sum(s.rt1);
      if (lane == 0) {
        if (s.c00) atomicAdd(&h[0], s.c00 << 18);
        if (s.c01) atomicAdd(&h[PIS_PROB_BINS + 1], s.c01 << 18);
        if (s.ct0) atomicAdd(&h[PIS_PROB_BINS], (s.ct0 << 18) + r0);
        if (s.ct1) atomicAdd(&h[2 * PIS_PROB_BINS + 1], (s.ct1 << 18) + r1);
      }
    }
    const unsigned long long w0 = prob_wave_sum(s.s2_0), w1 = prob_wave_sum(s.s2_1);
    if (lane == 0) {
      red[wv][0] = w0;
      red[wv][1] = w1;
      red[wv][2] = s.nnan;
    }
    __syncthreads();
    const size_t blk = (size_t)b * a.nblk + blockIdx.x;
    uint2* out = a.part + blk * PB_ENT;
    for (int e = tid; e < PB_ENT; e += PB_THREADS) {
      unsigned cnt = 0, sr = 0;
#pragma unroll
      for (int c = 0; c < NCOPY; ++c) {
        const unsigned w = hist[c * PB_ENT + e];
        cnt += w >> 18;
        sr += w & 0x3ffffu;
      }
      const int bin = e >= PIS_PROB_BINS + 1 ? e - (PIS_PROB_BINS + 1) : e;
      out[e] = make_uint2(cnt, bin ? cnt * (unsigned)(64 * (bin - 1) + 1) + sr : 0u);
    }
    if (tid < 4) {
      unsigned long long v = 0;
      if (tid < 3)
        for (int w = 0; w < PB_THREADS / 64; ++w) v += red[w][tid];
      a.bex[blk * 4 + tid] = v;
    }
    __syncthreads();
  }
}

constexpr int PROB_SUM_N = PB_ENT + 4;  // entries of the table, then the four words of extra

// 64 entries per block; the four waves take every fourth partial each, eight loads in flight per lane
__global__ __launch_bounds__(256) void prob_sum_kernel(ProbArgs a) {
  __shared__ unsigned long long sm[3][64][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const size_t blk0 = (size_t)b * a.nblk;
    unsigned long long s0 = 0, s1 = 0;
    if (e < PB_ENT) {
#pragma unroll 8
      for (int k = wv; k < a.nblk; k += 4) {
        const uint2 v = a.part[(blk0 + k) * PB_ENT + e];
        s0 += v.x;
        s1 += v.y;
      }
    } else if (e < PROB_SUM_N) {
#pragma unroll 8
      for (int k = wv; k < a.nblk; k += 4) s0 += a.bex[(blk0 + k) * 4 + (e - PB_ENT)];
    }
    if (wv) {
      sm[wv - 1][lane][0] = s0;
      sm[wv - 1][lane][1] = s1;
    }
    __syncthreads();
    if (wv == 0) {
      for (int w = 0; w < 3; ++w) {
        s0 += sm[w][lane][0];
        s1 += sm[w][lane][1];
      }
      if (e < PB_ENT) {
        a.table[((size_t)b * PB_ENT + e) * 2] = s0;
        a.table[((size_t)b * PB_ENT + e) * 2 + 1] = s1;
      } else if (e < PROB_SUM_N) {
        a.extra[(size_t)b * 4 + (e - PB_ENT)] = s0;
      }
    }
    __syncthreads();
  }
}

static size_t prob_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace pis

using namespace pis;

// per block of PB_PIX pixels: its widened histogram (2050 entries of 8 bytes) and four 8-byte sums
extern "C" size_t pis_probability_ws(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > PROB_MAX || W > PROB_MAX) return 0;
  const size_t nblk = (size_t)cdiv((int64_t)H * W, PB_PIX);
  return prob_align((size_t)B * nblk * PB_ENT * sizeof(uint2)) + prob_align((size_t)B * nblk * 4 * 8);
}

extern "C" int pis_probability_table(const float* p, const float* t, int B, int H, int W, int64_t* table,
                                     int64_t* extra, void* ws, size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(p && t && table && extra, "pis_probability_table: p, t, table or extra is NULL");
  PIS_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= PROB_MAX && W <= PROB_MAX,
                "pis_probability_table: bad shape B=%d H=%d W=%d (B >= 1, 1 <= H, W <= %d)", B, H, W, PROB_MAX);
  PIS_CHECK_ARG((((uintptr_t)p | (uintptr_t)t) & 3) == 0 && (((uintptr_t)table | (uintptr_t)extra) & 7) == 0,
                "pis_probability_table: p, t need 4-byte and table, extra 8-byte alignment");
  PIS_CHECK_ARG(ws != nullptr, "pis_probability_table: ws is NULL");
  PIS_CHECK_ARG(((uintptr_t)ws & 7) == 0, "pis_probability_table: ws needs 8-byte alignment");
  if (ws_bytes < pis_probability_ws(B, H, W)) {
    set_error("pis_probability_table: workspace too small (%zu < %zu bytes)", ws_bytes, pis_probability_ws(B, H, W));
    return PIS_ERR_WORKSPACE;
  }
  ProbArgs a{};
  a.p = p; a.t = t; a.B = B;
  a.npx = (long long)H * W;
  a.nblk = (int)cdiv(a.npx, PB_PIX);
  a.part = (uint2*)ws;
  a.bex = (unsigned long long*)((char*)ws + prob_align((size_t)B * a.nblk * PB_ENT * sizeof(uint2)));
  a.table = (unsigned long long*)table;
  a.extra = (unsigned long long*)extra;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)a.nblk, (unsigned)std::min(B, 65535));
  const double bytes = 8.0 * (double)B * (double)a.npx;
  const int v = tune_get(PIS_TUNE_PROB_VARIANT);
  launch_hook("prob_hist", 0, s, bytes);
#define PIS_PROB(E, C, M) hipLaunchKernelGGL((prob_hist_kernel<E, C, M>), grid, dim3(PB_THREADS), 0, s, a)
  switch (v & 7) {  // bit 0: end bins by ballot, bit 1: four histograms, bit 2: no merging
    case 0: PIS_PROB(false, 2, true); break;
    case 1: PIS_PROB(true, 2, true); break;
    case 2: PIS_PROB(false, 4, true); break;
    case 3: PIS_PROB(true, 4, true); break;
    case 4: PIS_PROB(false, 2, false); break;
    case 5: PIS_PROB(true, 2, false); break;
    case 6: PIS_PROB(false, 4, false); break;
    default: PIS_PROB(true, 4, false); break;
  }
#undef PIS_PROB
  launch_hook("prob_hist", 1, s, bytes);
  int rc = launch_status("prob_hist");
  if (rc) return rc;
  launch_hook("prob_sum", 0, s, bytes);
  hipLaunchKernelGGL(prob_sum_kernel, dim3((unsigned)cdiv(PROB_SUM_N, 64), (unsigned)std::min(B, 65535)), dim3(256),
                     0, s, a);
  launch_hook("prob_sum", 1, s, bytes);
  return launch_status("prob_sum");
}
