// Global-norm gradient clipping and the non-finite step guard (include/pis_capi.h):
// a deterministic float64 sum of squares over the segments of the flat gradient arena, a finalize
// launch that leaves the clip coefficient and the skip decision on the device, and the AdamW update
// that reads them there. HBM-streaming: one 16-byte read per four gradients, nothing written back.
#include "common.h"

#include <cmath>

namespace pis {

constexpr int GN_SLICE = 8192;           // floats per work item: one block, 8 float4 per thread
constexpr int GN_SLICE4 = GN_SLICE / 4;  // float4 per full slice
constexpr int GN_FIN_THREADS = 1024;     // finalize: 16 waves, a wave per segment

struct GradRecord {  // include/pis_capi.h: 'record'
  float coef;
  int apply;
  double norm;
};

// work items of a segment: ceil(len / GN_SLICE); 0 for a segment the contract does not allow
__device__ __forceinline__ int64_t gn_items(int64_t off, int64_t len) {
  return (off >= 0 && (off & 3) == 0 && len >= 1) ? (len + GN_SLICE - 1) / GN_SLICE : 0;
}

// Item `it` is slice (it - first(seg)) of segment seg, first(seg) the item count of the segments
// before it: a function of the table alone. A block walks the table once (wave-uniform, scalar
// loads) while it strides over the items; what it sums for an item, and in which order, does not
// depend on the grid: thread t takes float4 t, t + 256, ... of the slice in ascending order, the
// last slice's 1-3 tail elements go to threads 0-2, then the xor butterfly of the wave, then the
// four waves as (w0 + w1) + (w2 + w3). Squares of fp32 values are exact in float64.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g,
                                                         const int64_t* __restrict__ seg_off,
                                                         const int64_t* __restrict__ seg_len, int n_seg,
                                                         double* __restrict__ partial, int64_t cap) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  int seg = 0;
  int64_t first = 0;
  int64_t cnt = gn_items(seg_off[0], seg_len[0]);
  for (int64_t it = blockIdx.x; it < cap; it += gridDim.x) {  // partial[] holds cap items
    while (seg < n_seg && it >= first + cnt) {
      first += cnt;
      ++seg;
      if (seg < n_seg) cnt = gn_items(seg_off[seg], seg_len[seg]);
    }
    if (seg >= n_seg) break;
    const int64_t start = (it - first) * GN_SLICE;
    const int64_t left = seg_len[seg] - start;  // >= 1
    const int len = (int)(left < GN_SLICE ? left : GN_SLICE);
    const float* base = g + seg_off[seg] + start;  // 16-byte aligned: g is, offsets and slices are multiples of 4
    const f32x4* b4 = reinterpret_cast<const f32x4*>(base);
    const int n4 = len >> 2;
    double acc = 0.0;
    if (n4 == GN_SLICE4) {  // a full slice: all eight loads in flight before the first sum
      f32x4 x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = b4[tid + 256 * k];
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = (double)x[k][j];
          acc = fma(d, d, acc);
        }
    } else {
      for (int i = tid; i < n4; i += 256) {
        const f32x4 x = b4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = (double)x[j];
          acc = fma(d, d, acc);
        }
      }
    }
    if (tid < len - 4 * n4) {  // scalar tail of the segment's last slice
      const double d = (double)base[4 * n4 + tid];
      acc = fma(d, d, acc);
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[it] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
  }
}

// One block. Per chunk of 1024 segments: an integer scan of the item counts gives every segment its
// first item; a wave per segment adds the segment's partials (lane l takes partials l, l + 64, ... in
// ascending order, then the xor butterfly); thread 0 adds the chunk's segment sums to the total in
// segment order. Then the record and the statistics.
__global__ __launch_bounds__(GN_FIN_THREADS) void grad_finalize_kernel(
    const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len, int n_seg,
    const double* __restrict__ partial, int64_t cap, double grad_scale, double max_norm, int flags,
    double* __restrict__ seg_sumsq, GradRecord* __restrict__ rec, double* __restrict__ stats) {
  __shared__ int64_t scan[GN_FIN_THREADS];
  __shared__ int64_t sfirst[GN_FIN_THREADS];
  __shared__ int scnt[GN_FIN_THREADS];
  __shared__ double ssum[GN_FIN_THREADS];
  __shared__ int64_t carry;
  __shared__ double total_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    carry = 0;
    total_s = 0.0;
  }
  __syncthreads();
  for (int base = 0; base < n_seg; base += GN_FIN_THREADS) {
    const int s = base + tid;
    const int64_t cnt = s < n_seg ? gn_items(seg_off[s], seg_len[s]) : 0;
    scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < GN_FIN_THREADS; d <<= 1) {  // inclusive scan (integers: any order is exact)
      const int64_t t = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += t;
      __syncthreads();
    }
    sfirst[tid] = carry + scan[tid] - cnt;
    scnt[tid] = (int)cnt;  // a segment has fewer than 2^31 slices: its length fits the arena
    __syncthreads();
    const int live = n_seg - base < GN_FIN_THREADS ? n_seg - base : GN_FIN_THREADS;
    for (int k = wave; k < live; k += GN_FIN_THREADS / 64) {
      const int64_t f = sfirst[k];
      const int c = scnt[k];
      double a = 0.0;
      if (c == 0 || f + c > cap) {
        a = __builtin_nan("");  // a segment outside the contract, or a workspace too small for the table
      } else {
        for (int i = lane; i < c; i += 64) a += partial[f + i];
        a = wave_sum_d(a);
      }
      if (lane == 0) {
        seg_sumsq[base + k] = a;
        ssum[k] = a;
      }
    }
    __syncthreads();
    if (tid == 0) {
      double t = total_s;
      for (int k = 0; k < live; ++k) t += ssum[k];
      total_s = t;
      carry += scan[GN_FIN_THREADS - 1];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool short_ws = carry > cap;
    const double total = short_ws ? __builtin_nan("") : total_s;
    const double norm = sqrt(total) * grad_scale;
    const bool finite = isfinite(total);
    double c = 1.0;
    if (max_norm > 0.0) {
      const double q = max_norm / (norm + 1e-6);  // torch.nn.utils.clip_grad_norm_
      c = q > 1.0 ? 1.0 : q;                      // a NaN stays a NaN, as torch.clamp(max=1) keeps it
    }
    const float coef = (float)c;
    const int apply = short_ws ? 0 : ((flags & PIS_GRADNORM_SKIP_NONFINITE) ? (finite ? 1 : 0) : 1);
    rec->coef = coef;
    rec->apply = apply;
    rec->norm = norm;
    stats[0] += 1.0;
    if (apply && coef < 1.f) stats[1] += 1.0;
    if (!apply) stats[2] += 1.0;
    if (finite) {
      stats[3] += 1.0;
      stats[4] += norm;
      stats[5] = norm > stats[5] ? norm : stats[5];
    }
    stats[6] = norm;
    stats[7] = (double)coef;
  }
}

// adamw_kernel (csrc/pointwise.hip) with g' = (g * grad_scale) * coef; coef and apply come from the
// record pis_grad_sumsq left on the device (a wave-uniform address: one scalar load per wave)
__global__ void adamw_clipped_kernel(float* __restrict__ p, const float* __restrict__ g,
                                     float* __restrict__ m, float* __restrict__ v, int64_t n, float decay,
                                     float omb1, float beta2, float omb2, float eps, float step_size,
                                     float bc2_sqrt, float grad_scale, const GradRecord* __restrict__ rec) {
  if (rec->apply == 0) return;
  const float coef = rec->coef;
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + (n - n4 * 4);
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n4) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
      f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = (gg[j] * grad_scale) * coef;
        pp[j] = pp[j] * decay;
        mm[j] = mm[j] + omb1 * (gj - mm[j]);
        vv[j] = vv[j] * beta2 + omb2 * gj * gj;
        const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
        pp[j] = pp[j] + (-step_size) * (mm[j] / denom);
      }
      reinterpret_cast<f32x4*>(p)[i] = pp;
      reinterpret_cast<f32x4*>(m)[i] = mm;
      reinterpret_cast<f32x4*>(v)[i] = vv;
    } else {
      const int64_t k = n4 * 4 + (i - n4);
      const float gj = (g[k] * grad_scale) * coef;
      float pp = p[k] * decay;
      const float mm = m[k] + omb1 * (gj - m[k]);
      const float vv = v[k] * beta2 + omb2 * gj * gj;
      pp = pp + (-step_size) * (mm / (sqrtf(vv) / bc2_sqrt + eps));
      p[k] = pp; m[k] = mm; v[k] = vv;
    }
  }
}

}  // namespace pis

using namespace pis;

extern "C" size_t pis_grad_sumsq_ws(int n_seg, int64_t n_total) {
  if (!(n_seg > 0 && n_total >= n_seg)) {  // a size query has no error code: 0 bytes
    set_error("pis_grad_sumsq_ws: n_seg > 0 and n_total >= n_seg required");
    return 0;
  }
  // sum of ceil(len / slice) <= n_seg + (sum of len) / slice; one float64 partial per item
  return (size_t)(n_seg + n_total / GN_SLICE) * sizeof(double);
}

extern "C" int pis_grad_sumsq(const float* g, const int64_t* seg_off, const int64_t* seg_len, int n_seg,
                              double grad_scale, double max_norm, int flags, double* seg_sumsq,
                              void* record, void* stats, void* ws, size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(g && seg_off && seg_len && seg_sumsq && record && stats && n_seg > 0,
                "pis_grad_sumsq: bad arguments");
  PIS_CHECK_ARG(((uintptr_t)g | (uintptr_t)ws) % 16 == 0, "pis_grad_sumsq: g and ws must be 16-byte aligned");
  PIS_CHECK_ARG(((uintptr_t)seg_off | (uintptr_t)seg_len | (uintptr_t)seg_sumsq | (uintptr_t)record |
                 (uintptr_t)stats) % 8 == 0,
                "pis_grad_sumsq: seg_off, seg_len, seg_sumsq, record and stats must be 8-byte aligned");
  PIS_CHECK_ARG((flags & ~PIS_GRADNORM_SKIP_NONFINITE) == 0, "pis_grad_sumsq: unknown flags");
  PIS_CHECK_ARG(ws && ws_bytes >= pis_grad_sumsq_ws(n_seg, n_seg), "pis_grad_sumsq: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t cap = (int64_t)(ws_bytes / sizeof(double));
  // at most 2048 blocks (8 per CU: all resident at once), each taking the same number of items to
  // within one: a grid of one block per item runs the model's 2533 items as a full round and a
  // quarter-full one. The sums do not depend on the grid.
  const int64_t rounds = cdiv(cap, 2048);
  const int grid = (int)cdiv(cap, rounds);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, s, g, seg_off, seg_len, n_seg, (double*)ws, cap);
  int rc = launch_status("grad_sumsq");
  if (rc) return rc;
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(GN_FIN_THREADS), 0, s, seg_off, seg_len, n_seg,
                     (const double*)ws, cap, grad_scale, max_norm, flags, seg_sumsq, (GradRecord*)record,
                     (double*)stats);
  return launch_status("grad_finalize");
}

extern "C" int pis_adamw_step_clipped(float* p, const float* g, float* m, float* v, int64_t n, double lr,
                                      double beta1, double beta2, double eps, double weight_decay,
                                      double step_size, double bc2_sqrt, double grad_scale,
                                      const void* record, pis_stream_t stream) {
  // the scalars are rounded as in pis_adamw_step
  PIS_CHECK_ARG(p && g && m && v && record && n >= 0, "pis_adamw_step_clipped: bad arguments");
  PIS_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0,
                "pis_adamw_step_clipped: buffers must be 16-byte aligned");
  PIS_CHECK_ARG((uintptr_t)record % 8 == 0, "pis_adamw_step_clipped: record must be 8-byte aligned");
  if (n == 0) return PIS_OK;
  const float decay = (float)(1.0 - lr * weight_decay);
  const float omb1 = (float)(1.0 - beta1);
  const float omb2 = (float)(1.0 - beta2);
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n / 4 + 4, 256), 8192));
  hipLaunchKernelGGL(adamw_clipped_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     decay, omb1, (float)beta2, omb2, (float)eps, (float)step_size, (float)bc2_sqrt,
                     (float)grad_scale, (const GradRecord*)record);
  return launch_status("adamw_clipped");
}
