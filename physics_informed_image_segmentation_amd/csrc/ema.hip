// Exponential moving average of the weights inside the AdamW launch, and the exchange of two arenas'
// contents (include/pis_capi.h). Both are HBM-streaming: 16-byte loads and stores, a
// scalar tail, a grid-stride loop; no LDS, no atomics.
#include "common.h"

#include <cmath>

namespace pis {

struct EmaGradRecord {  // include/pis_capi.h: pis_grad_sumsq's 'record'
  float coef;
  int apply;
  double norm;
};

// torch's lerp: e + w (p - e) below w = 0.5, p - (p - e)(1 - w) from there on, so that w = 0 keeps e
// and w = 1 gives p without a rounding
__device__ __forceinline__ float ema_lerp(float e, float p, float w, float omw) {
  const float d = p - e;
  return w < 0.5f ? e + w * d : p - d * omw;
}

// adamw_kernel (csrc/pointwise.hip) or, with REC, adamw_clipped_kernel (csrc/gradnorm.hip): the same
// expressions in the same order for p, m and v; then the average moves towards the new p, which the
// thread still holds in registers
template <bool REC>
__global__ void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, float* __restrict__ ema, int64_t n, float decay,
                                 float omb1, float beta2, float omb2, float eps, float step_size,
                                 float bc2_sqrt, float grad_scale, float w, float omw,
                                 const EmaGradRecord* __restrict__ rec) {
  float coef = 1.f;
  if (REC) {
    if (rec->apply == 0) return;  // a skipped step: the average does not move either
    coef = rec->coef;
  }
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + (n - n4 * 4);
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n4) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
      f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = REC ? (gg[j] * grad_scale) * coef : gg[j] * grad_scale;
        pp[j] = pp[j] * decay;
        mm[j] = mm[j] + omb1 * (gj - mm[j]);
        vv[j] = vv[j] * beta2 + omb2 * gj * gj;
        const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
        pp[j] = pp[j] + (-step_size) * (mm[j] / denom);
        ee[j] = ema_lerp(ee[j], pp[j], w, omw);
      }
      reinterpret_cast<f32x4*>(p)[i] = pp;
      reinterpret_cast<f32x4*>(m)[i] = mm;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      reinterpret_cast<f32x4*>(ema)[i] = ee;
    } else {
      const int64_t k = n4 * 4 + (i - n4);
      const float gj = REC ? (g[k] * grad_scale) * coef : g[k] * grad_scale;
      float pp = p[k] * decay;
      const float mm = m[k] + omb1 * (gj - m[k]);
      const float vv = v[k] * beta2 + omb2 * gj * gj;
      pp = pp + (-step_size) * (mm / (sqrtf(vv) / bc2_sqrt + eps));
      p[k] = pp; m[k] = mm; v[k] = vv;
      ema[k] = ema_lerp(ema[k], pp, w, omw);
    }
  }
}

// a <-> b as raw 32-bit words: NaN payloads and the sign of zero pass through untouched
__global__ void arena_exchange_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4 + (n - n4 * 4);
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n4) {
      const u32x4 x = reinterpret_cast<u32x4*>(a)[i];
      const u32x4 y = reinterpret_cast<u32x4*>(b)[i];
      reinterpret_cast<u32x4*>(a)[i] = y;
      reinterpret_cast<u32x4*>(b)[i] = x;
    } else {
      const int64_t k = n4 * 4 + (i - n4);
      const uint32_t x = a[k], y = b[k];
      a[k] = y;
      b[k] = x;
    }
  }
}

// the grid of pis_adamw_step: a thread per float4 (and per tail element), at most 8192 blocks
static int stream_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n / 4 + 4, 256), 8192)); }

}  // namespace pis

using namespace pis;

extern "C" int pis_adamw_step_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                  double lr, double beta1, double beta2, double eps, double weight_decay,
                                  double step_size, double bc2_sqrt, double grad_scale, double ema_weight,
                                  const void* record, pis_stream_t stream) {
  // the scalars are rounded as in pis_adamw_step
  PIS_CHECK_ARG(p && g && m && v && ema && n >= 0, "pis_adamw_step_ema: bad arguments");
  PIS_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16 == 0,
                "pis_adamw_step_ema: buffers must be 16-byte aligned");
  PIS_CHECK_ARG((uintptr_t)record % 8 == 0, "pis_adamw_step_ema: record must be 8-byte aligned");
  PIS_CHECK_ARG(ema_weight >= 0.0 && ema_weight <= 1.0, "pis_adamw_step_ema: ema_weight must be in [0, 1]");  // NaN fails
  if (n == 0) return PIS_OK;
  const float decay = (float)(1.0 - lr * weight_decay);
  const float omb1 = (float)(1.0 - beta1);
  const float omb2 = (float)(1.0 - beta2);
  const float w = (float)ema_weight;
  const float omw = 1.f - w;
  const dim3 grid(stream_grid(n));
  if (record)
    hipLaunchKernelGGL(adamw_ema_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n,
                       decay, omb1, (float)beta2, omb2, (float)eps, (float)step_size, (float)bc2_sqrt,
                       (float)grad_scale, w, omw, (const EmaGradRecord*)record);
  else
    hipLaunchKernelGGL(adamw_ema_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n,
                       decay, omb1, (float)beta2, omb2, (float)eps, (float)step_size, (float)bc2_sqrt,
                       (float)grad_scale, w, omw, (const EmaGradRecord*)nullptr);
  return launch_status("adamw_ema");
}

extern "C" int pis_arena_exchange(float* a, float* b, int64_t n, pis_stream_t stream) {
  PIS_CHECK_ARG(a && b && n >= 0, "pis_arena_exchange: bad arguments");
  PIS_CHECK_ARG(((uintptr_t)a | (uintptr_t)b) % 16 == 0, "pis_arena_exchange: buffers must be 16-byte aligned");
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  PIS_CHECK_ARG(ua != ub && (ua < ub ? ub - ua >= bytes : ua - ub >= bytes),
                "pis_arena_exchange: the two ranges must not be equal or overlap");
  if (n == 0) return PIS_OK;
  hipLaunchKernelGGL(arena_exchange_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream,
                     (uint32_t*)a, (uint32_t*)b, n);
  return launch_status("arena_exchange");
}
