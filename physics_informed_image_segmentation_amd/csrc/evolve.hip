// PDE evolution of a probability map and its per-image physics quantities (include/pis_capi.h,
// DESIGN.md §14; pde.py:evolve_np / energies_np are the definitions of record, restated there in
// float32 numpy and agreeing bit for bit).
//
//   pis_pde_evolve     `steps` explicit Euler steps of u_t = D lap(u) + k u (1 - u) (u - a) + mu (u0 - u)
//                      on the reflect-padded 5-point stencil, T steps per launch inside LDS
//   pis_pde_energies   per image: mean squared reaction-diffusion residual, mean phase-field energy
//                      density, count of interface pixels; float64 sums in a fixed order
//
// Temporal blocking: a block owns an EV_TH x EV_TW output tile. It loads the tile plus a T-wide halo
// through the reflect index (any number of periods: an image may be narrower than the halo), then
// steps T times between two LDS planes; after step s every element at least s rings inside the
// plane is exact, so the tile (T rings inside) is exact after T steps. A step is one sweep over a
// linear range of the plane, rows [s, PH - s): the elements of ring s - 1 at the two row ends take
// a neighbour from the adjacent row and hold garbage, which no exact element ever reads (an exact
// element of step s + 1 reads only elements at least s rings inside). The step's summation order,
// (up + dn) + (lf + rt), makes it commute with the reflections, so the reflect extension of the
// field evolves to the reflect extension of the evolved field and the halo needs no exchange.
#include "common.h"

namespace pis {

constexpr int EV_TH = PIS_EVOLVE_TILE_H, EV_TW = PIS_EVOLVE_TILE_W;
constexpr int EV_THREADS = 256;

// the header's reflect(i, n), n >= 2, any number of periods out (infer.hip:tile_reflect)
__device__ __forceinline__ int ev_reflect(int i, int n) {
  const int p = 2 * n - 2;
  if ((unsigned)(i + (n - 1)) > (unsigned)(3 * n - 3)) {
    i %= p;
    if (i < 0) i += p;
  }
  i = i < 0 ? -i : i;
  return i >= n ? p - i : i;
}

// one correctly rounded operation each, which no neighbour fuses with (cache.hip, infer.hip)
__device__ __forceinline__ float ev_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float ev_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float ev_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

struct EvolveArgs {
  const float* src;  // the map this launch reads
  const float* u0;   // MU only
  float* dst;        // never src or u0
  uint8_t* mask;     // the last launch only, may be NULL
  int H, W, nbx, nby, h;  // h <= T steps in this launch
  float D, k, a, mu, dt, thr;
};

__device__ __forceinline__ float ev_lap(float c, float up, float dn, float lf, float rt) {
  return ev_sub(ev_add(ev_add(up, dn), ev_add(lf, rt)), ev_mul(4.f, c));
}
__device__ __forceinline__ float ev_react(float c, float a) {
  return ev_mul(ev_mul(c, ev_sub(1.f, c)), ev_sub(c, a));
}

template <bool MU, bool CLAMP, int T>
__global__ __launch_bounds__(EV_THREADS) void pde_evolve_kernel(EvolveArgs g) {
  constexpr int PH = EV_TH + 2 * T, PW = EV_TW + 2 * T, PN = PH * PW;
  __shared__ float plane[2][PN];
  __shared__ float plane0[MU ? PN : 1];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % g.nbx, by = (blockIdx.x / g.nbx) % g.nby, b = blockIdx.x / (g.nbx * g.nby);
  const int y0 = by * EV_TH, x0 = bx * EV_TW;
  const int H = g.H, W = g.W;
  const int64_t img = (int64_t)b * H * W;
  const float* __restrict__ src = g.src + img;

  for (int p = tid; p < PN; p += EV_THREADS) {
    const int ly = p / PW, lx = p - ly * PW;
    const int64_t at = (int64_t)ev_reflect(y0 - T + ly, H) * W + ev_reflect(x0 - T + lx, W);
    plane[0][p] = src[at];
    if (MU) plane0[p] = g.u0[img + at];
  }
  __syncthreads();

  int cur = 0;
  for (int s = 1; s <= g.h; ++s) {
    const float* __restrict__ in = plane[cur];
    float* __restrict__ out = plane[cur ^ 1];
    const int end = (PH - s) * PW - s;
    for (int p = s * PW + s + tid; p < end; p += EV_THREADS) {
      const float c = in[p];
      const float lap = ev_lap(c, in[p - PW], in[p + PW], in[p - 1], in[p + 1]);
      float t = ev_mul(g.D, lap);
      t = ev_add(t, ev_mul(g.k, ev_react(c, g.a)));
      if (MU) t = ev_add(t, ev_mul(g.mu, ev_sub(plane0[p], c)));
      float n = ev_add(c, ev_mul(g.dt, t));
      if (CLAMP) {
        n = n < 0.f ? 0.f : n;
        n = n > 1.f ? 1.f : n;
      }
      out[p] = n;
    }
    __syncthreads();
    cur ^= 1;
  }

  // the tile, in runs of 4 floats that start at multiples of 4 of the map's linear index: a whole
  // run inside the tile row and the image is one 16-byte store (dst is 16-byte aligned), the rest
  // scalar. A row of EV_TW pixels touches at most EV_TW / 4 + 1 such runs.
  const float* __restrict__ fin = plane[cur];
  constexpr int RUNS = EV_TW / 4 + 1;
  const int xe = min(x0 + EV_TW, W);
  for (int i = tid; i < EV_TH * RUNS; i += EV_THREADS) {
    const int r = i / RUNS, q = i - r * RUNS;
    const int y = y0 + r;
    if (y >= H) break;  // i ascends with r
    const int64_t row = img + (int64_t)y * W;
    const int x = (int)(((row + x0) & ~(int64_t)3) - row) + 4 * q;  // first pixel of run q, may lie left of x0
    const float* __restrict__ lp = fin + (T + r) * PW + (T - x0);
    if (x >= x0 && x + 4 <= xe) {
      const f32x4 v{lp[x], lp[x + 1], lp[x + 2], lp[x + 3]};
      *(f32x4*)(g.dst + row + x) = v;
      if (g.mask) {
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (v[j] > g.thr ? 1u : 0u) << (8 * j);
        *(uint32_t*)(g.mask + row + x) = m;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xx = x + j;
        if (xx >= x0 && xx < xe) {
          const float v = lp[xx];
          g.dst[row + xx] = v;
          if (g.mask) g.mask[row + xx] = v > g.thr ? 1 : 0;
        }
      }
    }
  }
}

// ---- energies -----------------------------------------------------------------------------------
constexpr int EN_ROWS = 8;  // rows of a band: one block

struct EnergyArgs {
  const float* u;
  double* part;    // [B * nb][2]
  int64_t* cnt;    // [B * nb]
  int H, W, nb;
  float D, a, he, ie;
};

// A block sums a band of EN_ROWS rows of one image: thread t takes pixels t, t + 256, ... of the band
// in ascending order, then the xor butterfly of the wave, then the four waves as (w0 + w1) + (w2 + w3)
// (gradnorm.hip's order). The neighbours come through the reflect index (a one-row halo above and
// below the band, read from cache).
__global__ __launch_bounds__(256) void pde_energy_kernel(EnergyArgs g) {
  __shared__ double red[4][2];
  __shared__ int64_t redc[4];
  const int tid = threadIdx.x;
  const int band = blockIdx.x % g.nb, b = blockIdx.x / g.nb;
  const int H = g.H, W = g.W;
  const float* __restrict__ u = g.u + (int64_t)b * H * W;
  const int ya = band * EN_ROWS, rows = min(EN_ROWS, H - ya);
  double s_rd = 0.0, s_pf = 0.0;
  int64_t n_if = 0;
  for (int p = tid; p < rows * W; p += 256) {
    const int r = p / W, x = p - r * W, y = ya + r;
    const int yu = y == 0 ? 1 : y - 1, yd = y == H - 1 ? H - 2 : y + 1;
    const int xl = x == 0 ? 1 : x - 1, xr = x == W - 1 ? W - 2 : x + 1;
    const float c = u[(int64_t)y * W + x];
    const float up = u[(int64_t)yu * W + x], dn = u[(int64_t)yd * W + x];
    const float lf = u[(int64_t)y * W + xl], rt = u[(int64_t)y * W + xr];
    const float res = ev_add(ev_mul(g.D, ev_lap(c, up, dn, lf, rt)), ev_react(c, g.a));
    const float gx = ev_mul(0.5f, ev_sub(rt, lf)), gy = ev_mul(0.5f, ev_sub(dn, up));
    const float gg = ev_add(ev_mul(gx, gx), ev_mul(gy, gy));
    const float omc = ev_sub(1.f, c);
    const float w = ev_mul(ev_mul(c, c), ev_mul(omc, omc));
    const float e = ev_add(ev_mul(g.he, gg), ev_mul(g.ie, w));
    const double rd = (double)res;
    s_rd += rd * rd;  // exact products; fused or not, the sum rounds once
    s_pf += (double)e;
    n_if += (0.1f < c && c < 0.9f) ? 1 : 0;
  }
  s_rd = wave_sum_d(s_rd);
  s_pf = wave_sum_d(s_pf);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_if += __shfl_xor(n_if, off, 64);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s_rd;
    red[tid >> 6][1] = s_pf;
    redc[tid >> 6] = n_if;
  }
  __syncthreads();
  if (tid == 0) {
    g.part[2 * (int64_t)blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    g.part[2 * (int64_t)blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    g.cnt[blockIdx.x] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
  }
}

// one wave per image: lane l adds bands l, l + 64, ... in ascending order, then the xor butterfly
__global__ __launch_bounds__(64) void pde_energy_reduce_kernel(const double* __restrict__ part,
                                                               const int64_t* __restrict__ cnt, int nb, double n_px,
                                                               double* __restrict__ out_f, int64_t* __restrict__ out_i) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double rd = 0.0, pf = 0.0;
  int64_t n = 0;
  for (int i = lane; i < nb; i += 64) {
    rd += part[2 * ((int64_t)b * nb + i)];
    pf += part[2 * ((int64_t)b * nb + i) + 1];
    n += cnt[(int64_t)b * nb + i];
  }
  rd = wave_sum_d(rd);
  pf = wave_sum_d(pf);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (lane == 0) {
    out_f[2 * b] = rd / n_px;
    out_f[2 * b + 1] = pf / n_px;
    out_i[b] = n;
  }
}

}  // namespace pis

using namespace pis;

static size_t ev_map_bytes(int B, int H, int W) { return ((size_t)B * H * W * sizeof(float) + 15) / 16 * 16; }

static bool ev_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 2 && H <= 4096 && W >= 2 && W <= 4096 &&
         (int64_t)B * cdiv(H, EV_TH) * cdiv(W, EV_TW) <= 0x7fffffffLL;
}

static int ev_T() {
  const int t = tune_get(PIS_TUNE_EVOLVE_T);
  return (t == 1 || t == 2 || t == 4 || t == 8) ? t : 0;
}

extern "C" size_t pis_pde_evolve_ws(int B, int H, int W, int steps) {
  if (!ev_shape_ok(B, H, W) || steps < 0 || steps > PIS_EVOLVE_MAX_STEPS) {  // a size query has no error code: 0 bytes
    set_error("pis_pde_evolve_ws: B >= 1, 2 <= H, W <= 4096 and 0 <= steps <= %d are needed", PIS_EVOLVE_MAX_STEPS);
    return 0;
  }
  // two scratch maps whatever T is (the tune key may change between the query and the call)
  return 2 * ev_map_bytes(B, H, W);
}

template <bool MU, bool CLAMP>
static void ev_launch(int T, unsigned blocks, hipStream_t s, const EvolveArgs& a) {
  switch (T) {
    case 1: hipLaunchKernelGGL((pde_evolve_kernel<MU, CLAMP, 1>), dim3(blocks), dim3(EV_THREADS), 0, s, a); break;
    case 2: hipLaunchKernelGGL((pde_evolve_kernel<MU, CLAMP, 2>), dim3(blocks), dim3(EV_THREADS), 0, s, a); break;
    case 4: hipLaunchKernelGGL((pde_evolve_kernel<MU, CLAMP, 4>), dim3(blocks), dim3(EV_THREADS), 0, s, a); break;
    default: hipLaunchKernelGGL((pde_evolve_kernel<MU, CLAMP, 8>), dim3(blocks), dim3(EV_THREADS), 0, s, a); break;
  }
}

// [p, p + np) meets [q, q + nq)
static bool ev_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

extern "C" int pis_pde_evolve(const float* u, const float* u0, float* out, uint8_t* mask, int B, int H, int W, float D,
                              float k, float a, float mu, float dt, int steps, int flags, float thr, void* ws,
                              size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(u && out, "pis_pde_evolve: u or out is NULL");
  PIS_CHECK_ARG(ev_shape_ok(B, H, W), "pis_pde_evolve: B = %d, H = %d, W = %d: B >= 1 and 2 <= H, W <= 4096 are needed", B,
                H, W);
  PIS_CHECK_ARG(steps >= 0 && steps <= PIS_EVOLVE_MAX_STEPS, "pis_pde_evolve: steps = %d: [0, %d] is needed", steps,
                PIS_EVOLVE_MAX_STEPS);
  PIS_CHECK_ARG((flags & ~PIS_EVOLVE_CLAMP) == 0, "pis_pde_evolve: unknown flags 0x%x", flags);
  PIS_CHECK_ARG(D >= 0.f && k >= 0.f && mu >= 0.f && a > 0.f && a < 1.f && dt > 0.f,
                "pis_pde_evolve: D >= 0, k >= 0, mu >= 0, 0 < a < 1 and dt > 0 are needed");
  PIS_CHECK_ARG((double)dt * (4.0 * D + (double)k + (double)mu) <= 1.0,
                "pis_pde_evolve: dt (4 D + k + mu) = %g exceeds 1: the explicit step is not monotone",
                (double)dt * (4.0 * D + (double)k + (double)mu));
  PIS_CHECK_ARG(thr == thr, "pis_pde_evolve: thr is NaN");
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  PIS_CHECK_ARG(((uintptr_t)u | (uintptr_t)u0 | (uintptr_t)out | (uintptr_t)ws) % 16 == 0 && (uintptr_t)mask % 4 == 0,
                "pis_pde_evolve: u, u0, out and ws must be 16-byte aligned, mask 4-byte aligned");
  PIS_CHECK_ARG(!ev_overlap(out, bytes, u, bytes) && !(u0 && ev_overlap(out, bytes, u0, bytes)),
                "pis_pde_evolve: out overlaps u or u0");
  const int T = ev_T();
  PIS_CHECK_ARG(T != 0, "pis_pde_evolve: pis_tune key %d holds %d: 1, 2, 4 or 8 is needed", PIS_TUNE_EVOLVE_T,
                tune_get(PIS_TUNE_EVOLVE_T));
  const int launches = steps == 0 ? 1 : (int)cdiv(steps, T);
  const size_t map = ev_map_bytes(B, H, W);
  const size_t need = (size_t)std::min(launches - 1, 2) * map;
  PIS_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "pis_pde_evolve: workspace missing or too small (%zu < %zu bytes)",
                ws_bytes, need);
  if (need)
    PIS_CHECK_ARG(!ev_overlap(ws, need, u, bytes) && !ev_overlap(ws, need, out, bytes) &&
                      !(u0 && ev_overlap(ws, need, u0, bytes)),
                  "pis_pde_evolve: ws overlaps u, u0 or out");
  EvolveArgs g{};
  g.H = H; g.W = W;
  g.nbx = (int)cdiv(W, EV_TW);
  g.nby = (int)cdiv(H, EV_TH);
  g.D = D; g.k = k; g.a = a; g.mu = mu; g.dt = dt; g.thr = thr;
  g.u0 = u0 ? u0 : u;
  const unsigned blocks = (unsigned)((int64_t)B * g.nbx * g.nby);
  const bool with_mu = mu != 0.f, clamp = (flags & PIS_EVOLVE_CLAMP) != 0;
  float* scratch[2] = {(float*)ws, (float*)((char*)ws + map)};
  const float* src = u;
  for (int i = 0, left = steps; i < launches; ++i) {
    const bool last = i == launches - 1;
    g.src = src;
    g.dst = last ? out : scratch[i & 1];  // launch i reads scratch[(i - 1) & 1] (u for i == 0): never what it writes
    g.mask = last ? mask : nullptr;
    g.h = std::min(left, T);
    left -= g.h;
    if (with_mu) {
      if (clamp) ev_launch<true, true>(T, blocks, (hipStream_t)stream, g);
      else ev_launch<true, false>(T, blocks, (hipStream_t)stream, g);
    } else {
      if (clamp) ev_launch<false, true>(T, blocks, (hipStream_t)stream, g);
      else ev_launch<false, false>(T, blocks, (hipStream_t)stream, g);
    }
    if (int rc = launch_status("pde_evolve")) return rc;
    src = g.dst;
  }
  return PIS_OK;
}

static bool en_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 2 && H <= 4096 && W >= 2 && W <= 4096 && (int64_t)B * cdiv(H, EN_ROWS) <= 0x7fffffffLL;
}

extern "C" size_t pis_pde_energies_ws(int B, int H, int W) {
  if (!en_shape_ok(B, H, W)) {
    set_error("pis_pde_energies_ws: B >= 1 and 2 <= H, W <= 4096 are needed");
    return 0;
  }
  return (size_t)B * cdiv(H, EN_ROWS) * (2 * sizeof(double) + sizeof(int64_t));
}

extern "C" int pis_pde_energies(const float* u, int B, int H, int W, float D, float a, float eps, double* out_f64,
                                int64_t* out_i64, void* ws, size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(u && out_f64 && out_i64, "pis_pde_energies: u, out_f64 or out_i64 is NULL");
  PIS_CHECK_ARG(en_shape_ok(B, H, W), "pis_pde_energies: B = %d, H = %d, W = %d: B >= 1 and 2 <= H, W <= 4096 are needed",
                B, H, W);
  PIS_CHECK_ARG(D >= 0.f && a > 0.f && a < 1.f && eps > 0.f, "pis_pde_energies: D >= 0, 0 < a < 1 and eps > 0 are needed");
  PIS_CHECK_ARG(((uintptr_t)out_f64 | (uintptr_t)out_i64 | (uintptr_t)ws) % 8 == 0 && (uintptr_t)u % 4 == 0,
                "pis_pde_energies: out_f64, out_i64 and ws must be 8-byte aligned");
  PIS_CHECK_ARG(ws && ws_bytes >= pis_pde_energies_ws(B, H, W), "pis_pde_energies: workspace missing or too small");
  EnergyArgs g{};
  g.u = u; g.H = H; g.W = W;
  g.nb = (int)cdiv(H, EN_ROWS);
  g.part = (double*)ws;
  g.cnt = (int64_t*)((double*)ws + 2 * (size_t)B * g.nb);
  g.D = D; g.a = a;
  g.he = eps / 2.f;
  g.ie = 1.f / eps;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pde_energy_kernel, dim3((unsigned)((int64_t)B * g.nb)), dim3(256), 0, s, g);
  if (int rc = launch_status("pde_energy")) return rc;
  hipLaunchKernelGGL(pde_energy_reduce_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)g.part,
                     (const int64_t*)g.cnt, g.nb, (double)H * W, out_f64, out_i64);
  return launch_status("pde_energy_reduce");
}
