// PDE evolution of a probability map and its per-image physics quantities (include/pis_capi.h,
// DESIGN.md §14; pde.py:evolve_np / energies_np are the definitions of record, restated there in
// float32 numpy and agreeing bit for bit).
//
//   pis_pde_evolve     `steps` explicit Euler steps of u_t = D lap(u) + k u (1 - u) (u - a) + mu (u0 - u)
//                      on the reflect-padded 5-point stencil, T steps per launch inside LDS
//   pis_pde_energies   per image: mean squared reaction-diffusion residual, mean phase-field energy
//                      density, count of interface pixels; float64 sums in a fixed order
//   pis_pde_unroll_fwd pis_pde_evolve's steps, keeping the state after every Tb-th step
//   pis_pde_unroll_bwd the vector-Jacobian product of those steps, one launch per Tb steps, last first
//                      (pde.py:unroll_vjp_np is its definition of record)
//   pis_pde_unroll_fwd_dev / pis_pde_unroll_bwd_dev
//                      the same two with D, k, a, mu, dt read from device memory, and on request the
//                      gradient with respect to those five (pde.py:unroll_coef_vjp_np)
//
// Coefficients from device memory: a kernel reads coef[5] once at its start and forms 4 D, dt D and dt mu
// with ev_mul, the three float32 products the host forms for the by-value entry points. The values are
// arithmetic operands only: none enters an address, a loop bound or a branch that guards a memory access,
// so no value (NaN and infinities included) can make a kernel read or write out of bounds. That path has
// no range check, which would be a host synchronisation; pde.py:LearnablePDELayer keeps the values in
// range by construction.
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
// the reverse sweep: its planes let one (Tb = 4) or two (Tb = 2) workgroups reside on a CU, so the waves
// come from the workgroup: 16 steps at 8 x 512^2, Tb = 2, took 438.9 us with 256 threads, 318.9 with 512
// and 278.7 with 1024 (forward included; profiles/pde_unroll.txt holds the shipped form)
constexpr int UN_THREADS = 1024;

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
  const float* coef;  // not NULL: D, k, a, mu, dt are read from it (device memory), the five above unused
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
  float cD = g.D, ck = g.k, ca = g.a, cmu = g.mu, cdt = g.dt;
  if (g.coef) {  // uniform
    cD = g.coef[0]; ck = g.coef[1]; ca = g.coef[2]; cmu = g.coef[3]; cdt = g.coef[4];
  }

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
      float t = ev_mul(cD, lap);
      t = ev_add(t, ev_mul(ck, ev_react(c, ca)));
      if (MU) t = ev_add(t, ev_mul(cmu, ev_sub(plane0[p], c)));
      float n = ev_add(c, ev_mul(cdt, t));
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

// ---- unrolled evolution: the reverse sweep (pde.py:unroll_vjp_np is the definition) ---
// A block owns an EV_TH x EV_TW tile of the gradient with respect to the state a temporal block of
// h <= T steps started from. The plane carries a 2 T halo: the block's starting state comes through
// the reflect index, the incoming gradient from the image itself (zero outside it). The h states are
// recomputed as in pde_evolve_kernel, kept before the clamp (n_s in st[s], exact s rings inside the
// plane): the clamp is applied when a state is read and the pass mask is read off the same value.
// The reverse step j (from c_(j+1) back to c_j) is a gather: it reads q = mask . g at the pixel and
// its four neighbours and c_j at the pixel, so after it g is exact 2 h - j rings inside the plane,
// 2 h <= 2 T for j = 0: the tile. The two gradient planes hold 0 outside the image and are never
// written there, which is the definition's "pixels outside the image contribute 0". A sweep covers
// a linear range of rows [r, PH - r) as the forward's does; what it writes less than r rings inside
// is never read by an exact element.
struct UnrollBwdArgs {
  const float* src;  // the state the block starts from: u or a checkpoint
  const float* u0;   // MU only
  const float* gin;  // gradient with respect to the block's last state
  float* gout;       // gradient with respect to src; never gin
  float* gz;         // MU: the running sum of (dt mu) q, read (unless first) and written on the tile only
  int H, W, nbx, nby, h;
  int first, fold;   // first: gz starts from 0; fold: gout = g + gz (u is its own u0, last launch)
  float k, a, mu, dt, fourD, dtD, dtmu;
  float D;
  const float* coef;  // not NULL: D, k, a, mu, dt are read from it (device memory), the eight above unused
  double* part;       // COEF: [blocks][UN_SLOT], a workgroup's sums of the five coefficient terms
};

__device__ __forceinline__ float un_clamp(float n) {
  n = n < 0.f ? 0.f : n;
  return n > 1.f ? 1.f : n;
}

constexpr int UN_NCOEF = 5, UN_SLOT = 8;  // D, k, a, mu, dt; a slot is padded to 8 doubles
constexpr int UN_WAVES = UN_THREADS / 64;

template <int T>
constexpr size_t un_lds_bytes(bool mu, bool coef = false) {
  constexpr size_t PN = (size_t)(EV_TH + 4 * T) * (EV_TW + 4 * T);
  return sizeof(float) * ((T + 3) * PN + (mu ? PN + (size_t)EV_TH * EV_TW : 0)) +
         (coef ? sizeof(double) * UN_WAVES * UN_NCOEF : 0);
}

// COEF (pde.py:unroll_coef_vjp_np is the definition): in the reverse step j the thread that
// owns an in-image pixel of the tile also forms the five products of q with the step's derivative with
// respect to D, k, a, mu and dt, from c_j and its four neighbours (the tile is 2 T rings inside the plane,
// c_j is exact j <= T - 1 rings inside, so the neighbours are exact too), and adds them to five float64
// sums it keeps over the launch's steps. Halo pixels add nothing: every pixel of the image is counted by the
// one workgroup whose tile holds it. Then wave_sum_d, the 16 waves pairwise in a fixed order, and thread c
// adds column c to the workgroup's own slot (the first launch of a backward stores instead).
template <bool MU, bool CLAMP, int T, bool COEF>
__global__ __launch_bounds__(UN_THREADS) void pde_unroll_bwd_kernel(UnrollBwdArgs g) {
  constexpr int R = 2 * T, PH = EV_TH + 2 * R, PW = EV_TW + 2 * R, PN = PH * PW;
  extern __shared__ __attribute__((aligned(16))) float un_lds[];
  float* const st = un_lds;             // [T + 1][PN]: c_0, then n_1 .. n_h before the clamp
  float* const gp = st + (T + 1) * PN;  // [2][PN]
  float* const z = gp + 2 * PN;         // MU: [PN] u0
  float* const gzt = z + PN;            // MU: [EV_TH * EV_TW]
  double* const red = (double*)(st + (T + 3) * PN + (MU ? PN + EV_TH * EV_TW : 0));  // COEF: [UN_WAVES][UN_NCOEF]
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % g.nbx, by = (blockIdx.x / g.nbx) % g.nby, b = blockIdx.x / (g.nbx * g.nby);
  const int y0 = by * EV_TH, x0 = bx * EV_TW;
  const int H = g.H, W = g.W, h = g.h;
  const int64_t img = (int64_t)b * H * W;
  float cD = g.D, ck = g.k, ca = g.a, cmu = g.mu, cdt = g.dt, fourD = g.fourD, dtD = g.dtD, dtmu = g.dtmu;
  if (g.coef) {  // uniform
    cD = g.coef[0]; ck = g.coef[1]; ca = g.coef[2]; cmu = g.coef[3]; cdt = g.coef[4];
    fourD = ev_mul(4.f, cD); dtD = ev_mul(cdt, cD); dtmu = ev_mul(cdt, cmu);
  }
  double acc[UN_NCOEF] = {0.0, 0.0, 0.0, 0.0, 0.0};

  for (int p = tid; p < PN; p += UN_THREADS) {
    const int ly = p / PW, lx = p - ly * PW;
    const int y = y0 - R + ly, x = x0 - R + lx;
    const int64_t at = img + (int64_t)ev_reflect(y, H) * W + ev_reflect(x, W);
    st[p] = g.src[at];
    if (MU) z[p] = g.u0[at];
    const bool inside = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    gp[p] = inside ? g.gin[img + (int64_t)y * W + x] : 0.f;
    gp[PN + p] = 0.f;
  }
  if (MU) {
    for (int i = tid; i < EV_TH * EV_TW; i += UN_THREADS) {
      const int y = y0 + i / EV_TW, x = x0 + i % EV_TW;
      gzt[i] = (!g.first && y < H && x < W) ? g.gz[img + (int64_t)y * W + x] : 0.f;
    }
  }
  __syncthreads();

  // the h states again, as pde_evolve_kernel computes them
  for (int s = 1; s <= h; ++s) {
    const float* __restrict__ in = st + (s - 1) * PN;
    float* __restrict__ out = st + s * PN;
    const bool cl = CLAMP && s > 1;  // st[0] is a state, the later planes are pre-clamp
    const int end = (PH - s) * PW - s;
    for (int p = s * PW + s + tid; p < end; p += UN_THREADS) {
      float c = in[p], up = in[p - PW], dn = in[p + PW], lf = in[p - 1], rt = in[p + 1];
      if (cl) {
        c = un_clamp(c); up = un_clamp(up); dn = un_clamp(dn); lf = un_clamp(lf); rt = un_clamp(rt);
      }
      float t = ev_mul(cD, ev_lap(c, up, dn, lf, rt));
      t = ev_add(t, ev_mul(ck, ev_react(c, ca)));
      if (MU) t = ev_add(t, ev_mul(cmu, ev_sub(z[p], c)));
      out[p] = ev_add(c, ev_mul(cdt, t));
    }
    __syncthreads();
  }

  int cur = 0;
  for (int j = h - 1; j >= 0; --j) {
    const float* __restrict__ nm = st + (j + 1) * PN;
    const float* __restrict__ cj = st + j * PN;
    const float* __restrict__ gi = gp + cur * PN;
    float* __restrict__ go = gp + (cur ^ 1) * PN;
    const int r = 2 * h - j;
    const int end = (PH - r) * PW - r;
    auto q_at = [&](int pp) -> float {
      if (CLAMP) {
        const float n = nm[pp];
        if (n < 0.f || n > 1.f) return 0.f;
      }
      return gi[pp];
    };
    for (int p = r * PW + r + tid; p < end; p += UN_THREADS) {
      const int ly = p / PW, lx = p - ly * PW;
      const int y = y0 - R + ly, x = x0 - R + lx;
      if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) continue;  // stays 0
      const float wau = y == 0 ? 0.f : (y == 1 ? 2.f : 1.f), wbd = y == H - 1 ? 0.f : (y == H - 2 ? 2.f : 1.f);
      const float wal = x == 0 ? 0.f : (x == 1 ? 2.f : 1.f), wbr = x == W - 1 ? 0.f : (x == W - 2 ? 2.f : 1.f);
      const float q = q_at(p);
      const float nb = ev_add(ev_add(ev_mul(wau, q_at(p - PW)), ev_mul(wbd, q_at(p + PW))),
                              ev_add(ev_mul(wal, q_at(p - 1)), ev_mul(wbr, q_at(p + 1))));
      float c = cj[p];
      if (CLAMP && j > 0) c = un_clamp(c);
      const float rp = ev_add(ev_mul(ev_sub(1.f, ev_mul(2.f, c)), ev_sub(c, ca)), ev_mul(c, ev_sub(1.f, c)));
      float s = ev_mul(ck, rp);
      s = ev_sub(s, fourD);
      if (MU) s = ev_sub(s, cmu);
      const float d = ev_add(1.f, ev_mul(cdt, s));
      go[p] = ev_add(ev_mul(d, q), ev_mul(dtD, nb));
      if (MU || COEF) {
        const int ty = ly - R, tx = lx - R;
        if ((unsigned)ty < (unsigned)EV_TH && (unsigned)tx < (unsigned)EV_TW) {
          if (MU) gzt[ty * EV_TW + tx] = ev_add(gzt[ty * EV_TW + tx], ev_mul(dtmu, q));
          if (COEF) {  // the forward step from c_j again, as the recompute loop forms it
            float up = cj[p - PW], dn = cj[p + PW], lf = cj[p - 1], rt = cj[p + 1];
            if (CLAMP && j > 0) {
              up = un_clamp(up); dn = un_clamp(dn); lf = un_clamp(lf); rt = un_clamp(rt);
            }
            const float lap = ev_lap(c, up, dn, lf, rt);
            const float cc = ev_mul(c, ev_sub(1.f, c));
            const float r = ev_mul(cc, ev_sub(c, ca));
            float t = ev_mul(cD, lap);
            t = ev_add(t, ev_mul(ck, r));
            if (MU) {
              const float zc = ev_sub(z[p], c);
              t = ev_add(t, ev_mul(cmu, zc));
              acc[3] += (double)ev_mul(q, ev_mul(cdt, zc));
            }
            acc[0] += (double)ev_mul(q, ev_mul(cdt, lap));
            acc[1] += (double)ev_mul(q, ev_mul(cdt, r));
            acc[2] += (double)ev_mul(q, ev_mul(cdt, ev_mul(ck, ev_sub(0.f, cc))));
            acc[4] += (double)ev_mul(q, t);
          }
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  const float* __restrict__ fin = gp + cur * PN;
  for (int i = tid; i < EV_TH * EV_TW; i += UN_THREADS) {
    const int ty = i / EV_TW, tx = i - ty * EV_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    const int64_t at = img + (int64_t)y * W + x;
    float v = fin[(R + ty) * PW + R + tx];
    float zsum = 0.f;
    if (MU) {
      zsum = gzt[i];
      g.gz[at] = zsum;
    }
    if (g.fold) v = ev_add(v, zsum);
    g.gout[at] = v;
  }

  if (COEF) {
#pragma unroll
    for (int c = 0; c < UN_NCOEF; ++c) acc[c] = wave_sum_d(acc[c]);
    if ((tid & 63) == 0) {
#pragma unroll
      for (int c = 0; c < UN_NCOEF; ++c) red[(tid >> 6) * UN_NCOEF + c] = acc[c];
    }
    __syncthreads();
    if (tid < UN_NCOEF) {  // ((w0 + w1) + (w2 + w3)) + ..., a balanced tree over the 16 waves
      double w[UN_WAVES];
#pragma unroll
      for (int i = 0; i < UN_WAVES; ++i) w[i] = red[i * UN_NCOEF + tid];
#pragma unroll
      for (int n = UN_WAVES / 2; n >= 1; n >>= 1) {
#pragma unroll
        for (int i = 0; i < n; ++i) w[i] = w[2 * i] + w[2 * i + 1];
      }
      double* const slot = g.part + (int64_t)UN_SLOT * blockIdx.x + tid;  // this workgroup's alone
      *slot = g.first ? w[0] : *slot + w[0];
    }
  }
}

// one wave per image: lane l adds the slots of tiles l, l + 64, ... in ascending order, then the xor butterfly
__global__ __launch_bounds__(64) void pde_coef_reduce_kernel(const double* __restrict__ part, int nt,
                                                             double* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s[UN_NCOEF] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < nt; i += 64) {
#pragma unroll
    for (int c = 0; c < UN_NCOEF; ++c) s[c] += part[UN_SLOT * ((int64_t)b * nt + i) + c];
  }
#pragma unroll
  for (int c = 0; c < UN_NCOEF; ++c) s[c] = wave_sum_d(s[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < UN_NCOEF; ++c) out[UN_NCOEF * b + c] = s[c];
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

// ---- unrolled evolution: checkpointed forward, reverse sweep --------------------------------------
static int un_tb(int tb) {
  if (tb == 0) tb = tune_get(PIS_TUNE_UNROLL_TB);
  return (tb == 1 || tb == 2 || tb == 4) ? tb : 0;
}

extern "C" size_t pis_pde_unroll_ws(int B, int H, int W, int steps, int tb) {
  const int T = un_tb(tb);
  if (!ev_shape_ok(B, H, W) || steps < 0 || steps > PIS_UNROLL_MAX_STEPS || T == 0) {
    set_error("pis_pde_unroll_ws: B >= 1, 2 <= H, W <= 4096, 0 <= steps <= %d and a temporal block of 1, 2 or 4 are needed",
              PIS_UNROLL_MAX_STEPS);
    return 0;
  }
  const int launches = steps == 0 ? 1 : (int)cdiv(steps, T);
  return (size_t)(launches - 1) * ev_map_bytes(B, H, W);
}

extern "C" size_t pis_pde_unroll_bwd_ws(int B, int H, int W) {
  if (!ev_shape_ok(B, H, W)) {
    set_error("pis_pde_unroll_bwd_ws: B >= 1 and 2 <= H, W <= 4096 are needed");
    return 0;
  }
  return 3 * ev_map_bytes(B, H, W);  // two gradient maps in turn, and the running sum when g_u0 is NULL
}

static size_t un_slot_bytes(int B, int H, int W) {
  return (size_t)B * cdiv(H, EV_TH) * cdiv(W, EV_TW) * UN_SLOT * sizeof(double);
}

extern "C" size_t pis_pde_unroll_bwd_dev_ws(int B, int H, int W) {
  if (!ev_shape_ok(B, H, W)) {
    set_error("pis_pde_unroll_bwd_dev_ws: B >= 1 and 2 <= H, W <= 4096 are needed");
    return 0;
  }
  return 3 * ev_map_bytes(B, H, W) + un_slot_bytes(B, H, W);  // pis_pde_unroll_bwd_ws's maps, then the slot table
}

static int un_check_shape(const char* who, int B, int H, int W, int steps, int flags, int known) {
  PIS_CHECK_ARG(ev_shape_ok(B, H, W), "%s: B = %d, H = %d, W = %d: B >= 1 and 2 <= H, W <= 4096 are needed", who, B, H, W);
  PIS_CHECK_ARG(steps >= 0 && steps <= PIS_UNROLL_MAX_STEPS, "%s: steps = %d: [0, %d] is needed", who, steps,
                PIS_UNROLL_MAX_STEPS);
  PIS_CHECK_ARG((flags & ~known) == 0, "%s: unknown flags 0x%x", who, flags);
  return PIS_OK;
}

// the scalar checks of pis_pde_evolve
static int un_check_scalars(const char* who, int B, int H, int W, float D, float k, float a, float mu, float dt, int steps,
                            int flags) {
  if (int rc = un_check_shape(who, B, H, W, steps, flags, PIS_EVOLVE_CLAMP)) return rc;
  PIS_CHECK_ARG(D >= 0.f && k >= 0.f && mu >= 0.f && a > 0.f && a < 1.f && dt > 0.f,
                "%s: D >= 0, k >= 0, mu >= 0, 0 < a < 1 and dt > 0 are needed", who);
  PIS_CHECK_ARG((double)dt * (4.0 * D + (double)k + (double)mu) <= 1.0,
                "%s: dt (4 D + k + mu) = %g exceeds 1: the explicit step is not monotone", who,
                (double)dt * (4.0 * D + (double)k + (double)mu));
  return PIS_OK;
}

// the checkpointed forward of both entry points: g holds the coefficients, by value or as g.coef
static int un_fwd(const char* who, const float* u, const float* u0, float* out, void* ckpt, size_t ckpt_bytes, int B,
                  int H, int W, EvolveArgs g, bool with_mu, int steps, int flags, int tb, pis_stream_t stream) {
  const int T = un_tb(tb);
  PIS_CHECK_ARG(T != 0, "%s: temporal block %d (pis_tune key %d holds %d): 1, 2 or 4 is needed", who, tb,
                PIS_TUNE_UNROLL_TB, tune_get(PIS_TUNE_UNROLL_TB));
  PIS_CHECK_ARG(((uintptr_t)u | (uintptr_t)u0 | (uintptr_t)out | (uintptr_t)ckpt) % 16 == 0 && (uintptr_t)g.coef % 4 == 0,
                "%s: u, u0, out and ckpt must be 16-byte aligned (coef 4-byte)", who);
  const size_t bytes = (size_t)B * H * W * sizeof(float), map = ev_map_bytes(B, H, W);
  const int launches = steps == 0 ? 1 : (int)cdiv(steps, T);
  const size_t need = (size_t)(launches - 1) * map;
  PIS_CHECK_ARG(need == 0 || (ckpt && ckpt_bytes >= need), "%s: checkpoint stack missing or too small (%zu < %zu bytes)",
                who, ckpt_bytes, need);
  PIS_CHECK_ARG(!ev_overlap(out, bytes, u, bytes) && !(u0 && ev_overlap(out, bytes, u0, bytes)) &&
                    (!need || (!ev_overlap(ckpt, need, u, bytes) && !ev_overlap(ckpt, need, out, bytes) &&
                               !(u0 && ev_overlap(ckpt, need, u0, bytes)))),
                "%s: out or ckpt overlaps another map", who);
  const size_t cb = UN_NCOEF * sizeof(float);
  PIS_CHECK_ARG(!g.coef || (!ev_overlap(out, bytes, g.coef, cb) && !(need && ev_overlap(ckpt, need, g.coef, cb))),
                "%s: out or ckpt overlaps coef", who);
  g.H = H; g.W = W;
  g.nbx = (int)cdiv(W, EV_TW);
  g.nby = (int)cdiv(H, EV_TH);
  g.thr = 0.f;
  g.u0 = u0 ? u0 : u;
  g.mask = nullptr;
  const unsigned blocks = (unsigned)((int64_t)B * g.nbx * g.nby);
  const bool clamp = (flags & PIS_EVOLVE_CLAMP) != 0;
  const float* src = u;
  for (int i = 0, left = steps; i < launches; ++i) {
    g.src = src;
    g.dst = i == launches - 1 ? out : (float*)((char*)ckpt + (size_t)i * map);  // slot i: the state after block i
    g.h = std::min(left, T);
    left -= g.h;
    if (with_mu) {
      if (clamp) ev_launch<true, true>(T, blocks, (hipStream_t)stream, g);
      else ev_launch<true, false>(T, blocks, (hipStream_t)stream, g);
    } else {
      if (clamp) ev_launch<false, true>(T, blocks, (hipStream_t)stream, g);
      else ev_launch<false, false>(T, blocks, (hipStream_t)stream, g);
    }
    if (int rc = launch_status("pde_unroll_fwd")) return rc;
    src = g.dst;
  }
  return PIS_OK;
}

extern "C" int pis_pde_unroll_fwd(const float* u, const float* u0, float* out, void* ckpt, size_t ckpt_bytes, int B, int H,
                                  int W, float D, float k, float a, float mu, float dt, int steps, int flags, int tb,
                                  pis_stream_t stream) {
  PIS_CHECK_ARG(u && out, "pis_pde_unroll_fwd: u or out is NULL");
  if (int rc = un_check_scalars("pis_pde_unroll_fwd", B, H, W, D, k, a, mu, dt, steps, flags)) return rc;
  EvolveArgs g{};
  g.D = D; g.k = k; g.a = a; g.mu = mu; g.dt = dt;
  return un_fwd("pis_pde_unroll_fwd", u, u0, out, ckpt, ckpt_bytes, B, H, W, g, mu != 0.f, steps, flags, tb, stream);
}

extern "C" int pis_pde_unroll_fwd_dev(const float* u, const float* u0, float* out, void* ckpt, size_t ckpt_bytes, int B,
                                      int H, int W, const float* coef, int steps, int flags, int tb,
                                      pis_stream_t stream) {
  PIS_CHECK_ARG(u && out && coef, "pis_pde_unroll_fwd_dev: u, out or coef is NULL");
  if (int rc = un_check_shape("pis_pde_unroll_fwd_dev", B, H, W, steps, flags, PIS_EVOLVE_CLAMP | PIS_EVOLVE_MU)) return rc;
  EvolveArgs g{};
  g.coef = coef;
  return un_fwd("pis_pde_unroll_fwd_dev", u, u0, out, ckpt, ckpt_bytes, B, H, W, g, (flags & PIS_EVOLVE_MU) != 0, steps,
                flags, tb, stream);
}

template <bool MU, bool CLAMP, bool COEF>
static void un_launch(int T, unsigned blocks, hipStream_t s, const UnrollBwdArgs& a) {
  switch (T) {
    case 1:
      hipLaunchKernelGGL((pde_unroll_bwd_kernel<MU, CLAMP, 1, COEF>), dim3(blocks), dim3(UN_THREADS),
                         un_lds_bytes<1>(MU, COEF), s, a);
      break;
    case 2:
      hipLaunchKernelGGL((pde_unroll_bwd_kernel<MU, CLAMP, 2, COEF>), dim3(blocks), dim3(UN_THREADS),
                         un_lds_bytes<2>(MU, COEF), s, a);
      break;
    default:
      hipLaunchKernelGGL((pde_unroll_bwd_kernel<MU, CLAMP, 4, COEF>), dim3(blocks), dim3(UN_THREADS),
                         un_lds_bytes<4>(MU, COEF), s, a);
      break;
  }
}
template <bool COEF>
static void un_launch_flags(bool with_mu, bool clamp, int T, unsigned blocks, hipStream_t s, const UnrollBwdArgs& a) {
  if (with_mu) {
    if (clamp) un_launch<true, true, COEF>(T, blocks, s, a);
    else un_launch<true, false, COEF>(T, blocks, s, a);
  } else {
    if (clamp) un_launch<false, true, COEF>(T, blocks, s, a);
    else un_launch<false, false, COEF>(T, blocks, s, a);
  }
}
static_assert(un_lds_bytes<4>(true, true) <= 160 * 1024, "the reverse sweep's planes must fit one workgroup's LDS");

// the reverse sweep of both entry points: g holds the coefficients, by value or as g.coef. g_coef (with
// g.coef only): the COEF kernels, their slot table behind the three maps of ws, and the reduce kernel.
static int un_bwd(const char* who, const float* u, const float* u0, const void* ckpt, const float* g_out, float* g_u,
                  float* g_u0, double* g_coef, int B, int H, int W, UnrollBwdArgs g, bool with_mu, int steps, int flags,
                  int tb, void* ws, size_t ws_bytes, pis_stream_t stream) {
  const int T = un_tb(tb);
  PIS_CHECK_ARG(T != 0, "%s: temporal block %d (pis_tune key %d holds %d): 1, 2 or 4 is needed", who, tb,
                PIS_TUNE_UNROLL_TB, tune_get(PIS_TUNE_UNROLL_TB));
  PIS_CHECK_ARG(((uintptr_t)u | (uintptr_t)u0 | (uintptr_t)ckpt | (uintptr_t)g_out | (uintptr_t)g_u | (uintptr_t)g_u0 |
                 (uintptr_t)ws) % 16 == 0 && (uintptr_t)g.coef % 4 == 0 && (uintptr_t)g_coef % 8 == 0,
                "%s: every map, ckpt and ws must be 16-byte aligned (coef 4-byte, g_coef 8-byte)", who);
  const size_t bytes = (size_t)B * H * W * sizeof(float), map = ev_map_bytes(B, H, W);
  const int launches = steps == 0 ? 0 : (int)cdiv(steps, T);
  const size_t stack = launches > 1 ? (size_t)(launches - 1) * map : 0;
  PIS_CHECK_ARG(stack == 0 || ckpt, "%s: ckpt is NULL (%d checkpoints are needed)", who, launches - 1);
  const bool clamp = (flags & PIS_EVOLVE_CLAMP) != 0;
  const bool carry_in_ws = with_mu && !g_u0;
  const size_t need = steps == 0 ? 0 : (size_t)(std::min(launches - 1, 2)) * map;  // the gradient maps in turn
  const size_t slots = g_coef && steps ? un_slot_bytes(B, H, W) : 0;                // behind the three maps
  const size_t need_all = slots ? 3 * map + slots : (carry_in_ws ? 3 * map : need);  // the running sum sits third
  PIS_CHECK_ARG(need_all == 0 || (ws && ws_bytes >= need_all), "%s: workspace missing or too small (%zu < %zu bytes)", who,
                ws_bytes, need_all);
  const size_t cb = UN_NCOEF * sizeof(float), gcb = (size_t)B * UN_NCOEF * sizeof(double);
  {
    const void* p[9] = {g_u, g_u0, need_all ? ws : nullptr, g_coef, g_out, u, u0, stack ? ckpt : nullptr, g.coef};
    const size_t n[9] = {bytes, bytes, need_all, gcb, bytes, bytes, bytes, stack, cb};
    // what is written (the first four) meets nothing; the inputs may meet each other (u0 may be u)
    bool ok = true;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 9; ++j)
        ok = ok && !(p[i] && p[j] && n[i] && n[j] && ev_overlap(p[i], n[i], p[j], n[j]));
    PIS_CHECK_ARG(ok, "%s: g_u, g_u0, ws or g_coef overlaps another argument", who);
  }
  hipStream_t s = (hipStream_t)stream;
  if ((steps == 0 || !with_mu) && g_u0) {  // nothing reaches u0
    const hipError_t e = hipMemsetAsync(g_u0, 0, bytes, s);
    if (e != hipSuccess) {
      set_error("%s: clearing g_u0: %s", who, hipGetErrorString(e));
      return PIS_ERR_LAUNCH;
    }
  }
  if (steps == 0) {  // the identity
    hipError_t e = hipMemcpyAsync(g_u, g_out, bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && g_coef) e = hipMemsetAsync(g_coef, 0, gcb, s);
    if (e != hipSuccess) {
      set_error("%s: copying g_out: %s", who, hipGetErrorString(e));
      return PIS_ERR_LAUNCH;
    }
    return PIS_OK;
  }
  g.H = H; g.W = W;
  g.nbx = (int)cdiv(W, EV_TW);
  g.nby = (int)cdiv(H, EV_TH);
  g.u0 = u0 ? u0 : u;
  g.gz = with_mu ? (g_u0 ? g_u0 : (float*)((char*)ws + 2 * map)) : nullptr;
  g.part = g_coef ? (double*)((char*)ws + 3 * map) : nullptr;
  const unsigned blocks = (unsigned)((int64_t)B * g.nbx * g.nby);
  float* scratch[2] = {(float*)ws, (float*)((char*)ws + map)};
  const float* gin = g_out;
  for (int t = 0; t < launches; ++t) {
    const int i = launches - 1 - t;  // the temporal block, last first
    const bool last = t == launches - 1;
    g.src = i == 0 ? u : (const float*)((const char*)ckpt + (size_t)(i - 1) * map);
    g.h = std::min(T, steps - i * T);
    g.gin = gin;
    g.gout = last ? g_u : scratch[t & 1];  // launch t reads scratch[(t - 1) & 1] (g_out for t == 0)
    g.first = t == 0;
    g.fold = last && !u0;
    if (g_coef) un_launch_flags<true>(with_mu, clamp, T, blocks, s, g);
    else un_launch_flags<false>(with_mu, clamp, T, blocks, s, g);
    if (int rc = launch_status("pde_unroll_bwd")) return rc;
    gin = g.gout;
  }
  if (g_coef) {
    hipLaunchKernelGGL(pde_coef_reduce_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)g.part, g.nbx * g.nby,
                       g_coef);
    return launch_status("pde_coef_reduce");
  }
  return PIS_OK;
}

extern "C" int pis_pde_unroll_bwd(const float* u, const float* u0, const void* ckpt, const float* g_out, float* g_u,
                                  float* g_u0, int B, int H, int W, float D, float k, float a, float mu, float dt,
                                  int steps, int flags, int tb, void* ws, size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(u && g_out && g_u, "pis_pde_unroll_bwd: u, g_out or g_u is NULL");
  PIS_CHECK_ARG(u0 || !g_u0, "pis_pde_unroll_bwd: g_u0 without u0 (u is then its own u0 and g_u holds the sum)");
  if (int rc = un_check_scalars("pis_pde_unroll_bwd", B, H, W, D, k, a, mu, dt, steps, flags)) return rc;
  UnrollBwdArgs g{};
  g.D = D; g.k = k; g.a = a; g.mu = mu; g.dt = dt;
  {
    // float32 products formed once, each rounded on its own (volatile: no contraction, no folding in double)
    volatile float four_d = 4.f * D, dt_d = dt * D, dt_mu = dt * mu;
    g.fourD = four_d; g.dtD = dt_d; g.dtmu = dt_mu;
  }
  return un_bwd("pis_pde_unroll_bwd", u, u0, ckpt, g_out, g_u, g_u0, nullptr, B, H, W, g, mu != 0.f, steps, flags, tb, ws,
                ws_bytes, stream);
}

extern "C" int pis_pde_unroll_bwd_dev(const float* u, const float* u0, const void* ckpt, const float* g_out, float* g_u,
                                      float* g_u0, double* g_coef, int B, int H, int W, const float* coef, int steps,
                                      int flags, int tb, void* ws, size_t ws_bytes, pis_stream_t stream) {
  PIS_CHECK_ARG(u && g_out && g_u && coef, "pis_pde_unroll_bwd_dev: u, g_out, g_u or coef is NULL");
  PIS_CHECK_ARG(u0 || !g_u0, "pis_pde_unroll_bwd_dev: g_u0 without u0 (u is then its own u0 and g_u holds the sum)");
  if (int rc = un_check_shape("pis_pde_unroll_bwd_dev", B, H, W, steps, flags, PIS_EVOLVE_CLAMP | PIS_EVOLVE_MU)) return rc;
  UnrollBwdArgs g{};
  g.coef = coef;
  return un_bwd("pis_pde_unroll_bwd_dev", u, u0, ckpt, g_out, g_u, g_u0, g_coef, B, H, W, g, (flags & PIS_EVOLVE_MU) != 0,
                steps, flags, tb, ws, ws_bytes, stream);
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
