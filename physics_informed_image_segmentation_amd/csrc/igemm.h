// Implicit-GEMM argument block shared by the direct (igemm.hip) and Winograd
// (winograd.hip) 3x3-conv paths, and the launchers and layout helpers of those paths. Which path
// runs is decided in conv3x3_plan.h.
#pragma once
#include "common.h"

namespace pis {

enum TapMode { TAP_CONV3 = 0, TAP_UP2 = 1, TAP_ONE = 2 };
enum EpiMode { EPI_NHWC = 0, EPI_SCATTER2 = 1 };

struct IGemmArgs {
  const float* src;  // NHWC source
  int lds;           // channel stride of src
  int Hs, Ws;        // source spatial dims
  int H, W;          // output pixel grid
  int M;             // B*H*W
  int Csrc;          // channels read per tap
  int ntaps;
  int tap_mode;
  const float* wt;   // Bt[N][ntaps*Csrc]
  int ldw;
  int N;
  // epilogue
  int epi;
  const float* bias;
  const float* scale;  // [B][N]
  const float* mask;   // [M][ldm]
  int ldm;
  float* dst;
  int ldd;
  int flags;
  int cout_t;          // EPI_SCATTER2: n = (i*2+j)*cout_t + o
  float* pool;         // F(4x4,3x3) forward only: also write the 2x2 max pool of dst here ([B][H/2][W/2][N])
  int w_unflipped;     // F(4x4,3x3) input gradient: wt holds the original KRSC weights (no flipped copy)
  int filter_ready;    // F(4x4,3x3): wt holds the layer's filter transform (pis_conv3x3_filter)
  int is_dgrad;        // an input gradient (pis_conv3x3_dgrad*): labels the direct kernel's launch / symbol
  // batched launches (gridDim.y > 1): per-batch element offsets
  int64_t bs_src, bs_wt, bs_dst;
};

// one value per kernel family of a 3x3 conv's forward / input gradient; conv3x3_plan.h chooses,
// the launchers below run what they are given
enum ConvAlgo {
  ALGO_NONE = 0,       // no such path (a resolve error: the message is set)
  ALGO_C1_ROW,         // Cin == 1, Cout == 64, W % 64 == 0: row kernel
  ALGO_C1_STREAM,      // Cin == 1: stream kernel
  ALGO_DIRECT_H3,      // direct fp16x3 (direct.hip)
  ALGO_WINO4_FUSED,    // F(4x4,3x3), contraction fused with the output transform
  ALGO_WINO4_GEMM,     // F(4x4,3x3) on the batched GEMM
  ALGO_WINO4_DGRAD_T,  // ... in the overlap-add input-gradient form (pis_tune key 51)
  ALGO_WINO6,          // F(6x6,3x3)
  ALGO_WINO2,          // F(2x2,3x3)
  ALGO_HALO,           // staged input halo
  ALGO_IGEMM,          // generic implicit GEMM
};

struct Conv3x3Plan;   // conv3x3_plan.h
struct WinoVariants;  // ... the kernel forms the Winograd launchers below instantiate

// generic implicit GEMM (all tap modes); `batches` independent problems via gridDim.y
int launch_igemm(const IGemmArgs& a, hipStream_t s, int batches = 1);
// 3x3 conv (fwd or dgrad-on-flipped-weights) from a staged input halo (W % 16 == 0, H % 8 == 0,
// 4-aligned Csrc and lds)
int launch_conv3x3_halo(const IGemmArgs& a, hipStream_t s);
// the Winograd pipelines of the same conv (winograd.hip; algo: one of the ALGO_WINO*); B = images in a.src
// workspace of the F(m x m, 3x3) pipelines, m = 4 or 2, and of F(6x6,3x3)
size_t wino_ws_bytes(int m, int B, int H, int W, int C, int N);
size_t wino6_ws_bytes(int B, int H, int W, int C, int N);
// keep_v (optional, F(4x4) only): V is written there instead of the workspace and left for
// the layer's weight gradient (pis_conv3x3_wgrad_keep)
// v_ready: V (F(4x4) only) is already in the workspace (pis_conv3x3_bwd_prep)
// p: the layer's plan (the batched GEMM of a's direction, the transform and fused-kernel forms)
int launch_wino3x3(ConvAlgo algo, const IGemmArgs& a, int B, void* ws, hipStream_t s, const Conv3x3Plan& p,
                   float* keep_v = nullptr, bool v_ready = false);
float* wino_v_slot(void* ws, int C, int N);
// one pass over dz: V (input-gradient input transform) and E + bias partials (weight gradient)
// (tmax != NULL: also the per-tile max |V| the fused fp16x3 dgrad reads, at wino_tmax_slot)
int launch_wino_dz2(const float* dz, int ldz, int B, int H, int W, int N, float* V, float* E, float* bpart,
                    hipStream_t s, const WinoVariants& v, float* tmax = nullptr);
float* wino_tmax_slot(void* ws, int B, int H, int W, int C, int N);
// pis_conv3x3_bwd_prep's record of the V it wrote into ws (checked by the prepared dgrad); e != NULL:
// the overlap-add form (pis_tune key 51) — no V, the input gradient contracts the weight
// gradient's E at e (C = Cout contraction channels, N = Cin)
void wino_prep_record(const void* ws, int B, int H, int W, int C, int N, bool tmax, const float* e = nullptr);
// Winograd weight-gradient pieces for tile edge m (2: F(3x3,2x2), 4: F(3x3,4x4)), nxi = (m+2)^2:
// V[nxi][T][C] of x, E[nxi][T][N] of dz, dW from M[nxi][N][C]
int launch_wino_input(const float* x, int ldx, int B, int H, int W, int C, float* V, hipStream_t s, int m,
                      const WinoVariants& v);
// bpart (m == 4 only, optional, N / 4 must divide 256): per-block channel sums of dz,
// [wino_dz_blocks()][N], for the bias gradient
int launch_wino_dz(const float* dz, int ldz, int B, int H, int W, int N, float* E, hipStream_t s, int m,
                   const WinoVariants& v, float* bpart = nullptr);
int wino_dz_blocks(int B, int H, int W, int N, int m);
// the filter operands computed ahead (pis_conv3x3_filter(s)): C contraction channels, N outputs;
// format as pis_conv3x3_filter_format
int launch_wino6_filter_only(const float* w, int C, int N, int dgrad, void* out, hipStream_t s);
int launch_wino4_filter_only(const float* w, int C, int N, int dgrad, int format, void* out, hipStream_t s,
                             const WinoVariants& v);
int launch_wino4_filter_batch(int n, const float* const* w, void* const* out, const int* C, const int* N,
                              const int* dgrad, const int* format, hipStream_t s, const WinoVariants& v);
int wino_dz_blocks_max(int B, int H, int W, int N, int m);  // the largest grid a dz pass of F(m x m) launches (rows of bias partials)
// M: nsplit split-K slabs sstride floats apart, summed in slab order (nsplit > 1 needs m == 4)
// The F(3x3,4x4) weight gradient's bias gradient, folded into its output-transform launch:
// db[n] (+)= scale x sum_{r < rows} part[r][n] (fixed order), part = the GEMM's [split][N] column
// sums of E plane WINO4_BIAS_XI; rows == 0: none
struct WgradOutBias {
  const float* part;
  int rows;
  float* db;
  float scale;
};
// E[7] = E[(1, 1)] = c^2 x (sum of the tile's 16 dz values), c = fp32(1/3) (w4_g4 row 1: the point 1)
constexpr int WINO4_BIAS_XI = 7;
constexpr float WINO4_BIAS_SCALE = (float)(1.0 / ((double)(1.0f / 3.0f) * (double)(1.0f / 3.0f)));
int launch_wino_wgrad_out(const float* M, int N, int C, float* dw, int accumulate, hipStream_t s, int m,
                          const WinoVariants& v, int nsplit = 1, int64_t sstride = 0, WgradOutBias bias = WgradOutBias{});

// direct 3x3 conv in fp16x3 (direct.hip): shapes it covers (a contraction of C channels into N
// outputs; the layer's weight gradient), its workspace (split weights), the launch (dgrad_orig: an
// input gradient whose a.wt holds the ORIGINAL KRSC weights)
bool direct_h3_shape_ok(int H, int W, int C, int N, int ldx);
bool direct_w_shape_ok(int B, int H, int W, int Cin, int Cout, int ldx, int ldz);
size_t direct_h3_ws_bytes(int C, int N);
int launch_direct_h3(const IGemmArgs& a, int B, void* ws, size_t ws_bytes, hipStream_t s, bool dgrad_orig,
                     bool ready = false);
int launch_direct_wsplit_batch(int n, const float* const* w, void* const* out, const int* Cin, const int* Cout,
                               const int* dgrad, hipStream_t s);
// the layer's weight gradient (the direct fp16x3 wgrad kernel): its workspace, launch
size_t direct_w_ws_bytes(int B, int H, int W, int Cin, int Cout);
int launch_direct_wgrad(const float* x, int ldx, const float* dz, int ldz, float* dw, float* db, int B, int H, int W,
                        int Cin, int Cout, int acc, void* ws, size_t ws_bytes, hipStream_t s);

}  // namespace pis
