// The 3x3-conv planner (conv3x3_plan.hip, host only): which kernel family runs a layer's forward,
// input gradient and weight gradient, and the workspace, kept-transform and filter-operand sizes
// that follow. It is the only code that reads pis_tune keys to choose a 3x3-conv path; the entry
// points (igemm.hip, wgrad.hip) ask it, per call, and launch what it says.
#pragma once
#include "igemm.h"

namespace pis {

// ---- weight-gradient detail plans (the split-K layouts of their branch) --------------------
struct WgradPlan {
  int bm, bn, splits, pps;
  size_t part_bytes, bias_bytes;
};
// tile sizes divide the per-tap group so tiles never straddle a tap (wgrad.hip)
WgradPlan plan_wgrad(int Mp, int Np, int P, int group_m, int group_n, int target_blocks = 2048);
size_t wgrad_ws_bytes(const WgradPlan& pl);
size_t colsum_ws(int64_t npix, int C);

// the split-K kernel families of wgrad.hip (run_wgrad launches the one chosen, on the plan's tile)
enum class WgradKernel {
  F32,        // wgrad_f32_kernel: fp32 MFMA, every operand form
  X6,         // wgrad_x6_kernel: bf16x6, operands staged by columns
  H3_COLS,    // wgrad_h3_kernel: fp16x3, operands staged by columns
  H3T,        // wgrad_h3t_kernel: fp16x3, operands staged by rows, 128 x 128 tiles
  H3T_EXACT,  // ... its form for whole K-steps and 31-bit row offsets (h3t_exact)
  H3T_TWIN,   // ... its timing twin (pis_tune key 2, wrong results)
  H3T_TILE,   // wgrad_h3t_tile_kernel: the Winograd weight gradient on 256 x 128 (bm = 256) or 128 x 256 tiles,
              // the transposed-conv one (a_up2) on 256 x 128
};
constexpr int WT_BK = 32;  // pixels per K-step of the row-staged kernels
// what the choice needs to know about a launch's operands A (rows lda) and B (rows ldb)
struct WgradOperands {
  bool plain;        // B is read as plain rows (not gathered from a 3x3 conv's taps)
  bool a_up2;        // A is the transposed conv's dy at the up-sampled pixels
  int W, P, Np;      // image width, pixels of the reduction, columns of B (plain: the input channels)
  int lda, ldb;
  int64_t bs_a, bs_b;  // batched launches: per-batch offsets
  bool aligned16;      // both base pointers
};
// wgrad_h3t_kernel's EX form: whole K-steps in every split and 31-bit row offsets for the buffer
// loads (the batch offsets go into the base pointers)
bool h3t_exact(const WgradPlan& pl, const WgradOperands& o);
// pis_tune keys 14 (arithmetic), 31 (row staging) and 2 (timing twins). `tile`: the launch's
// 256 x 128 candidate (WinoWgradPlan::tile; bm == 0: none), taken (H3T_TILE, to be launched on
// *tile, not pl) where the keys allow fp16x3 row staging and the operands meet its contract:
// 16-byte aligned, lda / ldb / bs_a / bs_b multiples of 4, h3t_exact
WgradKernel choose_wgrad_kernel(const WgradPlan& pl, const WgradOperands& o, const WgradPlan* tile = nullptr);

struct HaloPlan {
  bool use;
  int splits, seg_per_split, nseg;
  size_t part_bytes, bias_bytes;
};

// Winograd weight gradient (csrc/winograd.hip), F(3x3, 4x4) when the 4x4 tile grid fits (pis_tune
// key 11), else F(3x3, 2x2): V = B^T x B and E = G e G^T per tile, M_xi[n][c] = sum_tiles
// E_xi[t][n] V_xi[t][c] as nxi = (m+2)^2 batched split-K GEMMs over the T tiles (slabs
// [split][xi][Cout][Cin], one fixed-order reduction), dW = A^T M A; the bias gradient is a
// channel sum of dz.
struct WinoWgradPlan {
  bool use, fused_bias, gemm_bias;
  int m, nxi;
  int64_t T;
  WgradPlan gemm;
  // pis_tune key 58: the same GEMMs on wgrad_h3t_tile_kernel's tile, where the shape is in its
  // contract and (key = 1) in the measured set; bm == 0 otherwise. It lives in gemm's workspace
  // regions: the same slab pitch, splits <= gemm.splits, pps a multiple of 32.
  WgradPlan tile;
  size_t off_E, off_part, off_M, off_cs, total;
};

constexpr int C1_BLOCKS = 1024;  // blocks (= partial slabs) of the Cin == 1 stream weight gradient

enum WgradAlgo {
  WGRAD_NONE = 0,   // outside pis_conv3x3_wgrad's channel contract
  WGRAD_DIRECT,     // direct fp16x3 (direct.hip)
  WGRAD_WINO4,      // F(3x3,4x4)
  WGRAD_WINO2,      // F(3x3,2x2)
  WGRAD_HALO,
  WGRAD_C1_STREAM,  // Cin == 1, VALU stream
  WGRAD_C1_MFMA,    // Cin == 1, padded MFMA tile
  WGRAD_GENERIC,
};

// what pis_conv3x3_bwd_prep writes for the layer
enum PrepKind {
  PREP_NONE = 0,
  PREP_DZ2,       // V(dz) for the input gradient and E for the weight gradient, one pass
  PREP_DZ2_TMAX,  // ... with the tile maxima the fused fp16x3 input gradient reads
  PREP_E_ONLY,    // the overlap-add input gradient (key 51) contracts the weight gradient's E
};

// ---- the Winograd forward / input gradient's launch variants (winograd.hip launches what these say) ----
// the batched NT GEMM M_xi = V_xi U_xi^T of the F(m x m) pipelines: one value per instantiation
enum class WinoGemm {
  IGEMM,        // the generic implicit GEMM (launch_igemm), any shape
  F32_256,      // gemm_nt_kernel<128, 256>: fp32 MFMA
  F32_128,      // gemm_nt_kernel<128, 128>
  F32_64,       // gemm_nt_kernel<128, 64>
  X6_128,       // gemm_nt_x6_kernel<128, 128>: bf16x6, K-step 16
  X6_64,        // gemm_nt_x6_kernel<128, 64>
  X6_BK32_128,  // gemm_nt_x6_bk32_kernel<128, 128, 3>: bf16x6, K-step 32 (C % 32 == 0)
  X6_BK32_64,   // gemm_nt_x6_bk32_kernel<128, 64, 3>
  H3_128,       // gemm_nt_h3_bk32_kernel<128, 128, 3>: fp16x3, K-step 32
  H3_64,        // gemm_nt_h3_bk32_kernel<128, 64, 4>
};
// pis_tune key 10 for a contraction of C channels into N outputs (F(4x4) and F(2x2)); F(6x6) runs
// the fp16x3 pair whatever the key (64-aligned N, 32-aligned C: wino6_layer)
WinoGemm choose_wino_gemm(int N, int C);
inline WinoGemm choose_wino6_gemm(int N) { return N % 128 == 0 ? WinoGemm::H3_128 : WinoGemm::H3_64; }

// the forms of the transform and fused kernels: a function of the tune state alone
struct WinoVariants {
  int vw;                    // channels per thread of the F(4x4) input / output transforms, 2 or 4 (key 17)
  bool out_mask;             // the output transforms' masked form where a mask is given (key 46, vw == 2)
  bool input_cols, dz_cols;  // single-load-phase input transform / dz passes (key 50)
  bool dgrad_t;              // format-1 input-gradient filters are the overlap-add form's U' (key 51)
  bool dgrad_t_xcd;          // ... its output transform in XCD-major block order (key 51 != 2)
  int fused_g;               // tile groups per block the fused contraction wants (key 15)
  bool fused_h3;             // the fused contraction runs in fp16x3 (key 22): scales after its filter planes, tile maxima
  bool fused_stagger;        // ... with staggered wave pairs at 64 channels (key 25)
  int f6;                    // the F(6x6) transforms: 1 / 2 channels per thread, 3 the two-half form (key 47)
  bool wgrad_out_v4;         // the float4 weight-gradient output transform (key 48)
};
// wino4_gemm_out_x6_kernel<4, 2, kc, g, h3, stg> for kc = 64 or 128 contraction channels over
// `groups` groups of 32 tiles. The staggered form is G = 4 fp16x3 (128 channels: always, where 4
// divides the groups; its lockstep form spills); otherwise a wanted G that does not divide the
// groups falls to G = 1, not to the next smaller one.
struct FusedForm {
  int kc, g;
  bool h3, stg;
};
FusedForm wino_fused_form(int kc, int64_t groups, const WinoVariants& v);

// one direction of the layer: the forward (C = Cin, N = Cout) or the input gradient (C = Cout, N = Cin)
struct ConvDirPlan {
  int C, N;            // contraction channels, outputs
  bool direct;         // pis_tune key 29's policy takes it (given 4-aligned channel strides)
  bool wino_wanted;    // the Winograd policy takes it without a kept transform
  ConvAlgo wino;       // the Winograd pipeline it then runs (ALGO_NONE: the shape has none)
  ConvAlgo wino_kept;  // ... with a kept or prepared F(4x4) transform (never F(6x6)); a kept
                       // transform also overrides wino_wanted (resolve_conv3x3)
  WinoGemm gemm;       // the batched GEMM of wino_kept's pipeline (choose_wino_gemm)
  ConvAlgo fallback;   // small workspace or no policy: halo, generic, or the Cin == 1 kernels
  size_t direct_ws, wino_ws;
  int filter_format;   // pis_conv3x3_filter_format
  size_t filter_bytes;
};

struct Conv3x3Plan {
  int B, H, W, Cin, Cout;
  ConvDirPlan fwd, dgrad;
  WinoVariants wino;  // what the Winograd launchers of either direction and of the weight gradient instantiate
  size_t keep_bytes;  // pis_conv3x3_keep_bytes
  size_t ex_ws;       // pis_conv3x3_ex_ws
  WgradAlgo wgrad;           // with 16-byte aligned operands and the workspace below
  WgradAlgo wgrad_nodirect;  // what a misaligned operand or a small workspace demotes WGRAD_DIRECT to
  size_t wgrad_ws, wgrad_ws_nodirect;
  WinoWgradPlan wino_w;  // wgrad(_nodirect) == WGRAD_WINO4 / WGRAD_WINO2
  HaloPlan halo_w;       // WGRAD_HALO
  WgradPlan gemm_w;      // WGRAD_GENERIC, WGRAD_C1_MFMA
  PrepKind prep;         // given 4-aligned ldz and both workspaces large enough
};

// a pure function of its arguments and the current tune state
Conv3x3Plan plan_conv3x3(int B, int H, int W, int Cin, int Cout);

// does the forward's output epilogue write the 2x2 max pool too?
inline bool pool_fused(ConvAlgo a) {
  return a == ALGO_DIRECT_H3 || a == ALGO_WINO6 || a == ALGO_WINO4_FUSED || a == ALGO_WINO4_GEMM;
}

// the facts only a call knows
struct ConvCall {
  bool is_dgrad;
  int lds, ldd, ldm;  // channel strides of the source, the destination and (masked) the mask
  bool masked;
  bool has_ws;
  size_t ws_bytes;
  bool kept;      // a keep buffer was passed and the layer keeps a transform
  bool prepared, filter_ready, w_unflipped;  // PIS_WINO_PREPARED, PIS_FILTER_READY, PIS_W_UNFLIPPED
};
// the algorithm this call launches, or ALGO_NONE with the PIS_ERR_ARG message set
ConvAlgo resolve_conv3x3(const Conv3x3Plan& p, const ConvCall& c);
// the weight gradient of a call that passed pis_conv3x3_wgrad's argument checks (never WGRAD_NONE),
// or WGRAD_NONE with the message set: a direct layer that cannot run direct and whose workspace
// is below the fallback's
WgradAlgo resolve_wgrad(const Conv3x3Plan& p, const void* x, const void* dz, size_t ws_bytes);

}  // namespace pis
