// The transposed-conv planner (convt_plan.hip, host only): which kernel runs a ConvTranspose2d(k=2,
// s=2) layer's forward, input gradient and weight gradient, and the weight gradient's split-K layouts
// and workspace. The only code that reads pis_tune keys 13 and 56; the entry points (igemm.hip,
// wgrad.hip) ask it, per call, and launch what it says. Arms and contracts: DESIGN.md §4b.
#pragma once
#include "conv3x3_plan.h"

namespace pis {

constexpr int WU_BM = 256, WU_BN = 128;  // block tile of wgrad_h3t_tile_kernel<false, UP2> (wgrad.hip)

enum ConvtAlgo {  // forward / input gradient
  CONVT_NONE = 0,
  CONVT_H3_K32,    // convt_h3_kernel: fp16x3, K-step 32, epilogue through LDS
  CONVT_GEMM_H3,   // convt_gemm_kernel (K-step 16) in fp16x3,
  CONVT_GEMM_X6,   // ... bf16x6,
  CONVT_GEMM_F32,  // ... fp32 MFMA
  CONVT_IGEMM,     // generic implicit GEMM (igemm.hip)
};
enum ConvtWgradAlgo {
  CONVT_WGRAD_NONE = 0,
  CONVT_WGRAD_TILE,      // wgrad_h3t_tile_kernel<false, UP2>, 256 x 128 tiles
  CONVT_WGRAD_ROWS_UP2,  // wgrad_h3t_kernel<UP2>, row-staged 128 x 128 tiles
  CONVT_WGRAD_SPLITK,    // the generic split-K kernels (choose_wgrad_kernel)
};

// a weight-gradient candidate: the shape is inside its kernel's contract, the keys want it, its layout
struct ConvtWgradCand {
  bool shape, wanted;
  WgradPlan pl;
};
struct ConvtPlan {
  int B, H, W, Cin, Cout;
  ConvtAlgo fwd, dgrad;  // given a source stride % 4 == 0; CONVT_H3_K32 also needs resolve_convt's facts,
  ConvtAlgo fallback;    // else the call runs this
  bool wgrad_contract;   // pis_convt2x2_wgrad's: Cin, Cout multiples of 64 (else no candidates, wgrad_ws 0)
  ConvtWgradCand tile, rows, splitk;
  size_t wgrad_ws;  // the maximum over the candidates WHATEVER the keys say: the engine sizes its
                    // workspace once and keys 13 and 56 may change between any two calls
};
// a pure function of its arguments and the current tune state
ConvtPlan plan_convt2x2(int B, int H, int W, int Cin, int Cout);

// the facts only a call knows
struct ConvtCall {
  bool is_dgrad;
  int lds, ldd, ldm;  // channel strides of the source, the destination and (masked) the mask
  bool masked;
  bool aligned16;  // the source, the weights, the destination and the bias / mask passed: 16-B aligned
};
ConvtAlgo resolve_convt(const ConvtPlan& p, const ConvtCall& c);
struct ConvtWgradCall {
  int ldx, lddy;
  bool aligned16;  // x and dy
};
struct ConvtWgradChoice {
  ConvtWgradAlgo algo;
  WgradKernel kernel;  // run_wgrad's, on a_up2 operands (CONVT_WGRAD_TILE: H3T_TILE)
  WgradPlan pl;
};
ConvtWgradChoice resolve_convt_wgrad(const ConvtPlan& p, const ConvtWgradCall& c);

// the transposed-conv GEMMs (convt.hip): mode 0 forward, 1 input gradient; algo: any but CONVT_IGEMM
int launch_convt_gemm(ConvtAlgo algo, int mode, const float* a, int lda, const float* bt, int B, int h, int w, int cin,
                      int cout, const float* bias, const float* mask, int ldm, float* dst, int ldd, int flags,
                      hipStream_t s);

}  // namespace pis
