// The transposed-conv planner: every policy predicate of the layer's three products in one place
// (convt_plan.h; the arms, their contracts and the measurements behind them: DESIGN.md §4b). Host only.
#include "convt_plan.h"

namespace pis {
namespace {

// wgrad_h3t_tile_kernel<false, UP2>: one resident generation of about 512 blocks, chains of 512 .. 8192 pixels
WgradPlan plan_convt_tile(int Mp, int Np, int P) {
  WgradPlan p{};
  p.bm = WU_BM;
  p.bn = WU_BN;
  const int tiles = (Mp / WU_BM) * (Np / WU_BN);
  const int64_t want_splits = std::max<int64_t>(1, cdiv(512, tiles));
  int64_t pps = std::min<int64_t>(std::max<int64_t>(512, cdiv(P, want_splits)), 8192);
  pps = cdiv(pps, WT_BK) * WT_BK;
  p.pps = (int)pps;
  p.splits = (int)cdiv(P, pps);
  p.part_bytes = (size_t)p.splits * Mp * Np * sizeof(float);
  p.bias_bytes = (size_t)p.splits * Mp * sizeof(float);
  return p;
}

// key 13's kernel for a GEMM of M pixels into N columns; N = 4 Cout (forward) or Cin (input gradient)
ConvtAlgo plan_dir(int key, int M, int N, int W, int Cin, int Cout) {
  if (key == 0 || Cin % 16 || Cout % 16) return CONVT_IGEMM;
  const bool k32 = M % 128 == 0 && N % 128 == 0 && W % 32 == 0 && Cout % 32 == 0 && Cin % 32 == 0;
  if (key == 4) return k32 ? CONVT_H3_K32 : CONVT_GEMM_H3;
  return key == 1 ? CONVT_GEMM_X6 : key == 3 ? CONVT_GEMM_H3 : CONVT_GEMM_F32;
}

}  // namespace

ConvtPlan plan_convt2x2(int B, int H, int W, int Cin, int Cout) {
  ConvtPlan p{};
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  const int key = tune_get(PIS_TUNE_CONVT_GEMM), P = B * H * W;
  p.fwd = plan_dir(key, P, 4 * Cout, W, Cin, Cout);
  p.dgrad = plan_dir(key, P, Cin, W, Cin, Cout);
  p.fallback = CONVT_GEMM_H3;

  p.wgrad_contract = B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 64 == 0;
  if (!p.wgrad_contract) return p;
  const int Mp = 4 * Cout;
  p.tile.shape = W % WT_BK == 0 && Cin % WU_BN == 0 && Mp % WU_BM == 0;
  p.tile.wanted = tune_get(PIS_TUNE_CONVT_WGRAD_TILE) != 0 && key == 4;
  if (p.tile.shape) p.tile.pl = plan_convt_tile(Mp, Cin, P);
  p.rows.pl = plan_wgrad(Mp, Cin, P, Mp, Cin);  // 128 x 128 tiles (taps may share one)
  p.rows.shape = W % 32 == 0 && Mp % 128 == 0 && Cin >= 256 && Cin % 128 == 0 && p.rows.pl.pps % WT_BK == 0;
  p.rows.wanted = key == 4;
  p.splitk.pl = plan_wgrad(Mp, Cin, P, Cout, Cin);  // tiles inside one tap
  p.splitk.shape = p.splitk.wanted = true;
  p.wgrad_ws = std::max(wgrad_ws_bytes(p.splitk.pl), wgrad_ws_bytes(p.rows.pl));
  if (p.tile.shape) p.wgrad_ws = std::max(p.wgrad_ws, wgrad_ws_bytes(p.tile.pl));
  return p;
}

ConvtAlgo resolve_convt(const ConvtPlan& p, const ConvtCall& c) {
  const ConvtAlgo a = c.is_dgrad ? p.dgrad : p.fwd;
  if (c.lds % 4) return CONVT_IGEMM;
  if (a != CONVT_H3_K32) return a;
  // float4 rows of every operand, 16-B pixel stores
  const bool vec = c.ldd % 4 == 0 && c.aligned16 && (!c.is_dgrad || !c.masked || c.ldm % 4 == 0);
  return vec ? a : p.fallback;
}

ConvtWgradChoice resolve_convt_wgrad(const ConvtPlan& p, const ConvtWgradCall& c) {
  const bool vec = c.ldx % 4 == 0 && c.lddy % 4 == 0 && c.aligned16;  // float4 rows of x and dy
  if (p.tile.shape && p.tile.wanted && vec) return {CONVT_WGRAD_TILE, WgradKernel::H3T_TILE, p.tile.pl};
  WgradOperands o{};
  o.plain = true; o.a_up2 = true; o.W = p.W; o.P = p.B * p.H * p.W; o.Np = p.Cin;
  o.lda = c.lddy; o.ldb = c.ldx; o.aligned16 = c.aligned16;
  if (p.rows.shape && p.rows.wanted && vec)
    return {CONVT_WGRAD_ROWS_UP2, h3t_exact(p.rows.pl, o) ? WgradKernel::H3T_EXACT : WgradKernel::H3T, p.rows.pl};
  return {CONVT_WGRAD_SPLITK, choose_wgrad_kernel(p.splitk.pl, o), p.splitk.pl};
}

}  // namespace pis

using namespace pis;

extern "C" size_t pis_convt2x2_wgrad_ws(int B, int H, int W, int Cin, int Cout) {
  return plan_convt2x2(B, H, W, Cin, Cout).wgrad_ws;
}

extern "C" int pis_debug_convt2x2_wgrad_tile_splits(int B, int H, int W, int Cin, int Cout) {
  const ConvtPlan p = plan_convt2x2(B, H, W, Cin, Cout);
  return p.tile.shape ? p.tile.pl.splits : 0;
}

extern "C" int pis_debug_convt2x2_algo(int op, int B, int H, int W, int Cin, int Cout, int ld_src, int ld_dst,
                                       int aligned16) {
  const ConvtPlan p = plan_convt2x2(B, H, W, Cin, Cout);
  if (op == 0 || op == 1)
    return resolve_convt(p, ConvtCall{op == 1, ld_src, ld_dst, ld_dst, op == 1, aligned16 != 0});
  if (op != 2 || !p.wgrad_contract) return 0;
  const ConvtWgradChoice c = resolve_convt_wgrad(p, ConvtWgradCall{ld_src, ld_dst, aligned16 != 0});
  return c.algo | (c.algo == CONVT_WGRAD_TILE ? 0 : (int)c.kernel + 1) << 4 | (c.pl.bm / 64) << 8 | (c.pl.bn / 64) << 12;
}
