// The 3x3-conv planner: every policy predicate of the layer's three products in one place
// (conv3x3_plan.h). Host code only.
#include "conv3x3_plan.h"

namespace pis {
namespace {

// F(4x4,3x3) when the 4x4 tile grid fits and pis_tune key 11 allows it, else F(2x2,3x3)
int wino_tile(int H, int W) { return (tune_get(PIS_TUNE_WINO_F4) != 0 && H % 4 == 0 && W % 4 == 0) ? 4 : 2; }

// pis_tune key 29's policy for a contraction of C channels into N outputs on an H x W grid
bool direct_h3_wanted(int H, int W, int C, int N) {
  const int mode = tune_get(PIS_TUNE_DIRECT_H3);
  if (mode == 0 || !direct_h3_shape_ok(H, W, C, N, 4)) return false;
  const int lo = std::min(C, N), hi = std::max(C, N);
  if (mode == 3)  // + dec2.conv0 (256 <-> 128 at 256^2) and enc3.conv0 (128 <-> 256 at 128^2)
    return (H >= 256 && hi <= 256) || (H >= 128 && hi <= 256 && lo <= 128);
  if (mode == 4)  // + every <= 256-channel layer at 128^2 (enc3, dec3.conv1)
    return H >= 128 && hi <= 256;
  if (mode == 5)  // + every layer at 128^2 and above
    return H >= 128;
  return mode == 2 || (hi <= 128 && H >= 256);
}

// Winograd policy (winograd.hip): where its GEMMs stay MFMA-bound and beat the direct kernels
bool wino_wanted_dims(int H, int W, int C, int N) {
  const int mode = tune_get(PIS_TUNE_WINOGRAD);
  if (mode == 0 || H % 2 || W % 2 || C % 4 || N % 4) return false;
  if (mode == 2) return true;
  // measured (tools/bench_kernels.py --key 8 --variants 1,2 --ops fwd,dgrad, B=8):
  // F(4x4,3x3) beats the direct halo kernels from 128 channels on either side (dec1.conv0
  // fwd -22 %, dgrad -27 %; enc2.conv1 -41 %) and only loses at 64 -> 64 (+1.5-3 %);
  // F(2x2,3x3) needs >= 256 contraction channels and 128 outputs. With the bf16x6 GEMMs
  // (key 10 = 3) F(4x4,3x3) also wins at 64 -> 64 (enc1.conv1 fwd -13 %, dgrad -11 %).
  if (wino_tile(H, W) == 4)
    return C >= 128 || N >= 128 || (tune_get(PIS_TUNE_WINO_TILE) >= 3 && C >= 64 && N >= 64);
  return C >= 256 && N >= 128;
}

// fused path eligibility (pis_tune key 15): F(4x4), bf16x6 GEMMs, 64 -> 64 channels. Measured
// (tools/bench_kernels.py --key 15, C2): enc1.conv1 forward 1.13 -> 0.98 ms, input gradient
// 1.30 -> 1.13 ms; with 128 input or output channels (dec1.conv0, enc2.conv0) it is 2-8 % slower
// than the separate GEMM + output transform, so those keep the 3-pass pipeline.
// Does a contraction of C channels into N outputs at B x H x W take the fused F(4x4) kernel?
bool wino_fused_wanted(int B, int H, int W, int C, int N) {
  if (wino_tile(H, W) != 4) return false;
  const int64_t T = (int64_t)B * (H / 4) * (W / 4);
  // N = 128 (64-channel contractions into 128 outputs: enc2.conv0 forward, dec1.conv0 input
  // gradient) with pis_tune key 26: two blocks per tile group, V read twice (from L2), M never
  return tune_get(PIS_TUNE_WINO_GEMM_OUT) != 0 && tune_get(PIS_TUNE_WINO_TILE) >= 3 && T % 32 == 0 &&
         T >= 2 * (int64_t)C &&  // the filter planes fit in the M region
         (C == 64 || (C == 128 && tune_get(PIS_TUNE_FUSED_K128) != 0)) &&
         (N == 64 || (N % 64 == 0 && N <= 64 * (1 << tune_get(PIS_TUNE_FUSED_WIDE))));
}

// F(6x6,3x3) for a layer's forward and input gradient (pis_tune key 47; csrc/winograd.hip
// launch_wino6; symmetric in Cin / Cout): both directions on the batched fp16x3 GEMM
// (Winograd-wanted, neither direct nor fused), 64-aligned channels, an F(4x4)-capable grid (the
// weight gradient keeps F(3x3,4x4)), and at least 10 % fewer products on the ragged 6 x 6 tile
// grid: 128^2 and 64^2 at C2 (0.84 of F(4x4)'s), not 32^2 (ceil(32 / 6)^2 x 64 = 32^2 / 16 x 36:
// no gain)
bool wino6_layer(int B, int H, int W, int Cin, int Cout) {
  if (tune_get(PIS_TUNE_WINO_F6) == 0 || tune_get(PIS_TUNE_WINO_TILE) != 4 || B <= 0) return false;
  if (wino_tile(H, W) != 4 || Cin % 64 || Cout % 64) return false;
  if (direct_h3_wanted(H, W, Cin, Cout) || direct_h3_wanted(H, W, Cout, Cin)) return false;
  if (!wino_wanted_dims(H, W, Cin, Cout) || !wino_wanted_dims(H, W, Cout, Cin)) return false;
  if (wino_fused_wanted(B, H, W, Cin, Cout) || wino_fused_wanted(B, H, W, Cout, Cin)) return false;
  const int64_t p6 = (int64_t)64 * ((H + 5) / 6) * ((W + 5) / 6), p4 = (int64_t)36 * (H / 4) * (W / 4);
  return 10 * p6 <= 9 * p4;
}

HaloPlan halo_plan(int B, int H, int W, int Cin, int Cout) {
  HaloPlan p{};
  p.use = Cin % 64 == 0 && Cout % 64 == 0 && W % 16 == 0;
  if (!p.use) return p;
  p.nseg = (int)((int64_t)B * H * W / 16);
  const int tiles = (Cout / 64) * (Cin / 64);
  const size_t slab = (size_t)Cout * 9 * Cin * sizeof(float);
  // one round of blocks (2 per CU), 512..8192 pixels per split, <= ~160 MB of partial slabs
  int64_t splits = cdiv(std::max(64, tune_get(PIS_TUNE_WGRAD_BLOCKS)), tiles);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, (int64_t)((160u << 20) / slab)));
  int64_t sps = cdiv(p.nseg, splits);
  sps = std::max<int64_t>(32, std::min<int64_t>(512, sps));
  p.seg_per_split = (int)sps;
  p.splits = (int)cdiv(p.nseg, sps);
  p.part_bytes = (size_t)p.splits * slab;
  p.bias_bytes = (size_t)p.splits * Cout * sizeof(float);
  return p;
}

// pis_tune key 58: the Winograd weight gradient's GEMMs on wgrad_h3t_tile_kernel's 256 x 128 tile,
// inside the split-K layout of p.gemm (the workspace is sized from p.gemm alone and never depends
// on the key). Shape contract: T >= 512 in whole 32-row K-steps, both channel counts multiples of
// 128 and one of 256; the wide operand is E (output channels) where Cout % 256 == 0, else V.
// Key values: 0 never; 1 the measured set (wino_tile_adopted), on trimmed splits; 2 every shape in
// the contract on p.gemm's splits; 3 every shape, with the splits trimmed to one resident generation.
constexpr int WINO_TILE_RESIDENT = 512;  // blocks: two per CU

// key 58 = 1: the shapes where the tile form's isolated time (GEMM + output transform, minimum of
// three interleaved runs) beat the 128 x 128 form's by more than the latter's spread (DESIGN.md §4
// round 11, profiles/wino_wgrad_tile_ab.txt), always on the trimmed split count where one exists.
// Measured at batch 8 of 512^2 (GEMM + output transform, ms, 128 x 128 form -> tile form):
//   one side a single 128-column tile: 128 x 256 channels at T = 32768 0.387 -> 0.340, 256 x 128
//     at T = 8192 (bf16x6 before) 0.196 -> 0.112
//   splits trimmed to one generation: 256 x 512 at T = 8192 0.384 -> 0.319 (untrimmed 0.382: no
//     gain), 512 x 256 at T = 2048 0.121 -> 0.100
//   512 x 512: T = 2048 0.207 -> 0.204, T = 512 0.072 -> 0.069 (small, but beyond the spread)
// and not: 256 x 256 at T = 8192 (0.189 -> 0.176, inside the old form's spread of 0.041) and
// 512 x 1024 at T = 2048 (0.374 -> 0.371, 576 blocks that cannot be trimmed: one split). Shapes of
// neither kind keep the 128 x 128 form.
bool wino_tile_adopted(int Cin, int Cout, bool trimmed) {
  return std::min(Cin, Cout) == 128 || trimmed || (Cin == Cout && Cin >= 512);
}

WgradPlan wino_tile_plan(const WinoWgradPlan& p, int Cin, int Cout) {
  WgradPlan t{};
  const int key = tune_get(PIS_TUNE_WINO_WGRAD_TILE);
  if (key == 0 || p.T % WT_BK || p.T < 512 || Cin % 128 || Cout % 128 || (Cin % 256 && Cout % 256)) return t;
  const bool trim = key != 2;
  bool trimmed = false;
  t = p.gemm;  // pps: a multiple of 64
  t.bm = Cout % 256 == 0 ? 256 : 128;
  t.bn = Cout % 256 == 0 ? 128 : 256;
  const int tiles = (Cout / t.bm) * (Cin / t.bn);
  // a generation and an eighth (576 blocks where the 128 x 128 plan made 1152) runs as two: fewer,
  // longer splits that fit one, where at least two remain
  const int fit = WINO_TILE_RESIDENT / (tiles * p.nxi);
  if (trim && t.splits > 1 && tiles * t.splits * p.nxi > WINO_TILE_RESIDENT && fit >= 2) {
    const int64_t pps = cdiv(cdiv(p.T, (int64_t)fit), WT_BK) * WT_BK;
    if (pps <= 8192) {  // plan_wgrad's bound on an fp32 chain
      t.pps = (int)pps;
      t.splits = (int)cdiv(p.T, pps);
      trimmed = true;
    }
  }
  if (key == 1 && !wino_tile_adopted(Cin, Cout, trimmed)) return WgradPlan{};
  return t;
}

WinoWgradPlan wino_wgrad_plan(int B, int H, int W, int Cin, int Cout) {
  WinoWgradPlan p{};
  const int mode = tune_get(PIS_TUNE_WINOGRAD);
  // auto (tools/bench_kernels.py --key 8 --variants 1,2 --ops wgrad, B=8): dec1.conv0 -25 %,
  // enc2.conv0 -15 %, 64 -> 64 -2 % against the halo kernel
  const int m = wino_tile(H, W);
  // F(3x3,4x4) everywhere on 4-aligned grids (64 -> 64 at 512^2: -2 % alone, -27 % with the
  // forward's kept transform); F(3x3,2x2) only with >= 128 on both sides
  const bool wanted = m == 4 || (Cin >= 128 && Cout >= 128);
  p.use = mode != 0 && H % 2 == 0 && W % 2 == 0 && Cin % 64 == 0 && Cout % 64 == 0 && (mode == 2 || wanted);
  if (!p.use) return p;
  p.m = m;
  p.nxi = (p.m + 2) * (p.m + 2);
  p.T = (int64_t)B * (H / p.m) * (W / p.m);
  // the nxi GEMMs share one launch: split so all of them together make ~target blocks
  p.gemm = plan_wgrad(Cout, Cin, (int)p.T, Cout, Cin, std::max(16, tune_get(PIS_TUNE_WINO_WGRAD_BLOCKS) / p.nxi));
  p.tile = wino_tile_plan(p, Cin, Cout);
  auto al = [](size_t b) { return cdiv(b, 256) * 256; };
  const size_t V = al((size_t)p.nxi * p.T * Cin * 4), E = al((size_t)p.nxi * p.T * Cout * 4);
  const size_t part = al((size_t)p.gemm.splits * p.nxi * Cout * Cin * 4), M = al((size_t)p.nxi * Cout * Cin * 4);
  p.off_E = V;
  p.off_part = V + E;
  p.off_M = p.off_part + part;
  p.off_cs = p.off_M + M;
  // bias gradient. F(3x3,4x4): the GEMM's blocks of plane xi = 7 sum their E rows per column
  // (E[7] = (1/3)^2 x the tile's dz sum, w4_g4 row 1) into [split][Cout] partials, which the output
  // transform's bias blocks reduce in fixed order (no pass, no launch of its own). Else a
  // channel-sum pass over dz.
  p.gemm_bias = p.m == 4 && ((int64_t)Cout * Cin) % 64 == 0;
  p.fused_bias = false;
  const size_t cs = p.gemm_bias ? (size_t)p.gemm.splits * Cout * sizeof(float) : colsum_ws((int64_t)B * H * W, Cout);
  p.total = p.off_cs + al(cs) + 256;
  return p;
}

// the filter operand pis_conv3x3_{fwd_keep,fwd_pool,dgrad_ex} consume ahead (pis_conv3x3_filter;
// engine shapes: kept forward transforms, prepared 32-aligned input gradients): 0 none, 1 fp32
// U[36][N][C] for the batched GEMMs, 2 the planes of the fused contraction, 3 the direct fp16x3
// kernel's weight split, 4 the F(6x6,3x3) transform U[64][N][C] (input gradient: from the
// ORIGINAL weights)
int filter_format(const Conv3x3Plan& p, const ConvDirPlan& d, bool is_dgrad, bool wino6) {
  if (p.B <= 0 || p.H <= 0 || p.W <= 0 || p.Cin % 4 || p.Cout % 4 || p.Cin < 4) return 0;
  if (wino6) return 4;
  if (d.direct) return 3;
  if (is_dgrad ? (p.Cin % 32 || p.Cout % 32 || !d.wino_wanted) : (p.keep_bytes == 0 && !d.wino_wanted)) return 0;
  return d.wino_kept == ALGO_WINO4_FUSED ? 2 : wino_tile(p.H, p.W) == 4 ? 1 : 0;
}

size_t filter_bytes(const Conv3x3Plan& p, const ConvDirPlan& d) {
  const size_t nc = (size_t)36 * p.Cin * p.Cout;
  switch (d.filter_format) {
    case 1: return nc * sizeof(float);
    case 2:  // fp16x3: hi / lo planes + one scale per output; else the three bf16x6 planes
      return p.wino.fused_h3 ? 2 * nc * sizeof(_Float16) + (size_t)d.N * sizeof(float) : 3 * nc * sizeof(__bf16);
    case 3: return d.direct_ws;
    case 4: return (size_t)64 * p.Cin * p.Cout * sizeof(float);
    default: return 0;
  }
}

// the transform and fused-kernel forms (pis_tune keys 15, 17, 22, 25, 46, 47, 48, 50, 51)
WinoVariants wino_variants() {
  WinoVariants v{};
  v.vw = tune_get(PIS_TUNE_WINO_VW) != 4 ? 2 : 4;
  v.out_mask = tune_get(PIS_TUNE_WINO_OUT_MPF) != 0;
  const int xf = tune_get(PIS_TUNE_WINO_XFORM), dt = tune_get(PIS_TUNE_WINO_DGRAD_T), go = tune_get(PIS_TUNE_WINO_GEMM_OUT);
  // key 50: 1 (default) both single-load-phase forms, 0 neither; 2 / 4 the dz passes / the input transform alone
  v.dz_cols = xf == 1 || (xf & 2) != 0;
  v.input_cols = xf == 1 || (xf & 4) != 0;
  v.dgrad_t = dt != 0;
  v.dgrad_t_xcd = dt != 2;
  v.fused_g = go == 2 ? 1 : go == 3 ? 2 : go == 4 ? 8 : 4;  // key 15: 1 -> G = 4, 2 -> 1, 3 -> 2, 4 -> 8 (experiments)
  v.fused_h3 = tune_get(PIS_TUNE_WINO_GEMM_OUT_H3) != 0;
  v.fused_stagger = tune_get(PIS_TUNE_FUSED_STAGGER) != 0;
  v.f6 = tune_get(PIS_TUNE_WINO_F6);
  v.wgrad_out_v4 = tune_get(PIS_TUNE_WGRAD_OUT) == 1;
  return v;
}

ConvDirPlan plan_dir(int B, int H, int W, int C, int N, bool is_dgrad, bool wino6) {
  ConvDirPlan d{};
  d.C = C;
  d.N = N;
  d.direct = direct_h3_wanted(H, W, C, N);
  d.direct_ws = direct_h3_ws_bytes(C, N);
  d.wino_wanted = wino_wanted_dims(H, W, C, N);
  const int m = wino_tile(H, W);
  if (H % 2 || W % 2 || C % 4 || N % 4) d.wino_kept = ALGO_NONE;
  else if (m != 4) d.wino_kept = ALGO_WINO2;
  else if (wino_fused_wanted(B, H, W, C, N)) d.wino_kept = ALGO_WINO4_FUSED;
  // pis_tune key 51: an F(4x4,3x3) input gradient on the batched GEMM (not the fused contraction,
  // the direct or the F(6x6) layers) contracts the weight gradient's E with U' and ends in the
  // overlap-add transform (wino4_output_t_kernel)
  else if (is_dgrad && tune_get(PIS_TUNE_WINO_DGRAD_T) != 0) d.wino_kept = ALGO_WINO4_DGRAD_T;
  else d.wino_kept = ALGO_WINO4_GEMM;
  // F(6x6,3x3): the deep layers' forward and input gradient (no kept or prepared F(4x4) transforms)
  d.wino = (wino6 && d.wino_kept != ALGO_NONE) ? ALGO_WINO6 : d.wino_kept;
  d.gemm = choose_wino_gemm(N, C);
  d.wino_ws = wino_ws_bytes(m, B, H, W, C, N);
  if (wino6) d.wino_ws = std::max(d.wino_ws, wino6_ws_bytes(B, H, W, C, N));
  if (!is_dgrad && C == 1) d.fallback = (N == 64 && W % 64 == 0) ? ALGO_C1_ROW : ALGO_C1_STREAM;
  else d.fallback = (tune_get(PIS_TUNE_CONV_HALO) && W % 16 == 0 && H % 8 == 0 && C % 4 == 0) ? ALGO_HALO : ALGO_IGEMM;
  return d;
}

}  // namespace

bool h3t_exact(const WgradPlan& pl, const WgradOperands& o) {
  return o.P % WT_BK == 0 && pl.pps % WT_BK == 0 &&
         ((int64_t)o.P + WT_BK) * std::max(o.a_up2 ? 0 : o.lda, o.ldb) * 4 < (int64_t(1) << 31);
}

WgradKernel choose_wgrad_kernel(const WgradPlan& pl, const WgradOperands& o, const WgradPlan* tile) {
  // the Winograd weight gradient's 256 x 128 tile candidate (key 58, wino_tile_plan): fp16x3 row
  // staging allowed by keys 14 and 31 (at key 14 = 3 also the 128-input-channel layer that else
  // runs bf16x6), no timing twin, and the operand contract of its float4 buffer loads
  if (tile && tile->bm != 0 && o.plain && !o.a_up2 && tune_get(PIS_TUNE_WGRAD_X6) >= 2 && tune_get(PIS_TUNE_WGRAD_T) != 0 &&
      tune_get(PIS_TUNE_DEBUG_NOLOAD) == 0 && o.lda % 4 == 0 && o.ldb % 4 == 0 && o.bs_a % 4 == 0 && o.bs_b % 4 == 0 &&
      o.aligned16 && h3t_exact(*tile, o))
    return WgradKernel::H3T_TILE;
  // key 14 = 3 (auto): fp16x3 where the layer has >= 256 input channels. The bf16x6
  // and fp16x3 kernels take plain B operands only, where Np IS the input-channel count (Winograd:
  // Cin; convT: Cin); the 3x3 conv's gathered operand (Np = 9 Cin) runs the fp32 MFMA kernel. Their
  // columns hold 8 pixels of an image row (a_up2: W % 8 == 0)
  const int x6 = tune_get(PIS_TUNE_WGRAD_X6);
  const bool cols = o.plain && pl.pps % 16 == 0 && (!o.a_up2 || o.W % 8 == 0);
  if (cols && (x6 == 2 || (x6 == 3 && o.Np >= 256))) {
    // key 31: the row-staged kernel for plain 128 x 128 tiles (float4 rows: 16-B aligned)
    if (tune_get(PIS_TUNE_WGRAD_T) != 0 && pl.bm == 128 && pl.bn == 128 && !o.a_up2 && pl.pps % WT_BK == 0 &&
        o.lda % 4 == 0 && o.ldb % 4 == 0 && o.bs_a % 4 == 0 && o.bs_b % 4 == 0 && o.aligned16)
      return tune_get(PIS_TUNE_DEBUG_NOLOAD) ? WgradKernel::H3T_TWIN
             : h3t_exact(pl, o)              ? WgradKernel::H3T_EXACT
                                             : WgradKernel::H3T;
    return WgradKernel::H3_COLS;
  }
  return (cols && x6 != 0) ? WgradKernel::X6 : WgradKernel::F32;
}

WinoGemm choose_wino_gemm(int N, int C) {
  const int v = tune_get(PIS_TUNE_WINO_TILE);
  if (v == 1 && N % 256 == 0) return WinoGemm::F32_256;
  // key 10 >= 3: bf16x6, on the K-step 32 single-buffer kernel where C allows (2-9 % faster,
  // tools/bench_gemm.py); there key 10 = 4 runs fp16x3 with per-K-step power-of-two tile scales
  const bool k32 = C % 32 == 0;
  if (v >= 3 && N % 128 == 0) return !k32 ? WinoGemm::X6_128 : v == 4 ? WinoGemm::H3_128 : WinoGemm::X6_BK32_128;
  if (v >= 3 && N % 64 == 0) return !k32 ? WinoGemm::X6_64 : v == 4 ? WinoGemm::H3_64 : WinoGemm::X6_BK32_64;
  if (v == 2 && N % 128 == 0) return WinoGemm::F32_128;
  if (v == 2 && N % 64 == 0) return WinoGemm::F32_64;
  return WinoGemm::IGEMM;
}

FusedForm wino_fused_form(int kc, int64_t groups, const WinoVariants& v) {
  if (v.fused_h3 && groups % 4 == 0 && (kc == 128 || v.fused_stagger)) return {kc, 4, true, true};
  return {kc, groups % v.fused_g == 0 ? v.fused_g : 1, v.fused_h3, false};
}

Conv3x3Plan plan_conv3x3(int B, int H, int W, int Cin, int Cout) {
  Conv3x3Plan p{};
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  const bool wino6 = wino6_layer(B, H, W, Cin, Cout);
  p.fwd = plan_dir(B, H, W, Cin, Cout, false, wino6);
  p.dgrad = plan_dir(B, H, W, Cout, Cin, true, wino6);
  p.wino = wino_variants();

  // weight gradient: the direct kernel where its policy takes the forward, else Winograd, halo,
  // the Cin == 1 kernels, generic
  const bool direct_w = direct_w_shape_ok(B, H, W, Cin, Cout, 4, 4) && p.fwd.direct;
  p.wino_w = wino_wgrad_plan(B, H, W, Cin, Cout);
  p.halo_w = halo_plan(B, H, W, Cin, Cout);
  if (Cout % 64 == 0 && (Cin == 1 || Cin % 64 == 0)) {  // pis_conv3x3_wgrad's contract
    if (p.wino_w.use) {
      p.wgrad_nodirect = p.wino_w.m == 4 ? WGRAD_WINO4 : WGRAD_WINO2;
      p.wgrad_ws_nodirect = p.wino_w.total;
    } else if (p.halo_w.use) {
      p.wgrad_nodirect = WGRAD_HALO;
      p.wgrad_ws_nodirect = cdiv(p.halo_w.part_bytes, 256) * 256 + p.halo_w.bias_bytes + 256;
    } else if (Cin == 1 && tune_get(PIS_TUNE_C1_WGRAD) == 0) {
      p.wgrad_nodirect = WGRAD_C1_STREAM;
      p.wgrad_ws_nodirect = (size_t)C1_BLOCKS * 10 * Cout * sizeof(float) + 512;
    } else {
      p.wgrad_nodirect = Cin == 1 ? WGRAD_C1_MFMA : WGRAD_GENERIC;
      const int P = B * H * W;
      // Cin == 1 computes a padded [Cout][64] tile and compacts it through a staging slab
      p.gemm_w = Cin == 1 ? plan_wgrad(Cout, 64, P, Cout, 64) : plan_wgrad(Cout, 9 * Cin, P, Cout, Cin);
      p.wgrad_ws_nodirect = wgrad_ws_bytes(p.gemm_w) + (Cin == 1 ? (size_t)Cout * 64 * sizeof(float) + 256 : 0);
    }
    p.wgrad = direct_w ? WGRAD_DIRECT : p.wgrad_nodirect;
    p.wgrad_ws = direct_w ? direct_w_ws_bytes(B, H, W, Cin, Cout) : p.wgrad_ws_nodirect;
  }

  // the forward's F(4x4,3x3) input transform the weight gradient can take over: the same B^T on the
  // same 6x6 patches (not where the direct weight gradient reads x itself, nor an F(6x6) forward)
  const bool tile4 = wino_tile(H, W) == 4;
  if (Cin % 4 == 0 && tile4 && !wino6 && !direct_w && p.wino_w.use && p.wino_w.m == 4)
    p.keep_bytes = (size_t)p.wino_w.nxi * p.wino_w.T * Cin * sizeof(float);

  // a kept transform is computed either way: then Winograd wins even where the plain policy
  // prefers the direct kernel (64 -> 64 at 512^2: +2 % forward, -27 % weight gradient)
  if (p.fwd.direct) p.ex_ws = std::max(p.ex_ws, p.fwd.direct_ws);
  if (p.dgrad.direct) p.ex_ws = std::max(p.ex_ws, p.dgrad.direct_ws);
  if (p.keep_bytes > 0 || p.fwd.wino_wanted) p.ex_ws = std::max(p.ex_ws, p.fwd.wino_ws);
  if (p.dgrad.wino_wanted) p.ex_ws = std::max(p.ex_ws, p.dgrad.wino_ws);

  p.fwd.filter_format = filter_format(p, p.fwd, false, wino6);
  p.dgrad.filter_format = filter_format(p, p.dgrad, true, wino6);
  p.fwd.filter_bytes = filter_bytes(p, p.fwd);
  p.dgrad.filter_bytes = filter_bytes(p, p.dgrad);

  // pis_conv3x3_bwd_prep: one pass over dz where the input gradient runs F(4x4,3x3) (an F(6x6)
  // one transforms dz itself, the direct kernels read dz themselves) and the weight gradient
  // F(3x3,4x4) on pis_conv3x3_wgrad_keep's 64-aligned channels
  if (tune_get(PIS_TUNE_WINO_DZ2) != 0 && p.wgrad != WGRAD_DIRECT && p.wino_w.use && p.wino_w.m == 4 && tile4 &&
      p.dgrad.wino_kept != ALGO_NONE && p.dgrad.wino_wanted && !p.dgrad.direct && !wino6)
    p.prep = p.dgrad.wino_kept == ALGO_WINO4_DGRAD_T                  ? PREP_E_ONLY
             : p.dgrad.wino_kept == ALGO_WINO4_FUSED && p.wino.fused_h3 ? PREP_DZ2_TMAX
                                                                          : PREP_DZ2;
  return p;
}

ConvAlgo resolve_conv3x3(const Conv3x3Plan& p, const ConvCall& c) {
  const ConvDirPlan& d = c.is_dgrad ? p.dgrad : p.fwd;
  const auto fail = [](const char* msg) { return set_error("%s", msg), ALGO_NONE; };
  const bool strides_ok = c.lds % 4 == 0 && c.ldd % 4 == 0 && (!c.masked || c.ldm % 4 == 0);
  const bool direct_ok = c.has_ws && d.direct && c.lds % 4 == 0;
  if (c.w_unflipped && !c.prepared && !(direct_ok && c.ws_bytes >= d.direct_ws) &&
      !(c.has_ws && d.wino == ALGO_WINO6 && strides_ok && c.ws_bytes >= d.wino_ws))
    return fail("pis_conv3x3_dgrad_ex: PIS_W_UNFLIPPED needs the prepared F(4x4,3x3) path, the F(6x6,3x3) one or the "
                "direct one");
  // the direct fp16x3 kernel (pis_tune key 29) where its policy takes the layer
  // (PIS_FILTER_READY here: the weights are the layer's split from pis_conv3x3_filter(s), format 3)
  if (direct_ok && !c.prepared && (c.filter_ready || c.ws_bytes >= d.direct_ws)) return ALGO_DIRECT_H3;
  const ConvAlgo w = (c.kept || c.prepared) ? d.wino_kept : d.wino;
  if (c.has_ws && w != ALGO_NONE && strides_ok && (c.kept || d.wino_wanted) && c.ws_bytes >= d.wino_ws) {
    if (c.filter_ready && w == ALGO_WINO2) return fail("launch_wino3x3: PIS_FILTER_READY needs the F(4x4,3x3) GEMM path");
    if (w == ALGO_WINO2 && c.prepared) return fail("launch_wino3x3: prepared transforms need F(4x4,3x3)");
    if (w != ALGO_WINO6 && w != ALGO_WINO4_FUSED && c.w_unflipped && (w == ALGO_WINO2 || d.N % 32 || d.C % 32))
      return fail("launch_wino3x3: unflipped weights need F(4x4,3x3) and 32-aligned channels");
    return w;
  }
  if (c.filter_ready) return fail("conv3x3: PIS_FILTER_READY but this call does not take the F(4x4,3x3) path");
  if (c.prepared)
    return fail("pis_conv3x3_dgrad_ex: PIS_WINO_PREPARED but this call does not take the Winograd path");
  // a small workspace falls through to the halo kernel (4-aligned source rows), else generic
  return (d.fallback == ALGO_HALO && c.lds % 4 != 0) ? ALGO_IGEMM : d.fallback;
}

WgradAlgo resolve_wgrad(const Conv3x3Plan& p, const void* x, const void* dz, size_t ws_bytes) {
  if (p.wgrad != WGRAD_DIRECT) return p.wgrad_nodirect;
  // the direct kernel reads x and dz as float4s: 16-B aligned base pointers (a channel slice at an
  // offset that is not a multiple of 4 floats falls through to the Winograd / halo kernels, as does
  // a workspace smaller than the direct kernel's slabs)
  if (((uintptr_t)x & 15) == 0 && ((uintptr_t)dz & 15) == 0 && ws_bytes >= p.wgrad_ws) return WGRAD_DIRECT;
  if (ws_bytes >= p.wgrad_ws_nodirect) return p.wgrad_nodirect;
  set_error("pis_conv3x3_wgrad: x / dz not 16-byte aligned or workspace below the direct kernel's; "
            "the non-direct fallback needs a larger "
            "workspace than pis_conv3x3_wgrad_ws reports for this (direct) layer");
  return WGRAD_NONE;
}

}  // namespace pis

using namespace pis;

extern "C" int pis_debug_wino_wgrad_plan(int B, int H, int W, int Cin, int Cout, int aligned, int* splits, int* blocks) {
  if (splits) *splits = 0;
  if (blocks) *blocks = 0;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1;
  const Conv3x3Plan p = plan_conv3x3(B, H, W, Cin, Cout);
  const WgradAlgo algo = (p.wgrad == WGRAD_DIRECT && aligned) ? WGRAD_DIRECT : p.wgrad_nodirect;
  if (algo != WGRAD_WINO4 && algo != WGRAD_WINO2) return -1;
  const WinoWgradPlan& w = p.wino_w;
  // wino_wgrad's operands: E[xi][T][Cout] and V[xi][T][Cin]
  const WgradOperands o{true, false, (int)w.T, (int)w.T, Cin, Cout, Cin, w.T * Cout, w.T * Cin, aligned != 0};
  const WgradKernel k = choose_wgrad_kernel(w.gemm, o, &w.tile);
  const WgradPlan& pl = k == WgradKernel::H3T_TILE ? w.tile : w.gemm;
  if (splits) *splits = pl.splits;
  if (blocks) *blocks = (Cout / pl.bm) * (Cin / pl.bn) * pl.splits * w.nxi;
  return (int)k | (k == WgradKernel::H3T_TILE ? (pl.bm == 256 ? 1 : 2) << 4 : 0);
}

extern "C" int pis_debug_wino_wgrad_kernel(int B, int H, int W, int Cin, int Cout, int aligned) {
  return pis_debug_wino_wgrad_plan(B, H, W, Cin, Cout, aligned, nullptr, nullptr);
}

extern "C" int pis_debug_wino_gemm(int N, int C) { return (N > 0 && C > 0) ? (int)choose_wino_gemm(N, C) : -1; }

extern "C" int pis_debug_wino_fused_form(int C, int T) {
  if ((C != 64 && C != 128) || T <= 0 || T % 32) return -1;
  const FusedForm f = wino_fused_form(C, T / 32, wino_variants());
  return f.g | (f.h3 ? 16 : 0) | (f.stg ? 32 : 0);
}
