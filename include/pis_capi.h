/*
 * pis_capi.h — C-ABI of the MI355X (gfx950) training-step kernels for the
 * PDE-constrained U-Net (seemapoudel58/Physics_informed_image_segmentation).
 *
 * The reference is pure Python/PyTorch: its "operator API" is the module
 * surface of src/unet.py, src/pde.py, src/loss.py, src/metrics.py and the step
 * loop of src/train.py. Every entry point below replaces the ATen op(s) the
 * reference reaches at the cited line; the Python mirror of the reference
 * interface (physics_informed_image_segmentation_amd/) binds them with ctypes
 * (INTEGRATION.md).
 *
 * Conventions
 *  - Activations are pixel-major NHWC fp32. "ld*" is the channel stride of a
 *    tensor (elements between consecutive pixels), so a producer can write
 *    straight into a channel slice of a concat buffer (src/unet.py:190-202).
 *  - Conv weights are KRSC ([Cout][3][3][Cin]) = the physical layout of an
 *    OIHW channels_last parameter; ConvTranspose weights are stored
 *    [2][2][Cout][Cin] (logical (Cin, Cout, 2, 2), state_dict compatible).
 *  - The caller owns every buffer (workspace included); nothing allocates,
 *    nothing synchronises; kernels are launched on `stream` (a hipStream_t).
 *  - Return 0 on success, a negative PIS_ERR_* otherwise; the message is in
 *    pis_last_error() (thread-local). No C++ exception crosses the ABI.
 */
#ifndef PIS_CAPI_H
#define PIS_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pis_stream_t; /* hipStream_t */

#define PIS_OK 0
#define PIS_ERR_ARG (-1)
#define PIS_ERR_LAUNCH (-2)
#define PIS_ERR_WORKSPACE (-3)

/* epilogue / behaviour flags */
#define PIS_RELU 1       /* y = max(y, 0)                                     */
#define PIS_SCALE 2      /* y *= scale[b*C + c]  (Dropout2d keep-scale)       */
#define PIS_MASK 4       /* y *= (mask[pix*ldm + c] > 0)  (ReLU backward)     */
#define PIS_ACCUMULATE 8 /* dst += result instead of dst = result             */
#define PIS_WINO_PREPARED 16 /* conv3x3 dgrad_ex / wgrad_keep: pis_conv3x3_bwd_prep already wrote this
                                layer's dz transforms into the call's workspace          */
#define PIS_W_UNFLIPPED 32   /* conv3x3 dgrad_ex with PIS_WINO_PREPARED: w_flip is the layer's ORIGINAL
                                KRSC weight (the F(4x4) filter transform rotates it in place) */
#define PIS_FILTER_READY 64  /* conv3x3 fwd_ex / fwd_keep / fwd_pool / dgrad_ex: the weight argument is
                                the layer's filter transform from pis_conv3x3_filter (same shape and
                                direction), so the call launches no filter transform of its own */

const char* pis_last_error(void);
int pis_version(void);

/* Kernel-variant knobs (process-wide). value < 0 queries; returns the previous
 * value or PIS_ERR_ARG. Defaults are the measured best on MI355X.            */
#define PIS_TUNE_IGEMM_BK 1 /* implicit-GEMM K-step: 16 or 32 */
#define PIS_TUNE_DEBUG_NOLOAD 2 /* timing only: implicit GEMM skips its global loads (wrong results) */
#define PIS_TUNE_CONV_HALO 3 /* 1: 3x3 conv fwd/dgrad from a staged input halo (W%16==0, H%8==0) */
#define PIS_TUNE_HALO_VARIANT 4 /* 0: auto, 1: 4-channel slices for BN=64, 2: BN=256 tiles when N >= 256, 3: 8-channel slices for BN=64 */
#define PIS_TUNE_WGRAD_VARIANT 5 /* 0: one 16-pixel segment per stage, 1: two (default) */
#define PIS_TUNE_WGRAD_BLOCKS 6  /* target workgroups of the split-K halo wgrad (default 512: one round at 2 per CU) */
#define PIS_TUNE_C1_WGRAD 7      /* Cin == 1 weight gradient: 0 VALU stream kernel (default), 1 padded MFMA tile */
#define PIS_TUNE_WINOGRAD 8      /* 3x3 convs: 0 direct only; 1 (default) Winograd for fwd/dgrad (*_ex) with >= 256
                                    contraction and >= 128 output channels, for wgrad with >= 128 in and out;
                                    2 Winograd whenever legal */
#define PIS_TUNE_WINO_WGRAD_BLOCKS 9 /* target workgroups of the batched Winograd weight-gradient GEMMs (default 1024;
                                        2048 until round 3: the C2 step 0.6 % slower, profiles/r3_q33_ab_wgrad_blocks.txt) */
#define PIS_TUNE_WINO_TILE 10    /* Winograd batched GEMM: 0 generic igemm, 1 lean NT GEMM 128x256 (N % 256 == 0), 2 lean NT GEMM
                                    128x128|64 on fp32 MFMA, 3 the same at fp32 accuracy on bf16 MFMA ("bf16x6": exact
                                    3-way bf16 split of each operand, the six partial products >= 2^-24), 4 (default)
                                    "fp16x3" on fp16 MFMA: each K-step's operand tiles scaled by a power of two into
                                    fp16 range, split into hi + lo fp16 (22 significant bits), the three products
                                    above 2^-22 accumulated in fp32 (measured error below fp32 MFMA's and bf16x6's) */
#define PIS_TUNE_WINO_F4 11      /* Winograd tile: 0 F(2x2,3x3) fwd/dgrad + F(3x3,2x2) wgrad; 1 (default) F(4x4,3x3) +
                                    F(3x3,4x4) when H % 4 == W % 4 == 0 */
#define PIS_TUNE_WINO_FUSED 12   /* retired (round 3): the one-kernel F(4x4,3x3) was slower than the 3-pass pipeline
                                    on every layer; the key is accepted and ignored */
#define PIS_TUNE_CONVT_GEMM 13   /* transposed conv fwd/dgrad: lean NT GEMM with gather/scatter addressing when
                                    Cin, Cout % 16 == 0 — 4 (default) fp16x3, K-step 32 with the loads two K-steps
                                    ahead, epilogue through LDS (16-B pixel stores), and the weight gradient on the
                                    row-staged split-K kernel where Cin >= 256 (needs M, N % 128, w % 32; else 3);
                                    3 fp32-class fp16x3 on fp16 MFMA, K-step 16 (per-wave, per-K-step power-of-two
                                    scales), 1 bf16x6 on bf16 MFMA, 2 on fp32 MFMA; 0 generic implicit GEMM. The
                                    contract of every arm, and the only code that reads the key: the planner,
                                    csrc/convt_plan.h ("Transposed-conv arms") */
#define PIS_TUNE_WGRAD_X6 14     /* Winograd and transposed-conv weight-gradient GEMMs: 3 (default) fp16x3 where the
                                    layer has >= 256 input channels, bf16x6 elsewhere; 1 fp32-accurate bf16x6 on
                                    bf16 MFMA everywhere, 2 fp16x3 (as key 10 = 4) everywhere (-1 % on the step: the
                                    512^2 layers are HBM-bound), 0 fp32 MFMA */
#define PIS_TUNE_WINO_GEMM_OUT 15 /* F(4x4,3x3) 64 -> 64 channels: 1 (default) the 36 bf16x6 contractions fused with
                                     the output transform (M stays on chip; 4 groups of 32 tiles per block), 2 / 3 / 4
                                     the same with 1 / 2 / 8 groups per block (bitwise equal), 0 separate GEMM +
                                     output transform */
#define PIS_TUNE_WINO_DZ2 16     /* pis_conv3x3_bwd_prep: 1 (default) one pass over dz for both transforms, 0 off */
#define PIS_TUNE_WINO_VW 17      /* F(4x4) input / output transforms: 2 (default: half the registers, +2-11 % on the
                                    512^2-256^2 layers) or 4 channels per thread */
#define PIS_TUNE_LOSS_ROWS 18     /* pis_loss_fwd with W % 4 == 0: 1 (default) whole-row bands, 0 16x128 tiles;
                                    both followed by the one-block fixed-order finalize (deterministic) */
#define PIS_TUNE_LOSS_ROWMUL 19  /* whole-row loss forward: rows per block multiplier (1 default: about 1024 blocks;
                                    2, 4: fewer blocks, more row batches per thread) */
#define PIS_TUNE_SLAB_CHUNKS 20  /* thousands of partial slabs over <= 1024 columns (bias gradients): 1 (default)
                                    two-pass chunked row reduction, 0 one column per block. Applies to
                                    reduce_slabs and weights-only reduce_slabs2 calls; a weights + bias
                                    pair is always one merged single-pass launch (csrc/wgrad.hip) */
#define PIS_TUNE_WGRAD_PAIR 21   /* bf16x6 weight-gradient GEMM, 64-wide operand tiles: 0 (default) one 4-pixel run per
                                    lane (2-way conflicted ds_write_b64), 1 lane pairs stage the two 8-B halves of one 16-B
                                    chunk (conflict-free; the two 128-B pixel rows per load cost more: enc1.conv1 -4 %, up1
                                    +9 %, step -0.4 %) */
#define PIS_TUNE_WINO_GEMM_OUT_H3 22 /* the fused 64 -> 64 kernel (key 15): 1 fp16x3 (per-(tile, xi, K-step) power-of-two
                                        scales, hi + lo fp16, 3 products; its filter planes, also those written by
                                        pis_conv3x3_filter(s), switch format with it), 0 bf16x6 */
#define PIS_TUNE_WINO_H3_PRE 23  /* retired (round 3): producer-written row scales for the batched fp16x3 GEMM measured
                                    slower (GEMM +10 %, input transform +11 %, profiles/r2_q65_*); ignored */
#define PIS_TUNE_WINO_PERSIST 24 /* retired (round 3): the persistent batched GEMM was within +-1 % per layer and
                                    +0.4 % on the step (profiles/r2_q70_*, r2_q72_*); ignored */
#define PIS_TUNE_FUSED_STAGGER 25 /* fused 64 -> 64 kernel in fp16x3 (key 22): 1 the SIMD-partner waves fold one xi late
                                     (stagger; bit-for-bit the same), 0 (default) all waves in lockstep */
#define PIS_TUNE_FUSED_WIDE 26   /* v: the fused contraction + output transform (key 15) for up to 64 x 2^v output
                                    channels (N / 64 blocks per tile group, V re-read from L2, M never written):
                                    2 (default, N <= 256; enc3.conv0 forward -9 %), 1 (N <= 128: enc2.conv0 forward
                                    -21 %, dec1.conv0 input gradient -20 %), 0: 64 outputs only */
#define PIS_TUNE_FUSED_K128 27   /* 1 (default): the fused contraction + output transform also for 128-channel
                                    contractions (128 -> 64, and 128 -> 128 with key 26; the SIMD-partner waves always
                                    staggered: dec1.conv0 forward -11 %, enc2.conv0 input gradient -15 %);
                                    0: 64-channel contractions only */
#define PIS_TUNE_FUSED_PAIR 28   /* retired (round 3): two xi per barrier in the fused kernel was not faster; ignored */
#define PIS_TUNE_DIRECT_H3 29   /* direct 3x3 conv in fp16x3 (csrc/direct.hip; forward, input and weight gradient):
                                   0 off (Winograd / halo kernels), 1 (default) auto: the shallow layers (<= 128
                                   channels on both sides, H >= 256),
                                   2 every shape it covers (H % 8, W % 32, C % 16, N % 64 == 0),
                                   3 auto + the 128 <-> 256-channel layers at 256^2 and 128^2, 4 H >= 128 and
                                   <= 256 channels, 5 H >= 128 (3/4/5 measured slower on the C2 step:
                                   profiles/r3_q8_direct_policy.txt) */
#define PIS_TUNE_DIRECT_WG 30    /* retired (round 3): the double-buffered direct weight gradient (2-row tiles, 512
                                    registers per lane) measured slower than the single-buffer kernel, an eight-wave
                                    form neutral (profiles/r3_q19_wg8.txt); ignored */
#define PIS_TUNE_WGRAD_T 31      /* fp16x3 weight-gradient GEMM (key 14) on plain 128 x 128 tiles (the Winograd weight
                                    gradient): 1 operands staged as stored (float4 rows, transposed LDS reads, 32-pixel
                                    K-steps, block-wide scales), 0 the column-staged wgrad_h3_kernel */
#define PIS_TUNE_DIRECT_PIPE 32  /* direct fp16x3 input gradient (key 29): 1 (default) the epilogue's ReLU-mask rows
                                    loaded during the last chunk's MFMAs (enc1.conv1 -12 %), 0 in the epilogue */
#define PIS_TUNE_DIRECT_W8 33    /* retired (round 3): an 8-wave two-stage direct forward / input gradient (16-row tiles,
                                    one block per CU, next chunk's weights by LDS-DMA and its halo split while this
                                    chunk multiplies) measured 3-14 % slower than the 4-wave kernel
                                    (profiles/r3_q26_direct_w8.txt); ignored */
#define PIS_TUNE_DIRECT_WSTRIP 34 /* retired (round 5): the 2-row strip, LDS-ring and software-pipelined direct weight
                                     gradients measured 1.6-1.8 % slower on the C2 step than the 4-row kernel
                                     (profiles/r4_a_*, r4_b_ab_wblk.txt, r4_k_*); removed, the key is ignored */
#define PIS_TUNE_DIRECT_WBLOCKS 35 /* retired (round 5) with key 34; ignored */
#define PIS_TUNE_HEAD_LOSS_ROWS 36 /* pis_head_loss_fwd: image rows per block (0, default: 4096 / W, at most 16,
                                       doubled while the row bands exceed 2048; 8 at C2 measured 131 us against
                                       134-145 at 16, profiles/r4_ah_head_loss_rows.txt) */
#define PIS_TUNE_DIRECT_WGRAD_ALL 37 /* retired (round 5): the strip weight gradient on every layer was 6.3 % slower
                                        (profiles/r4_a_bench_k37_1.json); ignored */
#define PIS_TUNE_HEAD_LOSS_WIDE 38 /* pis_head_loss_fwd with W % 512 == 0: 1 (default) 1024-thread blocks (16 waves,
                                       one staged row per chunk), 2 the same with three register sets in flight
                                       (measured equal, profiles/r4_q_head_loss_fwd.txt), 0 the 256-thread form */
#define PIS_TUNE_WGRAD_T_DEPTH 39 /* retired (round 5): a third register set in wgrad_h3t_kernel was neutral
                                      (profiles/r4_f_ab.txt); two sets always; ignored */
#define PIS_TUNE_DZ_VW 40 /* retired (round 5): the dz passes take 2 channels per thread wherever 256 % (N / 2) == 0
                               (4 otherwise; the choice measured neutral, profiles/r4_g_ab.txt); ignored */
#define PIS_TUNE_GEMM_256 41 /* retired (round 5): the 256 x 256 LDS-DMA fp16x3 GEMMs measured 25-40 % slower per GEMM
                                  (profiles/r4_i_gemm_256.txt, r4_j_gemm_256_ring.txt); removed; ignored */
#define PIS_TUNE_LAST_WGRAD_MAIN 42 /* host schedule (physics_informed_image_segmentation_amd/unet.py): 1 (default) the
                                         step's last weight gradient (enc1.conv0) on the main stream, idle after
                                         enc1.conv1's input gradient, beside the side stream's enc1.conv1 weight
                                         gradient; 0 on the side stream after it (measured neutral: 22.67 vs
                                         22.66 ms, profiles/r4_l_ab_sched.txt) */
#define PIS_TUNE_DIRECT_W_VWALK 43 /* the 4-row direct weight gradient (key 34 = 0): 1 (default) each block walks a
                                        contiguous run of tiles down the image columns (vertical neighbours share
                                        two x halo rows: L2 hits) with the pairs of one split on one XCD; 0 the
                                        round-3 strided tile order. HBM reads per launch 2218 -> 1674 MB on
                                        dec1.conv0 (1.38x -> 1.04x algorithmic; enc1.conv1 1.03x either way,
                                        profiles/r4_o_direct_wgrad_traffic.txt), time unchanged (r4_n) */
#define PIS_TUNE_DIRECT_WGRAD_MAIN 44 /* retired as a tune key (ignored): the choice moved to the host schedule's
                                           PIS_DIRECT_WGRAD_MAIN environment variable (unet.py), whose default
                                           since round 5 is 1 = direct weight gradients on the main stream, the
                                           side stream ordered after them before its next weight gradient or
                                           bucket all-reduce */
#define PIS_TUNE_GEMM_PRIO 45 /* retired (round 5): s_setprio in the Winograd GEMM was neutral
                                   (profiles/r4_s_ab_gemm_prio.txt); ignored */
#define PIS_TUNE_WINO_OUT_MPF 46 /* Winograd output transform of a masked input gradient: 1 (default) the tile's
                                      ReLU-mask rows loaded with its M values (one memory round trip per tile,
                                      151 VGPRs); 0 in the epilogue. Step 22.25 -> 22.04 ms on one box, 22.43 ->
                                      22.39 on another (profiles/r4_t_ab_wino_out_mpf.txt, r4_u_*): 0.2-0.9 % */
#define PIS_TUNE_WINO_F6 47 /* Winograd F(6x6,3x3) for the forward and input gradient of the deep layers whose
                               contractions run the batched fp16x3 GEMM both ways (csrc/conv3x3_plan.hip
                               wino6_layer: 64-aligned channels, neither direct nor fused, >= 10 % fewer
                               products than F(4x4) on the ragged 6 x 6 tile grid — 128^2 and 64^2 at C2;
                               their weight gradients keep F(3x3,4x4) with their own transforms): 0
                               (default) F(4x4,3x3) with the kept / prepared transforms; 1 F(6x6), one
                               channel per thread in the transforms; 2 two channels; 3 two channels with
                               runtime-looped (lower-register) transforms. Measured slower on the C2 step
                               (358.7 vs 366.8 img/s, profiles/r6_f6*): the GEMMs -12 % per F(6x6)
                               launch but the 64-value transforms run at ~0.65 of F(4x4)'s bytes/s and
                               the weight gradients' own transforms load the side stream. Sizes
                               the workspaces and filter operands: needs a freshly planned engine */
#define PIS_TUNE_WGRAD_OUT 48 /* the F(3x3,4x4) weight gradient's slab sum + output transform
                                 (csrc/winograd.hip launch_wino_wgrad_out): 0 64 entries per block, one
                                 float per lane per slab row; 1 (default) float4 lanes, 64-256 entries
                                 per block (bitwise equal: same sums in the same order) */
#define PIS_TUNE_DIRECT_W_ROWS 49 /* the direct weight gradient's tile rows (csrc/direct.hip): 2 (default) two
                                     blocks per CU (51 KB LDS, <= 256 registers each), no register prefetch;
                                     4 (any other value) one block per CU, the next tile's loads in registers.
                                     2 vs 4: -2..-10 % per layer isolated, step 22.08 -> 21.76 ms
                                     (profiles/r6_d1_direct_wgrad_rows.txt). Sizes the weight-gradient
                                     workspace: needs a freshly planned engine */
#define PIS_TUNE_WINO_XFORM 50 /* the F(4x4) input transform and merged dz pass (csrc/winograd.hip
                                  wino4_input_cols_kernel / wino4_dz2_cols_kernel): 1 (default) the whole 6 x 6
                                  patch in one branch-free load phase (clamped coordinates, the border ring
                                  zeroed by a select), outputs produced column by column and stored as
                                  produced, E from the patch's interior (bitwise equal: same sums in the same
                                  order; dz2 162 -> 111 VGPRs, 140 -> 117 us per launch); 0 the row-by-row
                                  kernels (a full memory wait per patch row, the interior read twice);
                                  2 / 4: the dz pass / the input transform alone (the per-part A/B,
                                  profiles/r7_ab_wino_xform.txt) */
#define PIS_TUNE_WINO_DGRAD_T 51 /* F(4x4,3x3) input gradients on the batched GEMM (not the fused contraction, the
                                   direct kernel or F(6x6)): 1 the adjoint of the forward algorithm — the
                                   contraction reads the weight gradient's E = G4 dz G4^T (one dz transform for
                                   both gradients; pis_conv3x3_bwd_prep writes no V(dz)) with the filter
                                   U' = G' g G'^T of the unrotated weights, and the output transform
                                   overlap-adds the 6 x 6 patches (csrc/winograd.hip wino4_output_t_kernel: 64
                                   loads per tile instead of 36, blocks in XCD-major order so that a tile's
                                   neighbours share its L2; 2: the same without that order, its A/B); 0 V(dz) =
                                   BT patch BT^T with the rotated filter. Default 1: C2 step 21.77 -> 21.46 ms in
                                   one process, below in every round (profiles/r8_dgrad_t_ab.txt). Not bitwise
                                   equal to 0 (both about 1.1e-6 from float64). The key must not
                                   change between a pis_conv3x3_filter(s) / pis_conv3x3_bwd_prep and the
                                   pis_conv3x3_dgrad_ex that consumes it (the latter is checked) */
#define PIS_TUNE_PROB_VARIANT 52 /* pis_probability_table (csrc/probability.hip), a bit set; every form gives the same
                                    integers. 0 (default, the fastest on a constant field): every bin through LDS
                                    atomics, two histograms per block, equal neighbouring pixels of a lane merged
                                    into one add. 1: the two end bins counted per wave by ballot + popcount instead
                                    (+10 %); 2: four histograms per block (equal); 4: one LDS atomic per pixel,
                                    no merging (+15-25 % on constant and saturated fields). Measured in
                                    profiles/probability_metrics.txt by tools/bench_probability.py */
#define PIS_TUNE_DIRECT_MFMA16 53 /* the MFMA shape of the direct fp16x3 kernels (csrc/direct.hip), a bit set; a set
                                     bit = v_mfma_f32_16x16x32_f16, on which the chip holds a higher clock than on
                                     32x32x16 at equal cycles per FLOP. Bit 0: forward / pooled forward / input
                                     gradient (a K = 32 step spans two taps of a 16-channel chunk, the ninth tap
                                     takes 2 MFMAs: 14 per 16 x 16 tile and chunk against 13.5; set:
                                     conv3x3_h3_kernel<...>, clear: conv3x3_h3_alt_kernel<...>). Bit 1: the 2-row
                                     weight gradient (one K = 32 step per 32-pixel tile row; set:
                                     conv3x3_wgrad_h3r_kernel<2>, clear: conv3x3_wgrad_h3r_alt_kernel<2>). Default 3:
                                     -3..-8 % per launch, C2 step 20.70 -> 20.17 ms in one process
                                     (profiles/mfma16_direct_ab.txt). Same weight planes, slabs and workspaces for
                                     every value (the key may change between any two calls); the sums differ by
                                     their grouping only (all fp32-class against float64) */
#define PIS_TUNE_EVOLVE_T 54 /* pis_pde_evolve (csrc/evolve.hip): T, the explicit steps one launch advances inside
                                LDS (temporal blocking): 1, 2, 4 or 8, anything else is PIS_ERR_ARG. Every value
                                gives the same bits; 1 is the one-step-per-launch form. Default 8: the lowest
                                64-step time at 8 x 512^2 with mu = 0, 206.7 us against 267.7 (T = 4), 414.1
                                (T = 2) and 705.7 (T = 1); with the u0 plane staged (mu != 0) T = 4 is 17 %
                                faster there and 2 % slower at 2048^2 (tools/bench_evolve.py,
                                profiles/pde_evolve.txt). The key may change between any two calls (the
                                workspace does not depend on it) */
#define PIS_TUNE_EDT_PRUNE 55 /* pis_edt_sq / pis_surface_distances (csrc/distance.hip): what the row pass's outward
                                 search skips. 0: nothing; 1: whole 64-column blocks of radii, by the minimum of the
                                 column distances over the segments a block touches; 3: and 8-column steps, by the
                                 minima of the aligned groups a step touches. Anything else is PIS_ERR_ARG. Every
                                 value gives the same integers and uses the same workspace (the key may change
                                 between any two calls). Default 3: the lowest time of pis_edt_sq on disc-mask
                                 boundaries at 8 x 512^2 (the rule, fixed before measuring), 150.4 us against 156.3
                                 (1) and 158.3 (0); one set pixel in a corner of 2048^2 takes 421.9 / 458.2 /
                                 3247.5 us (tools/bench_surface.py, profiles/surface_metrics.txt) */
#define PIS_TUNE_CONVT_WGRAD_TILE 56 /* pis_convt2x2_wgrad (csrc/wgrad.hip): 1 (default) the fp16x3 kernel on 256 x 128
                                 block tiles (wgrad_h3t_tile_kernel<false, UP2>: 256 columns (i, j, o) of dy x 128
                                 input channels; a K-step of 32 pixels is staged once per tile, about 512 blocks,
                                 chains of 512 .. 8192 pixels) where key 13 = 4, W % 32 == 0, Cin % 128 == 0, (4 Cout) % 256 == 0, the strides
                                 are multiples of 4 and the operands 16-B aligned; 0: the 128 x 128 row-staged
                                 kernel (Cin >= 256) and the column-staged bf16x6 kernel, as every other shape.
                                 The key may change between any two calls: pis_convt2x2_wgrad_ws is the maximum
                                 over every plan. The contract and the only code that reads the key: the planner,
                                 csrc/convt_plan.h ("Transposed-conv arms") */
#define PIS_TUNE_UNROLL_TB 57 /* pis_pde_unroll_fwd / pis_pde_unroll_bwd (csrc/evolve.hip) called with tb = 0: Tb, the
                                 explicit steps one checkpoint spans and one reverse launch sweeps back inside LDS:
                                 1, 2 or 4, anything else is PIS_ERR_ARG. Every value gives the same bits. The rule
                                 for the default, fixed before measuring: the lowest forward-plus-backward time of
                                 16 steps at 8 x 512^2, mu = 0, clamp on. Default 2: about 279 us there against
                                 303 (Tb = 4) and 400 (Tb = 1); at 64 x 128^2 Tb = 4 is 3 % ahead of 2
                                 (tools/bench_unroll.py, profiles/pde_unroll.txt). The checkpoint stack is
                                 ceil(steps / Tb) - 1 maps. A forward and its backward must use the same Tb: a
                                 caller that cannot rule out a change of the key in between reads it once and
                                 passes tb explicitly (pde.py does) */
#define PIS_TUNE_WINO_WGRAD_TILE 58 /* pis_conv3x3_wgrad / _wgrad_keep, the Winograd weight gradient's batched GEMM
                                 (csrc/wgrad.hip): the fp16x3 row-staged kernel on 256 x 128 block tiles
                                 (wgrad_h3t_tile_kernel<WB>, key 56's kernel on the plain operands: 256 columns of
                                 E x 128 of V where Cout % 256 == 0, else 128 x 256; a K-step's 32 rows are staged
                                 once per tile). Contract: T = B (H/m) (W/m) tiles with T % 32 == 0 and T >= 512, Cin and Cout multiples of 128 and one
                                 of them of 256, keys 14 >= 2 and 31 != 0, 16-byte aligned operands. 0: never (the
                                 128 x 128 kernels and bf16x6, as every shape outside the contract); 1 (default):
                                 the shapes the planner's measured rule names (csrc/conv3x3_plan.hip
                                 wino_tile_adopted); 2: every shape in the contract, on the
                                 plan's split count; 3: every shape, the splits trimmed to one resident generation
                                 of blocks. The key may change between any two calls: pis_conv3x3_wgrad_ws does not
                                 depend on it (the tile form writes its slabs into the regions the 128 x 128 plan
                                 sizes, with no more splits) */
#define PIS_TUNE_NKEYS 59
#define PIS_DEBUG_NOLOAD (1 << 16)
int pis_tune(int key, int value);
/* Tooling (tools/bench_gemm.py): time one batched NT GEMM kernel variant in isolation,
 * C[b] = A[b] . B[b]^T row-major fp32 — 0 bf16x6 128x128 (the Winograd GEMM), 1/2 its
 * no-global-load / no-split timing twins (wrong results), 3 fp32 MFMA, 4 bf16x6 128x64, 5/6 the
 * K-step-32 single-LDS-buffer bf16x6 128x128 (2 / 3 waves per SIMD), 7 its 128x64, 10 / 11 the
 * fp16x3 128x128 GEMM unscaled / with per-K-step scales (11 is the Winograd default), 12 its 128x64,
 * 13 / 14 11's no-global-load / no-staging timing twins (wrong results).
 * 5-12 need K % 32 == 0. */
int pis_debug_gemm_nt(const float* A, const float* B, float* C, int M, int N, int K, int batch, int variant,
                      pis_stream_t stream);
/* Tooling (bench.py roofline_loss): one float4 grid-stride launch over n floats of a and b — dst = a + b
 * when dst is given (12 B per element), else a read reduced to one partial per block (8 B per element):
 * the floor any kernel moving the loss's bytes meets at the same size and cache state. */
int pis_debug_stream_probe(const float* a, const float* b, float* dst, int64_t n, float* partial, int grid,
                           pis_stream_t stream);

/* Tooling (tools/bench_head_loss.py --probe): read n floats (n % 4096 == 0) in 16-KB chunks with 1024-thread
 * blocks, eight chunks in flight per lane: mode 0 grid-stride sweep (concurrent reads in one window),
 * mode 1 one contiguous run per block (the row-band kernels' order); partial[grid * 16] wave sums. */
int pis_debug_band_probe(const float* a, int64_t n, int mode, float* partial, int grid, pis_stream_t stream);

/* Scheduling aid: arm an event (hipEvent_t) that the next F(4x4,3x3) convolution launched on this
 * thread (pis_conv3x3_fwd_ex / _dgrad_ex / _fwd_keep / _fwd_pool) records on its stream right after
 * its 36 contractions, before the output transform; the slot then disarms. Lets a caller start
 * MFMA-bound work on another stream while the HBM-bound output transform runs. Returns 1 when
 * the previously armed event was never recorded (NULL disarms), else 0. */
int pis_arm_gemm_event(void* event);

/* Owned HIP streams (hipStreamNonBlocking, the given priority: 0 normal, -1 high). torch's
 * torch.cuda.Stream() hands out a fixed round-robin pool, so a stream that took part in a HIP graph
 * capture is later handed to unrelated code; the engine's weight-gradient stream and the capture
 * stream of a graphed step are owned instead (wrapped with torch.cuda.ExternalStream) and recycled
 * among owners (the Python side never destroys one: PyTorch keeps raw stream handles in autograd
 * nodes and allocator blocks). pis_stream_capture_status: hipStreamCaptureStatus (0 none, 1 active,
 * 2 invalidated) or a negative error. */
int pis_stream_create(int priority, pis_stream_t* out);
/* pis_stream_destroy: for hosts that own their streams' lifetime; the Python host never calls it (its
 * owned streams are recycled, never destroyed: PyTorch keeps raw stream handles beyond their users). */
int pis_stream_destroy(pis_stream_t stream);
int pis_stream_capture_status(pis_stream_t stream);

/* Profiling hook: called on the launching thread right before (phase 0) and after (phase 1)
 * the enqueue of each heavy kernel ("conv3x3_halo", "wino_gemm", "wino_gemm_out", "wgrad3x3_halo",
 * "wino_wgrad_gemm", "direct_h3_fwd", "direct_h3_pool", "direct_h3_dgrad", "direct_wgrad_h3"), with
 * its stream and the MFMA FLOPs it executes ("head_loss_fwd": its algorithmic HBM bytes instead), so
 * a profiler can record HIP events on that stream around exactly that kernel. NULL removes it. */
typedef void (*pis_launch_hook_t)(const char* kernel, int phase, pis_stream_t stream, double flop,
                                  void* user);
void pis_set_launch_hook(pis_launch_hook_t fn, void* user);

/* ---- 3x3 convolution, padding 1, stride 1 (src/unet.py:29,38 nn.Conv2d) ----
 * fwd:  y[p][n] = epi(bias[n] + sum_{r,s,c} x[p+(r-1,s-1)][c] * w[n][r][s][c])
 *       flags: PIS_RELU, PIS_SCALE (scale is [B][Cout]).   Cin==1 or Cin%4==0. */
int pis_conv3x3_fwd(const float* x, int ldx, const float* w_krsc, const float* bias,
                    const float* scale, float* y, int ldy, int B, int H, int W, int Cin,
                    int Cout, int flags, pis_stream_t stream);
/* Same contraction as pis_conv3x3_fwd / pis_conv3x3_dgrad, with a workspace that admits the fast
 * paths: the direct fp16x3 kernel (csrc/direct.hip) on the shallow layers (<= 128 channels both
 * sides, H >= 256; pis_tune key 29), else Winograd F(4x4,3x3) (4x fewer MFMA FLOPs: filter, input
 * and output transforms around 36 batched fp16x3 GEMMs, or the fused contraction + output transform
 * for 64 / 128-channel contractions; F(2x2,3x3) only behind pis_tune(11, 0) or for grids not
 * divisible by 4). ws may be NULL (the fp32-MFMA halo / implicit-GEMM kernels). */
size_t pis_conv3x3_ex_ws(int B, int H, int W, int Cin, int Cout);
int pis_conv3x3_fwd_ex(const float* x, int ldx, const float* w_krsc, const float* bias,
                       const float* scale, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                       int flags, void* ws, size_t ws_bytes, pis_stream_t stream);
/* w_flip[c][r][s][n] = w[n][2-r][2-s][c]  (dgrad operand, rebuilt each step) */
int pis_conv3x3_flip(const float* w_krsc, float* w_flip, int Cin, int Cout, pis_stream_t stream);
/* dgrad: dx[p][c] = epi(sum_{r,s,n} dz[p+(r-1,s-1)][n] * w_flip[c][r][s][n])
 *        flags: PIS_MASK (mask = this conv's input x), PIS_SCALE ([B][Cin]). */
int pis_conv3x3_dgrad(const float* dz, int ldz, const float* w_flip, const float* mask, int ldm,
                      const float* scale, float* dx, int lddx, int B, int H, int W, int Cin,
                      int Cout, int flags, pis_stream_t stream);
int pis_conv3x3_dgrad_ex(const float* dz, int ldz, const float* w_flip, const float* mask, int ldm,
                         const float* scale, float* dx, int lddx, int B, int H, int W, int Cin,
                         int Cout, int flags, void* ws, size_t ws_bytes, pis_stream_t stream);
/* wgrad: dw[n][r][s][c] (+)= sum_p dz[p][n] x[p+(r-1,s-1)][c];  db[n] (+)= sum_p dz[p][n]
 *        (db may be NULL). flags: PIS_ACCUMULATE. */
/* Kept input transform (training forward -> weight gradient of the same layer): where the
 * forward runs Winograd F(4x4,3x3) and the weight gradient F(3x3,4x4), both transform the
 * same input x with the same B^T; pis_conv3x3_fwd_keep leaves that transform in `keep`
 * (pis_conv3x3_keep_bytes(), 0 = nothing to keep) and pis_conv3x3_wgrad_keep reads it instead
 * of recomputing it. x must be unchanged in between. keep == NULL: plain _ex / wgrad. */
size_t pis_conv3x3_keep_bytes(int B, int H, int W, int Cin, int Cout);
int pis_conv3x3_fwd_keep(const float* x, int ldx, const float* w_krsc, const float* bias,
                         const float* scale, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                         int flags, void* ws, size_t ws_bytes, float* keep, pis_stream_t stream);
/* The encoder's conv1 + MaxPool2d(2,2) (src/unet.py:126, :177-188): as pis_conv3x3_fwd_keep, and
 * pool[b][h/2][w/2][c] (ld = Cout) = the 2x2 max of the y it wrote — in the F(4x4,3x3) output
 * epilogue when that path runs (no second read of y), else by pis_maxpool2x2_fwd. H, W even; no
 * PIS_ACCUMULATE. */
int pis_conv3x3_fwd_pool(const float* x, int ldx, const float* w_krsc, const float* bias, const float* scale,
                         float* y, int ldy, int B, int H, int W, int Cin, int Cout, int flags, void* ws,
                         size_t ws_bytes, float* keep, float* pool, pis_stream_t stream);
int pis_conv3x3_wgrad_keep(const float* x, int ldx, const float* dz, int ldz, float* dw_krsc, float* db,
                           int B, int H, int W, int Cin, int Cout, int flags, void* ws, size_t ws_bytes,
                           const float* keep, pis_stream_t stream);
/* One pass over a layer's dz for both backward products (no reference counterpart: the two
 * reads of dz that conv2d's input- and weight-gradient make): writes the F(4x4,3x3) input
 * transform into ws_dgrad (for pis_conv3x3_dgrad_ex) and the F(3x3,4x4) dz transform + bias
 * partials into ws_wgrad (for pis_conv3x3_wgrad_keep); both calls then pass PIS_WINO_PREPARED.
 * Returns 1 when done, 0 when this layer / workspace does not take that path (call without the
 * flag), < 0 on error. ws_wgrad must stay untouched until its pis_conv3x3_wgrad_keep ran.
 * With pis_tune key 51 and an input gradient on the batched GEMM, only the F(3x3,4x4) transform E is
 * written (into ws_wgrad) and the prepared pis_conv3x3_dgrad_ex reads that same E in place: the
 * library remembers, per ws_dgrad pointer and shape, where the last pis_conv3x3_bwd_prep put it.
 * pis_conv3x3_wgrad_keep with PIS_WINO_PREPARED never writes the E region of ws_wgrad (it writes
 * the split-K slabs, the reduced planes and the bias partials, all behind E), so the two consumers
 * may run in either order or concurrently; ws_wgrad must then stay untouched until BOTH ran. */
/* The F(4x4,3x3) filter transform of a conv3x3 layer, ahead of its convolution call (so it can run
 * on another stream, off the critical path). dgrad = 0: for the forward, w = KRSC [Cout][9][Cin];
 * dgrad = 1: for the input gradient, w = the ORIGINAL KRSC weights (rotated in place, as
 * PIS_W_UNFLIPPED). The output format is the one the call with these shapes will consume (fp32
 * U[36][N][C] for the batched GEMMs (followed, with pis_tune(23, 1) and C, N % 64 == 0, by its
 * per-(output, 32-channel chunk) maxima umax[N][C / 32]); for the fused 64->64 contraction the fp16x3 hi / lo planes +
 * one inverse scale per output channel, or with pis_tune(22, 0) the bf16x6 planes: the tune key
 * must not change between this call and the conv call that consumes it); where the call takes the
 * direct fp16x3 kernel (pis_tune key 29) its weight split: fp16 hi / lo planes in the kernel's LDS
 * image + one inverse scale per output channel.
 * pis_conv3x3_filter_bytes returns its size, 0 when that call would take neither the F(4x4,3x3)
 * GEMM path nor the direct kernel (then PIS_FILTER_READY must not be used). Pass the result as the
 * weight argument with PIS_FILTER_READY (dgrad: with PIS_WINO_PREPARED | PIS_W_UNFLIPPED semantics
 * kept). pis_conv3x3_filters: the Winograd transforms in one launch, the direct splits in a second. */
size_t pis_conv3x3_filter_bytes(int B, int H, int W, int Cin, int Cout, int dgrad);
int pis_conv3x3_filter(const float* w, int B, int H, int W, int Cin, int Cout, int dgrad, void* out,
                       size_t out_bytes, pis_stream_t stream);
/* Several layers' filter transforms (as pis_conv3x3_filter) in ONE launch: a layer's own grid is
 * small and latency-bound, here all jobs' blocks run side by side. At most PIS_FILTER_MAX_JOBS. */
typedef struct pis_filter_job {
  const float* w;
  void* out;
  size_t out_bytes;
  int B, H, W, Cin, Cout, dgrad;
} pis_filter_job;
#define PIS_FILTER_MAX_JOBS 40
/* The filter operand format pis_conv3x3_filter(s) would write for these shapes (0 none, 1 F(4x4) U[36][N][C]
 * fp32, 2 the fused kernel's planes, 3 the direct kernel's weight split, 4 F(6x6) U[64][N][C] fp32). */
int pis_conv3x3_filter_format(int B, int H, int W, int Cin, int Cout, int dgrad);
int pis_conv3x3_filters(const pis_filter_job* jobs, int n, pis_stream_t stream);
/* 1 when pis_conv3x3_dgrad_ex of these shapes (and workspace) runs the direct fp16x3 kernel
 * (pis_tune key 29), which accepts PIS_W_UNFLIPPED (the original weights) without
 * PIS_WINO_PREPARED; 0 otherwise. */
int pis_conv3x3_dgrad_direct(int B, int H, int W, int Cin, int Cout, int ldz, size_t ws_bytes);
int pis_conv3x3_bwd_prep(const float* dz, int ldz, int B, int H, int W, int Cin, int Cout, void* ws_dgrad,
                         size_t ws_dgrad_bytes, void* ws_wgrad, size_t ws_wgrad_bytes, pis_stream_t stream);
/* 0 for a shape outside pis_conv3x3_wgrad's channel contract (Cout a multiple of 64, Cin 1 or a
 * multiple of 64): not supported, as the other size queries answer. */
size_t pis_conv3x3_wgrad_ws(int B, int H, int W, int Cin, int Cout);
int pis_conv3x3_wgrad(const float* x, int ldx, const float* dz, int ldz, float* dw_krsc, float* db,
                      int B, int H, int W, int Cin, int Cout, int flags, void* ws, size_t ws_bytes,
                      pis_stream_t stream);

/* ---- 2x2 stride-2 transposed convolution (src/unet.py:132-153) ----
 * H, W are the INPUT resolution; the output is 2H x 2W.
 * fwd: y[(2h+i,2w+j)][o] = bias[o] + sum_c x[(h,w)][c] * w[i][j][o][c]          */
int pis_convt2x2_fwd(const float* x, int ldx, const float* w_ijoc, const float* bias, float* y,
                     int ldy, int B, int H, int W, int Cin, int Cout, pis_stream_t stream);
/* w_cijo[c][i][j][o] = w_ijoc[i][j][o][c]  (dgrad operand) */
int pis_convt2x2_prep(const float* w_ijoc, float* w_cijo, int Cin, int Cout, pis_stream_t stream);
/* dgrad: dx[(h,w)][c] = epi(sum_{i,j,o} dy[(2h+i,2w+j)][o] * w[i][j][o][c]); flags: PIS_MASK */
int pis_convt2x2_dgrad(const float* dy, int lddy, const float* w_cijo, const float* mask, int ldm,
                       float* dx, int lddx, int B, int H, int W, int Cin, int Cout, int flags,
                       pis_stream_t stream);
/* wgrad: dw[i][j][o][c] (+)= sum_(h,w) dy[(2h+i,2w+j)][o] x[(h,w)][c]; db[o] (+)= sum dy[.][o]
 * (Cin, Cout multiples of 64; the size query answers 0 outside that contract) */
size_t pis_convt2x2_wgrad_ws(int B, int H, int W, int Cin, int Cout);
int pis_convt2x2_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw_ijoc,
                       float* db, int B, int H, int W, int Cin, int Cout, int flags, void* ws,
                       size_t ws_bytes, pis_stream_t stream);
/* Tooling and tests: the number of split-K slabs of the 256 x 128 tile plan (PIS_TUNE_CONVT_WGRAD_TILE) at this
 * shape, 0 where the shape is outside that kernel's contract. */
int pis_debug_convt2x2_wgrad_tile_splits(int B, int H, int W, int Cin, int Cout);
/* Tooling and tests (host only, no GPU): the split-K kernel the Winograd weight gradient of pis_conv3x3_wgrad
 * launches for this layer under the current keys, `aligned`: x and dz (and a kept transform) 16-byte aligned.
 * -1: the layer's weight gradient is not a Winograd one (direct, halo, ...). Else bits 0..3: 0 fp32 MFMA,
 * 1 bf16x6, 2 fp16x3 column-staged, 3 / 4 fp16x3 row-staged 128 x 128 (4: whole K-steps, buffer loads),
 * 5 its timing twin, 6 the 256 x 128 tile kernel (PIS_TUNE_WINO_WGRAD_TILE), then bits 4..5: 1 the wide operand
 * is E (output channels), 2 V (input channels). _plan also stores the launch's split count and its blocks
 * (tiles x splits x transform planes) where the pointers are not NULL. */
int pis_debug_wino_wgrad_kernel(int B, int H, int W, int Cin, int Cout, int aligned);
int pis_debug_wino_wgrad_plan(int B, int H, int W, int Cin, int Cout, int aligned, int* splits, int* blocks);
/* Tooling and tests (host only, no GPU): the launch variants the planner (csrc/conv3x3_plan.h) names for the
 * Winograd forward / input gradient under the current keys. _gemm: the batched NT GEMM of a contraction of C
 * channels into N outputs (PIS_TUNE_WINO_TILE) — 0 generic implicit GEMM, 1 / 2 / 3 fp32 MFMA 128x256 / 128x128 /
 * 128x64, 4 / 5 bf16x6 K-step 16 128x128 / 128x64, 6 / 7 bf16x6 K-step 32, 8 / 9 fp16x3 K-step 32 (WinoGemm).
 * _fused_form: the fused contraction of C = 64 or 128 channels over T tiles (T % 32 == 0) — tile groups per block
 * G | 16 (fp16x3) | 32 (staggered wave pairs). -1: outside those arguments. */
int pis_debug_wino_gemm(int N, int C);
int pis_debug_wino_fused_form(int C, int T);
/* Tooling and tests: the algorithm the planner (csrc/convt_plan.h) resolves for a call of this shape under the
 * current keys. op 0: pis_convt2x2_fwd with ld_src = ldx, ld_dst = ldy and a bias; op 1: pis_convt2x2_dgrad with
 * ld_src = lddy, ld_dst = lddx = ldm and PIS_MASK; op 2: pis_convt2x2_wgrad with ld_src = ldx, ld_dst = lddy.
 * aligned16 != 0: every pointer of the call is 16-byte aligned; 0: none is. Launches nothing.
 * op 0 / 1: 1 fp16x3 K-step 32, 2 / 3 / 4 the K-step-16 GEMM in fp16x3 / bf16x6 / fp32 MFMA, 5 implicit GEMM
 * (ConvtAlgo). op 2: arm | (kernel + 1) << 4 | (bm / 64) << 8 | (bn / 64) << 12 with arm 1 the 256 x 128 tile
 * kernel (kernel field 0), 2 the row-staged 128 x 128 kernel, 3 generic split-K (ConvtWgradAlgo), kernel 0 fp32
 * MFMA, 1 bf16x6, 2 fp16x3 by columns, 3 fp16x3 by rows, 4 its whole-K-step form, 5 its timing twin
 * (WgradKernel), bm x bn the block tile; 0 outside pis_convt2x2_wgrad's contract or for another op. */
int pis_debug_convt2x2_algo(int op, int B, int H, int W, int Cin, int Cout, int ld_src, int ld_dst, int aligned16);

/* ---- 2x2 max pooling (src/unet.py:126,181-186) ----
 * H, W are the INPUT resolution. y is contiguous (ld = C).
 * bwd (fused with the skip-gradient sum and the ReLU backward of the pooled
 * block's output):  dx[p][c] = (dskip[p][c] + [p = argmax] dy[q][c]) * (x[p][c] > 0)
 * dskip may be NULL; dx has ld = lddx.
 * C and every ld are multiples of 4, every ld >= C, and x, y, dy, dskip, dx are 16-byte aligned
 * (float4 accesses); anything else is PIS_ERR_ARG.                                  */
int pis_maxpool2x2_fwd(const float* x, int ldx, float* y, int B, int H, int W, int C,
                       pis_stream_t stream);
int pis_maxpool2x2_bwd(const float* x, int ldx, const float* dy, const float* dskip, int ldskip,
                       float* dx, int lddx, int B, int H, int W, int C, pis_stream_t stream);

/* ---- output head: 1x1 conv C->1 + sigmoid (src/unet.py:157,206-210) ----
 * fwd: z[p] = b + sum_c x[p][c] w[c];  u[p] = 1 / (1 + exp(-z[p]))
 * bwd: d[p] = g[p] * u[p] (1 - u[p]) when u != NULL (sigmoid backward), else g[p];
 *      dx[p][c] = d[p] w[c] (x[p][c] > 0)  (ReLU backward of dec1 fused);
 *      dw[c] (+)= sum_p d[p] x[p][c];  db (+)= sum_p d[p]
 * fwd's z and bwd's u and db may be NULL. C % 4 == 0 (bwd: C <= 1024), ldx and lddx multiples of 4
 * and >= C, x, w, dx and ws 16-byte aligned (g, u, z, b, dw, db need none); ws holds at least
 * pis_head_bwd_ws(npix, C) bytes. Anything else is PIS_ERR_ARG; pis_head_bwd_ws answers 0 (and
 * sets pis_last_error) for sizes pis_head_bwd refuses.                              */
int pis_head_fwd(const float* x, int ldx, const float* w, const float* b, float* z, float* u,
                 int64_t npix, int C, pis_stream_t stream);
size_t pis_head_bwd_ws(int64_t npix, int C);
int pis_head_bwd(const float* x, int ldx, const float* w, const float* g, const float* u, float* dx,
                 int lddx, float* dw, float* db, int64_t npix, int C, int flags, void* ws,
                 size_t ws_bytes, pis_stream_t stream);

/* ---- fused Dice + BCE + reaction-diffusion + phase-field loss ----
 * src/loss.py:114-162, src/pde.py:49-212, src/metrics.py:38-73, src/evaluate.py:62-97.
 * p, t: (B, H, W) fp32 (C = 1). Terms are whole-batch means (src/loss.py:130-143). */
typedef struct pis_loss_params {
  float dice_w, bce_w;   /* src/loss.py:144-147                        */
  float rd_w, pf_w;      /* lambda_RD, lambda_PF; a term enters the total only if > 0 */
  float smooth;          /* Dice smoothing (1e-6)                      */
  float D, a;            /* diffusion coefficient, reaction threshold   */
  float eps;             /* phase-field interface width                */
  float thr;             /* metric threshold (0.5, strict '>')         */
  int flags;             /* PIS_LOSS_ALL_TERMS | PIS_LOSS_NO_REACTION                  */
} pis_loss_params;
#define PIS_LOSS_ALL_TERMS 1
#define PIS_LOSS_CHAIN_SIGMOID 2 /* bwd writes dL/dz = dL/dp * p (1 - p) */
#define PIS_LOSS_NO_REACTION 4   /* residual r = D Lap(u) only (src/ablation.py:53-86,107-154
                                    DiffusionOnlyLoss, use_reaction_term=False)           */
/* out_terms: [0] total [1] dice_loss [2] bce_loss [3] rd_loss [4] pf_loss [5] I=sum p t
 *            [6] P=sum p [7] T=sum t.
 * counts: [B][3] = exact (I_hat, P_hat, T) of the thresholded prediction per sample.
 * scores: [B][2] = (Dice, IoU) per sample (src/metrics.py:67-70, src/evaluate.py:91-94). */
#define PIS_LOSS_NTERMS 8
/* ws: pis_loss_ws(B, H, W) bytes of device scratch (no state between calls). */
size_t pis_loss_ws(int B, int H, int W);
int pis_loss_fwd(const float* p, const float* t, int B, int H, int W, const pis_loss_params* prm,
                 float* out_terms, int* counts, float* scores, void* ws, size_t ws_bytes,
                 pis_stream_t stream);
/* dst = grad_out * dL/dp (or dL/dz with PIS_LOSS_CHAIN_SIGMOID); grad_out is a device
 * scalar (NULL = 1).  terms = out_terms of the forward on the same p, t.          */
int pis_loss_bwd(const float* p, const float* t, int B, int H, int W, const pis_loss_params* prm,
                 const float* terms, const float* grad_out, float* dst, int flags,
                 pis_stream_t stream);

/* Loss backward fused into the head backward (src/loss.py:114-162 + src/unet.py:210 out_conv +
 * sigmoid): dz = dL/du u (1 - u) per pixel from u (B,H,W), t, terms of pis_loss_fwd, then
 * dx = dz w (x > 0), dw = sum dz x, db = sum dz as pis_head_bwd. du_out (may be NULL) receives
 * dL/du, i.e. what pis_loss_bwd writes.
 * W <= 1024. flags: PIS_ACCUMULATE (dw, db). */
/* The U-Net head (1x1 conv C -> 1 + sigmoid, src/unet.py:206-210) fused with pis_loss_fwd (replaces the
 * criterion call after model(x), src/train.py:108-110 / src/loss.py:130-160): from the head input x
 * ([B*H*W][ldx], C == 64) writes z (logits) and u = sigmoid(z) (B*H*W each, bitwise those of
 * pis_head_fwd) and every loss term / counter / score exactly as pis_loss_fwd(u, t) would; one pass
 * over x. Applicable when pis_head_loss_fwd_ok(B, H, W, C) (C == 64, W % 64 == 0, W <= 2048); else
 * use pis_head_fwd + pis_loss_fwd. Workspace pis_head_loss_fwd_ws(B, H, W) bytes. */
size_t pis_head_loss_fwd_ws(int B, int H, int W);
int pis_head_loss_fwd_ok(int B, int H, int W, int C);
int pis_head_loss_fwd(const float* x, int ldx, const float* w, const float* bias, const float* t, float* z,
                      float* u, int B, int H, int W, int C, const pis_loss_params* prm, float* out_terms,
                      int* counts, float* scores, void* ws, size_t ws_bytes, pis_stream_t stream);
size_t pis_head_loss_bwd_ws(int B, int H, int W, int C);
int pis_head_loss_bwd(const float* x, int ldx, const float* w, const float* u, const float* t,
                      float* du_out, int B, int H, int W, int C, const pis_loss_params* prm,
                      const float* terms, const float* grad_out, float* dx, int lddx, float* dw,
                      float* db, int flags, void* ws, size_t ws_bytes, pis_stream_t stream);
/* Per-pixel PDE fields of src/pde.py (any output may be NULL):
 * lap = Lap(u) (:49-79), residual = D Lap(u) + u(1-u)(u-a) (:101-122),
 * gradmag2 = gx^2 + gy^2 (:147-178), all on reflect-padded stencils.           */
int pis_pde_fields(const float* u, int B, int H, int W, float D, float a, float* lap,
                   float* residual, float* gradmag2, pis_stream_t stream);
/* Their adjoint: du = sum over the fields of (d field / du)^T g_field (any g may be NULL), so
 * PDERegularization.compute_laplacian / reaction_term / compute_residual /
 * compute_gradient_magnitude are differentiable as in the reference (src/pde.py:49-178). */
int pis_pde_fields_bwd(const float* u, const float* g_lap, const float* g_residual,
                       const float* g_gradmag2, int B, int H, int W, float D, float a, float* du,
                       pis_stream_t stream);

/* ---- decoupled AdamW over one flat parameter arena (src/train.py:658-662) ----
 * torch.optim.AdamW single-tensor semantics (torch/optim/adam.py):
 *   p *= 1 - lr*wd;  m += (1-b1)(g' - m);  v = b2 v + (1-b2) g'^2;
 *   p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)     with g' = g * grad_scale.   */
int pis_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, double step_size, double bc2_sqrt,
                   double grad_scale, pis_stream_t stream);

/* ---- global-norm gradient clipping and the non-finite step guard ----
 * pis_grad_sumsq reads the flat gradient g once and leaves, on the device, what
 * torch.nn.utils.clip_grad_norm_ and an isfinite check would have computed on the host:
 *   seg_sumsq[s] = sum_{i < seg_len[s]} (double)g[seg_off[s] + i]^2          (float64, exact squares)
 *   total = sum_s seg_sumsq[s]                                               (float64, in segment order)
 *   norm  = sqrt(total) * grad_scale          (the norm of the gradient AdamW applies, g' = g * grad_scale)
 *   c     = max_norm / (norm + 1e-6);  coef = (float)(c > 1 ? 1 : c)         (max_norm <= 0: coef = 1)
 *   apply = !(flags & PIS_GRADNORM_SKIP_NONFINITE) || isfinite(total)
 * and pis_adamw_step_clipped is pis_adamw_step with g' = (g * grad_scale) * coef, returning without a
 * write to p, m or v when apply == 0. g itself is never written. With coef == 1 the update is bitwise
 * pis_adamw_step's. Without the guard a non-finite norm gives coef = 0 (Inf) or NaN (NaN) as torch's
 * formula does, and the step proceeds (0 * Inf = NaN reaches p, as it would with torch).
 *
 * seg_off / seg_len are DEVICE tables of n_seg segments in floats: offsets >= 0 and multiples of 4,
 * lengths >= 1; nothing outside the segments is read (the padding between them may hold anything).
 * A segment with a bad offset or length counts as NaN (with the guard: the step is skipped).
 * Deterministic: a segment is cut into slices of 8192 floats, one partial per slice summed in a
 * fixed order by one block, partials and segments combined in a fixed order; no atomics; the result
 * does not depend on the grid and is bitwise equal run to run.
 *
 * record: 16 bytes {float coef; int apply; double norm}, written every call.
 * stats: PIS_GRADNORM_NSTATS doubles the caller zeroes once and may zero again between calls:
 *   [0] steps seen  [1] steps clipped (applied with coef < 1)  [2] steps skipped  [3] steps with a
 *   finite norm  [4] sum of the finite norms  [5] largest finite norm  [6] the last norm  [7] the last coef.
 * ws: pis_grad_sumsq_ws(n_seg, n_total) bytes, n_total >= the sum of the lengths; 16-byte aligned.
 * The lengths live on the device, so the host can only refuse a workspace below
 * pis_grad_sumsq_ws(n_seg, n_seg); one that is too small for the table makes the call a skipped
 * step with a NaN norm (apply = 0 whatever the flags) instead of a write past its end.
 * pis_grad_sumsq_ws answers 0 (and names itself in pis_last_error()) for n_seg <= 0 or n_total < n_seg. */
#define PIS_GRADNORM_SKIP_NONFINITE 1
#define PIS_GRADNORM_NSTATS 8
size_t pis_grad_sumsq_ws(int n_seg, int64_t n_total);
int pis_grad_sumsq(const float* g, const int64_t* seg_off, const int64_t* seg_len, int n_seg,
                   double grad_scale, double max_norm /* <= 0: no clipping */,
                   int flags /* PIS_GRADNORM_SKIP_NONFINITE */, double* seg_sumsq, void* record,
                   void* stats, void* ws, size_t ws_bytes, pis_stream_t stream);
int pis_adamw_step_clipped(float* p, const float* g, float* m, float* v, int64_t n, double lr,
                           double beta1, double beta2, double eps, double weight_decay,
                           double step_size, double bc2_sqrt, double grad_scale, const void* record,
                           pis_stream_t stream);

/* ---- exponential moving average of the weights in the AdamW launch ----
 * pis_adamw_step_ema updates p, m and v exactly as pis_adamw_step does (record == NULL) or as
 * pis_adamw_step_clipped does (record: the 16 bytes pis_grad_sumsq left on the device), with the
 * same host rounding of the scalars: the three arrays come out bitwise equal to those launches'.
 * The thread that holds the new p then moves the average towards it, w = (float)ema_weight:
 *   e = w < 0.5 ? e + w (p_new - e) : p_new - (p_new - e)(1 - w)            (torch.lerp's two forms)
 * i.e. e + w (p_new - e) in exact arithmetic; w = 0 leaves e and w = 1 gives e = p_new, bit for bit.
 * What is bitwise: p, m, v; e at w = 0 and w = 1. What is bounded: e otherwise, within the fp32
 * rounding of one lerp per step (the compiler may contract it into an FMA, torch rounds twice).
 * With a record whose apply == 0 the launch writes nothing: a skipped step does not move the average.
 * ema_weight outside [0, 1] or NaN, a null pointer, n < 0, a buffer that is not 16-byte aligned and a
 * record that is not 8-byte aligned are PIS_ERR_ARG; n == 0 is PIS_OK without a launch.
 *
 * pis_arena_exchange swaps the contents of a and b as raw 32-bit words (NaN payloads and -0.0
 * survive). Equal or overlapping ranges, a buffer that is not 16-byte aligned and n < 0 are
 * PIS_ERR_ARG; n == 0 is a no-op. Addresses do not change hands: views into either array, filter-job
 * tables and captured graphs stay valid. */
int pis_adamw_step_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr,
                       double beta1, double beta2, double eps, double weight_decay, double step_size,
                       double bc2_sqrt, double grad_scale, double ema_weight,
                       const void* record /* NULL, or pis_grad_sumsq's record */, pis_stream_t stream);
int pis_arena_exchange(float* a, float* b, int64_t n, pis_stream_t stream);

/* ---- channel sums (bias gradients): out[c] (+)= sum_p src[p*ld + c] ----
 * ld >= C; ws holds at least pis_colsum_ws(npix, C) bytes. When C % 4 == 0, ld % 4 == 0 and src
 * and ws are 16-byte aligned (float4 loads); any other C, and out always, needs no alignment.
 * Anything else is PIS_ERR_ARG. */
size_t pis_colsum_ws(int64_t npix, int C);
int pis_colsum(const float* src, int ld, int64_t npix, int C, float* out, int flags, void* ws,
               size_t ws_bytes, pis_stream_t stream);

/* ---- on-device synthetic batches (the disc generator of §8(c),
 * physics_informed_image_segmentation_amd/dataset.py:disc_sample) ----
 * discs: [B][max_discs][3] (cx, cy, r) drawn on the host from each sample's generator;
 * ndisc: [B] (device). Masks are bit-identical to the host generator's; the N(0, 0.1^2)
 * image noise is a counter-based hash of (seed, sample_ids[b] or b, pixel).
 * img, mask: (B, 1, H, W) fp32, img min-max normalised per sample. */
size_t pis_synth_ws(int B, int H, int W);
int pis_synth_discs(const float* discs, const int* ndisc, int max_discs, uint64_t seed,
                    const int64_t* sample_ids, float* img, float* mask, int B, int H, int W,
                    void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- boundary F1 / Hausdorff counters of a batch (src/evaluate.py:102-275), exact ----
 * p: probabilities, t: masks, both (B, H, W) fp32. Foreground is p > thr (strict; NaN is
 * background) and t > 0. The boundary set of an image is its foreground pixels with a
 * 4-neighbour in the outer background: the 4-connected background component that touches a
 * zero frame around the image (out-of-image neighbours count); holes and whatever is nested in
 * them contribute nothing. With Bp, Bt the boundary sets of sample b and d(q, X) the Euclidean
 * distance from pixel q to the nearest pixel of X,
 *   counts[b] = { n_p = |Bp|, n_t = |Bt|,
 *                 m_p = #{q in Bp : d(q, Bt)^2 <= tolerance^2}, m_t = #{q in Bt : d(q, Bp)^2 <= tolerance^2},
 *                 h2_pt = max_{q in Bp} d(q, Bt)^2, h2_tp = max_{q in Bt} d(q, Bp)^2 }
 * all exact integers (m_* = 0 and h2_* = -1 when either set is empty), independent of launch
 * order and bitwise reproducible. bnd_p / bnd_t (each may be NULL) receive the boundary maps as
 * uint8 (B, H, W). B >= 1, 1 <= H, W <= 4096, tolerance >= 0; anything else is PIS_ERR_ARG, a
 * workspace below pis_boundary_ws(B, H, W) bytes PIS_ERR_WORKSPACE (pis_boundary_ws is 0 for an
 * unsupported shape). A fixed sequence of launches on `stream`, no host synchronisation, no
 * state in ws between calls. */
size_t pis_boundary_ws(int B, int H, int W);
int pis_boundary_metrics(const float* p, const float* t, int B, int H, int W, float thr, int tolerance,
                         int* counts, uint8_t* bnd_p, uint8_t* bnd_t, void* ws, size_t ws_bytes,
                         pis_stream_t stream);

/* ---- object-level counters of a batch: connected components, detection matches and the
 * Aggregated Jaccard Index (no reference counterpart; evaluate.py:object_counts), exact ----
 * p: probabilities, t: masks, both (B, H, W) fp32. Foreground is p > thr (strict; NaN is
 * background) and t > 0. An object is a connected component of the foreground under
 * `connectivity` (4 or 8). The objects of an image are numbered 1..n in row-major order of their
 * first pixel. Predicted objects with fewer than min_area pixels are removed before the numbering
 * and before everything else; targets are never filtered. labels_p / labels_t (each may be NULL)
 * receive these numbers as int32 (B, H, W); background and removed objects are 0.
 * With A_p, A_t the areas of a kept predicted object p and a true object t of sample b,
 * I(p,t) = |p n t| and U(p,t) = A_p + A_t - I(p,t),
 *   counts[b] = { n_p       predicted objects kept,
 *                 n_t       true objects,
 *                 tp50      pairs with IoU > 0.5, tested in integers as 3 I > A_p + A_t,
 *                 tp75      pairs with IoU > 0.75, tested as 7 I > 3 (A_p + A_t),
 *                 aji_inter AJI numerator,
 *                 aji_union AJI denominator,
 *                 area_p    foreground pixels of the kept predicted objects,
 *                 removed   predicted objects dropped by min_area }
 * (above IoU 0.5 a pair is unique in both directions, so tp50 and tp75 need no assignment).
 * AJI (Kumar et al., in the HoVer-Net form): every true object t takes the predicted object
 * p*(t) that overlaps it (I > 0) with the largest I / U, fractions compared by int64
 * cross-multiplication, ties to the smaller object number (= the smaller first-pixel index);
 * aji_inter += I(p*, t), aji_union += U(p*, t), and p* is marked used. A true object that no
 * prediction overlaps adds A_t to aji_union; finally every kept predicted object that is not
 * used adds A_p to aji_union. The counters are int64 (a prediction may be the best match of many
 * true objects, so aji_union can pass 2^31). All exact integers, independent of launch order
 * and bitwise reproducible; should the pair table ever give up on an insert (it is sized so
 * that it cannot), all eight counters of that sample are -1.
 * B >= 1, 1 <= H, W <= 4096, connectivity 4 or 8, min_area >= 0; anything else is PIS_ERR_ARG, a
 * workspace below pis_objects_ws(B, H, W) bytes PIS_ERR_WORKSPACE (pis_objects_ws is 0 for an
 * unsupported shape). A fixed sequence of launches on `stream`, no host synchronisation, no
 * state in ws between calls. */
size_t pis_objects_ws(int B, int H, int W);
int pis_object_metrics(const float* p, const float* t, int B, int H, int W, float thr,
                       int connectivity, int min_area, int64_t* counts, int32_t* labels_p,
                       int32_t* labels_t, void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- probability-level table of a batch: the one integer table the threshold sweep, AUROC,
 * average precision, ECE and Brier score derive from (no reference counterpart;
 * evaluate.py:probability_table), exact ----
 * p: probabilities, t: masks, both (B, H, W) fp32, 4-byte aligned. Per pixel, every float step exact:
 *   x   = p * 65536.0f
 *   q   = clamp(ceil(x), 0, 65536) as an integer; NaN gives 0 (and counts in n_nan), -Inf and
 *         negatives give 0, values above 1 and +Inf give 65536
 *   bin = (q + 63) >> 6, in 0..PIS_PROB_BINS (= ceil(p * 1024) clamped; bin 0 holds q = 0 only), so
 *         that p > j / 1024 holds exactly when bin > j, for every float p and j = 0..1023
 *   cls = t > 0.5f (the target test of the loss kernel's counters; a NaN target is class 0)
 *   table[b][cls][bin] = { count, sum of q }                       int64 (B, 2, 1025, 2)
 *   extra[b] = { sum of q^2 over class 0, sum of q^2 over class 1, n_nan, 0 }
 * All exact integers (count <= 2^24, sum of q <= 2^40, sum of q^2 <= 2^56), independent of launch
 * order and bitwise reproducible. B >= 1, 1 <= H, W <= 4096; anything else and a NULL pointer are
 * PIS_ERR_ARG, a workspace below pis_probability_ws(B, H, W) bytes PIS_ERR_WORKSPACE
 * (pis_probability_ws is 0 for an unsupported shape). Two launches on `stream`, no host
 * synchronisation, no state in ws between calls. */
#define PIS_PROB_BINS 1024
#define PIS_PROB_QBITS 16
size_t pis_probability_ws(int B, int H, int W);
int pis_probability_table(const float* p, const float* t, int B, int H, int W, int64_t* table,
                          int64_t* extra, void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- batches from a device-resident dataset cache (no reference counterpart: replaces the
 * DataLoader workers + host-to-device copies around src/dataset.py:55-84 once the samples have been
 * preprocessed on the host; physics_informed_image_segmentation_amd/dataset.py:DeviceCachedLoader) ----
 * The cache holds N samples of H x W pixels, sample i at img + i * img_stride and mask + i * mask_stride
 * (strides in bytes, multiples of 16, at least one sample long; bases 16-byte aligned):
 *   PIS_CACHE_IMG_U8    H*W uint8 grey values; norm[i] = (lo, den) fp32, pixel = (float(v) - lo) / den in
 *                       correctly rounded fp32 (bit-identical to the host loader's min-max)
 *   PIS_CACHE_IMG_F32   H*W fp32, copied
 *   PIS_CACHE_MASK_BITS one bit per pixel, pixel p = bit (p & 31) of 32-bit word p >> 5 -> 0.0f / 1.0f
 *   PIS_CACHE_MASK_F32  H*W fp32, copied
 * One launch writes img_out and mask_out, both (B, 1, H, W) fp32 contiguous, for the samples idx[0..B)
 * (device memory; repeats allowed). sym == NULL: identity; else one code per batch entry (device memory),
 * applied to image and mask alike: bit 0 flips W, bit 1 flips H, then bit 2 transposes (H == W only), i.e.
 *   t = sample; if (s & 1) t = flip_W(t); if (s & 2) t = flip_H(t); if (s & 4) t = transpose(t).
 * What the host cannot see never faults: an idx outside [0, N), a code above 7 or bit 2 with H != W fills
 * that entry's two outputs with NaN and reads nothing of the cache. Unknown formats, a u8 image without
 * norm, bad strides or alignment, B > 65535 or H * W > 2^30 are PIS_ERR_ARG. No workspace, no state. */
#define PIS_CACHE_IMG_U8 0
#define PIS_CACHE_IMG_F32 1
#define PIS_CACHE_MASK_BITS 0
#define PIS_CACHE_MASK_F32 1
int pis_cache_batch(const void* img, int img_fmt, size_t img_stride, const void* mask, int mask_fmt,
                    size_t mask_stride, const float* norm, const int64_t* idx, const uint8_t* sym, int64_t N,
                    float* img_out, float* mask_out, int B, int H, int W, pis_stream_t stream);

/* The same batch, every entry resampled under its own affine map and tone curve (random rotation, scale,
 * shift, flip, brightness: dataset.py:AffineAugment). Arguments as pis_cache_batch with sym replaced by
 * params: B records of 32 bytes in device memory, 16-byte aligned, required:
 *   int32 a[6]; float gain; float bias;
 * The geometry is 16.16 fixed point, so that a host restatement (dataset.py:PackedSamples.warp) agrees
 * bit for bit. For output pixel (y, x), with 64-bit integer sums:
 *   SX = a[0]*x + a[1]*y + a[2]      SY = a[3]*x + a[4]*y + a[5]          source coordinates
 *   x0 = SX >> 16, y0 = SY >> 16 (floor)     fx = (SX >> 8) & 255, fy = (SY >> 8) & 255
 *   reflect(i, n) = 0 if n == 1, else m = i mod (2n - 2) >= 0, m < n ? m : 2n - 2 - m   (no repeated edge)
 * u8 image:  I = (256-fy)*((256-fx)*v00 + fx*v01) + fy*((256-fx)*v10 + fx*v11) over the uint8 pixels at the
 *            reflected (y0 | y0+1, x0 | x0+1), an exact integer below 2^24; t = float(I) * 2^-16;
 *            img = (t - lo) / den
 * f32 image: w00 = (256-fy)*(256-fx), w01 = (256-fy)*fx, w10 = fy*(256-fx), w11 = fy*fx as floats;
 *            img = ((w00*v00 + w01*v01) + (w10*v10 + w11*v11)) * 2^-16
 * mask:      the value (bit or float) at reflect((SY + 32768) >> 16, H), reflect((SX + 32768) >> 16, W)
 * tone:      img_out = gain * img + bias, no clamp
 * every float operation correctly rounded on its own (no fused multiply-add). The record
 * {65536, 0, 0, 0, 65536, 0}, 1.0f, 0.0f gives what pis_cache_batch gives with sym == NULL.
 * An idx outside [0, N) fills that entry's two outputs with NaN and reads nothing of the cache.
 * PIS_ERR_ARG as pis_cache_batch, and for params NULL or not 16-byte aligned, and for H or W above 4096:
 * with |a[k]| < 2^31 that bound keeps SX >> 16 and SY >> 16 inside 32 bits, where the reflection is done. */
int pis_cache_batch_affine(const void* img, int img_fmt, size_t img_stride, const void* mask, int mask_fmt,
                           size_t mask_stride, const float* norm, const int64_t* idx, const void* params,
                           int64_t N, float* img_out, float* mask_out, int B, int H, int W, pis_stream_t stream);

/* ---- whole-image inference: overlapping tiles under test-time symmetries, gathered before the forwards
 * and blended after them (no reference counterpart; predict.py:Predictor) ----
 * The tiling is a pure function of the by-value arguments; predict.py:tile_plan / gather_tiles_np /
 * blend_tiles_np restate it in float32 numpy and agree bit for bit.
 * Tile origins: along an axis of length n with tile t and overlap o the stride is t - o,
 *   K(n, t, o)  = 1 if n <= t, else ceil((n - o) / (t - o))
 *   origin(k)   = min(k (t - o), max(n - t, 0))     the last tile is pulled back to end at the image edge;
 *                                                   a single tile on an axis shorter than t starts at 0 and
 *                                                   its excess is reflection
 * Ky = K(H, th, ov), Kx = K(W, tw, ov). Symmetries: sym_mask is a non-empty 8-bit set of the codes of
 * pis_cache_batch (bit 0 flips W, bit 1 flips H, then bit 2 transposes); bit q set means code q is used, in
 * ascending order, Ns = popcount(sym_mask); a code >= 4 needs th == tw. Jobs are numbered
 *   j = ((s Ky + ky) Kx + kx) Ns + qi               for source s of S, J = S Ky Kx Ns jobs in all.
 * reflect(i, n) is the one of pis_cache_batch_affine: it wraps as often as needed, so a 5 x 7 image under a
 * 16 x 16 tile is defined.
 *
 * pis_tile_count: Ky and Kx of one image, on the host (no GPU call).
 *
 * pis_tile_gather: one launch writes out (n_jobs, 1, th, tw) fp32 contiguous for the jobs
 * [first_job, first_job + n_jobs). The S sources are H x W images in one of the cache's two image formats,
 * source s at src + s * src_stride (bytes, a multiple of 16, at least one image long; base 16-byte aligned):
 * PIS_CACHE_IMG_U8 with norm[s] = (lo, den), pixel = (float(v) - lo) / den correctly rounded, or
 * PIS_CACHE_IMG_F32, copied. With (y0, x0) = (origin(ky), origin(kx)) and q the job's code,
 *   T[ly][lx] = src[s][reflect(y0 + ly, H)][reflect(x0 + lx, W)]        0 <= ly < th, 0 <= lx < tw
 *   out[j - first_job] = t = T; if (q & 1) t = flip_W(t); if (q & 2) t = flip_H(t); if (q & 4) t = transpose(t).
 *
 * pis_tile_blend: one launch reads u (J, 1, th, tw) fp32 — one value per gathered element, for ALL J jobs —
 * and writes prob (S, H, W) fp32 and, if mask is not NULL, mask (S, H, W) uint8 in {0, 1}. In gather form,
 * one result per output pixel, no atomics. For pixel (s, y, x), every tile that covers it is visited in the
 * order ky ascending, kx ascending, qi ascending; with ly = y - origin(ky), lx = x - origin(kx):
 *   v    = the element of u[j] that the job's symmetry sent T[ly][lx] to (the inverse of the gather)
 *   w    = w1(ly, th, ov) * w1(lx, tw, ov), an integer: w1(l, t, o) = min(l + 1, t - l, o) for o >= 1, 1 for
 *          o == 0 (a ramp over the overlap, in the image frame: the Ns symmetries of one tile share it)
 *   acc  = acc + float(w) * v      the multiply and the add each correctly rounded on its own (no fused
 *                                  multiply-add), acc starting at 0.0f
 *   wsum = wsum + w                an integer
 *   prob = acc / float(wsum)       correctly rounded
 *   mask = prob > thr              strict, the comparison of the loss kernel's counters; NaN gives 0
 * ov <= 256 bounds w by 2^16, and at most 3 tiles per axis cover a pixel (two neighbours and the pulled-back
 * last tile), so wsum over at most 3 * 3 * 8 covers is an exact integer in fp32.
 *
 * PIS_ERR_ARG (all three): th or tw no multiple of 16 in [16, 2048]; ov outside [0, min(th, tw) / 2] or
 * above 256; H or W outside [1, 32768]; S < 1; an empty sym_mask or one above 0xFF; a code >= 4 with
 * th != tw; a NULL pointer (mask may be NULL); gather: an unknown format, a u8 source without norm, a bad
 * stride, src or out not 16-byte aligned, a chunk not within [0, J); blend: u or prob not 16-byte aligned,
 * mask not 4-byte aligned. All indexing is 64-bit. No workspace, no state, no host synchronisation. */
int pis_tile_count(int H, int W, int th, int tw, int ov, int* Ky, int* Kx);
int pis_tile_gather(const void* src, int src_fmt, size_t src_stride, const float* norm, int S, int H, int W,
                    int th, int tw, int ov, int sym_mask, int64_t first_job, int64_t n_jobs, float* out,
                    pis_stream_t stream);
int pis_tile_blend(const float* u, int S, int H, int W, int th, int tw, int ov, int sym_mask, float thr,
                   float* prob, uint8_t* mask, pis_stream_t stream);

/* ---- PDE evolution of a probability map, and the physics quantities of one (no reference counterpart;
 * pde.py:evolve_np / energies_np restate both in float32 numpy and agree bit for bit) ----
 * Maps are (B, H, W) fp32 contiguous, 2 <= H, W <= 4096, no divisibility requirement. With
 * p = the map padded by one pixel under reflect(i, n) of pis_cache_batch_affine (no repeated edge) and
 *   up, dn, lf, rt = p[y-1][x], p[y+1][x], p[y][x-1], p[y][x+1]
 * every operation below is float32 and correctly rounded on its own (no fused multiply-add):
 *   lap = ((up + dn) + (lf + rt)) - 4 c
 *   r   = (c (1 - c)) (c - a)
 *
 * pis_pde_evolve: `steps` explicit Euler steps of u_t = D lap(u) + k u (1 - u) (u - a) + mu (u0 - u), per step
 *   t  = D lap;  t = t + k r;  if mu != 0: t = t + mu (u0 - c)         u0 NULL: the input map u
 *   c' = c + dt t;  with PIS_EVOLVE_CLAMP: c' = c' < 0 ? 0 : c', then c' = c' > 1 ? 1 : c'
 * The pairing (up + dn) + (lf + rt) is part of the definition: each pair commutes, so a step commutes bit
 * for bit with an H flip, a W flip and a transpose, and the reflect extension of a map evolves to the reflect
 * extension of the evolved map. The kernel relies on it: a launch advances up to T steps (pis_tune key
 * PIS_TUNE_EVOLVE_T) on PIS_EVOLVE_TILE_H x PIS_EVOLVE_TILE_W tiles whose T-wide halo is loaded once through
 * reflect (any number of periods) and never exchanged. ceil(steps / T) launches on `stream`, chained through
 * at most two scratch maps in ws (16-byte aligned, pis_pde_evolve_ws(B, H, W, steps) bytes; fewer than three
 * launches need less, and none is read by the launch that writes it); the last launch writes out and, when
 * mask is not NULL, mask (B, H, W) uint8 = (c > thr), strict. steps == 0 copies u to out (and writes mask). u and
 * u0 are not written. No host synchronisation; capturable in a graph.
 * PIS_ERR_ARG before any GPU work: u or out NULL; B < 1; H or W outside [2, 4096]; steps outside
 * [0, PIS_EVOLVE_MAX_STEPS]; unknown flags; D < 0, k < 0, mu < 0, a outside (0, 1), dt <= 0 or
 * dt (4 D + k + mu) > 1 (in float64: under that bound the step is monotone in every argument, so [0, 1] is
 * invariant in exact arithmetic and the clamp only removes rounding excursions); NaN scalars; u, u0, out or ws
 * not 16-byte aligned, mask not 4-byte aligned; out overlapping u or u0; ws missing, too small, or overlapping
 * a map; a tune key that holds no legal T. pis_pde_evolve_ws answers 0 (and sets the message) for a shape or
 * step count outside these bounds.
 *
 * pis_pde_energies: per image s, out_f64[s][0] = rd, out_f64[s][1] = pf, out_i64[s] = interface:
 *   rd        = (sum over pixels of double(res)^2) / (H W),   res = D lap + r
 *   pf        = (sum over pixels of double(e)) / (H W),       gx = 0.5 (rt - lf), gy = 0.5 (dn - up),
 *               g = gx gx + gy gy, w = (c c) ((1 - c) (1 - c)), e = he g + ie w, he = eps / 2, ie = 1 / eps in fp32
 *   interface = the number of pixels with 0.1f < c < 0.9f
 * Two launches: row bands write float64 partial sums and int64 counts into ws (8-byte aligned,
 * pis_pde_energies_ws(B, H, W) bytes), a second launch adds them per image in a fixed order; no floating-point
 * atomics, so the result is bitwise equal from run to run. The float32 per-pixel values are the definition's;
 * only the order of the float64 sum differs from a host sum (relative (n - 1) 2^-53 at most: the terms are
 * non-negative).
 * PIS_ERR_ARG: a NULL pointer; a shape outside the bounds above; D < 0, a outside (0, 1), eps <= 0; out_f64,
 * out_i64 or ws not 8-byte aligned; ws missing or too small. */
#define PIS_EVOLVE_CLAMP 1
#define PIS_EVOLVE_TILE_H 32
#define PIS_EVOLVE_TILE_W 64
#define PIS_EVOLVE_MAX_STEPS 65536
size_t pis_pde_evolve_ws(int B, int H, int W, int steps);
int pis_pde_evolve(const float* u, const float* u0, float* out, uint8_t* mask, int B, int H, int W, float D, float k,
                   float a, float mu, float dt, int steps, int flags, float thr, void* ws, size_t ws_bytes,
                   pis_stream_t stream);
size_t pis_pde_energies_ws(int B, int H, int W);
int pis_pde_energies(const float* u, int B, int H, int W, float D, float a, float eps, double* out_f64,
                     int64_t* out_i64, void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- the evolution above as a differentiable layer: checkpointed forward and reverse sweep (no reference
 * counterpart; pde.py:unroll_vjp_np is the definition of record and agrees bit for bit) ----
 * tb is the temporal block Tb in {1, 2, 4}; 0 reads pis_tune key PIS_TUNE_UNROLL_TB. The same Tb must be
 * given to the forward and to its backward.
 *
 * pis_pde_unroll_fwd: pis_pde_evolve's steps (same kernel, same bits in out) in ceil(steps / Tb) launches;
 * launch i < the last writes the state after (i + 1) Tb steps into map i of ckpt (16-byte aligned,
 * pis_pde_unroll_ws(B, H, W, steps, tb) bytes = ceil(steps / Tb) - 1 maps, each rounded up to 16 bytes), the
 * last writes out. steps == 0 copies u.
 *
 * pis_pde_unroll_bwd: given g_out = dL/d out, writes g_u = dL/du and, when u0 was given, g_u0 = dL/du0 (g_u0
 * may be NULL if it is not wanted; with u0 NULL it must be). Per step, last first, with c the step's input, n
 * its update before the clamp and g' the gradient with respect to its output:
 *   q  = (n < 0 or n > 1) and PIS_EVOLVE_CLAMP ? 0 : g'
 *   nb = (wa_H[y] q[y-1][x] + wb_H[y] q[y+1][x]) + (wa_W[x] q[y][x-1] + wb_W[x] q[y][x+1])
 *        wa[i] = 0, 2, 1, 1, ...: i = 0, 1, 2, ...      wb[i] = 0, 2, 1, 1, ...: i = n-1, n-2, n-3, ...
 *        (the transpose of the reflect padding; a q outside the image is 0)
 *   rp = ((1 - 2 c) (c - a)) + (c (1 - c));  s = k rp;  s = s - (4 D);  if mu != 0: s = s - mu
 *   g  = (1 + dt s) q + (dt D) nb;           if mu != 0: gz = gz + (dt mu) q
 * every operation float32 and rounded on its own, 4 D, dt D and dt mu formed once. g_u0 = gz; with u0 NULL
 * g_u = g + gz (one add, also when mu == 0). steps == 0: g_u = g_out as bits, g_u0 = 0.
 * One launch per temporal block, last block first: a workgroup reloads the block's starting state (u or a
 * checkpoint) with a 2 Tb halo through reflect, recomputes the Tb states in LDS and sweeps the gradient back
 * as a gather: no atomics, no halo exchange, bitwise reproducible and independent of Tb. The gradient passes
 * through two maps in ws in turn; gz is carried in g_u0 (or a third map of ws), each tile touching its own
 * pixels only. ws: 16-byte aligned, pis_pde_unroll_bwd_ws(B, H, W) bytes. No host synchronisation.
 * PIS_ERR_ARG before any GPU work: as pis_pde_evolve, with steps in [0, PIS_UNROLL_MAX_STEPS] (the bound on
 * the checkpoint stack; a choice), an illegal tb or key, g_u0 without u0, a missing or short ckpt or ws, and
 * any written range (out, ckpt; g_u, g_u0, ws) overlapping another argument. The size queries answer 0. */
#define PIS_UNROLL_MAX_STEPS 1024
size_t pis_pde_unroll_ws(int B, int H, int W, int steps, int tb);
size_t pis_pde_unroll_bwd_ws(int B, int H, int W);
int pis_pde_unroll_fwd(const float* u, const float* u0, float* out, void* ckpt, size_t ckpt_bytes, int B, int H, int W,
                       float D, float k, float a, float mu, float dt, int steps, int flags, int tb,
                       pis_stream_t stream);
int pis_pde_unroll_bwd(const float* u, const float* u0, const void* ckpt, const float* g_out, float* g_u, float* g_u0,
                       int B, int H, int W, float D, float k, float a, float mu, float dt, int steps, int flags, int tb,
                       void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- the layer above with its coefficients in device memory, and their gradient (no reference counterpart;
 * pde.py:unroll_coef_vjp_np is the definition of record) ----
 * coef points to five float32 in device memory, D, k, a, mu, dt in that order (4-byte aligned), read by every
 * kernel at its start; 4 D, dt D and dt mu are formed on the device, each one rounded float32 product, as the
 * host forms them for the entry points above. flags: PIS_EVOLVE_CLAMP | PIS_EVOLVE_MU; the host cannot see mu,
 * so PIS_EVOLVE_MU says whether the mu (u0 - c) term is formed (with mu = 0 it adds a zero). With the same
 * float32 values pis_pde_unroll_fwd_dev writes the bits of pis_pde_unroll_fwd, and pis_pde_unroll_bwd_dev
 * the g_u and g_u0 of pis_pde_unroll_bwd.
 * NO RANGE CHECK is made on the five values: it would be a host synchronisation. They are arithmetic operands
 * only and enter no address, loop bound or guard of a memory access, so no value can make a kernel fault; a
 * value outside the ranges pis_pde_evolve checks gives a map that means nothing. The caller keeps them in
 * range (pde.py:LearnablePDELayer does so by construction).
 * g_coef (may be NULL: no sums, the kernels of pis_pde_unroll_bwd): [B][5] float64, 8-byte aligned. Per image
 * the sum over all pixels and steps of, with q, c, n as above and lap, r, t the forward step's from c,
 *   q (dt lap)    q (dt r)    q (dt (k (0 - (c (1 - c)))))    q (dt (u0 - c)) [PIS_EVOLVE_MU, else 0]    q t
 * each term float32, every operation rounded on its own, the sum float64: dL/dD, dL/dk, dL/da, dL/dmu, dL/ddt
 * of that image's part of the loss. Order of the sum: a thread over its pixels and steps, the wave's xor
 * butterfly, the 16 waves pairwise, a workgroup's launches in turn (the first stores into its slot of ws, the
 * later ones add to it), then per image one wave over the tiles. No atomics: bitwise reproducible at a fixed
 * Tb; across Tb the grouping differs, so the sums agree to H W steps 2^-53 times the sum of the terms'
 * magnitudes. steps == 0: g_coef = 0. ws: pis_pde_unroll_bwd_dev_ws(B, H, W) bytes, the three maps of
 * pis_pde_unroll_bwd_ws and one slot of 8 doubles per tile; it needs no clearing.
 * PIS_ERR_ARG before any GPU work: the checks of the entry points above except the scalar ones; coef NULL or
 * misaligned; g_coef misaligned; out, ckpt, g_u, g_u0, ws or g_coef overlapping coef or another argument. */
#define PIS_EVOLVE_MU 2
size_t pis_pde_unroll_bwd_dev_ws(int B, int H, int W);
int pis_pde_unroll_fwd_dev(const float* u, const float* u0, float* out, void* ckpt, size_t ckpt_bytes, int B, int H,
                           int W, const float* coef, int steps, int flags, int tb, pis_stream_t stream);
int pis_pde_unroll_bwd_dev(const float* u, const float* u0, const void* ckpt, const float* g_out, float* g_u,
                           float* g_u0, double* g_coef, int B, int H, int W, const float* coef, int steps, int flags,
                           int tb, void* ws, size_t ws_bytes, pis_stream_t stream);

/* ---- exact squared Euclidean distance transform of a batch of binary images, and the per-pixel
 * surface distances between two boundary maps (no reference counterpart;
 * evaluate.py:distance_transform_sq_np / surface_distances) ----
 * pis_edt_sq: set is (N, H, W) uint8, a pixel belongs to the set of its image when its byte is not 0.
 *   d2[n][y][x] = min over the set pixels (y', x') of image n of (y - y')^2 + (x - x')^2     int32 (N, H, W)
 * 0 inside the set, PIS_EDT_NONE at every pixel of an image whose set is empty. Exact (the largest
 * value is 2 * 4095^2 < 2^26). Three launches on `stream` whatever the data (column masks, column
 * distances, one wave per row), no host synchronisation, no atomics: bitwise reproducible.
 * pis_surface_distances: bnd_p, bnd_t are (B, H, W) uint8 boundary maps (pis_boundary_metrics writes
 * them). The transforms of all 2 B maps run in the same three launches, evaluated only where needed:
 *   d2_pt[b][q] = the transform of bnd_t[b] at q where bnd_p[b][q] != 0, else -1           int32 (B, H, W)
 *   d2_tp[b][q] = the transform of bnd_p[b] at q where bnd_t[b][q] != 0, else -1
 * so a boundary pixel whose opposite boundary is empty holds PIS_EDT_NONE.
 * N, B >= 1 (B <= 2^24), 1 <= H, W <= 4096; anything else and a NULL pointer are PIS_ERR_ARG, a
 * workspace below pis_edt_ws(N, H, W) / pis_surface_distances_ws(B, H, W) bytes PIS_ERR_WORKSPACE (both
 * answer 0 for an unsupported shape). No state in ws between calls; the outputs may not overlap ws. */
#define PIS_EDT_NONE 0x7FFFFFFF
size_t pis_edt_ws(int N, int H, int W);
int pis_edt_sq(const uint8_t* set, int N, int H, int W, int32_t* d2, void* ws, size_t ws_bytes,
               pis_stream_t stream);
size_t pis_surface_distances_ws(int B, int H, int W);
int pis_surface_distances(const uint8_t* bnd_p, const uint8_t* bnd_t, int B, int H, int W, int32_t* d2_pt,
                          int32_t* d2_tp, void* ws, size_t ws_bytes, pis_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PIS_CAPI_H */
