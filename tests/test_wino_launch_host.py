"""The planner's choice of the Winograd forward / input gradient's launch variants on a GPU-less host
(csrc/conv3x3_plan.hip choose_wino_gemm, wino_fused_form), through pis_debug_wino_gemm and
pis_debug_wino_fused_form, against a transcription of the launch ladders that csrc/winograd.hip held
before the planner named the variants (launch_wino3x3's `if` ladder on key 10, launch_wino_gemm_out's
on keys 15, 22 and 25)."""
import pytest

from physics_informed_image_segmentation_amd import _hip

# WinoGemm (csrc/conv3x3_plan.h)
IGEMM, F32_256, F32_128, F32_64, X6_128, X6_64, X6_BK32_128, X6_BK32_64, H3_128, H3_64 = range(10)
H3, STG = 16, 32  # pis_debug_wino_fused_form's flag bits above G

NS = (36, 64, 128, 192, 256, 512)
CS = (4, 16, 48, 64, 96, 128)
GROUPS = (1, 2, 3, 4, 6, 8, 12, 16)


class tuned:
    def __init__(self, lib, kv):
        self.lib, self.kv = lib, tuple(kv)

    def __enter__(self):
        self.prev = [(k, self.lib.pis_tune(k, v)) for k, v in self.kv]
        assert all(p >= 0 for _, p in self.prev), self.lib.pis_last_error()

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            self.lib.pis_tune(k, v)


def old_gemm_ladder(v, N, C):
    """launch_wino3x3's arms, in their order."""
    if v == 1 and N % 256 == 0:
        return F32_256
    if v == 4 and N % 64 == 0 and C % 32 == 0:
        return H3_128 if N % 128 == 0 else H3_64
    if v >= 3 and N % 128 == 0:
        return X6_BK32_128 if C % 32 == 0 else X6_128
    if v >= 3 and N % 64 == 0:
        return X6_BK32_64 if C % 32 == 0 else X6_64
    if v == 2 and N % 128 == 0:
        return F32_128
    if v == 2 and N % 64 == 0:
        return F32_64
    return IGEMM


def old_fused_ladder(C, groups, k15, k22, k25):
    """launch_wino_gemm_out's arms: the <KC, G, H3, STG> it instantiated, as G | flags."""
    G = {2: 1, 3: 2, 4: 8}.get(k15, 4)
    if k22 and groups % 4 == 0 and (C == 128 or k25):  # 128 channels: staggered whatever key 25 says
        return 4 | H3 | STG
    for g in (8, 4, 2):
        if G == g and groups % g == 0:
            return g | (H3 if k22 else 0)
    return 1 | (H3 if k22 else 0)


@pytest.mark.parametrize("v", (0, 1, 2, 3, 4))
def test_gemm_choice(v):
    lib = _hip.lib()
    with tuned(lib, [(10, v)]):
        got = {(N, C): lib.pis_debug_wino_gemm(N, C) for N in NS for C in CS}
    assert got == {(N, C): old_gemm_ladder(v, N, C) for N in NS for C in CS}
    # the grid reaches both K-steps of the bf16x6 arm, and 36 outputs never leave the generic GEMM
    if v == 3:
        assert {X6_128, X6_64, X6_BK32_128, X6_BK32_64} <= set(got.values())
    assert all(got[36, C] == IGEMM for C in CS)


def test_gemm_choice_default_is_fp16x3():
    lib = _hip.lib()
    assert lib.pis_tune(10, -1) == 4
    assert lib.pis_debug_wino_gemm(256, 128) == H3_128 and lib.pis_debug_wino_gemm(64, 128) == H3_64
    assert lib.pis_debug_wino_gemm(128, 48) == X6_128  # C % 32 != 0: the K-step-16 bf16x6 kernel
    assert lib.pis_debug_wino_gemm(0, 64) == -1


@pytest.mark.parametrize("k15", (1, 2, 3, 4))
def test_fused_form(k15):
    lib = _hip.lib()
    seen = set()
    for k22 in (0, 1):
        for k25 in (0, 1):
            with tuned(lib, [(15, k15), (22, k22), (25, k25)]):
                for C in (64, 128):
                    for groups in GROUPS:
                        got = lib.pis_debug_wino_fused_form(C, 32 * groups)
                        assert got == old_fused_ladder(C, groups, k15, k22, k25), (C, groups, k15, k22, k25)
                        seen.add(got)
    # a wanted G that does not divide the groups falls to G = 1, never to the next smaller G
    want = {2: 1, 3: 2, 4: 8}.get(k15, 4)
    assert {f & 15 for f in seen} <= {1, 4, want}
    assert lib.pis_debug_wino_fused_form(64, 48) == -1 and lib.pis_debug_wino_fused_form(96, 64) == -1
