"""The planner's side of the Winograd weight gradient's 256 x 128 tile arm (pis_tune key 58,
csrc/conv3x3_plan.hip) on a GPU-less host: the workspace never depends on the key, the debug query
names the adopted arm of the eleven Winograd layers of the flagship step (batch 8, 512 x 512), and
every case of the two dispatch recordings keeps the kernel it was recorded with."""
import ctypes

import pytest
from test_conv3x3_dispatch_gpu import CASES as CONV_CASES
from test_conv3x3_plan_host import BATCHES, CINS, COUTS, GRIDS, in_wgrad_contract
from test_convt_dispatch_gpu import CASES as CONVT_CASES

from physics_informed_image_segmentation_amd import _hip

KEY = _hip.PIS_TUNE_WINO_WGRAD_TILE
X6, H3T_EXACT, TILE, WIDE_E, WIDE_V = 1, 4, 6, 1 << 4, 2 << 4


class key58:
    def __init__(self, lib, value, extra=()):
        self.lib, self.kv = lib, ((KEY, value),) + tuple(extra)

    def __enter__(self):
        self.prev = [(k, self.lib.pis_tune(k, v)) for k, v in self.kv]

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            self.lib.pis_tune(k, v)


def plan(lib, shape, aligned=1):
    sp, bl = ctypes.c_int(0), ctypes.c_int(0)
    arm = lib.pis_debug_wino_wgrad_plan(*shape, aligned, ctypes.byref(sp), ctypes.byref(bl))
    assert arm == lib.pis_debug_wino_wgrad_kernel(*shape, aligned)
    return arm, sp.value, bl.value


def test_key_is_known_and_on():
    lib = _hip.lib()
    assert lib.pis_tune(KEY, -1) == 1
    assert lib.pis_tune(KEY + 1, -1) < 0  # 58 is the last key


def test_workspace_does_not_depend_on_the_key():
    """pis_conv3x3_wgrad_ws over the grid of tests/test_conv3x3_plan_host.py under key 58 = 0, 1, 2, 3."""
    lib = _hip.lib()
    shapes = [(B, H, W, Cin, Cout) for B in BATCHES for H, W in GRIDS for Cin in CINS for Cout in COUTS
              if in_wgrad_contract(Cin, Cout)]
    sizes = {}
    for v in (0, 1, 2, 3):
        with key58(lib, v):
            sizes[v] = [lib.pis_conv3x3_wgrad_ws(*s) for s in shapes]
    assert sizes[0] == sizes[1] == sizes[2] == sizes[3]
    assert sum(1 for n in sizes[0] if n > 0) > 500


# the eleven Winograd weight gradients of the flagship step: (H = W, Cin, Cout) -> under key 58 = 0:
# (arm, splits, blocks); under the default: the same, or the tile arm as adopted
C2_OLD = {
    (256, 256, 128): (H3T_EXACT, 14, 1008),   # dec2.conv0
    (128, 128, 256): (X6, 13, 936),           # enc3.conv0
    (128, 256, 256): (H3T_EXACT, 7, 1008),    # enc3.conv1, dec3.conv1
    (128, 512, 256): (H3T_EXACT, 4, 1152),    # dec3.conv0
    (64, 256, 512): (H3T_EXACT, 4, 1152),     # enc4.conv0
    (64, 512, 512): (H3T_EXACT, 2, 1152),     # enc4.conv1, dec4.conv1
    (64, 1024, 512): (H3T_EXACT, 1, 1152),    # dec4.conv0
    (32, 512, 512): (H3T_EXACT, 1, 576),      # the bottleneck's two
}
C2_FORCED = {  # key 58 = 2 / 3: (arm, splits on the plan's count, splits trimmed to one generation)
    (256, 256, 128): (TILE | WIDE_V, 14, 14),
    (128, 128, 256): (TILE | WIDE_E, 13, 13),
    (128, 256, 256): (TILE | WIDE_E, 7, 7),
    (128, 512, 256): (TILE | WIDE_E, 4, 3),
    (64, 256, 512): (TILE | WIDE_E, 4, 3),
    (64, 512, 512): (TILE | WIDE_E, 2, 2),
    (64, 1024, 512): (TILE | WIDE_E, 1, 1),
    (32, 512, 512): (TILE | WIDE_E, 1, 1),
}


def c2(layer):
    H, Cin, Cout = layer
    return (8, H, H, Cin, Cout)


def test_flagship_layers_old_and_forced():
    lib = _hip.lib()
    for layer, want in C2_OLD.items():
        with key58(lib, 0):
            assert plan(lib, c2(layer)) == want, layer
        arm, s2, s3 = C2_FORCED[layer]
        H, Cin, Cout = layer
        tiles = (Cin // 128) * (Cout // 128) // 2
        with key58(lib, 2):
            assert plan(lib, c2(layer)) == (arm, s2, 36 * tiles * s2), layer
        with key58(lib, 3):
            assert plan(lib, c2(layer)) == (arm, s3, 36 * tiles * s3), layer
            assert 36 * tiles * s3 <= 512 or s3 == s2
        # a misaligned operand or a key that rules fp16x3 row staging out: never the tile arm
        for extra, aligned in (((), 0), (((14, 0),), 1), (((14, 1),), 1), (((31, 0),), 1), (((2, 1),), 1)):
            with key58(lib, 2, extra):
                assert plan(lib, c2(layer), aligned)[0] & 15 != TILE, (layer, extra, aligned)


# the default (key 58 = 1) as adopted from the per-layer measurements
C2_ADOPTED = {
    (256, 256, 128): (TILE | WIDE_V, 14, 504),
    (128, 128, 256): (TILE | WIDE_E, 13, 468),
    (128, 256, 256): C2_OLD[(128, 256, 256)],  # inside the old form's spread
    (128, 512, 256): (TILE | WIDE_E, 3, 432),  # on the trimmed splits
    (64, 256, 512): (TILE | WIDE_E, 3, 432),
    (64, 512, 512): (TILE | WIDE_E, 2, 576),
    (64, 1024, 512): C2_OLD[(64, 1024, 512)],  # no gain: 576 blocks, one split
    (32, 512, 512): (TILE | WIDE_E, 1, 288),
}


def test_flagship_layers_as_adopted():
    lib = _hip.lib()
    assert lib.pis_tune(KEY, -1) == 1
    assert set(C2_ADOPTED) == set(C2_OLD)
    for layer, want in C2_ADOPTED.items():
        assert plan(lib, c2(layer)) == want, layer
    # the other layers of the step take the direct weight gradient: no Winograd GEMM to name
    for layer in ((512, 64, 64), (256, 64, 128), (256, 128, 128)):
        assert plan(lib, c2(layer))[0] == -1, layer


def test_dispatch_recordings_keep_their_kernels():
    """Every case of tests/golden/conv3x3_dispatch.json and convt_dispatch.json that launches the Winograd
    weight-gradient GEMM: the query names, under the case's keys, the kernel it names with key 58 = 0 and
    never the tile arm; the convt recording's wino cases name the kernel the case is written for."""
    lib = _hip.lib()
    n = 0
    for name, (H, W, Cin, Cout, keys, *_rest, hooks) in CONV_CASES.items():
        if "wino_wgrad_gemm" not in hooks:
            continue
        for aligned in (1, 0):
            with key58(lib, 0, keys.items()):
                old = plan(lib, (1, H, W, Cin, Cout), aligned)
            with key58(lib, 1, keys.items()):
                assert plan(lib, (1, H, W, Cin, Cout), aligned) == old, name
            assert old[0] >= 0 and old[0] & 15 != TILE, name
        n += 1
    for name, (kind, shape, keys, _off, _f, _d, kernel) in CONVT_CASES.items():
        if kind != "wino":
            continue
        with key58(lib, 1, keys.items()):
            assert plan(lib, shape)[0] == kernel, name
        n += 1
    assert n == 13
