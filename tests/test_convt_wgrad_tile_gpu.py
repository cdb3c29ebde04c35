"""The transposed-conv weight gradient on 256 x 128 block tiles (pis_tune key 56, csrc/wgrad.hip
wgrad_h3t_tile_kernel<false, UP2>) against float64 on the CPU:

    dW[i][j][o][c] = sum_p dy[b, 2y+i, 2x+j, o] * x[b, y, x, c],   db[o] = sum dy

Shapes (B, H, W of the low-resolution input, Cin, Cout) are the smallest that reach each way the
kernel can go wrong: one tile / one split / 2 K-steps (fewer than the load-ahead depth); two N tiles
with a batch boundary inside the chain; two M tiles of two whole taps each and two K-steps per image
row; several splits with a shorter last one.

Tolerance on Gaussian operands: the rule of tests/test_kernels_gpu.py's float64 accuracy test for the
fp16x3 transposed-conv kernels (its h3k32 arm): the error against float64 is at most 1.25x the error
of the native fp32-MFMA path (pis_tune(13, 2) with key 14 = 0) at the same shape, and below 5e-6.
"""
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

pytestmark = pytest.mark.gpu

ACC = 8
KEY = _hip.PIS_TUNE_CONVT_WGRAD_TILE
SHAPES = [(1, 2, 32, 128, 64), (2, 3, 32, 256, 64), (1, 4, 64, 128, 128), (1, 20, 32, 128, 64)]
OUTSIDE = [(1, 4, 16, 128, 64), (1, 2, 32, 64, 64)]  # W % 32 != 0; Cin % 128 != 0
_cache = {}


def s():
    return torch.cuda.current_stream().cuda_stream


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def reference(x, dy):
    """float64: x [B][H][W][Cin], dy [B][2H][2W][Cout] -> dW [2][2][Cout][Cin], db [Cout]"""
    B, H, W, _ = x.shape
    d = dy.double().view(B, H, 2, W, 2, -1)
    return torch.einsum("byixjo,byxc->ijoc", d, x.double()), dy.double().sum(dim=(0, 1, 2))


def operands(shape, kind):
    """Operands and their float64 reference, made once per (shape, kind) and never written to."""
    if (shape, kind) not in _cache:
        B, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(B + 10 * H + 1000 * W + Cin + 3 * Cout + (kind == "int"))
        if kind == "gauss":
            x = torch.relu(torch.randn(B, H, W, Cin, generator=g))
            dy = torch.randn(B, 2 * H, 2 * W, Cout, generator=g)
        else:  # small integers: every product and sum exact in fp16x3 and fp32
            x = torch.randint(-4, 5, (B, H, W, Cin), generator=g).float()
            dy = torch.randint(-4, 5, (B, 2 * H, 2 * W, Cout), generator=g).float()
        _cache[shape, kind] = (x, dy) + reference(x, dy)
    return _cache[shape, kind]


def wgrad(hip, shape, xd, ldx, dyd, lddy, flags=0, dw=None, db="new", key=None, tune=()):
    """One pis_convt2x2_wgrad call on device operands; returns (dw, db) on the CPU."""
    B, H, W, Cin, Cout = shape
    nws = hip.pis_convt2x2_wgrad_ws(B, H, W, Cin, Cout)  # sized before any key changes
    ws = torch.empty(nws // 4 + 1, device="cuda")
    if dw is None:
        dw = torch.full((2, 2, Cout, Cin), float("nan"), device="cuda")
    if isinstance(db, str):
        db = torch.full((Cout,), float("nan"), device="cuda")
    prev = [(k, hip.pis_tune(k, v)) for k, v in tune]
    pk = hip.pis_tune(KEY, -1 if key is None else key)
    try:
        rc = hip.pis_convt2x2_wgrad(xd.data_ptr(), ldx, dyd.data_ptr(), lddy, dw.data_ptr(),
                                    db.data_ptr() if db is not None else 0, B, H, W, Cin, Cout, flags,
                                    ws.data_ptr(), nws, s())
        assert rc == 0, hip.pis_last_error()
        torch.cuda.synchronize()
    finally:
        hip.pis_tune(KEY, pk)
        for k, v in reversed(prev):
            hip.pis_tune(k, v)
    return dw, db


def test_key_default_and_plan(hip):
    """The key is on by default; the plan covers the in-contract shapes only; shape 4 has several splits."""
    assert hip.pis_tune(KEY, -1) == 1
    assert hip.pis_tune(13, -1) == 4
    for shape in SHAPES:
        assert hip.pis_debug_convt2x2_wgrad_tile_splits(*shape) >= 1, shape
    assert hip.pis_debug_convt2x2_wgrad_tile_splits(*SHAPES[3]) > 1  # P = 640: 512 + 128 pixels
    for shape in OUTSIDE:
        assert hip.pis_debug_convt2x2_wgrad_tile_splits(*shape) == 0, shape
    # C2: 512 blocks per layer
    for H, Cin, Cout in [(256, 128, 64), (128, 256, 128), (64, 512, 256), (32, 512, 512)]:
        tiles = (4 * Cout // 256) * (Cin // 128)
        assert tiles * hip.pis_debug_convt2x2_wgrad_tile_splits(8, H, H, Cin, Cout) == 512


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_vs_float64(hip, shape):
    """Error against float64 at most 1.25x the fp32-MFMA path's at the same shape; identical bits on a rerun."""
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "gauss")
    xd, dyd = x.cuda(), dy.cuda()
    dw, db = wgrad(hip, shape, xd, Cin, dyd, Cout)
    dw2, db2 = wgrad(hip, shape, xd, Cin, dyd, Cout)
    dwf, dbf = wgrad(hip, shape, xd, Cin, dyd, Cout, tune=((13, 2), (14, 0)))
    e_w, e_b = rel_err(dw, dw_ref), rel_err(db, db_ref)
    f_w, f_b = rel_err(dwf, dw_ref), rel_err(dbf, db_ref)
    print(f"{shape}: dW err tile {e_w:.3e} fp32 {f_w:.3e}; db err tile {e_b:.3e} fp32 {f_b:.3e}")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert e_w <= 1.25 * f_w + 1e-9 and e_w < 5e-6, (e_w, f_w)
    assert e_b <= 1.25 * f_b + 1e-9 and e_b < 5e-6, (e_b, f_b)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_placement(hip, shape):
    """Small-integer operands: dW and db equal the integer result exactly, and every (tap, 64 output
    channels, 128 input channels) block of that result differs from every other, so a block written to
    another's place cannot pass."""
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "int")
    blocks = [dw_ref[i, j, o:o + 64, c:c + 128] for i in range(2) for j in range(2) for o in range(0, Cout, 64)
              for c in range(0, Cin, 128)]
    for a in range(len(blocks)):
        for b in range(a + 1, len(blocks)):
            assert not torch.equal(blocks[a], blocks[b])
    xd, dyd = x.cuda(), dy.cuda()
    dw, db = wgrad(hip, shape, xd, Cin, dyd, Cout)
    assert torch.equal(dw.cpu().double(), dw_ref)
    assert torch.equal(db.cpu().double(), db_ref)
    dw2, db2 = wgrad(hip, shape, xd, Cin, dyd, Cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_strided_slices_nan_padding(hip):
    """dy as the first Cout channels of a 2 Cout-wide buffer and x with ldx > Cin, the rest NaN: the
    same bits as from contiguous operands, so nothing outside the slices reaches a sum."""
    shape = SHAPES[0]
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "gauss")
    dw0, db0 = wgrad(hip, shape, x.cuda(), Cin, dy.cuda(), Cout)
    xb = torch.full((B, H, W, Cin + 64), float("nan"))
    xb[..., :Cin] = x
    dyb = torch.full((B, 2 * H, 2 * W, 2 * Cout), float("nan"))
    dyb[..., :Cout] = dy
    dw, db = wgrad(hip, shape, xb.cuda(), Cin + 64, dyb.cuda(), 2 * Cout)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    assert rel_err(dw, dw_ref) < 5e-6 and rel_err(db, db_ref) < 5e-6


def test_accumulate_and_null_bias(hip):
    """Two PIS_ACCUMULATE calls give twice the reference (exactly twice one call: r + r); db = NULL
    leaves dW bitwise equal to the call with db."""
    shape = SHAPES[1]
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "gauss")
    xd, dyd = x.cuda(), dy.cuda()
    dw1, db1 = wgrad(hip, shape, xd, Cin, dyd, Cout)
    dw = torch.zeros(2, 2, Cout, Cin, device="cuda")
    db = torch.zeros(Cout, device="cuda")
    wgrad(hip, shape, xd, Cin, dyd, Cout, flags=ACC, dw=dw, db=db)
    wgrad(hip, shape, xd, Cin, dyd, Cout, flags=ACC, dw=dw, db=db)
    assert torch.equal(dw, 2 * dw1) and torch.equal(db, 2 * db1)
    assert rel_err(dw, 2 * dw_ref) < 5e-6 and rel_err(db, 2 * db_ref) < 5e-6
    dwn, _ = wgrad(hip, shape, xd, Cin, dyd, Cout, db=None)
    assert torch.equal(dwn, dw1)


@pytest.mark.parametrize("shape", OUTSIDE)
def test_outside_contract_runs_old_path(hip, shape):
    """W = 16 or Cin = 64: the key changes nothing (the older kernels run) and the result still matches."""
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "gauss")
    xd, dyd = x.cuda(), dy.cuda()
    dw1, db1 = wgrad(hip, shape, xd, Cin, dyd, Cout, key=1)
    dw0, db0 = wgrad(hip, shape, xd, Cin, dyd, Cout, key=0)
    assert torch.equal(dw1, dw0) and torch.equal(db1, db0)
    assert rel_err(dw1, dw_ref) < 5e-6 and rel_err(db1, db_ref) < 5e-6


def test_key_off_matches_on_shape_inside(hip):
    """Key 0 (the older kernels) and key 1 agree to the fp32 class on an in-contract shape."""
    shape = SHAPES[2]
    B, H, W, Cin, Cout = shape
    x, dy, dw_ref, db_ref = operands(shape, "gauss")
    xd, dyd = x.cuda(), dy.cuda()
    dw1, db1 = wgrad(hip, shape, xd, Cin, dyd, Cout, key=1)
    dw0, db0 = wgrad(hip, shape, xd, Cin, dyd, Cout, key=0)
    assert rel_err(dw1, dw0) < 5e-6 and rel_err(db1, db0) < 5e-6
    assert rel_err(dw0, dw_ref) < 5e-6
