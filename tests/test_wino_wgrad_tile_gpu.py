"""The Winograd weight gradient's batched GEMM on 256 x 128 block tiles (pis_tune key 58, csrc/wgrad.hip
wgrad_h3t_tile_kernel) through pis_conv3x3_wgrad / pis_conv3x3_wgrad_keep, against float64 on the CPU.

Every case that is meant to run the new kernel sets key 58 = 2 (every shape in the contract, whatever the
measured default takes) and asserts the arm and its orientation through pis_debug_wino_wgrad_plan.

Shapes (B, H, W, Cin, Cout), the smallest that reach each thing that can go wrong (T >= 512 tiles of
F(3x3,4x4) needs 2 x 64 x 64):
  A    (2, 64, 64, 256, 256)  T = 512, one split, wide E, two Cin tiles
  ONE  (2, 64, 64, 128, 256)  one block owns a whole plane of dW
  WB   (2, 64, 64, 256, 128)  wide V (Cout = 128)
  S2   (4, 64, 64, 256, 256)  T = 1024: two splits, summed inside the output transform
  C4   (2, 64, 64, 512, 256)  four Cin tiles, the bias blocks among them
More than 16 splits is out of reach here: a split is at least 512 tiles and the plan wants at most 28 /
(tiles of 128 x 128) splits, so inside the contract (>= 2 such tiles) at most 14; with key 9 raised it
needs T > 8192, operands of hundreds of MB. The reduce_slabs_pitched branch it would take is reached
through F(3x3,2x2) instead (key 11 = 0 on shape A), which always takes it.

Bounds: those of tests/test_kernels_gpu.py::test_wgrad_rowstaged_fp16x3. dW's relative error in norm
against float64 is at most 1.25 x the fp32-MFMA path's (key 14 = 0) + 1e-9 and below 5e-6; db below 1e-5.
"""
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

pytestmark = pytest.mark.gpu

ACC, PREP = 8, 16
KEY = _hip.PIS_TUNE_WINO_WGRAD_TILE
H3_COLS, H3T, H3T_EXACT, TILE, WIDE_E, WIDE_V = 2, 3, 4, 6, 1 << 4, 2 << 4
A, ONE, WB, S2, C4 = (2, 64, 64, 256, 256), (2, 64, 64, 128, 256), (2, 64, 64, 256, 128), (4, 64, 64, 256, 256), \
    (2, 64, 64, 512, 256)
ARM = {A: TILE | WIDE_E, ONE: TILE | WIDE_E, WB: TILE | WIDE_V, S2: TILE | WIDE_E, C4: TILE | WIDE_E}
SPLITS = {A: 1, ONE: 1, WB: 1, S2: 2, C4: 1}
# per-sample dz magnitudes (alternating) and the magnitude of x: the scale jumps inside one chain, in both
# orders; both operands small; and dz ~ 1e-30 against x ~ 1e-2, where the two scales multiply beyond fp32
MAGS = [(1.0, 1.0, 1.0), (1.0, 1e-30, 1.0), (1e-30, 1.0, 1.0), (1e-9, 1e-9, 1.0), (1e-30, 1e-30, 1e-2)]
_cache = {}


def s():
    return torch.cuda.current_stream().cuda_stream


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-300)).item()


def reference(x, dz):
    """float64, NHWC operands: dW [Cout][3][3][Cin] of the zero-padded 3x3 conv and db [Cout]."""
    B, H, W, Cin = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x.double()
    d = dz.double().reshape(B * H * W, -1)
    dw = torch.empty(d.shape[1], 3, 3, Cin, dtype=torch.float64)
    for r in range(3):
        for c in range(3):
            dw[:, r, c] = d.t() @ xp[:, r:r + H, c:c + W].reshape(B * H * W, Cin)
    return dw, d.sum(dim=0)


def operands(shape, mags=MAGS[0], sparse=False):
    """NHWC fp32 operands and their float64 reference, made once per case and never written to.
    sparse: x keeps one input channel and dz one output channel per 32-column block (the first, the last
    or an interior one in turn), so every 32 x 32 accumulator block of every wave, half and tile owns
    exactly one nonzero (n, c) pair per tap."""
    key = (shape, mags, sparse)
    if key not in _cache:
        B, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(71 + Cin + 3 * Cout + B)
        x = torch.relu(torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)) * mags[2]
        dz = torch.randn(B, H, W, Cout, generator=g, dtype=torch.float64)
        for i in range(B):
            dz[i] *= mags[i % 2]
        x, dz = x.float(), dz.float()
        keep_c = keep_n = None
        if sparse:
            keep_c = [32 * k + (0, 31, 13)[k % 3] for k in range(Cin // 32)]
            keep_n = [32 * k + (31, 17, 0)[k % 3] for k in range(Cout // 32)]
            xs, dzs = torch.zeros_like(x), torch.zeros_like(dz)
            xs[..., keep_c] = x[..., keep_c]
            dzs[..., keep_n] = dz[..., keep_n]
            x, dz = xs, dzs
        _cache[key] = (x, dz) + reference(x, dz) + (keep_c, keep_n)
    return _cache[key]


def query(hip, shape, aligned=1):
    import ctypes
    sp, bl = ctypes.c_int(0), ctypes.c_int(0)
    arm = hip.pis_debug_wino_wgrad_plan(*shape, aligned, ctypes.byref(sp), ctypes.byref(bl))
    return arm, sp.value, bl.value


def wgrad(hip, shape, xd, dzd, key, flags=0, dw=None, db="new", tune=(), expect=None, keep=None, ws=None):
    """One pis_conv3x3_wgrad (or, with a kept transform, pis_conv3x3_wgrad_keep) call under key 58 = key;
    returns (dw, db) on the device. expect: the arm the debug query must name under the same keys."""
    B, H, W, Cin, Cout = shape
    if dw is None:
        dw = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")
    if isinstance(db, str):
        db = torch.full((Cout,), float("nan"), device="cuda")
    prev = [(k, hip.pis_tune(k, v)) for k, v in tune]
    try:
        nws = hip.pis_conv3x3_wgrad_ws(*shape)  # sized before key 58 changes
        prev.append((KEY, hip.pis_tune(KEY, key)))
        assert hip.pis_conv3x3_wgrad_ws(*shape) == nws
        if ws is None:
            ws = torch.full((nws // 4 + 1,), float("nan"), device="cuda")
        if expect is not None:
            aligned = int(keep is None or keep % 16 == 0)
            assert query(hip, shape, aligned)[0] == expect, (shape, key, query(hip, shape, aligned))
        dbp = db.data_ptr() if db is not None else 0
        if keep is None:
            rc = hip.pis_conv3x3_wgrad(xd.data_ptr(), Cin, dzd.data_ptr(), Cout, dw.data_ptr(), dbp, B, H, W, Cin, Cout,
                                       flags, ws.data_ptr(), nws, s())
        else:
            rc = hip.pis_conv3x3_wgrad_keep(xd.data_ptr(), Cin, dzd.data_ptr(), Cout, dw.data_ptr(), dbp, B, H, W, Cin,
                                            Cout, flags, ws.data_ptr(), nws, keep, s())
        assert rc == 0, hip.pis_last_error()
        torch.cuda.synchronize()
    finally:
        for k, v in reversed(prev):
            hip.pis_tune(k, v)
    return dw, db


def test_plans_of_the_test_shapes(hip):
    """Key 58 = 2 puts every shape above on the tile arm with the orientation and split count its case is
    about; key 0 leaves the kernels of before (bf16x6 at 128 input channels)."""
    for shape in ARM:
        prev = hip.pis_tune(KEY, 2)
        try:
            arm, splits, blocks = query(hip, shape)
        finally:
            hip.pis_tune(KEY, prev)
        B, H, W, Cin, Cout = shape
        assert (arm, splits) == (ARM[shape], SPLITS[shape]), shape
        assert blocks == 36 * splits * (Cin // 128) * (Cout // 128) // 2
        prev = hip.pis_tune(KEY, 0)
        try:
            assert query(hip, shape)[0] == (1 if Cin == 128 else H3T_EXACT), shape
        finally:
            hip.pis_tune(KEY, prev)


@pytest.mark.parametrize("shape,mags", [(sh, m) for sh in (A, WB) for m in MAGS] + [(sh, MAGS[0]) for sh in (ONE, S2, C4)])
def test_accuracy_vs_float64(hip, shape, mags):
    x, dz, dw_ref, db_ref, _, _ = operands(shape, mags)
    xd, dzd = x.cuda(), dz.cuda()
    dw, db = wgrad(hip, shape, xd, dzd, 2, expect=ARM[shape])
    dw2, db2 = wgrad(hip, shape, xd, dzd, 2)
    dwf, dbf = wgrad(hip, shape, xd, dzd, 2, tune=((14, 0),), expect=0)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    e_w, f_w, e_b = rel_err(dw, dw_ref), rel_err(dwf, dw_ref), rel_err(db, db_ref)
    print(f"{shape} {mags}: dW err tile {e_w:.3e} fp32 {f_w:.3e}; db err {e_b:.3e}")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)  # bitwise repeatable
    assert e_w <= 1.25 * f_w + 1e-9 and e_w < 5e-6, (e_w, f_w)
    assert e_b < 1e-5, e_b


def test_f2_tiles_and_the_slab_reduction(hip):
    """F(3x3,2x2) (key 11 = 0) has plain operands too: T = 2048 tiles of 2 x 2, four splits, and its slabs
    go through reduce_slabs_pitched and its bias through the channel sum (no bias partials in the GEMM)."""
    shape = A
    x, dz, dw_ref, db_ref, _, _ = operands(shape)
    xd, dzd = x.cuda(), dz.cuda()
    prev = [(11, hip.pis_tune(11, 0)), (KEY, hip.pis_tune(KEY, 2))]
    try:
        assert query(hip, shape) == (TILE | WIDE_E, 4, 16 * 4 * 2)
    finally:
        for k, v in reversed(prev):
            hip.pis_tune(k, v)
    dw, db = wgrad(hip, shape, xd, dzd, 2, tune=((11, 0),), expect=TILE | WIDE_E)
    dw2, db2 = wgrad(hip, shape, xd, dzd, 2, tune=((11, 0),))
    dwf, dbf = wgrad(hip, shape, xd, dzd, 2, tune=((11, 0), (14, 0)), expect=0)
    e_w, f_w, e_b = rel_err(dw, dw_ref), rel_err(dwf, dw_ref), rel_err(db, db_ref)
    print(f"{shape} F(2x2): dW err tile {e_w:.3e} fp32 {f_w:.3e}; db err {e_b:.3e}")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert e_w <= 1.25 * f_w + 1e-9 and e_w < 5e-6, (e_w, f_w)
    assert e_b < 1e-5, e_b


@pytest.mark.parametrize("shape", [C4, WB])
def test_exact_placement(hip, shape):
    """x nonzero in one input channel and dz in one output channel per 32-column block: dW is exactly 0.0
    outside those (n, c) pairs and within the bound on them. Both orientations; C4 has two Cout halves
    of one wide tile and four Cin tiles, WB the two Cin halves of a wide-V tile."""
    x, dz, dw_ref, db_ref, keep_c, keep_n = operands(shape, sparse=True)
    dw, db = wgrad(hip, shape, x.cuda(), dz.cuda(), 2, expect=ARM[shape])
    dw = dw.cpu()
    on = torch.zeros(dw.shape, dtype=torch.bool)
    on[torch.tensor(keep_n)[:, None], :, :, torch.tensor(keep_c)[None, :]] = True
    assert on.sum().item() == 9 * len(keep_n) * len(keep_c)
    assert (dw_ref[on] != 0).all()
    assert (dw[~on] == 0.0).all()
    # on the kept pairs (everything else is zero on both sides): the accuracy bound, in norm
    dwf, _ = wgrad(hip, shape, x.cuda(), dz.cuda(), 2, tune=((14, 0),), expect=0)
    e_w, f_w = rel_err(dw, dw_ref), rel_err(dwf, dw_ref)
    assert e_w <= 1.25 * f_w + 1e-9 and e_w < 5e-6, (e_w, f_w)
    # and every kept pair's nine taps on their own, for placement only: two pairs that swapped places hold
    # independent sums and differ by their whole magnitude (relative error about 1.4), while nine values of
    # one pair can carry a few times the whole tensor's relative error; 1e-3 separates the two by 1000 x
    pair_err = ((dw.double() - dw_ref)[on].reshape(len(keep_n), 9, len(keep_c)).norm(dim=1) /
                dw_ref[on].reshape(len(keep_n), 9, len(keep_c)).norm(dim=1))  # [on] runs over (n, tap, c)
    print(f"{shape}: sparse dW err tile {e_w:.3e} fp32 {f_w:.3e}; worst pair {pair_err.max().item():.3e}")
    assert pair_err.max().item() < 1e-3, pair_err.max().item()
    assert rel_err(db, db_ref) < 1e-5
    assert (db.cpu()[[n for n in range(shape[4]) if n not in keep_n]] == 0.0).all()


@pytest.mark.parametrize("shape", [A, WB])
def test_accumulate_and_null_bias(hip, shape):
    """Two PIS_ACCUMULATE calls into zeros give exactly twice one call; db = NULL leaves dW's bits."""
    B, H, W, Cin, Cout = shape
    x, dz, dw_ref, db_ref, _, _ = operands(shape)
    xd, dzd = x.cuda(), dz.cuda()
    dw1, db1 = wgrad(hip, shape, xd, dzd, 2, expect=ARM[shape])
    dw = torch.zeros(Cout, 3, 3, Cin, device="cuda")
    db = torch.zeros(Cout, device="cuda")
    wgrad(hip, shape, xd, dzd, 2, flags=ACC, dw=dw, db=db)
    wgrad(hip, shape, xd, dzd, 2, flags=ACC, dw=dw, db=db)
    assert torch.equal(dw, 2 * dw1) and torch.equal(db, 2 * db1)
    assert rel_err(dw, 2 * dw_ref) < 5e-6 and rel_err(db, 2 * db_ref) < 1e-5
    dwn, _ = wgrad(hip, shape, xd, dzd, 2, db=None)
    assert torch.equal(dwn, dw1)


def kept_transform(hip, shape, xd):
    """The forward's kept F(4x4) input transform of x (pis_conv3x3_fwd_keep), as a float tensor."""
    B, H, W, Cin, Cout = shape
    nk = hip.pis_conv3x3_keep_bytes(*shape)
    assert nk > 0
    keep = torch.empty(nk // 4, device="cuda")
    nws = hip.pis_conv3x3_ex_ws(*shape)
    ws = torch.empty(nws // 4 + 1, device="cuda")
    w = torch.zeros(Cout, 3, 3, Cin, device="cuda")
    y = torch.empty(B, H, W, Cout, device="cuda")
    assert hip.pis_conv3x3_fwd_keep(xd.data_ptr(), Cin, w.data_ptr(), 0, 0, y.data_ptr(), Cout, B, H, W, Cin, Cout, 0,
                                    ws.data_ptr(), nws, keep.data_ptr(), s()) == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    return keep, ws, nws


def test_kept_and_prepared_path(hip):
    """pis_conv3x3_wgrad_keep on the forward's kept transform, and after pis_conv3x3_bwd_prep with
    PIS_WINO_PREPARED: the bits of the plain call, on the tile arm."""
    shape = A
    B, H, W, Cin, Cout = shape
    x, dz, dw_ref, db_ref, _, _ = operands(shape)
    xd, dzd = x.cuda(), dz.cuda()
    dw0, db0 = wgrad(hip, shape, xd, dzd, 2, expect=ARM[shape])
    keep, wsd, nwsd = kept_transform(hip, shape, xd)
    dw1, db1 = wgrad(hip, shape, xd, dzd, 2, keep=keep.data_ptr(), expect=ARM[shape])
    assert torch.equal(dw1, dw0) and torch.equal(db1, db0)
    nwg = hip.pis_conv3x3_wgrad_ws(*shape)
    wsg = torch.full((nwg // 4 + 1,), float("nan"), device="cuda")
    prev = hip.pis_tune(KEY, 2)
    try:
        rc = hip.pis_conv3x3_bwd_prep(dzd.data_ptr(), Cout, B, H, W, Cin, Cout, wsd.data_ptr(), nwsd, wsg.data_ptr(), nwg, s())
    finally:
        hip.pis_tune(KEY, prev)
    assert rc == 1, hip.pis_last_error()
    dw2, db2 = wgrad(hip, shape, xd, dzd, 2, flags=PREP, keep=keep.data_ptr(), ws=wsg, expect=ARM[shape])
    assert torch.equal(dw2, dw0) and torch.equal(db2, db0)


@pytest.mark.parametrize("shape", [(1, 32, 32, 256, 256), (2, 36, 36, 256, 256), (2, 64, 64, 64, 256)])
def test_outside_the_contract_same_bits(hip, shape):
    """T = 64, T = 162 and Cin = 64: keys 58 = 0, 1 and 2 run the same kernel and give the same bits."""
    x, dz, dw_ref, db_ref, _, _ = operands(shape)
    xd, dzd = x.cuda(), dz.cuda()
    prev = hip.pis_tune(KEY, 0)
    try:
        arm0 = query(hip, shape)[0]
    finally:
        hip.pis_tune(KEY, prev)
    assert arm0 not in (-1, TILE | WIDE_E, TILE | WIDE_V)
    dw0, db0 = wgrad(hip, shape, xd, dzd, 0, expect=arm0)
    for key in (1, 2):
        dw1, db1 = wgrad(hip, shape, xd, dzd, key, expect=arm0)
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0), key
    assert rel_err(dw0, dw_ref) < 5e-6 and rel_err(db0, db_ref) < 1e-5


def test_misaligned_kept_transform_same_bits(hip):
    """A kept transform 4 bytes off 16-byte alignment: the float4 buffer loads of the row-staged kernels
    are out, the column-staged fp16x3 kernel runs under every value of key 58, same bits."""
    shape = A
    x, dz, dw_ref, db_ref, _, _ = operands(shape)
    xd, dzd = x.cuda(), dz.cuda()
    keep, _, _ = kept_transform(hip, shape, xd)
    off = torch.empty(keep.numel() + 8, device="cuda")
    off[1:1 + keep.numel()].copy_(keep)
    ptr = off.data_ptr() + 4
    assert ptr % 16 == 4
    dw0, db0 = wgrad(hip, shape, xd, dzd, 0, keep=ptr, expect=H3_COLS)
    for key in (1, 2):
        dw1, db1 = wgrad(hip, shape, xd, dzd, key, keep=ptr, expect=H3_COLS)
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0), key
    assert rel_err(dw0, dw_ref) < 5e-6 and rel_err(db0, db_ref) < 1e-5
