"""The direct fp16x3 kernels under both MFMA shapes (csrc/direct.hip, pis_tune key 53: bit 0 forward /
pooled forward / input gradient, bit 1 weight gradient; 0 = every role on 32x32x16, 3 = every role
that has a 16x16x32 form on it).

Exact placement: integer operands make fp16x3 exact, so a wrong lane / tap / half / block map shows
as an unequal integer. Accuracy: the bounds of tests/test_direct_gpu.py against float64 (<= 1.25 x
the native fp32 kernel's error + 1e-9, < 2e-6 for the convolutions) on the smallest shapes that reach
each code path. One training step against the oracle, and the ready-split bitwise check."""
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

td = importlib.import_module("test_direct_gpu")
Knobs, DIRECT, NATIVE = td.Knobs, td.DIRECT, td.NATIVE
nhwc, nchw, krsc, rel, s = td.nhwc, td.nchw, td.krsc, td.rel, td.s
RELU, SCALE, MASK, ACC, UNFLIPPED = td.RELU, td.SCALE, td.MASK, td.ACC, td.UNFLIPPED

KEY = [0, 3]
TAPS = [(r, c) for r in range(3) for c in range(3)]


def _ints(shape, seed):
    return torch.randint(0, 8, shape, generator=torch.Generator().manual_seed(seed)).double()


def _dgrad(hip, dz, w, x, scale, flags, unflipped, base=0.0):
    """dx (NCHW, cpu) of pis_conv3x3_dgrad_ex on the direct kernel; w is (Cout, Cin, 3, 3)."""
    B, Cout, H, W = dz.shape
    Cin = w.shape[1]
    wd = krsc(w.float()).cuda()
    wf = torch.empty(Cin * 9 * Cout, device="cuda")
    assert hip.pis_conv3x3_flip(wd.data_ptr(), wf.data_ptr(), Cin, Cout, s()) == 0
    nws = max(hip.pis_conv3x3_ex_ws(B, H, W, Cin, Cout), 4)
    ws = torch.empty(nws // 4 + 1, device="cuda")
    assert hip.pis_conv3x3_dgrad_direct(B, H, W, Cin, Cout, Cout, nws)
    xd = nhwc(x.float()).cuda() if x is not None else torch.ones(B, H, W, Cin, device="cuda")
    sd = scale.float().cuda() if scale is not None else torch.ones(B, Cin, device="cuda")
    dx = torch.full((B, H, W, Cin), base, device="cuda")
    dzd = nhwc(dz.float()).cuda()
    rc = hip.pis_conv3x3_dgrad_ex(dzd.data_ptr(), Cout, (wd if unflipped else wf).data_ptr(),
                                  xd.data_ptr(), Cin, sd.data_ptr(),
                                  dx.data_ptr(), Cin, B, H, W, Cin, Cout, flags | (UNFLIPPED if unflipped else 0),
                                  ws.data_ptr(), nws, s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    return nchw(dx.cpu())


@pytest.mark.parametrize("key", KEY)
def test_fwd_exact_placement(hip, key):
    """One-hot weights at every (tap, c in both 8-channel halves, n in both 32-channel groups), and one
    filter with a different integer per tap, on integer x: the forward equals F.conv2d exactly."""
    B, H, W, C, N = 1, 8, 32, 16, 64
    x = _ints((B, C, H, W), 81)
    filters = []
    for r, c in TAPS:
        for ch in (3, 11):
            for n in (5, 37):
                w = torch.zeros(N, C, 3, 3, dtype=torch.float64)
                w[n, ch, r, c] = 1.0
                filters.append(w)
    w = torch.zeros(N, C, 3, 3, dtype=torch.float64)
    for t, (r, c) in enumerate(TAPS):
        for ch in (3, 11):
            for n in (5, 37):
                w[n, ch, r, c] = t + 1.0
    filters.append(w)
    with Knobs(hip, k53=key, **DIRECT):
        assert hip.pis_conv3x3_filter_format(B, H, W, C, N, 0) == 3
        for w in filters:
            y = td._fwd(hip, x, w, None, None, 0)
            assert torch.equal(y.double(), F.conv2d(x, w, padding=1)), w.nonzero()[:4]


@pytest.mark.parametrize("unflipped", [False, True])
@pytest.mark.parametrize("key", KEY)
def test_dgrad_exact_placement(hip, key, unflipped):
    """The same for the input gradient (contraction over 16 output channels, 64 input channels): one-hot
    and per-tap-integer weights on integer dz, from flipped and from original weights."""
    B, H, W, Cin, Cout = 1, 8, 32, 64, 16
    dz = _ints((B, Cout, H, W), 82)
    filters = []
    for r, c in TAPS:
        for co in (3, 11):
            for ci in (5, 37):
                w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
                w[co, ci, r, c] = 1.0
                filters.append(w)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    for t, (r, c) in enumerate(TAPS):
        for co in (3, 11):
            for ci in (5, 37):
                w[co, ci, r, c] = t + 1.0
    filters.append(w)
    with Knobs(hip, k53=key, **DIRECT):
        for w in filters:
            dx = _dgrad(hip, dz, w, None, None, 0, unflipped)
            assert torch.equal(dx.double(), torch.nn.grad.conv2d_input((B, Cin, H, W), w, dz, padding=1)), w.nonzero()[:4]


@pytest.mark.parametrize("k43", [0, 1])
@pytest.mark.parametrize("key", KEY)
def test_wgrad_exact_placement(hip, key, k43):
    """dz one-hot in (pixel, n) — pixels at a tile corner, a tile edge, inside a tile and on the image
    border, n in every 16-channel block — on integer x: dW[n] is exactly x shifted by each tap (zero where
    the tap leaves the image), every other n exactly zero, db the one-hot counts."""
    B, H, W, Cin, Cout = 1, 8, 64, 64, 64
    x = _ints((B, Cin, H, W), 83)
    dz = torch.zeros(B, Cout, H, W, dtype=torch.float64)
    hot = [(2, 32, 5), (3, 40, 21), (5, 31, 37), (4, 47, 53), (0, 0, 12), (7, 63, 44), (0, 33, 63), (6, 0, 0)]
    for r, c, n in hot:
        dz[0, n, r, c] = 1.0
    ref = torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dz, padding=1)
    with Knobs(hip, k53=key, k43=k43, **DIRECT):
        nws = hip.pis_conv3x3_wgrad_ws(B, H, W, Cin, Cout)
        ws = torch.empty(nws // 4 + 1, device="cuda")
        dw = torch.empty(Cout, 3, 3, Cin, device="cuda")
        db = torch.empty(Cout, device="cuda")
        xd, dzd = nhwc(x.float()).cuda(), nhwc(dz.float()).cuda()
        rc = hip.pis_conv3x3_wgrad(xd.data_ptr(), Cin, dzd.data_ptr(), Cout, dw.data_ptr(), db.data_ptr(), B, H, W, Cin,
                                   Cout, 0, ws.data_ptr(), nws, s())
        assert rc == 0, hip.pis_last_error()
        torch.cuda.synchronize()
    got = dw.cpu().double().permute(0, 3, 1, 2)
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, bad[:8]
    assert torch.equal(db.cpu().double(), dz.sum(dim=(0, 2, 3)))


FWD_SHAPES = [(1, 8, 32, 16, 64), (1, 8, 32, 48, 64), (2, 16, 64, 64, 128), (1, 8, 32, 128, 64)]


@pytest.mark.parametrize("B,H,W,Cin,Cout", FWD_SHAPES)
@pytest.mark.parametrize("key", KEY)
def test_fwd_is_fp32_accurate(hip, key, B, H, W, Cin, Cout):
    """One chunk (peeled only), an odd chunk count, several tiles with interior halos and two output
    slices, eight chunks: data scaled by 1, 1e-12, 1e6 with the 2^-60 patch, against float64."""
    with Knobs(hip, k53=key):
        td.test_direct_fwd_is_fp32_accurate(hip, B, H, W, Cin, Cout, dict())


@pytest.mark.parametrize("key", KEY)
def test_fwd_pool_and_row_pitch(hip, key):
    """The pooled forward from a wider pitch (ldx = Cin + 64): the pool bitwise max_pool2d of the written y."""
    with Knobs(hip, k53=key):
        td.test_direct_fwd_pool_and_row_pitch(hip)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 64, 16), (1, 8, 32, 64, 48), (2, 16, 64, 128, 64),
                                           (1, 8, 32, 64, 128)])
@pytest.mark.parametrize("k32", [0, 1])
@pytest.mark.parametrize("unflipped", [False, True])
@pytest.mark.parametrize("key", KEY)
def test_dgrad_is_fp32_accurate(hip, key, unflipped, k32, B, H, W, Cin, Cout):
    """The input gradient plain and with MASK | SCALE | ACC, from flipped and original weights, with and
    without the mask prefetch (key 32), for unit and gradient-sized dz, against float64 and the native
    fp32 kernel (which reads flipped weights)."""
    g = torch.Generator().manual_seed(84)
    x = F.relu(torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)).float().double()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) / (3 * Cin ** 0.5)).float().double()
    scale = ((torch.rand(B, Cin, generator=g) > 0.2).double() / 0.8).float().double()
    dz0 = torch.randn(B, Cout, H, W, generator=g, dtype=torch.float64)
    for sc in (1.0, 1e-9):
        dz = (dz0 * sc).float().double()
        plain = torch.nn.grad.conv2d_input(x.shape, w, dz, padding=1)
        base = 0.5 * sc
        based = torch.tensor(base, dtype=torch.float32).double()
        for flags, ref in ((0, plain), (MASK | SCALE | ACC, plain * (x > 0) * scale[:, :, None, None])):
            b0 = base if flags else 0.0
            with Knobs(hip, k53=key, k32=k32, **DIRECT):
                dx = _dgrad(hip, dz, w, x if flags else None, scale if flags else None, flags, unflipped, b0)
            e_direct = rel(dx.double() - (based if flags else 0.0), ref)
            with Knobs(hip, **NATIVE):
                wd = krsc(w.float()).cuda()
                wf = torch.empty(Cin * 9 * Cout, device="cuda")
                assert hip.pis_conv3x3_flip(wd.data_ptr(), wf.data_ptr(), Cin, Cout, s()) == 0
                nws = max(hip.pis_conv3x3_ex_ws(B, H, W, Cin, Cout), 4)
                ws = torch.empty(nws // 4 + 1, device="cuda")
                dn = torch.full((B, H, W, Cin), b0, device="cuda")
                xd, sd, dzd = nhwc(x.float()).cuda(), scale.float().cuda(), nhwc(dz.float()).cuda()
                rc = hip.pis_conv3x3_dgrad_ex(dzd.data_ptr(), Cout, wf.data_ptr(),
                                              xd.data_ptr() if flags else 0, Cin, sd.data_ptr() if flags else 0,
                                              dn.data_ptr(), Cin, B, H, W, Cin, Cout, flags, ws.data_ptr(), nws, s())
                assert rc == 0, hip.pis_last_error()
                torch.cuda.synchronize()
            e_native = rel(nchw(dn.cpu()).double() - (based if flags else 0.0), ref)
            print(f"dgrad key {key} sc {sc} flags {flags}: direct {e_direct:.3e} native {e_native:.3e}")
            assert e_direct <= 1.25 * e_native + 1e-9, (sc, flags, e_direct, e_native)
            assert e_direct < 2e-6, (sc, flags, e_direct)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 64, 64), (2, 16, 64, 64, 128), (1, 8, 32, 128, 64),
                                           (3, 24, 64, 64, 64)])
@pytest.mark.parametrize("k43", [0, 1])
@pytest.mark.parametrize("key", KEY)
def test_wgrad_is_fp32_accurate(hip, key, k43, B, H, W, Cin, Cout):
    """The weight and bias gradients, accumulated into existing ones, in either tile order (key 43): a
    single split chain, two (Cout, Cin) blocks, two c blocks, a tile count the splits do not divide."""
    with Knobs(hip, k53=key):
        td.test_direct_wgrad_is_fp32_accurate(hip, B, H, W, Cin, Cout, dict(k43=k43))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 64, 64, 64)])
@pytest.mark.parametrize("key", KEY)
def test_wgrad_scales_any_magnitude(hip, key, B, H, W, Cin, Cout):
    with Knobs(hip, k53=key):
        td.test_direct_wgrad_scales_any_magnitude(hip, B, H, W, Cin, Cout, dict())
        td.test_direct_wgrad_x_magnitude_down_the_strip(hip, dict())


@pytest.mark.parametrize("key", KEY)
def test_train_step(hip, key):
    """One training step at 2 x 64 x 64 with every eligible conv on the direct kernels (key 29 = 2),
    against the oracle with tests/test_direct_gpu.py's bounds."""
    with Knobs(hip, k53=key):
        td.test_train_step_with_direct_convs(hip, dict(rd_w=1e-2, pf_w=1e-2, D=5.0, a=0.5, eps=0.05), dict(k29=2))


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64)])
def test_split_ready_bitwise(hip, cin, cout):
    """The ready weight split and the on-the-fly one agree bit for bit with every 16x16x32 form on."""
    with Knobs(hip, k53=3):
        td.test_direct_split_ready_bitwise(hip, cin, cout)
