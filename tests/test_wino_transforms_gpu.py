"""The single-load-phase F(4x4) input transform and merged dz pass (pis_tune key 50 = 1, the
default: csrc/winograd.hip wino4_input_cols_kernel / wino4_dz2_cols_kernel) against the row-by-row
kernels they replace (key 50 = 0), through the C-ABI: the same sums in the same order, so every
output is compared bit for bit; and against float64."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RELU, SCALE, MASK, ACC, PREP, UNFLIPPED = 1, 2, 4, 8, 16, 32
KEY, KEY_FUSED = 50, 15

# (B, H, W, Cin, Cout): every tile on the border with corner tiles clamped both ways; interior and
# border tiles on a non-square grid with 32 and 64 channel pairs per tile; 128 channel pairs (one
# pair per thread in the bias partials); 96 channel pairs, which do not divide 256, so the dz pass
# takes its float4 form.
SHAPES = [(1, 8, 8, 64, 64), (2, 16, 32, 128, 64), (2, 16, 32, 64, 128), (1, 16, 16, 256, 256), (1, 8, 16, 192, 192)]
# the dgrad_ex flag sets on top of PREP | UNFLIPPED: the engine's, with dropout scales, the
# ReLU + scale epilogue, and accumulation onto a filled dx
DGRAD_FLAGS = [MASK, MASK | SCALE, RELU | SCALE, MASK | ACC]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def krsc(w):  # (O, I, 3, 3) -> [O][3][3][I]
    return w.permute(0, 2, 3, 1).contiguous()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def s():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int32)


_inputs = {}


def layer_inputs(shape):
    """The layer's host tensors, made once per shape and left unchanged."""
    if shape not in _inputs:
        B, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(71)
        x = F.relu(torch.randn(B, Cin, H, W, generator=g))
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
        b = torch.randn(Cout, generator=g)
        dz = torch.randn(B, Cout, H, W, generator=g)
        sy = (torch.rand(B, Cout, generator=g) > 0.2).float() / 0.8
        sx = (torch.rand(B, Cin, generator=g) > 0.2).float() / 0.8
        _inputs[shape] = (x, w, b, dz, sy, sx)
    return _inputs[shape]


def run_layer(hip, shape, key, fused):
    """Forward (kept V; pooled), dz prep, weight gradient and the input gradients of one layer
    with key 50 = `key`; workspaces start as NaN."""
    B, H, W, Cin, Cout = shape
    x, w, b, dz, sy, sx = layer_inputs(shape)
    xd, wd, bd, dzd, syd, sxd = nhwc(x).cuda(), krsc(w).cuda(), b.cuda(), nhwc(dz).cuda(), sy.cuda(), sx.cuda()
    nan = float("nan")
    nk = hip.pis_conv3x3_keep_bytes(B, H, W, Cin, Cout)
    nws = hip.pis_conv3x3_ex_ws(B, H, W, Cin, Cout)
    nwg = hip.pis_conv3x3_wgrad_ws(B, H, W, Cin, Cout)
    out = {}
    prev = hip.pis_tune(KEY, key), hip.pis_tune(KEY_FUSED, fused)
    try:
        keep = torch.full((nk // 4 + 1,), nan, device="cuda")
        ws = torch.full((nws // 4 + 1,), nan, device="cuda")
        y = torch.full((B, H, W, Cout), nan, device="cuda")
        assert hip.pis_conv3x3_fwd_keep(xd.data_ptr(), Cin, wd.data_ptr(), bd.data_ptr(), syd.data_ptr(), y.data_ptr(),
                                        Cout, B, H, W, Cin, Cout, RELU | SCALE, ws.data_ptr(), nws, keep.data_ptr(),
                                        s()) == 0, hip.pis_last_error()
        out["y"], out["keep"] = y.cpu(), bits(keep).cpu()

        keep2 = torch.full((nk // 4 + 1,), nan, device="cuda")
        ws = torch.full((nws // 4 + 1,), nan, device="cuda")
        y = torch.full((B, H, W, Cout), nan, device="cuda")
        pool = torch.full((B, H // 2, W // 2, Cout), nan, device="cuda")
        assert hip.pis_conv3x3_fwd_pool(xd.data_ptr(), Cin, wd.data_ptr(), bd.data_ptr(), syd.data_ptr(), y.data_ptr(),
                                        Cout, B, H, W, Cin, Cout, RELU | SCALE, ws.data_ptr(), nws, keep2.data_ptr(),
                                        pool.data_ptr(), s()) == 0, hip.pis_last_error()
        out["y_pool"], out["pool"] = y.cpu(), pool.cpu()

        for i, flags in enumerate(DGRAD_FLAGS):
            wsd = torch.full((nws // 4 + 1,), nan, device="cuda")
            wsg = torch.full((nwg // 4 + 1,), nan, device="cuda")
            rc = hip.pis_conv3x3_bwd_prep(dzd.data_ptr(), Cout, B, H, W, Cin, Cout, wsd.data_ptr(), nws,
                                          wsg.data_ptr(), nwg, s())
            assert rc == 1, (rc, hip.pis_last_error())
            if i == 0:
                dw = torch.full((Cout, 3, 3, Cin), nan, device="cuda")
                db = torch.full((Cout,), nan, device="cuda")
                assert hip.pis_conv3x3_wgrad_keep(xd.data_ptr(), Cin, dzd.data_ptr(), Cout, dw.data_ptr(),
                                                  db.data_ptr(), B, H, W, Cin, Cout, PREP, wsg.data_ptr(), nwg,
                                                  keep.data_ptr(), s()) == 0, hip.pis_last_error()
                out["dw"], out["db"] = dw.cpu(), db.cpu()
            dx = torch.full((B, H, W, Cin), 0.5 if flags & ACC else nan, device="cuda")
            assert hip.pis_conv3x3_dgrad_ex(dzd.data_ptr(), Cout, wd.data_ptr(), xd.data_ptr(), Cin, sxd.data_ptr(),
                                            dx.data_ptr(), Cin, B, H, W, Cin, Cout, flags | PREP | UNFLIPPED,
                                            wsd.data_ptr(), nws, s()) == 0, hip.pis_last_error()
            out[f"dx_{flags}"] = dx.cpu()
        torch.cuda.synchronize()
    finally:
        hip.pis_tune(KEY, prev[0])
        hip.pis_tune(KEY_FUSED, prev[1])
    return out


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_new_forms_equal_old_bitwise(hip, shape, fused):
    """Key 50 = 1 against 0: y, the kept V, the pooled copy, dW, db and dx under every flag set are
    bit for bit the same. fused = 0 (key 15) takes the 64- and 128-channel contractions off the
    fused contraction + output kernel, whose V carries the tile maxima, so both forms of the
    transforms (with and without them) run at those shapes."""
    old, new = run_layer(hip, shape, 0, fused), run_layer(hip, shape, 1, fused)
    assert old.keys() == new.keys()
    for name in old:
        assert torch.equal(old[name], new[name]), name


def test_new_forms_against_float64(hip):
    """Key 50 = 1 against float64 within test_conv3x3_bwd_prep's bound."""
    shape = (2, 16, 32, 128, 64)
    x, w, b, dz, sy, sx = layer_inputs(shape)
    out = run_layer(hip, shape, 1, 1)
    y_ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)) * sy.double()[:, :, None, None]
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), dz.double(), padding=1) * (x > 0)
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), w.shape, dz.double(), padding=1)
    assert rel_err(nchw(out["y"]), y_ref) < 1e-5
    assert rel_err(nchw(out["pool"]), F.max_pool2d(y_ref, 2)) < 1e-5
    assert rel_err(nchw(out[f"dx_{MASK}"]), dx_ref) < 1e-5
    assert rel_err(nchw(out[f"dx_{MASK | SCALE}"]), dx_ref * sx.double()[:, :, None, None]) < 1e-5
    assert rel_err(nchw(out[f"dx_{MASK | ACC}"]) - 0.5, dx_ref) < 1e-5
    assert rel_err(out["dw"].permute(0, 3, 1, 2), dw_ref) < 1e-5
    assert rel_err(out["db"], dz.double().sum(dim=(0, 2, 3))) < 1e-5
