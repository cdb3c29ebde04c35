"""The overlap-add F(4x4,3x3) input gradient (pis_tune key 51 = 1: csrc/winograd.hip
wino4_output_t_kernel, the filter U' = G' g G'^T and the contraction on the weight gradient's E)
against the V(dz) form (key 51 = 0), through the C-ABI, on the batched-GEMM path (Winograd always,
direct kernels off, fused contraction off).

Shapes: the smallest at which the overlap-add can go wrong — one tile row (no vertical
neighbours; a tile's t - 1 / t + 1 at a row end is another image's tile), one tile column, a 2 x 2
tile grid (every tile a corner tile), a non-square grid and one with interior tiles; 32 -> 64,
64 -> 32 and 128 -> 128 channels. pis_conv3x3_bwd_prep and the Winograd weight gradient take
64-aligned channels only (their API contract: prep returns 0 otherwise), so the prepared flag set
and the dW / db comparison run on the 128 -> 128 pairs and the other pairs assert the 0."""
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_torch as rt

pytestmark = pytest.mark.gpu

RELU, SCALE, MASK, ACC, PREP, UNFLIPPED = 1, 2, 4, 8, 16, 32
KEY = 51
FORCE = {8: 2, 29: 0, 15: 0}  # Winograd always, direct off, fused contraction off
GRIDS = [(2, 4, 12), (2, 12, 4), (2, 8, 8), (1, 8, 16), (2, 16, 32)]
CHANNELS = [(32, 64), (64, 32), (128, 128)]
CASES = [g + c for g in GRIDS for c in CHANNELS]
PAD, OFF = 32, 16  # the strided set: dx and the mask are channel slices [OFF, OFF + Cin) of Cin + PAD
SETS = ["plain", "mask", "mask_acc", "strided"]
TOL_STEP = 1e-4  # tests/test_unet_gpu.py TOL: the engine-vs-oracle bound per gradient tensor


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


class Knobs:
    def __init__(self, hip, kv):
        self.hip, self.kv, self.prev = hip, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.prev[k] = self.hip.pis_tune(k, v)

    def __exit__(self, *a):
        for k, v in self.prev.items():
            self.hip.pis_tune(k, v)


_inputs, _refs, _runs = {}, {}, {}


def layer_inputs(case, single=False):
    """Host tensors of one layer, made once and left unchanged. dz: distinct values per pixel, or
    (single) non-zero in the one pixel (3, 3) of the LAST image — next to a tile corner, so its 3 x 3
    footprint lands in four tiles."""
    if (case, single) not in _inputs:
        B, H, W, Cin, Cout = case
        g = torch.Generator().manual_seed(51)
        x = torch.randn(B, Cin, H, W, generator=g)  # its sign is the ReLU mask
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
        dz = torch.randn(B, Cout, H, W, generator=g)
        if single:
            keep = torch.zeros_like(dz)
            keep[B - 1, :, 3, 3] = dz[B - 1, :, 3, 3]
            dz = keep
        _inputs[case, single] = (x, w, dz)
    return _inputs[case, single]


def reference(case, single=False):
    """float64 dx per flag set, computed once."""
    if (case, single) not in _refs:
        B, H, W, Cin, Cout = case
        x, w, dz = layer_inputs(case, single)
        dx = torch.nn.grad.conv2d_input(x.shape, w.double(), dz.double(), padding=1)
        m = dx * (x > 0)
        _refs[case, single] = {"plain": dx, "mask": m, "mask_acc": m + 0.5, "strided": m}
    return _refs[case, single]


def run_layer(hip, case, key, single=False):
    """Every dgrad_ex flag set, unprepared from the flipped copy and (64-aligned channels) prepared
    from the original weights, plus dW / db from the prepared E, with key 51 = `key`."""
    B, H, W, Cin, Cout = case
    x, w, dz = layer_inputs(case, single)
    xd, wd, dzd = nhwc(x).cuda(), krsc(w).cuda(), nhwc(dz).cuda()
    xw = torch.zeros(B, H, W, Cin + PAD, device="cuda")
    xw[..., OFF:OFF + Cin] = xd
    nan = float("nan")
    out = {}
    with Knobs(hip, {**FORCE, KEY: key}):
        assert hip.pis_conv3x3_filter_format(B, H, W, Cin, Cout, 1) == (1 if Cin % 32 == 0 and Cout % 32 == 0 else 0)
        nws = hip.pis_conv3x3_ex_ws(B, H, W, Cin, Cout)
        assert nws > 0
        aligned = Cin % 64 == 0 and Cout % 64 == 0
        nwg = hip.pis_conv3x3_wgrad_ws(B, H, W, Cin, Cout) if aligned else 1024
        wf = torch.empty(Cin * 9 * Cout, device="cuda")
        assert hip.pis_conv3x3_flip(wd.data_ptr(), wf.data_ptr(), Cin, Cout, s()) == 0
        for prepared in (False, True):
            for name in SETS:
                wsd = torch.full((nws // 4 + 1,), nan, device="cuda")
                wsg = torch.full((nwg // 4 + 1,), nan, device="cuda")
                flags, wptr = {"plain": 0, "mask": MASK, "mask_acc": MASK | ACC, "strided": MASK}[name], wf.data_ptr()
                if prepared:
                    rc = hip.pis_conv3x3_bwd_prep(dzd.data_ptr(), Cout, B, H, W, Cin, Cout, wsd.data_ptr(), nws,
                                                  wsg.data_ptr(), nwg, s())
                    assert rc == (1 if aligned else 0), (rc, hip.pis_last_error())
                    if not aligned:
                        continue
                    flags, wptr = flags | PREP | UNFLIPPED, wd.data_ptr()
                if name == "strided":
                    dx = torch.full((B, H, W, Cin + PAD), 7.0, device="cuda")
                    dptr, ldd, mptr, ldm = dx.data_ptr() + 4 * OFF, Cin + PAD, xw.data_ptr() + 4 * OFF, Cin + PAD
                else:
                    dx = torch.full((B, H, W, Cin), 0.5 if flags & ACC else nan, device="cuda")
                    dptr, ldd, mptr, ldm = dx.data_ptr(), Cin, xd.data_ptr(), Cin
                assert hip.pis_conv3x3_dgrad_ex(dzd.data_ptr(), Cout, wptr, mptr if flags & MASK else 0, ldm, 0, dptr,
                                                ldd, B, H, W, Cin, Cout, flags, wsd.data_ptr(), nws, s()) == 0, \
                    hip.pis_last_error()
                if name == "strided":
                    assert torch.all(dx[..., :OFF] == 7.0) and torch.all(dx[..., OFF + Cin:] == 7.0)
                    dx = dx[..., OFF:OFF + Cin].contiguous()
                out[name, prepared] = dx.cpu()
                if prepared and name == "plain":  # the weight gradient from the E the input gradient just read
                    nk = hip.pis_conv3x3_keep_bytes(B, H, W, Cin, Cout)
                    assert nk > 0
                    keep = torch.full((nk // 4 + 1,), nan, device="cuda")
                    y = torch.empty(B, H, W, Cout, device="cuda")
                    ws = torch.empty(nws // 4 + 1, device="cuda")
                    assert hip.pis_conv3x3_fwd_keep(xd.data_ptr(), Cin, wd.data_ptr(), 0, 0, y.data_ptr(), Cout, B, H, W,
                                                    Cin, Cout, 0, ws.data_ptr(), nws, keep.data_ptr(), s()) == 0
                    dw = torch.full((Cout, 3, 3, Cin), nan, device="cuda")
                    db = torch.full((Cout,), nan, device="cuda")
                    assert hip.pis_conv3x3_wgrad_keep(xd.data_ptr(), Cin, dzd.data_ptr(), Cout, dw.data_ptr(),
                                                      db.data_ptr(), B, H, W, Cin, Cout, PREP, wsg.data_ptr(), nwg,
                                                      keep.data_ptr(), s()) == 0, hip.pis_last_error()
                    out["dw"], out["db"] = dw.cpu(), db.cpu()
        torch.cuda.synchronize()
    return out


def cached(hip, case, key, single=False):
    if (case, key, single) not in _runs:
        _runs[case, key, single] = run_layer(hip, case, key, single)
    return _runs[case, key, single]


@pytest.mark.parametrize("case", CASES)
def test_dx_against_float64(hip, case):
    """dx of every flag set with key 51 = 1 against torch.nn.grad.conv2d_input in float64, at
    test_conv3x3_bwd_prep's bound for the same quantity; the error of both key values is printed."""
    ref = reference(case)
    old, new = cached(hip, case, 0), cached(hip, case, 1)
    for k in sorted(new, key=str):
        if k in ("dw", "db"):
            continue
        e0, e1 = rel_err(nchw(old[k]), ref[k[0]]), rel_err(nchw(new[k]), ref[k[0]])
        print(f"dgrad_t {case} {k}: rel err key0 {e0:.3e} key1 {e1:.3e}")
        assert e1 < 1e-5, (case, k, e0, e1)


@pytest.mark.parametrize("channels", CHANNELS)
def test_single_pixel_next_to_a_tile_corner(hip, channels):
    """dz non-zero in pixel (3, 3) of the last image only: its footprint spans four tiles (one own,
    two edge and one corner contribution); the other image stays exactly zero."""
    case = (2, 8, 8) + channels
    ref = reference(case, True)
    new = cached(hip, case, 1, True)
    for k in [k for k in new if k not in ("dw", "db")]:
        e = rel_err(nchw(new[k]), ref[k[0]])
        print(f"dgrad_t single {case} {k}: rel err key1 {e:.3e}")
        assert e < 1e-5, (k, e)
    assert torch.all(new["plain", False][0] == 0)
    assert torch.all(new["mask_acc", False][0] == 0.5)


@pytest.mark.parametrize("case", CASES)
def test_repeatable_and_prepared_equals_unprepared(hip, case):
    """Key 1 run twice is bitwise equal; the prepared input gradient (original weights, the weight
    gradient's E read in place) equals the unprepared one (flipped copy, its own E) bitwise."""
    a, b = cached(hip, case, 1), run_layer(hip, case, 1)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for name in SETS:
        if (name, True) in a:
            assert torch.equal(a[name, False], a[name, True]), name
    assert ((("plain", True) in a) == (case[3] % 64 == 0 and case[4] % 64 == 0))


@pytest.mark.parametrize("case", [c for c in CASES if c[3] % 64 == 0 and c[4] % 64 == 0])
def test_weight_gradient_untouched(hip, case):
    """dW and db are bitwise the same for key 0 and key 1: E and the weight gradient do not change."""
    old, new = cached(hip, case, 0), cached(hip, case, 1)
    assert torch.equal(old["dw"], new["dw"]) and torch.equal(old["db"], new["db"])
    x, w, dz = layer_inputs(case)
    assert rel_err(new["dw"].permute(0, 3, 1, 2), torch.nn.grad.conv2d_weight(x.double(), w.shape, dz.double(),
                                                                               padding=1)) < 1e-5


def _step(hip, key, B=2, H=64, W=64, seed=11):
    from physics_informed_image_segmentation_amd import DiceBCEPDELoss, UNet
    with Knobs(hip, {**FORCE, KEY: key}):
        # the 64^2 .. 4^2 levels all run the batched GEMM both ways
        assert hip.pis_conv3x3_filter_format(B, H, W, 64, 64, 1) == 1
        assert hip.pis_conv3x3_filter_format(B, H // 4, W // 4, 512, 256, 1) == 1
        img, mask = rt.synthetic_batch(B, H, W, seed=seed)
        torch.manual_seed(seed)
        net = UNet(1, 1, 64).cuda().train()
        net.set_dropout_scales(rt.make_drop_scales(rt.UNetRef(1, 1, 64), B, torch.Generator().manual_seed(seed)))
        crit = DiceBCEPDELoss(pde_weight=1e-2, phase_field_weight=1e-2, diffusion_coeff=5.0, epsilon=0.05)
        u = net(img.cuda())
        crit(u, mask.cuda()).backward()
        torch.cuda.synchronize()
        return u.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def test_whole_step_key1_against_key0(hip):
    """One training step at 2 x 64 x 64 with every 3 x 3 layer on the batched GEMM: the forward is
    untouched (bitwise u) and every gradient with key 1 is within the engine-vs-oracle tolerance of
    key 0's."""
    u0, g0 = _step(hip, 0)
    u1, g1 = _step(hip, 1)
    assert torch.equal(u0, u1)
    worst = sorted(((rel_err(g1[n], g0[n]), n) for n in g0), reverse=True)
    print(f"dgrad_t whole step: worst gradient differences key1 vs key0 {worst[:3]}")
    assert worst[0][0] < TOL_STEP, worst[:5]
    assert any(not torch.equal(g0[n], g1[n]) for n in g0)  # the new path did run
