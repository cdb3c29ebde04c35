"""Which kernels a 3x3-conv layer launches, and the bits they write, against a recording made
before the planner (csrc/conv3x3_plan.hip) existed: tests/golden/conv3x3_dispatch.json, written on
the MI355X by tests/golden/record_conv3x3_dispatch.py.

One layer per case, through the C-ABI in the order the engine (unet.py) uses: the filter operands
ahead (pis_conv3x3_filters), pis_conv3x3_fwd_keep and pis_conv3x3_fwd_pool, pis_conv3x3_bwd_prep,
pis_conv3x3_wgrad_keep, pis_conv3x3_dgrad_ex with the engine's choice of flags. The same kernels
launched with the same arguments give the same bits, so the SHA-256 of every output and the
sequence of launch-hook names must equal the recording.

Shapes (B = 1): the smallest that reaches each kernel family under the default keys."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_dispatch.json")
RELU, SCALE, MASK, ACC, PREP, UNFLIPPED, READY = 1, 2, 4, 8, 16, 32, 64

# name: (H, W, Cin, Cout, tune keys, options, (filter format fwd, dgrad), hook names that must appear)
CASES = {
    # the auto policy of the direct kernels needs H >= 256: the image stays narrow
    "direct": (256, 32, 64, 64, {}, {}, (3, 3), ("direct_h3_fwd", "direct_h3_pool", "direct_wgrad_h3", "direct_h3_dgrad")),
    # T = 128 tiles: T % 32 == 0 and T >= 2 C (32 x 32 has T = 64 < 2 C and stays on the batched GEMM)
    "fused_f4": (32, 64, 64, 64, {}, {}, (2, 2), ("wino_gemm_out", "wino_wgrad_gemm")),
    # batched GEMM forward; its input gradient in the overlap-add form (key 51)
    "batched_f4": (16, 16, 128, 256, {}, {}, (1, 1), ("wino_gemm", "wino_wgrad_gemm")),
    # F(2x2,3x3) wants >= 256 contraction channels and 128 outputs (64 -> 64 here runs the generic kernel)
    "f2": (30, 34, 256, 256, {}, {}, (0, 0), ("wino_gemm", "wino_wgrad_gemm")),
    "generic": (6, 10, 64, 64, {}, {}, (0, 0), ()),
    "wgrad_halo": (6, 16, 64, 64, {}, {}, (0, 0), ("wgrad3x3_halo",)),
    # a Winograd layer without workspace for its forward / input gradient: the halo kernel
    "halo_small_ws": (8, 16, 64, 64, {}, {"ex_ws": 0}, None, ("conv3x3_halo", "wino_wgrad_gemm")),
    "c1_row": (8, 64, 1, 64, {}, {}, (0, 0), ()),
    "f6": (24, 24, 256, 256, {47: 1}, {}, (4, 4), ("wino_gemm", "wino_wgrad_gemm")),
}

# The Winograd launch variants (csrc/conv3x3_plan.h WinoGemm, WinoVariants, wino_fused_form), one key off its
# default per case, recorded from the launch ladders that csrc/winograd.hip held before the planner named them.
BATCHED, FUSED = (16, 16, 128, 256), (32, 64, 64, 64)  # 16 tiles; 128 tiles = 4 groups of 32
for _key, _values in ((10, (0, 1, 2, 3)), (17, (4,)), (46, (0,)), (48, (0,)), (50, (0, 2, 4)), (51, (0, 2))):
    for _v in _values:  # the batched GEMM's arithmetic; transform widths and forms; the overlap-add input gradient
        CASES[f"batched_f4_k{_key}_{_v}"] = (*BATCHED, {_key: _v}, {}, (1, 1), ("wino_gemm",))
CASES["f2_k11_0"] = (16, 16, 256, 256, {11: 0}, {}, (0, 0), ("wino_gemm",))
for _key, _values in ((15, (2, 3, 4)), (22, (0,)), (25, (0,)), (17, (4,))):
    for _v in _values:  # groups per block, bf16x6 planes, lockstep waves, 4-channel transforms
        CASES[f"fused_f4_k{_key}_{_v}"] = (*FUSED, {_key: _v}, {}, (2, 2), ("wino_gemm_out",))
CASES["fused_f4_8groups_k15_4"] = (64, 64, 64, 64, {15: 4}, {}, (2, 2), ("wino_gemm_out",))
# the 128-channel fused form needs T >= 2 C tiles
CASES["fused_f4_c128"] = (64, 64, 128, 128, {}, {}, (2, 2), ("wino_gemm_out",))
CASES["fused_f4_c128_k22_0"] = (64, 64, 128, 128, {22: 0}, {}, (2, 2), ("wino_gemm_out",))
CASES["f6_k47_2"] = (24, 24, 256, 256, {47: 2}, {}, (4, 4), ("wino_gemm",))
CASES["f6_k47_3"] = (24, 24, 256, 256, {47: 3}, {}, (4, 4), ("wino_gemm",))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(lib, name):
    """-> {"formats": [fwd, dgrad], "hooks": [...], "sha256": {output: digest}}"""
    H, W, Cin, Cout, keys, opt, _, _ = CASES[name]
    B = 1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (3 * Cin ** 0.5)).cuda()
    bias = torch.randn(Cout, generator=g).cuda()
    dz = torch.randn(B, H, W, Cout, generator=g).cuda()
    st = torch.cuda.current_stream().cuda_stream
    dev = dict(device="cuda")
    hooks, prev, out = [], {}, {}
    for k, v in keys.items():
        prev[k] = lib.pis_tune(k, v)
    _hip.set_launch_hook(lambda kernel, phase, stream, flop: hooks.append(kernel) if phase == 0 else None)
    try:
        s = (B, H, W, Cin, Cout)
        fmt = [lib.pis_conv3x3_filter_format(*s, 0), lib.pis_conv3x3_filter_format(*s, 1)]
        nws = lib.pis_conv3x3_ex_ws(*s)
        nwg = lib.pis_conv3x3_wgrad_ws(*s)
        nk = lib.pis_conv3x3_keep_bytes(*s)
        wsd = torch.zeros(nws // 4 + 256, **dev)
        wsg = torch.zeros(nwg // 4 + 256, **dev)
        keep = torch.zeros(nk // 4 + 1, **dev) if nk else None
        wsb = opt.get("ex_ws", nws)  # bytes offered to the forward / input gradient
        ahead = "ex_ws" not in opt and Cin > 1
        # 1. the filter operands, both directions, in one call
        filt = {}
        for dg in (0, 1):
            nb = lib.pis_conv3x3_filter_bytes(*s, dg) if ahead else 0
            if nb:
                filt[dg] = torch.zeros(nb // 4 + 1, **dev)
        if filt:
            jobs = (_hip.FilterJob * len(filt))()
            for i, (dg, buf) in enumerate(filt.items()):
                jobs[i] = _hip.FilterJob(w.data_ptr(), buf.data_ptr(), buf.numel() * 4, B, H, W, Cin, Cout, dg)
            _hip.call("pis_conv3x3_filters", ctypes.addressof(jobs), len(jobs), st)
        # 2. forward, kept transform; then the pooled forward of the same layer
        wptr, flags = (filt[0].data_ptr(), RELU | READY) if 0 in filt else (w.data_ptr(), RELU)
        nan = float("nan")
        y = torch.full((B, H, W, Cout), nan, **dev)
        _hip.call("pis_conv3x3_fwd_keep", x.data_ptr(), Cin, wptr, bias.data_ptr(), 0, y.data_ptr(), Cout, *s, flags,
                  wsd.data_ptr(), wsb, _hip.ptr(keep), st)
        out["y"] = sha(y)
        out["keep"] = sha(keep) if nk else None
        if Cin > 1 and H % 2 == 0 and W % 2 == 0:
            y2 = torch.full((B, H, W, Cout), nan, **dev)
            pool = torch.full((B, H // 2, W // 2, Cout), nan, **dev)
            _hip.call("pis_conv3x3_fwd_pool", x.data_ptr(), Cin, wptr, bias.data_ptr(), 0, y2.data_ptr(), Cout, *s, flags,
                      wsd.data_ptr(), wsb, _hip.ptr(keep), pool.data_ptr(), st)
            out["y_pooled_call"], out["pool"] = sha(y2), sha(pool)
        # 3. one pass over dz for both backward products, where the layer has one
        prep = 0
        if Cin > 1 and nk:
            prep = lib.pis_conv3x3_bwd_prep(dz.data_ptr(), Cout, *s, wsd.data_ptr(), wsb, wsg.data_ptr(), nwg, st)
            assert prep >= 0, lib.pis_last_error()
        out["prep"] = prep
        # 4. weight and bias gradient
        dw = torch.full((Cout, 3, 3, Cin), nan, **dev)
        db = torch.full((Cout,), nan, **dev)
        _hip.call("pis_conv3x3_wgrad_keep", x.data_ptr(), Cin, dz.data_ptr(), Cout, dw.data_ptr(), db.data_ptr(), *s,
                  PREP if prep else 0, wsg.data_ptr(), nwg, _hip.ptr(keep), st)
        out["dw"], out["db"] = sha(dw), sha(db)
        # 5. input gradient through the ReLU mask of x, the engine's operand choice
        if Cin > 1:
            flags, wf = MASK, None
            if prep:
                wf, flags = w, flags | PREP | UNFLIPPED
                if 1 in filt:
                    wf, flags = filt[1], flags | READY
            elif lib.pis_conv3x3_dgrad_direct(*s, Cout, wsb):
                wf, flags = w, flags | UNFLIPPED
                if 1 in filt:
                    wf, flags = filt[1], flags | READY
            elif 1 in filt and fmt[1] == 4:
                wf, flags = filt[1], flags | UNFLIPPED | READY
            else:
                wf = torch.empty(Cin * 9 * Cout, **dev)
                _hip.call("pis_conv3x3_flip", w.data_ptr(), wf.data_ptr(), Cin, Cout, st)
            dx = torch.full((B, H, W, Cin), nan, **dev)
            _hip.call("pis_conv3x3_dgrad_ex", dz.data_ptr(), Cout, wf.data_ptr(), x.data_ptr(), Cin, 0, dx.data_ptr(), Cin,
                      *s, flags, wsd.data_ptr(), wsb, st)
            out["dx"] = sha(dx)
            out["dgrad_flags"] = flags
        torch.cuda.synchronize()
    finally:
        _hip.set_launch_hook(None)
        for k, v in prev.items():
            lib.pis_tune(k, v)
    return {"formats": fmt, "hooks": hooks, "sha256": out}


def check_path(name, got):
    """The case reached the kernel family it is named for."""
    _, _, _, _, _, _, formats, names = CASES[name]
    if formats is not None:
        assert tuple(got["formats"]) == formats, (name, got["formats"])
    for n in names:
        assert n in got["hooks"], (name, n, got["hooks"])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_same_kernels_same_bits(hip, golden, name):
    got = run_case(hip, name)
    check_path(name, got)
    want = golden[name]
    assert got["formats"] == want["formats"]
    assert got["hooks"] == want["hooks"]
    assert got["sha256"] == want["sha256"]
