"""Which kernels a transposed-conv layer (ConvTranspose2d(k=2, s=2)) launches, and the bits they
write, against a recording made before the planner (csrc/convt_plan.hip) existed:
tests/golden/convt_dispatch.json, written on the MI355X by tests/golden/record_convt_dispatch.py.

One layer per case through the C-ABI: pis_convt2x2_fwd, pis_convt2x2_prep, pis_convt2x2_dgrad
(masked, then masked with PIS_ACCUMULATE onto a seeded dx), pis_convt2x2_wgrad. The "wino" cases run
pis_conv3x3_wgrad on a F(3x3,4x4) layer instead: its split-K GEMM takes the same kernel choice
(choose_wgrad_kernel) as the transposed conv's generic arm. The same kernels launched with the same
arguments give the same bits, so the SHA-256 of every output must equal the recording, and
pis_debug_convt2x2_algo must name the arm the case is meant for.

Shapes (B, H, W of the low-resolution input, Cin, Cout): the smallest that reach each arm."""
import hashlib
import json
import os

import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convt_dispatch.json")
MASK, ACC = 4, 8

# csrc/convt_plan.h ConvtAlgo / ConvtWgradAlgo, csrc/conv3x3_plan.h WgradKernel
H3_K32, GEMM_H3, GEMM_X6, GEMM_F32, IGEMM = 1, 2, 3, 4, 5
TILE, ROWS_UP2, SPLITK = 1, 2, 3
F32, X6, H3_COLS, H3T, H3T_EXACT, H3T_TWIN = range(6)


def wcode(algo, kernel, bm, bn):
    """pis_debug_convt2x2_algo's op 2 answer (kernel None: the arm has a kernel of its own)."""
    return algo | (0 if kernel is None else kernel + 1) << 4 | (bm // 64) << 8 | (bn // 64) << 12


# name: (kind, (B, H, W, Cin, Cout), tune keys, destination offset in floats,
#        forward arm, input-gradient arm, weight-gradient arm)
T1, T2, R1, C128, C64, W4, K32 = ((1, 2, 32, 128, 64), (1, 20, 32, 128, 64), (1, 2, 32, 256, 64), (1, 2, 32, 128, 64),
                                  (1, 2, 16, 64, 64), (1, 4, 4, 64, 64), (1, 4, 32, 128, 32))
CASES = {
    # M = B H W = 64 pixels: not a whole 128-row tile, the forward and input gradient fall through
    "tile": ("convt", T1, {}, 0, GEMM_H3, GEMM_H3, wcode(TILE, None, 256, 128)),
    "tile_splits": ("convt", T2, {}, 0, H3_K32, H3_K32, wcode(TILE, None, 256, 128)),
    "rows_up2": ("convt", R1, {56: 0}, 0, GEMM_H3, GEMM_H3, wcode(ROWS_UP2, H3T_EXACT, 128, 128)),
    "x6_cols_128": ("convt", C128, {56: 0}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, X6, 64, 128)),
    "x6_cols_64": ("convt", C64, {}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, X6, 64, 64)),
    "h3_cols_128": ("convt", C128, {56: 0, 14: 2}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, H3_COLS, 64, 128)),
    "h3_cols_64": ("convt", C64, {14: 2}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, H3_COLS, 64, 64)),
    "f32_128": ("convt", C128, {56: 0, 14: 0}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, F32, 64, 128)),
    "f32_64": ("convt", C64, {14: 0}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, F32, 64, 64)),
    # the column-staged kernels read 8 pixels of an image row: W % 8 != 0 runs fp32 MFMA
    "f32_w4": ("convt", W4, {}, 0, GEMM_H3, GEMM_H3, wcode(SPLITK, F32, 64, 64)),
    # Cout = 32: outside the weight gradient's contract, forward and input gradient only
    "k32": ("convt", K32, {}, 0, H3_K32, H3_K32, None),
    "k32_dst_offset": ("convt", K32, {}, 1, GEMM_H3, GEMM_H3, None),
    "gemm_x6": ("convt", K32, {13: 1}, 0, GEMM_X6, GEMM_X6, None),
    "gemm_f32": ("convt", K32, {13: 2}, 0, GEMM_F32, GEMM_F32, None),
    "gemm_h3": ("convt", K32, {13: 3}, 0, GEMM_H3, GEMM_H3, None),
    "igemm": ("convt", (1, 2, 4, 8, 8), {13: 0}, 0, IGEMM, IGEMM, None),
    # pis_conv3x3_wgrad, F(3x3,4x4): (B, H, W, Cin, Cout) of the 3x3 layer; the last entry is the
    # split-K kernel its GEMM is meant to take. batched_f4 of tests/test_conv3x3_dispatch_gpu.py
    # has 128 input channels: key 14's auto rule keeps bf16x6 whatever key 31 says
    "wino_f4": ("wino", (1, 16, 16, 128, 256), {}, 0, None, None, X6),
    "wino_f4_key31": ("wino", (1, 16, 16, 128, 256), {31: 0}, 0, None, None, X6),
    "wino_f4_key14": ("wino", (1, 16, 16, 128, 256), {14: 1}, 0, None, None, X6),
    # 256 input channels: the row-staged fp16x3 kernel (T = 16 tiles: its tail form)
    "wino_h3t": ("wino", (1, 16, 16, 256, 256), {}, 0, None, None, H3T),
    "wino_h3_cols": ("wino", (1, 16, 16, 256, 256), {31: 0}, 0, None, None, H3_COLS),
    "wino_x6": ("wino", (1, 16, 16, 256, 256), {14: 1}, 0, None, None, X6),
    "wino_f32": ("wino", (1, 16, 16, 256, 256), {14: 0}, 0, None, None, F32),
    # T = 64 tiles: whole K-steps
    "wino_h3t_exact": ("wino", (1, 32, 32, 256, 256), {}, 0, None, None, H3T_EXACT),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def nan_dst(shape, off):
    """A NaN-filled destination `off` floats past a 16-byte aligned address."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    return buf[off:off + n].view(shape)


def spread(t, g):
    """t with every pixel and every channel scaled by its own log-normal factor: the fp16x3 kernels
    scale by the maximum of a wave's, a block's, a 16- or a 32-wide K-step's operands, so on operands
    of one magnitude two of them can write the same bits."""
    for shape in (t.shape[:-1] + (1,), (1,) * (t.dim() - 1) + t.shape[-1:]):
        t = t * torch.exp(1.5 * torch.randn(shape, generator=g))
    return t


def run_convt(lib, shape, off, st):
    B, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(11)
    x = spread(torch.relu(torch.randn(B, H, W, Cin, generator=g)), g).cuda()
    dy = spread(torch.randn(B, 2 * H, 2 * W, Cout, generator=g), g).cuda()
    w = (spread(torch.randn(2, 2, Cout, Cin, generator=g), g) / Cin ** 0.5).cuda()
    bias = torch.randn(Cout, generator=g).cuda()
    dx0 = torch.randn(B, H, W, Cin, generator=g)
    out = {}
    y = nan_dst((B, 2 * H, 2 * W, Cout), off)
    _hip.call("pis_convt2x2_fwd", x.data_ptr(), Cin, w.data_ptr(), bias.data_ptr(), y.data_ptr(), Cout, *shape, st)
    out["y"] = sha(y)
    wc = torch.full((Cin, 2, 2, Cout), float("nan"), device="cuda")
    _hip.call("pis_convt2x2_prep", w.data_ptr(), wc.data_ptr(), Cin, Cout, st)
    dx = nan_dst((B, H, W, Cin), off)
    _hip.call("pis_convt2x2_dgrad", dy.data_ptr(), Cout, wc.data_ptr(), x.data_ptr(), Cin, dx.data_ptr(), Cin, *shape,
              MASK, st)
    out["dx"] = sha(dx)
    dxa = nan_dst((B, H, W, Cin), off)
    dxa.copy_(dx0)
    _hip.call("pis_convt2x2_dgrad", dy.data_ptr(), Cout, wc.data_ptr(), x.data_ptr(), Cin, dxa.data_ptr(), Cin, *shape,
              MASK | ACC, st)
    out["dx_acc"] = sha(dxa)
    nws = None
    if Cin % 64 == 0 and Cout % 64 == 0:  # pis_convt2x2_wgrad's contract
        nws = lib.pis_convt2x2_wgrad_ws(*shape)
        ws = torch.zeros(nws // 4 + 1, device="cuda")
        dw = torch.full((2, 2, Cout, Cin), float("nan"), device="cuda")
        db = torch.full((Cout,), float("nan"), device="cuda")
        _hip.call("pis_convt2x2_wgrad", x.data_ptr(), Cin, dy.data_ptr(), Cout, dw.data_ptr(), db.data_ptr(), *shape, 0,
                  ws.data_ptr(), nws, st)
        out["dw"], out["db"] = sha(dw), sha(db)
    return out, nws


def run_wino(lib, shape, st):
    B, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(12)
    x = spread(torch.relu(torch.randn(B, H, W, Cin, generator=g)), g).cuda()
    dz = spread(torch.randn(B, H, W, Cout, generator=g), g).cuda()
    nws = lib.pis_conv3x3_wgrad_ws(*shape)
    ws = torch.zeros(nws // 4 + 1, device="cuda")
    dw = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    _hip.call("pis_conv3x3_wgrad", x.data_ptr(), Cin, dz.data_ptr(), Cout, dw.data_ptr(), db.data_ptr(), *shape, 0,
              ws.data_ptr(), nws, st)
    return {"dw": sha(dw), "db": sha(db)}, nws


def run_case(lib, name):
    """-> {"sha256": {output: digest}, "hooks": [...], "wgrad_ws": bytes or None}"""
    kind, shape, keys, off = CASES[name][:4]
    st = torch.cuda.current_stream().cuda_stream
    hooks, prev = [], {}
    for k, v in keys.items():
        prev[k] = lib.pis_tune(k, v)
    _hip.set_launch_hook(lambda kernel, phase, stream, flop: hooks.append(kernel) if phase == 0 else None)
    try:
        out, nws = run_convt(lib, shape, off, st) if kind == "convt" else run_wino(lib, shape, st)
        torch.cuda.synchronize()
    finally:
        _hip.set_launch_hook(None)
        for k, v in prev.items():
            lib.pis_tune(k, v)
    return {"sha256": out, "hooks": hooks, "wgrad_ws": nws}


def arms(name):
    return CASES[name][4:]


def check_discriminates(results):
    """Two cases on one shape that are meant for different arms wrote different bits."""
    names = list(results)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if CASES[a][:2] != CASES[b][:2]:
                continue
            (fa, da, wa), (fb, db_, wb) = arms(a), arms(b)
            sa, sb = results[a]["sha256"], results[b]["sha256"]
            if fa != fb:
                assert sa["y"] != sb["y"], (a, b, "y")
            if da != db_:
                assert sa["dx"] != sb["dx"] and sa["dx_acc"] != sb["dx_acc"], (a, b, "dx")
            if wa != wb and wa is not None and wb is not None:
                assert sa["dw"] != sb["dw"], (a, b, "dw")


def planned_arms(lib, name):
    """What pis_debug_convt2x2_algo answers for the case's calls, under the case's keys."""
    kind, shape, keys, off = CASES[name][:4]
    B, H, W, Cin, Cout = shape
    prev = {k: lib.pis_tune(k, v) for k, v in keys.items()}
    try:
        al = 0 if off else 1
        return (lib.pis_debug_convt2x2_algo(0, *shape, Cin, Cout, al), lib.pis_debug_convt2x2_algo(1, *shape, Cout, Cin, al),
                lib.pis_debug_convt2x2_algo(2, *shape, Cin, Cout, 1) if Cin % 64 == 0 and Cout % 64 == 0 else None)
    finally:
        for k, v in prev.items():
            lib.pis_tune(k, v)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_match_the_fixture(golden):
    assert sorted(golden) == sorted(CASES)
    check_discriminates(golden)


@pytest.mark.parametrize("name", list(CASES))
def test_same_kernels_same_bits(hip, golden, name):
    got = run_case(hip, name)
    want = golden[name]
    assert got["wgrad_ws"] == want["wgrad_ws"]
    assert got["hooks"] == want["hooks"]
    assert got["sha256"] == want["sha256"]
    if CASES[name][0] == "convt":
        assert planned_arms(hip, name) == arms(name)
    else:
        assert "wino_wgrad_gemm" in got["hooks"]
