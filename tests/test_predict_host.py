"""Whole-image inference, the host side (predict.py): the numpy definition of the tiling against
hand-written origins, reflection indices, weights and sums; the host path of clean_mask on
hand-drawn masks; the prediction CLI's refusals; pis_tile_count and the PIS_ERR_ARG cases of the
tile entry points through the loaded library (no compute call: every refused call returns before
its launch, and the pointers it is given are never dereferenced)."""
import ctypes

import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import predict as pr


# ---------------------------------------------------------------------------- tile_plan

@pytest.mark.parametrize("n, t, o, want", [
    (5, 16, 8, [0]),                    # n < t: one tile at 0, its excess is reflection
    (16, 16, 8, [0]),                   # n == t
    (17, 16, 8, [0, 1]),                # n == t + 1: the second tile pulled back to end at the edge
    (40, 16, 8, [0, 8, 16, 24]),        # the last tile ends exactly at the edge
    (41, 16, 8, [0, 8, 16, 24, 25]),    # a clamped last tile
    (40, 16, 0, [0, 16, 24]),           # o == 0: the last tile clamped from 32 to 24
    (56, 32, 16, [0, 16, 24]),          # o == t / 2, clamped from 32
    (64, 32, 16, [0, 16, 32]),          # o == t / 2, exact
])
def test_tile_origins_explicit(n, t, o, want):
    assert pr.tile_origins(n, t, o) == want
    assert pr.tile_count(n, t, o) == len(want)
    covered = np.zeros(max(n, t), int)
    for y0 in want:
        assert y0 >= 0 and (y0 + t <= n or n < t)
        covered[y0:y0 + t] += 1
    assert (covered[:n] >= 1).all() and covered.max() <= 3
    assert want == sorted(set(want))


def test_tile_plan_per_image_tile_and_jobs():
    p = pr.tile_plan(80, 96, 64, 16, "d4")
    assert (p.th, p.tw, p.ov, p.oy, p.ox, p.codes) == (64, 64, 16, (0, 16), (0, 32), tuple(range(8)))
    assert p.jobs(3) == 3 * 2 * 2 * 8 and p.sym_mask == 0xFF
    p = pr.tile_plan(20, 600, 512, 64, "flip")     # th shrinks to 32, and the overlap with it
    assert (p.th, p.tw, p.ov, p.codes) == (32, 512, 16, (0, 1, 2, 3))
    assert p.oy == (0,) and p.ox == (0, 88)
    p = pr.tile_plan(20, 600, 512, 64, "d4")       # a transpose needs a square tile
    assert (p.th, p.tw) == (512, 512)
    p = pr.tile_plan(5, 7, 512, 64, None)
    assert (p.th, p.tw, p.ov, p.codes, p.jobs()) == (16, 16, 0, (0,), 1)      # one tile: no overlap to ramp over
    assert pr.tile_plan(64, 64, 64, 16, "d4").ov == 0 and pr.tile_plan(64, 65, 64, 16, None).ov == 16
    p = pr.tile_plan(40, 56, (16, 32), 8, 0x0A)    # an explicit tile and set of codes
    assert (p.th, p.tw, p.codes) == (16, 32, (1, 3))
    for bad in (dict(tile=100), dict(tile=8), dict(tile=4096), dict(overlap=300), dict(overlap=-1),
                dict(tile=64, overlap=33), dict(tta="rot"), dict(tile=(16, 32), overlap=4, tta=0x10),
                dict(tile=(16, 32), overlap=9), dict(tta=0), dict(tta=0x100)):
        with pytest.raises(ValueError):
            pr.tile_plan(40, 56, **bad)
    with pytest.raises(ValueError):
        pr.tile_plan(0, 56)
    with pytest.raises(ValueError):
        pr.tile_plan(40, 40000)


def test_chunk_starts():
    assert pr.chunk_starts(32, 8) == (8, [0, 8, 16, 24])
    assert pr.chunk_starts(32, 5) == (5, [0, 5, 10, 15, 20, 25, 27])   # the last chunk pulled back
    assert pr.chunk_starts(3, 8) == (3, [0])
    assert pr.chunk_starts(1, 1) == (1, [0])


# ---------------------------------------------------------------------------- gather_tiles_np

ROWS_5 = [0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]       # reflect(i, 5), i = 0..15: period 8
COLS_7 = [0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0, 1, 2, 3]       # reflect(i, 7): period 12


def test_reflect_index():
    assert pr.reflect_index(np.arange(16), 5).tolist() == ROWS_5
    assert pr.reflect_index(np.arange(16), 7).tolist() == COLS_7
    assert pr.reflect_index(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert pr.reflect_index(np.arange(-9, 0), 5).tolist() == [1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert pr.reflect_index([0, 1, 2, 3], 2).tolist() == [0, 1, 0, 1]


def test_gather_5x7_under_16x16():
    img = (np.arange(35, dtype=np.float32).reshape(1, 5, 7) + 1) / 64
    plan = pr.tile_plan(5, 7, 16, 0, "d4")
    assert (plan.th, plan.tw, plan.oy, plan.ox) == (16, 16, (0,), (0,))
    out = pr.gather_tiles_np(img, plan)
    assert out.shape == (8, 1, 16, 16) and out.dtype == np.float32
    T = np.array([[img[0, r, c] for c in COLS_7] for r in ROWS_5], np.float32)
    want = [T, T[:, ::-1], T[::-1, :], T[::-1, ::-1], T.T, T[:, ::-1].T, T[::-1, :].T, T[::-1, ::-1].T]
    for q in range(8):
        np.testing.assert_array_equal(out[q, 0], want[q], err_msg=f"code {q}")
    # the same as dataset.apply_symmetry
    from physics_informed_image_segmentation_amd.dataset import apply_symmetry
    for q in range(8):
        np.testing.assert_array_equal(out[q, 0], apply_symmetry(torch.from_numpy(T), q).numpy())
    # a chunk is a slice of the whole
    np.testing.assert_array_equal(pr.gather_tiles_np(img, plan, first_job=3, n_jobs=4), out[3:7])
    with pytest.raises(ValueError):
        pr.gather_tiles_np(img, plan, first_job=7, n_jobs=2)


def test_gather_1x1_and_u8_norm():
    plan = pr.tile_plan(1, 1, 16, 0, "flip")
    out = pr.gather_tiles_np(np.full((2, 1, 1), 0.375, np.float32), plan)
    assert out.shape == (8, 1, 16, 16) and (out == np.float32(0.375)).all()
    # u8: (float(v) - lo) / den in float32
    img = np.array([[[10, 20, 30], [40, 50, 250]]], np.uint8)
    norm = np.array([[10, 240]], np.float32)
    plan = pr.tile_plan(2, 3, 16, 0, None)
    out = pr.gather_tiles_np(img, plan, norm)
    want = (img[0].astype(np.float32) - np.float32(10)) / np.float32(240)
    np.testing.assert_array_equal(out[0, 0, :2, :3], want)
    assert out[0, 0, 2, 0] == want[0, 0] and out[0, 0, 3, 1] == want[1, 1] and out[0, 0, 0, 3] == want[0, 1]
    with pytest.raises(ValueError):
        pr.gather_tiles_np(img, plan)          # u8 without norm


# ---------------------------------------------------------------------------- blend_tiles_np

def test_ramp_weights():
    assert pr.ramp_weights(16, 8).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert pr.ramp_weights(16, 3).tolist() == [1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 1]
    assert pr.ramp_weights(16, 0).tolist() == [1] * 16


def test_blend_two_tiles_hand_computed():
    """16 x 24 under 16 x 16 with overlap 8: tiles at x = 0 and x = 8, constant 0.25 and 0.75. In the
    overlap x = 8..15 tile 0 weighs 8, 7, .., 1 and tile 1 weighs 1, 2, .., 8 (times the row's wy,
    which cancels): prob = (w0 0.25 + w1 0.75) / 9; every product and sum is exact."""
    plan = pr.tile_plan(16, 24, (16, 16), 8, None)
    assert plan.oy == (0,) and plan.ox == (0, 8)
    u = np.empty((2, 1, 16, 16), np.float32)
    u[0], u[1] = 0.25, 0.75
    prob, mask = pr.blend_tiles_np(u, plan, 1, 0.5)
    assert prob.shape == (1, 16, 24) and prob.dtype == np.float32 and mask.dtype == np.uint8
    want = [0.25] * 8 + [(8 - i) * 0.25 / 9 + (1 + i) * 0.75 / 9 for i in range(8)] + [0.75] * 8
    wy = [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    for y in range(16):
        for x in range(24):
            if 8 <= x < 16:
                w0, w1 = wy[y] * (16 - x), wy[y] * (x - 7)
                assert w0 + w1 == 9 * wy[y]
                exact = np.float32(w0 * 0.25 + w1 * 0.75) / np.float32(w0 + w1)   # one float32 division
                assert prob[0, y, x] == exact
            assert abs(float(prob[0, y, x]) - want[x]) < 1e-7
    np.testing.assert_array_equal(mask, (prob > np.float32(0.5)).astype(np.uint8))
    assert mask[0, 0].tolist() == [0] * 12 + [1] * 12     # x = 11: (5 0.25 + 4 0.75) / 9 = 0.472; x = 12: 0.528


def test_blend_clamped_tiles_and_symmetries():
    # o == 0 on 16 x 40: tiles at 0, 16, 24, so x = 24..31 is covered twice with weight 1 each
    plan = pr.tile_plan(16, 40, (16, 16), 0, None)
    assert plan.ox == (0, 16, 24)
    u = np.empty((3, 1, 16, 16), np.float32)
    u[0], u[1], u[2] = 0.125, 0.5, 1.0
    prob, _ = pr.blend_tiles_np(u, plan)
    assert prob[0, 3].tolist() == [0.125] * 16 + [0.5] * 8 + [0.75] * 8 + [1.0] * 8
    # two symmetries of one tile: prob = (A + flip_W^-1(u1)) / 2
    plan = pr.tile_plan(16, 16, (16, 16), 0, 0x03)
    A = (np.arange(256, dtype=np.float32).reshape(16, 16)) / 256
    B = A.T.copy()
    u = np.stack([A, B[:, ::-1]])[:, None]
    prob, _ = pr.blend_tiles_np(u, plan)
    np.testing.assert_array_equal(prob[0], (A + B) / 2)
    # a transposing code: u[j] = apply(T, 5) comes back as T
    plan = pr.tile_plan(16, 16, (16, 16), 0, 0x20)
    prob, _ = pr.blend_tiles_np(pr.apply_symmetry_np(A, 5)[None, None], plan)
    np.testing.assert_array_equal(prob[0], A)
    # gather then blend of all eight: the image itself (every weight is 1, sums of 8 equal values are exact)
    plan = pr.tile_plan(16, 16, 16, 0, "d4")
    prob, _ = pr.blend_tiles_np(pr.gather_tiles_np(A[None], plan), plan)
    np.testing.assert_array_equal(prob[0], A)
    # NaN stays NaN and is background
    u = np.full((1, 1, 16, 16), np.nan, np.float32)
    prob, mask = pr.blend_tiles_np(u, pr.tile_plan(16, 16, 16, 0, None))
    assert np.isnan(prob).all() and not mask.any()


# ---------------------------------------------------------------------------- clean_mask, host path

def _m(rows):
    return torch.tensor([[int(c) for c in r] for r in rows], dtype=torch.uint8)


def test_clean_mask_ring():
    ring = _m(["000000000",
               "011111000",
               "010001000",
               "010101000",      # a speck inside the hole
               "010001000",
               "011111000",
               "000000001"])     # and one outside
    out = pr.clean_mask(ring, fill_holes=True)
    assert out.dtype == torch.uint8 and out.shape == ring.shape
    want = ring.clone()
    want[2:5, 2:5] = 1
    assert torch.equal(out, want)
    out = pr.clean_mask(ring, min_area=2)                      # both specks go, the hole stays
    want = ring.clone()
    want[3, 3] = want[6, 8] = 0
    assert torch.equal(out, want)
    out = pr.clean_mask(ring, min_area=2, fill_holes=True)
    want[2:5, 2:5] = 1
    assert torch.equal(out, want)
    assert torch.equal(pr.clean_mask(ring), ring)              # nothing asked: nothing changes
    assert torch.equal(pr.clean_mask(ring.float()[None, None], fill_holes=True)[0, 0], pr.clean_mask(ring, fill_holes=True))
    assert pr.clean_mask(ring[None].repeat(2, 1, 1), min_area=2).shape == (2, 7, 9)


def test_clean_mask_ring_touching_the_frame():
    ring = _m(["11111",
               "10001",
               "10001",
               "11111"])       # the ring lies on the frame, its hole does not touch it
    assert pr.clean_mask(ring, fill_holes=True).all()
    cup = _m(["10001",
              "10001",
              "10001",
              "11111"])        # open to the frame: the background inside touches it, no hole
    assert torch.equal(pr.clean_mask(cup, fill_holes=True), cup)


def test_clean_mask_diagonal_gap():
    m = _m(["000000",
            "011100",
            "010100",
            "011000",
            "000000"])
    # 8-connected foreground: the background is 4-connected, (2, 2) cannot leave through the diagonal gap
    want = m.clone()
    want[2, 2] = 1
    assert torch.equal(pr.clean_mask(m, fill_holes=True, connectivity=8), want)
    # 4-connected foreground: the background is 8-connected and leaks out through (3, 3)
    assert torch.equal(pr.clean_mask(m, fill_holes=True, connectivity=4), m)
    # two diagonal pixels: one object of 2 pixels under 8, two specks under 4
    d = _m(["1000", "0100", "0000", "0011"])
    assert torch.equal(pr.clean_mask(d, min_area=2, connectivity=8), d)
    assert torch.equal(pr.clean_mask(d, min_area=2, connectivity=4), _m(["0000", "0000", "0000", "0011"]))


def test_clean_mask_refusals():
    m = torch.zeros(4, 4)
    for kw in (dict(connectivity=6), dict(min_area=-1), dict(backend="gpu")):
        with pytest.raises(ValueError):
            pr.clean_mask(m, **kw)
    with pytest.raises(ValueError):
        pr.clean_mask(m, backend="device")      # a CPU tensor


# ---------------------------------------------------------------------------- Predictor, before any GPU work

def test_predictor_refusals():
    class Net(torch.nn.Module):
        pass
    for kw in (dict(tile=100), dict(overlap=300), dict(tile=64, overlap=40), dict(tta="rot90"), dict(batch_tiles=0)):
        with pytest.raises(ValueError):
            pr.Predictor(Net(), **kw)
    p = pr.Predictor(Net(), tile=512, overlap=64, tta="d4", max_workspace_bytes=1 << 20)
    with pytest.raises(_hip.HipError):
        p.predict_batch(torch.zeros(1, 1, 600, 600))     # a CPU tensor: no fallback


# ---------------------------------------------------------------------------- the CLI's refusals

@pytest.mark.parametrize("extra", [
    ["--tile", "100"], ["--tile", "8"], ["--tile", "4096"], ["--overlap", "300"], ["--overlap", "-1"],
    ["--tile", "64", "--overlap", "40"], ["--tta", "rot"], ["--threshold", "1.5"], ["--connectivity", "6"],
    ["--min-object-area", "-3"], ["--resize", "64"], ["--resize", "0", "64"], ["--bogus"],
])
def test_cli_refuses_bad_arguments(tmp_path, extra, capsys):
    import predict as cli
    model, img = tmp_path / "m.pth", tmp_path / "a.png"
    model.write_bytes(b"x")
    img.write_bytes(b"x")
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--model", str(model), "--input", str(img), "--output", str(tmp_path / "o")] + extra)
    assert e.value.code == 2
    assert "usage" in capsys.readouterr().err


def test_cli_refuses_missing_files(tmp_path):
    import predict as cli
    model, img = tmp_path / "m.pth", tmp_path / "a.png"
    model.write_bytes(b"x")
    img.write_bytes(b"x")
    (tmp_path / "empty").mkdir()
    out = str(tmp_path / "o")
    for argv in (["--model", str(tmp_path / "none.pth"), "--input", str(img), "--output", out],
                 ["--model", str(model), "--input", str(tmp_path / "none.png"), "--output", out],
                 ["--model", str(model), "--input", str(tmp_path / "empty"), "--output", out],
                 ["--model", str(model), "--input", str(img)]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
    args = cli.parse_args(["--model", str(model), "--input", str(tmp_path), "--output", out, "--resize", "64", "48"])
    assert args.files == [img] and args.resize == [64, 48] and args.tta == "none" and args.tile == 512


def test_eval_cli_accepts_tta():
    import evaluate as cli
    assert cli.parse_args(["--baseline", "a", "--pde", "b"]).tta is None
    assert cli.parse_args(["--baseline", "a", "--pde", "b", "--tta", "d4"]).tta == "d4"
    with pytest.raises(SystemExit):
        cli.parse_args(["--baseline", "a", "--pde", "b", "--tta", "none"])


# ---------------------------------------------------------------------------- the C-ABI, no compute call

def _count(H, W, th, tw, ov):
    ky, kx = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _hip.lib().pis_tile_count(H, W, th, tw, ov, ctypes.byref(ky), ctypes.byref(kx))
    return rc, ky.value, kx.value


def test_tile_count_is_the_plan():
    for H, W, th, tw, ov in ((40, 56, 16, 16, 0), (40, 56, 16, 16, 8), (40, 56, 32, 32, 16), (40, 56, 16, 32, 8),
                             (5, 7, 16, 16, 8), (1, 1, 16, 16, 0), (17, 16, 16, 16, 8), (2048, 2048, 512, 512, 64),
                             (32768, 32768, 2048, 2048, 256), (32768, 1, 16, 16, 0)):
        assert _count(H, W, th, tw, ov) == (0, pr.tile_count(H, th, ov), pr.tile_count(W, tw, ov))
    assert _count(2048, 2048, 512, 512, 64) == (0, 5, 5)


FAKE_SRC, FAKE_OUT = 1 << 20, 2 << 20      # aligned, never dereferenced: every call below is refused


def _gather_rc(H=40, W=56, th=16, tw=16, ov=8, sym=0x01, first=0, n=1, S=2, fmt=_hip.PIS_CACHE_IMG_F32, stride=None,
               src=FAKE_SRC, out=FAKE_OUT, norm=0):
    stride = (H * W * 4 + 15) // 16 * 16 if stride is None else stride
    return _hip.lib().pis_tile_gather(src, fmt, stride, norm, S, H, W, th, tw, ov, sym, first, n, out, 0)


def _blend_rc(H=40, W=56, th=16, tw=16, ov=8, sym=0x01, S=2, u=FAKE_SRC, prob=FAKE_OUT, mask=0):
    return _hip.lib().pis_tile_blend(u, S, H, W, th, tw, ov, sym, ctypes.c_float(0.5), prob, mask, 0)


@pytest.mark.parametrize("kw, word", [
    (dict(th=24, tw=24), b"multiples of 16"),     # a tile not a multiple of 16
    (dict(th=16, tw=8), b"multiples of 16"),
    (dict(th=4096, tw=4096), b"multiples of 16"),
    (dict(ov=9), b"overlap"),                     # ov > t / 2
    (dict(th=32, tw=16, ov=12), b"overlap"),      # ... of the smaller side
    (dict(ov=-1), b"overlap"),
    (dict(th=1024, tw=1024, ov=257), b"overlap"),  # ov > 256
    (dict(th=16, tw=32, sym=0x10), b"th == tw"),  # a code >= 4 with th != tw
    (dict(th=16, tw=32, sym=0xFF), b"th == tw"),
    (dict(sym=0), b"sym_mask"),                   # an empty set
    (dict(sym=0x100), b"sym_mask"),
    (dict(H=0), b"32768"),
    (dict(W=32769), b"32768"),
    (dict(S=0), b"sources"),
])
def test_tile_geometry_errors(kw, word):
    lib = _hip.lib()
    assert _gather_rc(**kw) == -1
    assert b"pis_tile_gather" in lib.pis_last_error() and word in lib.pis_last_error()
    assert _blend_rc(**kw) == -1
    assert b"pis_tile_blend" in lib.pis_last_error() and word in lib.pis_last_error()
    if "sym" not in kw and "S" not in kw:
        g = dict(H=40, W=56, th=16, tw=16, ov=8)
        g.update(kw)
        assert _count(**g)[0] == -1 and b"pis_tile_count" in lib.pis_last_error()


def test_tile_chunk_and_pointer_errors():
    lib = _hip.lib()
    J = 2 * 4 * 6 * 4          # two sources, 4 x 6 tiles of 16 x 16 with overlap 8 on 40 x 56, 4 codes
    assert pr.tile_plan(40, 56, (16, 16), 8, 0x0F).jobs(2) == J
    for first, n in ((J, 1), (-1, 1), (0, 0), (0, -1), (J - 1, 2), (0, J + 1), (1 << 62, 1 << 62)):
        assert _gather_rc(sym=0x0F, first=first, n=n) == -1
        assert b"not within [0, 192)" in lib.pis_last_error()
    for kw, word in ((dict(src=0), b"NULL"), (dict(out=0), b"NULL"), (dict(src=FAKE_SRC + 4), b"aligned"),
                     (dict(out=FAKE_OUT + 8), b"aligned"), (dict(stride=40 * 56 * 4 - 16), b"stride"),
                     (dict(stride=40 * 56 * 4 + 4), b"stride"), (dict(fmt=2), b"format"),
                     (dict(fmt=_hip.PIS_CACHE_IMG_U8, stride=40 * 56), b"norm")):
        assert _gather_rc(**kw) == -1
        assert word in lib.pis_last_error(), (kw, lib.pis_last_error())
    for kw, word in ((dict(u=0), b"NULL"), (dict(prob=0), b"NULL"), (dict(u=FAKE_SRC + 4), b"aligned"),
                     (dict(mask=FAKE_OUT + 2), b"aligned")):
        assert _blend_rc(**kw) == -1
        assert word in lib.pis_last_error(), (kw, lib.pis_last_error())
    assert lib.pis_tile_count(40, 56, 16, 16, 8, None, None) == -1
