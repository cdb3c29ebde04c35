"""Edge cases of the bandwidth-bound kernels of every training step: 2x2 max pooling, the 1x1
head, decoupled AdamW (csrc/pointwise.hip), pis_colsum and the slab reductions behind every
weight and bias gradient (csrc/wgrad.hip: reduce_slabs_kernel, the merged reduce_slabs2_kernel
and the chunked two-pass reduce_rows_chunk_kernel, pis_tune key 20).

The sum kernels run on small integers and dyadic fractions: every product and every partial sum
is then exact in fp32 in any order (the tests assert that the sum of the terms' magnitudes, in
units of the data's finest bit, stays below 2^24), the reference is int64 / float64 numpy and
the comparison is torch.equal: a dropped, doubled or misrouted row shows as a wrong integer.
One random-normal case per kernel keeps the ordinary rel_err check. Padding channels (ld > C)
hold a large sentinel that must reach no sum and must not be overwritten.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_small_kernels_host import (ADAMW_CONFIGS, ADAMW_MARGIN, ADAMW_N, BETA1, BETA2, adamw_ratios,
                                     adamw_reference, adamw_scalars)

pytestmark = pytest.mark.gpu

ACC = 8            # PIS_ACCUMULATE
KEY_CHUNKS = 20    # PIS_TUNE_SLAB_CHUNKS
SENT = 3.0e7       # sentinel of padding channels and guard elements
EXACT = 1 << 24


def s():
    return torch.cuda.current_stream().cuda_stream


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def padded(a, ld):
    """[rows][ld] device buffer holding a in its first columns, the sentinel in the rest."""
    buf = np.full((a.shape[0], ld), SENT, np.float32)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()


class tuned:
    """pis_tune(key, value) for the block, the previous value back afterwards (None: leave it)."""

    def __init__(self, hip, key, value):
        self.hip, self.key, self.value = hip, key, value

    def __enter__(self):
        self.prev = None if self.value is None else self.hip.pis_tune(self.key, self.value)

    def __exit__(self, *exc):
        if self.prev is not None:
            self.hip.pis_tune(self.key, self.prev)


# ---------------------------------------------------------------------------------------------
# pis_colsum
# ---------------------------------------------------------------------------------------------
def colsum_slabs(hip, npix, C):
    return hip.pis_colsum_ws(npix, C) // (4 * C)


def run_colsum(hip, src_d, ld, npix, C, out0, flags, out_off=4):
    """out lives out_off floats into a sentinel-filled buffer; returns the C sums after checking
    that nothing around them was written."""
    buf = torch.full((C + 12,), SENT, device="cuda")
    out = buf[out_off:out_off + C]
    out.copy_(torch.from_numpy(out0))
    nws = hip.pis_colsum_ws(npix, C)
    ws = torch.empty(nws // 4 + 4, device="cuda")
    rc = hip.pis_colsum(src_d.data_ptr(), ld, npix, C, out.data_ptr(), flags, ws.data_ptr(), nws, s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    assert torch.all(buf[:out_off] == SENT) and torch.all(buf[out_off + C:] == SENT)
    return out.cpu()


def colsum_case(npix, C, ld, seed=0):
    rng = np.random.default_rng(1000 + seed + npix + 7 * C)
    src = ints(rng, (npix, C), -4, 4)
    out0 = ints(rng, (C,), -4, 4)
    assert np.abs(src.astype(np.int64)).sum(0).max() + 4 < EXACT
    col = src.astype(np.int64).sum(0)
    return src, out0, col


COLSUM_CASES = [
    (1, 64, 64, None), (1, 1, 1, None),                         # the two calls of the training step
    (63, 4, 4, None), (64, 4, 4, None), (65, 4, 4, None),       # the 64-pixel split boundary
    (1000, 12, 16, None), (1000, 48, 48, None),                 # lane groups that leave idle lanes
    (777, 1024, 1024, None),                                    # one row per block
    (300, 1028, 1028, None),                                    # scalar kernel, float4 reduction
    (500, 3, 5, None), (500, 7, 7, None),                       # scalar throughout
    (65537, 4, 4, None),                                        # 1009 slabs: single pass
    (40000, 16, 16, None),                                      # 625 slabs over 64 groups: the 8-deep loop
    (65536, 4, 4, 1), (65536, 4, 4, 0),                         # 1024 slabs: chunked two-pass (key 20 = 1)
    (65536, 64, 128, 1), (65536, 64, 128, 0),                   # and the single pass with 256 slab groups
    (66560, 8, 8, 1), (66560, 8, 8, 0),
    # 16 slabs per chunk over 5 rows of 51 float4 lanes (one lane idle): row 0 runs the four-chain
    # loop, rows 1..4 the three tail loads. The narrower cases above have more rows than slabs per
    # chunk and never leave the first chain.
    (65536, 204, 208, 1), (65536, 204, 208, 0),
]


@pytest.mark.parametrize("flags", [0, ACC])
@pytest.mark.parametrize("npix,C,ld,chunks", COLSUM_CASES)
def test_colsum_exact(hip, npix, C, ld, chunks, flags):
    src, out0, col = colsum_case(npix, C, ld)
    if chunks is not None:
        assert colsum_slabs(hip, npix, C) >= 1024 and C <= 1024  # the regime key 20 switches
    elif npix == 65537:
        assert colsum_slabs(hip, npix, C) == 1009
    ref = torch.from_numpy((col + (out0.astype(np.int64) if flags else 0)).astype(np.float32))
    with tuned(hip, KEY_CHUNKS, chunks):
        out = run_colsum(hip, padded(src, ld), ld, npix, C, out0, flags)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("flags", [0, ACC])
@pytest.mark.parametrize("npix,C,ld", [(1000, 12, 16), (65536, 64, 128), (66560, 8, 8)])
def test_colsum_unaligned_out(hip, npix, C, ld, flags):
    """out one float past a 16-byte boundary: the slab sum takes its scalar columns (and, with
    1024 slabs, never the chunked form, whose second pass is float4)."""
    src, out0, col = colsum_case(npix, C, ld, seed=1)
    ref = torch.from_numpy((col + (out0.astype(np.int64) if flags else 0)).astype(np.float32))
    out = run_colsum(hip, padded(src, ld), ld, npix, C, out0, flags, out_off=5)
    assert torch.equal(out, ref)


def test_colsum_random(hip):
    npix, C, ld = 1000, 48, 64
    src = np.random.default_rng(3).standard_normal((npix, C)).astype(np.float32)
    out = run_colsum(hip, padded(src, ld), ld, npix, C, np.zeros(C, np.float32), 0)
    assert rel_err(out, src.astype(np.float64).sum(0)) < 1e-5


# ---------------------------------------------------------------------------------------------
# pis_head_bwd
# ---------------------------------------------------------------------------------------------
def head_bwd_case(npix, C, seed=0):
    rng = np.random.default_rng(2000 + seed + npix + 13 * C)
    x = ints(rng, (npix, C), 0, 4)
    w = ints(rng, (C,), -4, 4)
    g = ints(rng, (npix,), -4, 4)
    u = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=npix)
    return x, w, g, u, ints(rng, (C,), -4, 4), ints(rng, (1,), -4, 4)


def head_bwd_ref(x, w, g, u):
    """float64, exact on this data: d is a multiple of 1/16 (g u (1 - u)) or an integer (u NULL)."""
    d = g.astype(np.float64)
    unit = 1.0
    if u is not None:
        d = d * (1.0 - u.astype(np.float64)) * u.astype(np.float64)
        unit = 1.0 / 16
    terms = np.abs(d)[:, None] * x.astype(np.float64)
    assert max(terms.sum(0).max(), np.abs(d).sum()) / unit + 4 / unit < EXACT
    dx = (d[:, None] * w.astype(np.float64)[None, :]) * (x > 0)
    dw = (d[:, None] * x.astype(np.float64)).sum(0)
    return dx.astype(np.float32), dw, np.array([d.sum()])


def run_head_bwd(hip, xd, wd, gd, ud, ld, npix, C, dw0, db0, flags, with_db=True):
    dxb = torch.full((npix, ld), SENT, device="cuda")
    dwb = torch.full((C + 8,), SENT, device="cuda")
    dbb = torch.full((8,), SENT, device="cuda")
    dw, db = dwb[4:4 + C], dbb[4:5]
    dw.copy_(torch.from_numpy(dw0))
    db.copy_(torch.from_numpy(db0))
    nws = hip.pis_head_bwd_ws(npix, C)
    ws = torch.empty(nws // 4 + 4, device="cuda")
    rc = hip.pis_head_bwd(xd.data_ptr(), ld, wd.data_ptr(), gd.data_ptr(), 0 if ud is None else ud.data_ptr(),
                          dxb.data_ptr(), ld, dw.data_ptr(), db.data_ptr() if with_db else 0, npix, C, flags,
                          ws.data_ptr(), nws, s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    assert torch.all(dxb[:, C:] == SENT)  # padding channels of dx are not written
    assert torch.all(dwb[:4] == SENT) and torch.all(dwb[4 + C:] == SENT)
    assert torch.all(dbb[:4] == SENT) and torch.all(dbb[5:] == SENT)
    return dxb[:, :C], dw, db


HEAD_BWD_GRID = [(n, C) for C in (4, 12, 48, 64, 1024) for n in (1, 255, 256, 257, 4099) if C < 1024 or n <= 257]


@pytest.mark.parametrize("npix,C", HEAD_BWD_GRID)
def test_head_bwd_exact(hip, npix, C):
    x, w, g, u, dw0, db0 = head_bwd_case(npix, C)
    ld = C + 64
    xd, wd, gd, ud = padded(x, ld), torch.from_numpy(w).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(u).cuda()
    for uu, ud_ in ((None, None), (u, ud)):
        dx_ref, dw_ref, db_ref = head_bwd_ref(x, w, g, uu)
        for flags in (0, ACC):
            dx, dw, db = run_head_bwd(hip, xd, wd, gd, ud_, ld, npix, C, dw0, db0, flags)
            what = f"u {'given' if uu is not None else 'NULL'}, flags {flags}"
            assert torch.equal(dx.cpu(), torch.from_numpy(dx_ref)), what
            assert torch.equal(dw.cpu(), torch.from_numpy((dw_ref + (dw0 if flags else 0)).astype(np.float32))), what
            assert torch.equal(db.cpu(), torch.from_numpy((db_ref + (db0 if flags else 0)).astype(np.float32))), what


@pytest.mark.parametrize("npix,blocks", [(262144, 1024), (300000, 1172), (524293, 2041)])
def test_head_bwd_many_slabs_exact(hip, npix, blocks):
    """1024..2048 partial slabs of C = 8: without db the weights-only slab sum (chunked two-pass
    with key 20 = 1, one column per block with key 20 = 0), with db the merged launch over 256 slab
    groups. The rows are C + 8 floats apart here, not C + 64, to keep the buffers at 32 MB."""
    C = 8
    ld = C + 8
    assert hip.pis_head_bwd_ws(npix, C) == blocks * (C + 1) * 4 + 256
    x, w, g, _, dw0, db0 = head_bwd_case(npix, C)
    dx_ref, dw_ref, db_ref = head_bwd_ref(x, w, g, None)
    xd, wd, gd = padded(x, ld), torch.from_numpy(w).cuda(), torch.from_numpy(g).cuda()
    dx_ref_d = torch.from_numpy(dx_ref).cuda()
    for with_db, chunks in ((False, 1), (False, 0), (True, None)):
        for flags in (0, ACC):
            with tuned(hip, KEY_CHUNKS, chunks):
                dx, dw, db = run_head_bwd(hip, xd, wd, gd, None, ld, npix, C, dw0, db0, flags, with_db)
            what = f"db {'given' if with_db else 'NULL'}, key 20 = {chunks}, flags {flags}"
            assert torch.equal(dx, dx_ref_d), what
            assert torch.equal(dw.cpu(), torch.from_numpy((dw_ref + (dw0 if flags else 0)).astype(np.float32))), what
            if with_db:
                assert torch.equal(db.cpu(), torch.from_numpy((db_ref + (db0 if flags else 0)).astype(np.float32))), what
            else:
                assert torch.equal(db.cpu(), torch.from_numpy(db0)), what  # not touched


def test_head_bwd_random(hip):
    npix, C = 4099, 48
    ld = C + 64
    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal((npix, C)), 0).astype(np.float32)
    w, g = rng.standard_normal(C).astype(np.float32), rng.standard_normal(npix).astype(np.float32)
    u = rng.random(npix).astype(np.float32)
    d = g.astype(np.float64) * u.astype(np.float64) * (1.0 - u.astype(np.float64))
    zero = np.zeros(C, np.float32)
    dx, dw, db = run_head_bwd(hip, padded(x, ld), torch.from_numpy(w).cuda(), torch.from_numpy(g).cuda(),
                              torch.from_numpy(u).cuda(), ld, npix, C, zero, zero[:1], 0)
    assert rel_err(dx, (d[:, None] * w.astype(np.float64)[None, :]) * (x > 0)) < 1e-5
    assert rel_err(dw, (d[:, None] * x.astype(np.float64)).sum(0)) < 1e-5
    assert rel_err(db, np.array([d.sum()])) < 1e-5


# ---------------------------------------------------------------------------------------------
# pis_head_fwd
# ---------------------------------------------------------------------------------------------
def run_head_fwd(hip, xd, ld, wd, bd, npix, C, with_z=True):
    zb = torch.full((npix + 8,), SENT, device="cuda")
    ub = torch.full((npix + 8,), SENT, device="cuda")
    rc = hip.pis_head_fwd(xd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), zb[4:].data_ptr() if with_z else 0,
                          ub[4:].data_ptr(), npix, C, s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    for b in (zb, ub):
        assert torch.all(b[:4] == SENT) and torch.all(b[4 + npix:] == SENT)
    if not with_z:
        assert torch.all(zb == SENT)
    return zb[4:4 + npix].cpu(), ub[4:4 + npix].cpu()


@pytest.mark.parametrize("C", [4, 64, 68, 128])
@pytest.mark.parametrize("npix", [3, 4, 5, 4097])
def test_head_fwd_exact(hip, npix, C):
    """Dyadic data: z is the float64 sum bit for bit; u = sigmoid(z) within the project's 1e-6; with
    z = NULL the same u. C = 64 is the 4-pixels-per-group kernel, the others the generic one (68: a
    second trip of the channel loop for one lane of 16)."""
    rng = np.random.default_rng(3000 + npix + C)
    x = ints(rng, (npix, C), -4, 4)
    w = ints(rng, (C,), -4, 4) / np.float32(4)
    b = np.array([0.375], np.float32)
    assert (np.abs(x.astype(np.float64)) * np.abs(w.astype(np.float64))).sum(1).max() * 8 + 8 < EXACT
    z_ref = x.astype(np.float64) @ w.astype(np.float64) + 0.375
    u_ref = 1.0 / (1.0 + np.exp(-z_ref))
    ld = C + 64
    xd, wd, bd = padded(x, ld), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    z, u = run_head_fwd(hip, xd, ld, wd, bd, npix, C)
    assert torch.equal(z, torch.from_numpy(z_ref.astype(np.float32)))
    assert rel_err(u, u_ref) < 1e-6
    _, u2 = run_head_fwd(hip, xd, ld, wd, bd, npix, C, with_z=False)
    assert torch.equal(u2, u)


def test_head_fwd_random(hip):
    npix, C = 4097, 68
    ld = C + 64
    rng = np.random.default_rng(6)
    x = rng.standard_normal((npix, C)).astype(np.float32)
    w = (rng.standard_normal(C) / C ** 0.5).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32)
    z_ref = x.astype(np.float64) @ w.astype(np.float64) + float(b[0])
    z, u = run_head_fwd(hip, padded(x, ld), ld, torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), npix, C)
    assert rel_err(z, z_ref) < 1e-5
    assert rel_err(u, 1.0 / (1.0 + np.exp(-z_ref))) < 1e-6


# ---------------------------------------------------------------------------------------------
# pis_maxpool2x2_fwd / _bwd
# ---------------------------------------------------------------------------------------------
def pool_input(B, H, W, C, rng):
    """(B, C, H, W): values from a five-element set, so ties, zeros and negatives are everywhere; the
    first window of the first image holds, channel by channel, the 15 non-empty subsets of its four
    positions at the maximum, then an all-zero, an all-negative and a mixed -0.0 / +0.0 window."""
    x = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32), size=(B, C, H, W))
    pos = [(0, 0), (0, 1), (1, 0), (1, 1)]
    kinds = set()
    for c in range(C):
        k = c % 18
        kinds.add(k)
        for i, (r, q) in enumerate(pos):
            if k < 15:  # subset k + 1 (bit i = position i) holds the maximum 2, the rest 1 or -1
                x[0, c, r, q] = 2.0 if (k + 1) >> i & 1 else (1.0 if (c // 18) % 2 == 0 else -1.0)
            elif k == 15:
                x[0, c, r, q] = 0.0
            elif k == 16:
                x[0, c, r, q] = -1.0 if i % 2 else -0.5
            else:
                x[0, c, r, q] = -0.0 if i in (0, 3) else 0.0
    return x, kinds


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (2, 2, 6, 12), (1, 6, 2, 64), (1, 4, 4, 260)])
def test_maxpool_exact(hip, B, H, W, C, with_skip):
    rng = np.random.default_rng(4000 + C)
    xn, kinds = pool_input(B, H, W, C, rng)
    assert len(kinds) == min(C, 18)
    x = torch.from_numpy(xn).requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    dy = torch.from_numpy(ints(rng, tuple(y.shape), -4, 4) / np.float32(4))
    y.backward(dy)
    dskip = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
    ref = (x.grad + dskip if with_skip else x.grad) * (x.detach() > 0)
    if C >= 15:  # the gradient of a tied window goes to its first position in row-major order
        for k in range(15):
            first = [i for i in range(4) if (k + 1) >> i & 1][0]
            got = x.grad[0, k, :2, :2].reshape(4)
            assert got[first] == dy[0, k, 0, 0] and got.abs().sum() == dy[0, k, 0, 0].abs()

    def rows(t):  # (B, C, H, W) -> [B*H*W][C]
        return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()

    ldx, lddx, ldskip = C + 4, C + 8, C + 12
    xd = padded(rows(x), ldx)
    yb = torch.full((B * (H // 2) * (W // 2) * C + 8,), SENT, device="cuda")
    yd = yb[4:4 + B * (H // 2) * (W // 2) * C]
    rc = hip.pis_maxpool2x2_fwd(xd.data_ptr(), ldx, yd.data_ptr(), B, H, W, C, s())
    assert rc == 0, hip.pis_last_error()
    dyd = torch.from_numpy(rows(dy).copy()).cuda()
    skd = padded(rows(dskip), ldskip) if with_skip else None
    dxb = torch.full((B * H * W, lddx), SENT, device="cuda")
    rc = hip.pis_maxpool2x2_bwd(xd.data_ptr(), ldx, dyd.data_ptr(), 0 if skd is None else skd.data_ptr(),
                                ldskip if with_skip else 0, dxb.data_ptr(), lddx, B, H, W, C, s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    assert torch.all(yb[:4] == SENT) and torch.all(yb[-4:] == SENT)
    assert torch.all(dxb[:, C:] == SENT)
    assert torch.equal(yd.cpu().reshape(-1, C), torch.from_numpy(rows(y).copy()))
    assert torch.equal(dxb[:, :C].cpu(), torch.from_numpy(rows(ref).copy()))


def test_maxpool_random(hip):
    B, H, W, C = 2, 6, 10, 12
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    dy = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    y.backward(dy)
    dskip = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
    ref = (x.grad.double() + dskip.double()) * (x.detach() > 0)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    xd, dyd, skd = nhwc(x).cuda(), nhwc(dy).cuda(), nhwc(dskip).cuda()
    yd = torch.empty(B, H // 2, W // 2, C, device="cuda")
    dx = torch.empty(B, H, W, C, device="cuda")
    assert hip.pis_maxpool2x2_fwd(xd.data_ptr(), C, yd.data_ptr(), B, H, W, C, s()) == 0
    assert hip.pis_maxpool2x2_bwd(xd.data_ptr(), C, dyd.data_ptr(), skd.data_ptr(), C, dx.data_ptr(), C, B, H, W, C,
                                  s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), nhwc(y))
    assert rel_err(dx, nhwc(ref)) < 1e-5


# ---------------------------------------------------------------------------------------------
# pis_adamw_step
# ---------------------------------------------------------------------------------------------
GUARD = 8


def run_adamw(hip, cfg, inputs, n):
    """The kernel on the first n elements of the inputs; [(p, m, v)] after every step (numpy). The
    GUARD elements behind each buffer must keep their sentinel."""
    p0, m0, v0, grads = inputs

    def dev(a):
        t = torch.full((n + GUARD,), SENT, device="cuda")
        t[:n].copy_(torch.tensor(a[:n]))  # a copy: the shared inputs are read-only
        return t

    p, m, v = dev(p0), dev(m0), dev(v0)
    out = []
    for i, g in enumerate(grads):
        gd = dev(g)
        step_size, bc2_sqrt = adamw_scalars(cfg, cfg["first_step"] + i)
        rc = hip.pis_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, cfg["lr"], BETA1, BETA2,
                                cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"], s())
        assert rc == 0, hip.pis_last_error()
        torch.cuda.synchronize()
        for t in (p, m, v, gd):
            assert torch.all(t[n:] == SENT)
        out.append(tuple(t[:n].cpu().numpy() for t in (p, m, v)))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, ADAMW_N])
@pytest.mark.parametrize("name", ["existing", "scaled", "all_terms", "late"])
def test_adamw_against_float64(hip, name, n):
    """p, m and v after every step against the float64 formula of include/pis_capi.h. The bound is
    measured, not chosen: 4 x the max-abs error of torch.optim.AdamW in fp32 on the CPU on the same
    gradients (pre-multiplied by grad_scale). The sizes below 1003 run the first n elements of the
    same data (float4 body, scalar tail and both) against the same per-configuration bound: the
    error of a handful of elements is no yardstick of its own."""
    cfg = ADAMW_CONFIGS[name]
    inputs, ref, terr = adamw_reference(name)
    ratios = adamw_ratios(run_adamw(hip, cfg, inputs, n), ref, terr, n=n)
    print(f"adamw kernel / torch error, {name}, n = {n}: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN


def test_adamw_grid_stride_and_tail(hip):
    """More float4 items than the capped grid has threads (8192 blocks x 256), plus three scalar tail
    elements: every element still gets exactly one update."""
    n = 8192 * 256 * 4 + 4099
    cfg = ADAMW_CONFIGS["one_step"]
    inputs, ref, terr = adamw_reference("one_step", n)
    ratios = adamw_ratios(run_adamw(hip, cfg, inputs, n), ref, terr)
    print(f"adamw kernel / torch error, one_step, n = {n}: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN


def test_adamw_of_nothing_touches_nothing(hip):
    bufs = [torch.full((8,), SENT, device="cuda") for _ in range(4)]
    rc = hip.pis_adamw_step(*[b.data_ptr() for b in bufs], 0, 1e-3, BETA1, BETA2, 1e-8, 1e-2, 1e-3, 1.0, 1.0, s())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(torch.all(b == SENT) for b in bufs)


# ---- through optim.AdamW: parameters and gradients as views of flat arenas
ARENA_LAYOUT = [(0, (5,)), (8, (3, 4)), (20, (1,)), (24, (251,))]  # offsets multiples of 4 floats, with gaps
ARENA_N = 24 + 251


def make_arena(p0):
    arena = torch.from_numpy(p0.copy()).cuda()
    params = [torch.nn.Parameter(arena[o:o + int(np.prod(shape))].view(shape)) for o, shape in ARENA_LAYOUT]
    return arena, params


def arena_grads(params, g, flat):
    """.grad of every parameter from the flat gradient g: views of one gradient arena (the single
    flat launch) or fresh tensors (the per-tensor launches)."""
    garena = torch.from_numpy(g.copy()).cuda()
    for p, (o, shape) in zip(params, ARENA_LAYOUT):
        view = garena[o:o + p.numel()].view(shape)
        p.grad = view if flat else view.clone()


def optim_inputs():
    cfg = ADAMW_CONFIGS["optim"]
    inputs, ref, terr = adamw_reference("optim", ARENA_N)
    p0, m0, v0, grads = inputs
    live = np.zeros(ARENA_N, bool)
    for o, shape in ARENA_LAYOUT:
        live[o:o + int(np.prod(shape))] = True
    assert not live.all()
    return cfg, (p0, grads), ref, terr, live


def test_optim_adamw_grad_scale(hip):
    """optim.AdamW(grad_scale = 1/4) over an arena against the float64 formula, within 4 x the error of
    torch fed 0.25 * grad; m and v through the optimizer's state."""
    from physics_informed_image_segmentation_amd import AdamW
    cfg, (p0, grads), ref, terr, live = optim_inputs()
    arena, params = make_arena(p0)
    opt = AdamW(params, lr=cfg["lr"], eps=cfg["eps"], weight_decay=cfg["wd"], grad_scale=cfg["grad_scale"])
    states = []
    for g in grads:
        arena_grads(params, g, flat=True)
        opt.step()
        torch.cuda.synchronize()
        m, v = np.zeros(ARENA_N, np.float32), np.zeros(ARENA_N, np.float32)
        for p, (o, shape) in zip(params, ARENA_LAYOUT):
            assert opt.state[p]["exp_avg"].shape == p.shape
            m[o:o + p.numel()] = opt.state[p]["exp_avg"].reshape(-1).cpu().numpy()
            v[o:o + p.numel()] = opt.state[p]["exp_avg_sq"].reshape(-1).cpu().numpy()
        states.append(tuple(a[live] for a in (arena.cpu().numpy(), m, v)))
    ref_live = [tuple(a[live] for a in r) for r in ref]
    ratios = adamw_ratios(states, ref_live, terr)
    print(f"optim.AdamW / torch error: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN


def test_optim_adamw_per_tensor_equals_flat(hip):
    """Gradients assigned as fresh tensors take one launch per parameter (each with its own float4
    body and scalar tail): bitwise the single launch over the arenas."""
    from physics_informed_image_segmentation_amd import AdamW
    cfg, (p0, grads), _, _, live = optim_inputs()
    runs = []
    for flat in (True, False):
        arena, params = make_arena(p0)
        opt = AdamW(params, lr=cfg["lr"], eps=cfg["eps"], weight_decay=cfg["wd"], grad_scale=cfg["grad_scale"])
        for g in grads:
            arena_grads(params, g, flat)
            opt.step()
        torch.cuda.synchronize()
        st = opt._flat[0]
        runs.append([t.cpu()[torch.from_numpy(live)] for t in (arena, st["m"], st["v"])])
        if not flat:  # the gaps between the parameters belong to nobody
            assert torch.equal(arena.cpu()[torch.from_numpy(~live)], torch.from_numpy(p0[~live]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], torch.from_numpy(p0[live]))


def test_optim_adamw_skips_param_without_grad(hip):
    """A parameter whose .grad is None keeps p, m and v bit for bit while the others step exactly as
    they do when every parameter has a gradient."""
    from physics_informed_image_segmentation_amd import AdamW
    cfg, (p0, grads), _, _, _ = optim_inputs()
    runs = []
    for drop in (None, 1):
        arena, params = make_arena(p0)
        opt = AdamW(params, lr=cfg["lr"], eps=cfg["eps"], weight_decay=cfg["wd"], grad_scale=cfg["grad_scale"])
        arena_grads(params, grads[0], flat=False)
        opt.step()
        torch.cuda.synchronize()
        before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                  for p in params]
        arena_grads(params, grads[1], flat=False)
        if drop is not None:
            params[drop].grad = None
        opt.step()
        torch.cuda.synchronize()
        after = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                 for p in params]
        runs.append((before, after))
    (_, full), (before, after) = runs
    for i in range(len(ARENA_LAYOUT)):
        want = before[1] if i == 1 else full[i]
        for a, b in zip(after[i], want):
            assert torch.equal(a, b), i
        if i != 1:
            assert not torch.equal(after[i][0], before[i][0])
    assert all(a.abs().sum() > 0 for a in before[1][1:])  # its moments were live
