"""Global-norm gradient clipping and the non-finite step guard on the GPU (csrc/gradnorm.hip,
optim.AdamW(max_grad_norm=, skip_nonfinite=)), against the float64 definition of
tests/test_gradnorm_host.py (itself pinned to torch.nn.utils.clip_grad_norm_).

Bounds. The square of an fp32 value is exact in float64, so a segment's sum of squares is a plain
sum of n exact non-negative terms: any summation order is within (n - 1) 2^-53 relative of the
true sum. The tests allow n 2^-53 per segment and N 2^-53 (N the element count) for the total norm,
against math.fsum (correctly rounded). The gaps between the segments and a guard region behind the
arena hold NaN or 1e30: one element read from them fails every comparison.
"""
import gc
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from test_gradnorm_host import (ARENA_SEGS, CLIP_CFG, CLIPPED, FINITE, LAST_COEF, LAST_NORM, NORM_MAX, NORM_SUM,
                                NSTATS, SKIPPED, SLICE, STEPS, U64, gradnorm_reference, seg_sumsq_float64)
from test_gradnorm_host import clip_yardstick as yardstick
from test_small_kernels_host import ADAMW_MARGIN, BETA1, BETA2, adamw_inputs, adamw_ratios, adamw_scalars

pytestmark = pytest.mark.gpu

GUARD = 64          # floats behind the arena, poisoned
SENT = 3.0e7        # sentinel behind the AdamW buffers
WS_GUARD = 64       # bytes behind the workspace
SKIP = 1            # PIS_GRADNORM_SKIP_NONFINITE


def s():
    return torch.cuda.current_stream().cuda_stream


def layout(lengths, gap=4):
    """(offset, length) per segment: offsets multiples of 4 floats, at least `gap` floats of padding
    between a segment's end and the next one's start."""
    segs, off = [], 0
    for n in lengths:
        segs.append((off, n))
        off = (off + n + gap + 3) // 4 * 4
    return segs


def _lens_1_to_7(count, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, 8, size=count)]


ARENAS = {
    "arena_layout": ARENA_SEGS,                                  # offsets 0, 8, 20, 24; lengths 5, 12, 1, 251
    "small_lengths": layout([1, 2, 3, 4, 5, 7, 8, 4099]),
    "multi_slice": layout([SLICE + 3, 3 * SLICE + 1]),           # one slice + 3 and three slices + 1
    "300_segments": layout(_lens_1_to_7(300, 1)),
    "single": [(0, 1003)],
    "1100_segments": layout(_lens_1_to_7(1100, 2)),              # a second chunk of the finalize's segment loop
}


def span(segs):
    return max(o + n for o, n in segs)


def live_mask(segs, total):
    live = np.zeros(total, bool)
    for o, n in segs:
        assert not live[o:o + n].any() and o % 4 == 0
        live[o:o + n] = True
    return live


def make_arena(segs, poison, seed=0, values=None):
    """fp32 arena (numpy) of span(segs) + GUARD floats: standard-normal (or `values(rng, n)`) inside
    the segments, `poison` everywhere else."""
    total = span(segs) + GUARD
    rng = np.random.default_rng(seed)
    g = np.full(total, poison, np.float32)
    for o, n in segs:
        g[o:o + n] = rng.standard_normal(n).astype(np.float32) if values is None else values(rng, n)
    return g


class Norm:
    """One set of device buffers for pis_grad_sumsq: table, segment sums, record, statistics and a
    workspace with a guard behind it."""

    def __init__(self, hip, segs, ws_extra=0):
        self.hip, self.segs = hip, segs
        self.off = torch.tensor([o for o, _ in segs], dtype=torch.int64, device="cuda")
        self.len = torch.tensor([n for _, n in segs], dtype=torch.int64, device="cuda")
        self.sumsq = torch.full((len(segs) + 2,), -7.0, dtype=torch.float64, device="cuda")
        self.record = torch.zeros(2, dtype=torch.float64, device="cuda")
        self.stats = torch.zeros(NSTATS, dtype=torch.float64, device="cuda")
        self.ws_bytes = hip.pis_grad_sumsq_ws(len(segs), sum(n for _, n in segs)) + ws_extra
        assert self.ws_bytes >= 8
        self.ws = torch.full((self.ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def run(self, g, grad_scale=1.0, max_norm=0.0, flags=0):
        rc = self.hip.pis_grad_sumsq(g.data_ptr(), self.off.data_ptr(), self.len.data_ptr(), len(self.segs),
                                     grad_scale, max_norm, flags, self.sumsq.data_ptr(), self.record.data_ptr(),
                                     self.stats.data_ptr(), self.ws.data_ptr(), self.ws_bytes, s())
        assert rc == 0, self.hip.pis_last_error()
        torch.cuda.synchronize()
        assert torch.all(self.sumsq[len(self.segs):] == -7.0)
        assert torch.all(self.ws[self.ws_bytes:] == 0xA5)
        return dict(sumsq=self.sumsq[:len(self.segs)].cpu().numpy().copy(),
                    coef=self.record[:1].view(torch.float32)[0].cpu().numpy().copy(),
                    apply=int(self.record[:1].view(torch.int32)[1].item()),
                    norm=float(self.record[1].item()), stats=self.stats.cpu().numpy().copy())


def check_sums(out, g_host, segs, grad_scale=1.0):
    """seg_sumsq within length 2^-53 and the norm within N 2^-53, relative, of the float64 truth."""
    want = seg_sumsq_float64(g_host, segs)
    for (o, n), got, w in zip(segs, out["sumsq"], want):
        assert abs(got - w) <= n * U64 * w, (o, n, got, w)
    N = sum(n for _, n in segs)
    norm = math.sqrt(math.fsum(want)) * grad_scale
    assert abs(out["norm"] - norm) <= N * U64 * norm, (out["norm"], norm)
    return norm


def bits(t):
    return t.view(torch.int32).clone()


# ---------------------------------------------------------------------------------------------
# Segment shapes, poisoned padding, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("name", list(ARENAS))
def test_segment_sums(hip, name, poison):
    """Every segment sum and the total norm within the summation bound; the gaps and the guard are
    neither read into a sum nor written; two runs, and a run with a larger workspace (which changes
    the grid: it is sized from the workspace's capacity), are bitwise identical."""
    segs = ARENAS[name]
    g_host = make_arena(segs, poison, seed=len(segs))
    live = live_mask(segs, g_host.size)
    assert not live.all() or name == "single"
    g = torch.from_numpy(g_host).cuda()
    before = bits(g)
    nb = Norm(hip, segs)
    a = nb.run(g)
    check_sums(a, g_host, segs)
    assert a["apply"] == 1 and a["coef"] == 1.0
    b = nb.run(g)
    c = Norm(hip, segs, ws_extra=8 * 777).run(g)
    for other in (b, c):
        assert a["sumsq"].tobytes() == other["sumsq"].tobytes()
        assert np.float64(a["norm"]).tobytes() == np.float64(other["norm"]).tobytes()
    assert torch.equal(bits(g), before)


def test_short_workspace_skips_instead_of_overrunning(hip):
    """The lengths live on the device, so a workspace that passes the host's check (the least any
    table of n_seg segments needs) can still be too small for this table: the call then writes
    nothing past it, reports a NaN norm and apply = 0 whatever the flags."""
    segs = ARENAS["multi_slice"]  # 2 + 4 slices
    g = torch.from_numpy(make_arena(segs, float("nan"))).cuda()
    nb = Norm(hip, segs)
    nb.ws_bytes = hip.pis_grad_sumsq_ws(2, 2) + 8  # 3 partials for 6 slices
    nb.ws = torch.full((nb.ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = nb.run(g, max_norm=1.0, flags=0)
    assert out["apply"] == 0 and math.isnan(out["norm"]) and out["stats"][SKIPPED] == 1


# ---------------------------------------------------------------------------------------------
# Magnitudes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny", "huge", "mixed"])
def test_magnitudes(hip, case):
    """1e-30 gradients do not underflow to a zero norm (their squares, 1e-60, are normal float64
    numbers), 1e30 ones do not overflow, and a segment of 1e30 beside one of 1e-30 keeps both sums."""
    segs = layout([1003, 517])
    mags = {"tiny": (1e-30, 1e-30), "huge": (1e30, 1e30), "mixed": (1e30, 1e-30)}[case]
    it = iter(mags)
    g_host = make_arena(segs, float("nan"), seed=4,
                        values=lambda rng, n: (next(it) * (0.5 + rng.random(n))).astype(np.float32))
    out = Norm(hip, segs).run(torch.from_numpy(g_host).cuda(), max_norm=1.0, flags=SKIP)
    norm = check_sums(out, g_host, segs)
    assert np.all(out["sumsq"] > 0) and np.all(np.isfinite(out["sumsq"]))
    assert math.isfinite(out["norm"]) and out["norm"] > 0 and out["apply"] == 1
    assert out["stats"][FINITE] == 1 and out["stats"][NORM_MAX] == out["norm"]
    assert (norm > 1.0) == (out["coef"] < 1.0)


# ---------------------------------------------------------------------------------------------
# Coefficient and statistics
# ---------------------------------------------------------------------------------------------
def test_coefficient_and_counters(hip):
    """Above, below and exactly at the threshold and with clipping off: coef is the host definition
    evaluated on the device's own seg_sumsq, to 1 fp32 ulp, and the statistics block follows the
    definition step by step (clipped_steps counts only coef < 1). On the MI355X the coefficient, the
    norm and every statistic came out bit-exact in all four cases: float64 sqrt, divide and add are
    correctly rounded there as on the host."""
    segs = ARENAS["small_lengths"]
    g_host = make_arena(segs, float("nan"), seed=7)
    g = torch.from_numpy(g_host).cuda()
    nb = Norm(hip, segs)
    gs = 0.125
    norm0 = nb.run(g, grad_scale=gs)["norm"]
    nb.stats.zero_()
    stats, exact = None, []
    for label, max_norm, clipped in (("above", norm0 / 2, True), ("below", norm0 * 2, False),
                                     ("at", norm0, True), ("off", None, False)):
        out = nb.run(g, grad_scale=gs, max_norm=max_norm or 0.0, flags=SKIP)
        ref = gradnorm_reference(out["sumsq"], gs, max_norm, True, stats)
        stats = ref["stats"]
        print(f"coef {label}: device {out['coef']!r} host {ref['coef']!r} norm device {out['norm']!r} host {ref['norm']!r}")
        assert abs(float(out["coef"]) - float(ref["coef"])) <= float(np.spacing(ref["coef"])), label
        assert (out["coef"] < 1.0) == clipped and out["apply"] == 1
        assert abs(out["norm"] - ref["norm"]) <= 2 * U64 * ref["norm"]
        assert list(out["stats"][:4]) == list(stats[:4]), label
        for k in (NORM_SUM, NORM_MAX, LAST_NORM, LAST_COEF):
            assert abs(out["stats"][k] - stats[k]) <= 1e-15 * abs(stats[k]), (label, k)
        exact.append(out["coef"] == ref["coef"] and out["norm"] == ref["norm"] and
                     out["stats"].tobytes() == stats.tobytes())
    print("coefficient, norm and statistics bit-exact per case:", exact)
    assert stats[STEPS] == 4 and stats[CLIPPED] == 2 and stats[SKIPPED] == 0


def test_norm_no_worse_than_torch(hip):
    """|norm_device - norm_float64| <= |norm_torch_fp32 - norm_float64| + N 2^-53 norm, torch's fp32
    clip_grad_norm_ on the CPU copy: no worse than the function it stands in for."""
    for name in ("small_lengths", "multi_slice"):
        segs = ARENAS[name]
        g_host = make_arena(segs, float("nan"), seed=11)
        out = Norm(hip, segs).run(torch.from_numpy(g_host).cuda())
        truth = math.sqrt(math.fsum(seg_sumsq_float64(g_host, segs)))
        params = []
        for o, n in segs:
            p = torch.zeros(n, requires_grad=True)
            p.grad = torch.from_numpy(g_host[o:o + n].copy())
            params.append(p)
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, 1e30))
        N = sum(n for _, n in segs)
        print(f"{name}: device error {abs(out['norm'] - truth):.3e} torch fp32 error {abs(norm_t - truth):.3e}")
        assert abs(out["norm"] - truth) <= abs(norm_t - truth) + N * U64 * truth


# ---------------------------------------------------------------------------------------------
# pis_adamw_step_clipped
# ---------------------------------------------------------------------------------------------
_clip_inputs = {}


def clip_inputs():
    if "v" not in _clip_inputs:
        v = adamw_inputs(CLIP_CFG)
        for arr in v[:3] + tuple(v[3]):
            arr.setflags(write=False)
        _clip_inputs["v"] = v
    return _clip_inputs["v"]


def dev(a, n):
    t = torch.full((n + 8,), SENT, device="cuda")
    t[:n].copy_(torch.tensor(a[:n]))
    return t


def clipped_step(hip, p, g, m, v, n, cfg, step, record):
    step_size, bc2_sqrt = adamw_scalars(cfg, step)
    rc = hip.pis_adamw_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, cfg["lr"], BETA1,
                                    BETA2, cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"],
                                    record.data_ptr(), s())
    assert rc == 0, hip.pis_last_error()
    torch.cuda.synchronize()
    for t in (p, g, m, v):
        assert torch.all(t[n:] == SENT)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 1003])
def test_clipped_update_against_float64(hip, n):
    """Three steps with grad_scale = 0.125 and a threshold that clips on every step, on the first n
    elements of a shared 1003-element data set (float4 body, scalar tail, both), sentinels behind
    every buffer. p, m and v against the float64 formula fed g * grad_scale * coef with the
    device's own coef; the bound is ADAMW_MARGIN x the error of torch's fp32 AdamW on the same
    pre-multiplied gradients over the shared data set (the yardstick of
    test_small_kernels_gpu.py::test_adamw_against_float64: the error of a handful of elements is no
    yardstick of its own)."""
    cfg = CLIP_CFG
    inputs = clip_inputs()
    p0, m0, v0, grads = inputs
    gs = cfg["grad_scale"]
    max_norm = 0.25 * min(gs * math.sqrt(math.fsum(np.square(g[:n].astype(np.float64)))) for g in grads)
    p, m, v = dev(p0, n), dev(m0, n), dev(v0, n)
    nb = Norm(hip, [(0, n)])
    states, coefs = [], []
    for i, g in enumerate(grads):
        gd = dev(g, n)
        out = nb.run(gd, grad_scale=gs, max_norm=max_norm, flags=SKIP)
        assert out["coef"] < 0.3 and out["apply"] == 1
        coefs.append(out["coef"])
        clipped_step(hip, p, gd, m, v, n, cfg, cfg["first_step"] + i, nb.record)
        states.append(tuple(t[:n].cpu().numpy() for t in (p, m, v)))
    assert nb.stats.cpu()[CLIPPED] == 3
    pre64 = [g.astype(np.float64) * gs * float(c) for g, c in zip(grads, coefs)]
    pre32 = [(g * np.float32(gs)) * np.float32(c) for g, c in zip(grads, coefs)]
    ref, terr = yardstick(cfg, inputs, pre64, pre32)
    ratios = adamw_ratios(states, ref, terr, n=n)
    print(f"clipped adamw / torch error, n = {n}: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN


def test_unclipped_coefficient_is_bitwise_adamw_step(hip):
    """coef == 1 (norm below the threshold): (g * grad_scale) * 1 is g * grad_scale, so the update
    is bit for bit pis_adamw_step's."""
    cfg, n = CLIP_CFG, 1003
    p0, m0, v0, grads = clip_inputs()
    a = [dev(x, n) for x in (p0, m0, v0)]
    b = [dev(x, n) for x in (p0, m0, v0)]
    nb = Norm(hip, [(0, n)])
    for i, g in enumerate(grads):
        gd = dev(g, n)
        assert nb.run(gd, grad_scale=cfg["grad_scale"], max_norm=1e6)["coef"] == 1.0
        clipped_step(hip, a[0], gd, a[1], a[2], n, cfg, 1 + i, nb.record)
        step_size, bc2_sqrt = adamw_scalars(cfg, 1 + i)
        assert hip.pis_adamw_step(b[0].data_ptr(), gd.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), n, cfg["lr"],
                                  BETA1, BETA2, cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"],
                                  s()) == 0
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0][:n].cpu(), torch.from_numpy(p0[:n].copy()))


# ---------------------------------------------------------------------------------------------
# Guard
# ---------------------------------------------------------------------------------------------
GUARD_SEGS = [(0, 5), (8, 1), (12, 251)]  # the last one: 62 float4 and a scalar tail of 3
GUARD_SPOTS = {"first": 0, "tail": 12 + 250, "length1": 8}


@pytest.mark.parametrize("spot", list(GUARD_SPOTS))
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_guard_skips_then_resumes(hip, bad, spot):
    """One NaN or +Inf gradient with the guard on: p, m and v keep their bits and skipped_steps is
    1; the next, finite step applies with step number 2 (the host counter advanced over the skipped
    step), within ADAMW_MARGIN x torch's error of the float64 formula at that step number."""
    cfg = dict(CLIP_CFG, steps=1)
    n = span(GUARD_SEGS)
    p0, m0, v0, grads = (clip_inputs()[0][:n], clip_inputs()[1][:n], clip_inputs()[2][:n],
                         [clip_inputs()[3][0][:n]])
    g_bad = grads[0].copy()
    g_bad[GUARD_SPOTS[spot]] = bad
    p, m, v = dev(p0, n), dev(m0, n), dev(v0, n)
    before = [bits(t) for t in (p, m, v)]
    nb = Norm(hip, GUARD_SEGS)
    gd = dev(g_bad, n)
    out = nb.run(gd, grad_scale=cfg["grad_scale"], max_norm=1e6, flags=SKIP)
    assert out["apply"] == 0 and out["stats"][SKIPPED] == 1 and out["stats"][FINITE] == 0
    assert not math.isfinite(out["norm"])
    clipped_step(hip, p, gd, m, v, n, cfg, 1, nb.record)
    for t, b in zip((p, m, v), before):
        assert torch.equal(bits(t), b)
    gd = dev(grads[0], n)
    out = nb.run(gd, grad_scale=cfg["grad_scale"], max_norm=1e6, flags=SKIP)
    assert out["apply"] == 1 and out["coef"] == 1.0 and list(out["stats"][:4]) == [2, 0, 1, 1]
    clipped_step(hip, p, gd, m, v, n, cfg, 2, nb.record)
    states = [tuple(t[:n].cpu().numpy() for t in (p, m, v))]
    gs = cfg["grad_scale"]
    ref, terr = yardstick(cfg, (p0, m0, v0, None), [grads[0].astype(np.float64) * gs],
                          [grads[0] * np.float32(gs)], first_step=2)
    ratios = adamw_ratios(states, ref, terr)
    print(f"step after a skipped one / torch error: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN
    ref1, _ = yardstick(cfg, (p0, m0, v0, None), [grads[0].astype(np.float64) * gs], [grads[0] * np.float32(gs)])
    assert np.abs(states[0][0] - ref1[0][0]).max() > 100 * terr[0][0]  # step number 1 is a different update


@pytest.mark.parametrize("spot", list(GUARD_SPOTS))
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_without_guard_the_nan_reaches_p(hip, bad, spot):
    """Guard off, clipping on: coef is NaN (NaN norm) or 0 (Inf norm, and 0 * Inf = NaN), the step
    proceeds and p holds a NaN where the bad gradient was, as with torch's clip_grad_norm_ + AdamW."""
    cfg = dict(CLIP_CFG, steps=1)
    n = span(GUARD_SEGS)
    p0, m0, v0, grads = clip_inputs()
    g_bad = grads[0][:n].copy()
    g_bad[GUARD_SPOTS[spot]] = bad
    p, m, v, gd = dev(p0, n), dev(m0, n), dev(v0, n), dev(g_bad, n)
    nb = Norm(hip, GUARD_SEGS)
    out = nb.run(gd, grad_scale=cfg["grad_scale"], max_norm=1.0, flags=0)
    assert out["apply"] == 1 and out["stats"][SKIPPED] == 0
    assert math.isnan(out["coef"]) if math.isnan(bad) else out["coef"] == 0.0
    clipped_step(hip, p, gd, m, v, n, cfg, 1, nb.record)
    assert math.isnan(p[GUARD_SPOTS[spot]].item())
    q = torch.from_numpy(p0[:n].copy()).requires_grad_(True)
    q.grad = torch.from_numpy(g_bad) * cfg["grad_scale"]
    torch.nn.utils.clip_grad_norm_([q], 1.0)
    torch.optim.AdamW([q], lr=cfg["lr"], eps=cfg["eps"], weight_decay=cfg["wd"], foreach=False).step()
    assert math.isnan(q[GUARD_SPOTS[spot]].item())


# ---------------------------------------------------------------------------------------------
# Through optim.AdamW and the model
# ---------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _stage2_loss():
    from physics_informed_image_segmentation_amd import DiceBCEPDELoss
    return DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0, epsilon=0.05)


def _unet(seed=42, dropout=None):
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(seed)
    return UNet(1, 1, 64).cuda() if dropout is None else UNet(1, 1, 64, dropout=dropout).cuda()


class _Names:
    """_hip tracer that keeps the names of the C-ABI calls."""

    def __init__(self):
        self.names = []

    def begin(self, name, args):
        self.names.append(name)

    def end(self, tok):
        pass


def test_optim_adamw_clips_like_torch(hip):
    """Seed-42 U-Net at 2 x 64^2, Stage-II loss, two steps with max_grad_norm at half the first
    step's measured norm: the weights against a CPU replica fed the HIP step's own gradients through
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, within the 1e-6 of
    tests/test_unet_gpu.py::test_adamw_two_steps_match_torch (norm-wise per tensor, which is that
    test's whole allowance for near-zero gradients: no element-wise comparison). per_tensor_norm and
    total_norm against the CPU float64 norms; step() leaves the gradient arena bit for bit; the
    second step runs with the arena's padding poisoned."""
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, _hip
    img, mask = rt.synthetic_batch(2, 64, 64, seed=42)
    x, t = img.cuda(), mask.cuda()
    net = _unet(42).eval()  # no dropout
    torch.manual_seed(42)
    ref = rt.UNetRef(1, 1, 64).eval()
    crit = _stage2_loss()
    net.zero_grad()
    crit(net(x), t).backward()
    norm0 = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in net.parameters()))
    max_norm = 0.5 * norm0
    opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, max_grad_norm=max_norm, skip_nonfinite=True)
    opt_ref = rt.make_adamw(ref, lr=1e-3, weight_decay=1e-5)
    live = torch.zeros(net.arena.numel(), dtype=torch.bool)
    for _, o, n in net.arena_entries():
        live[o:o + n] = True
    assert not live.all()
    tracer = _Names()
    for step in range(2):
        opt.zero_grad()
        crit(net(x), t).backward()
        if step == 1:
            net.grad_arena()[~live.cuda()] = 1e30  # padding belongs to nobody: it must reach no norm
        for p, q in zip(net.parameters(), ref.parameters()):
            q.grad = p.grad.detach().cpu().clone()
        want = [math.sqrt(float(q.grad.double().pow(2).sum())) for q in ref.parameters()]
        g_before = bits(net.grad_arena())
        _hip.set_tracer(tracer)
        try:
            opt.step()
        finally:
            _hip.set_tracer(None)
        stats = opt.grad_stats()
        torch.cuda.synchronize()
        assert torch.equal(bits(net.grad_arena()), g_before)
        got = stats["per_tensor_norm"].cpu().numpy()
        assert got.shape == (len(want),)
        for q, a, w in zip(ref.parameters(), got, want):
            assert abs(a - w) <= (q.numel() / 2 + 2) * U64 * w, (q.shape, a, w)
        total = math.sqrt(math.fsum(w * w for w in want))
        N = int(live.sum())
        assert abs(float(stats["total_norm"]) - total) <= N * U64 * total
        norm_t = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        assert abs(norm_t - total) <= 1e-5 * total
        opt_ref.step()
        if step == 0:
            assert float(stats["clip_coef"]) == pytest.approx(max_norm / (norm0 + 1e-6), rel=1e-6)
        assert int(stats["applied"]) == 1
    assert tracer.names == ["pis_grad_sumsq", "pis_adamw_step_clipped"] * 2
    worst = max(rel(p, q) for p, q in zip(net.parameters(), ref.parameters()))
    print(f"clipped optim.AdamW against torch: worst per-tensor relative error {worst:.3e}")
    assert worst < 1e-6
    pop = opt.pop_grad_stats()
    assert pop["steps"] == 2 and pop["clipped_steps"] >= 1 and pop["skipped_steps"] == 0
    assert opt.pop_grad_stats()["steps"] == 0


def test_options_unset_is_the_plain_step(hip):
    """An optimizer with both options unset issues exactly pis_adamw_step and leaves bitwise the
    weights of a model stepped without the new arguments."""
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, _hip
    img, mask = rt.synthetic_batch(2, 64, 64, seed=42)
    x, t = img.cuda(), mask.cuda()
    crit = _stage2_loss()
    arenas = []
    for kw in ({}, dict(max_grad_norm=None, skip_nonfinite=False)):
        net = _unet(42).eval()
        opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, **kw)
        tracer = _Names()
        for _ in range(2):
            opt.zero_grad()
            crit(net(x), t).backward()
            _hip.set_tracer(tracer)
            try:
                opt.step()
            finally:
                _hip.set_tracer(None)
        torch.cuda.synchronize()
        assert tracer.names == ["pis_adamw_step"] * 2
        arenas.append(net.arena.clone())
    assert torch.equal(arenas[0], arenas[1])


def test_norm_path_needs_the_flat_path(hip):
    """Gradients that do not view one arena: the unclipped optimizer falls back to per-tensor
    launches, the norm path refuses."""
    from physics_informed_image_segmentation_amd import AdamW
    arena = torch.zeros(32, device="cuda")
    params = [torch.nn.Parameter(arena[0:5]), torch.nn.Parameter(arena[8:20])]
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError, match="flat"):
        AdamW(params, max_grad_norm=1.0).step()
    AdamW(params).step()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# train_epoch
# ---------------------------------------------------------------------------------------------
def test_train_epoch_reports_grad_stats(hip):
    """With the options on, a 3-batch epoch returns grad_norm (mean over the finite steps),
    grad_norm_max, clipped_steps and skipped_steps, equal to what a hand-rolled loop over the same
    batches collects from grad_stats() step by step; with the options off the key set is today's."""
    from torch.utils.data import DataLoader

    from physics_informed_image_segmentation_amd import AdamW, SyntheticDiscDataset, train_epoch
    from physics_informed_image_segmentation_amd.train import _forward_loss
    dl = DataLoader(SyntheticDiscDataset(6, (64, 64), seed=1), batch_size=2)
    dev_ = torch.device("cuda")
    crit = _stage2_loss()
    kw = dict(max_grad_norm=1e-3, skip_nonfinite=True)
    net = _unet(3, dropout=0.0)
    opt = AdamW(net.parameters(), lr=1e-4, weight_decay=1e-5, **kw)
    tr = train_epoch(net, dl, crit, opt, dev_, return_components=True, compute_metrics=False)
    hand = _unet(3, dropout=0.0).train()
    opt_h = AdamW(hand.parameters(), lr=1e-4, weight_decay=1e-5, **kw)
    per_step = []
    for images, masks in dl:
        opt_h.zero_grad()
        _, loss = _forward_loss(hand, images.to(dev_), masks.to(dev_), crit)
        loss.backward()
        opt_h.step()
        per_step.append(opt_h.grad_stats())
    norms = [float(st["total_norm"]) for st in per_step]
    assert len(norms) == 3 and all(math.isfinite(v) and v > 0 for v in norms)
    mean = 0.0
    for v in norms:
        mean += v
    assert tr["grad_norm"] == mean / 3
    assert tr["grad_norm_max"] == max(norms)
    assert tr["clipped_steps"] == sum(float(st["clip_coef"]) < 1.0 for st in per_step) == 3
    assert tr["skipped_steps"] == 0
    assert [int(st["steps"]) for st in per_step] == [1, 2, 3]
    assert torch.equal(net.arena, hand.arena)
    new = {"grad_norm", "grad_norm_max", "clipped_steps", "skipped_steps"}
    plain = _unet(3, dropout=0.0)
    off = train_epoch(plain, dl, crit, AdamW(plain.parameters(), lr=1e-4, weight_decay=1e-5), dev_,
                      return_components=True, compute_metrics=False)
    assert set(off) == set(tr) - new and new <= set(tr)
    assert set(off) == {"loss", "dice_loss", "bce_loss", "pde_loss", "phase_field_loss"}


# ---------------------------------------------------------------------------------------------
# StepGraph with a clipping optimizer (after tests/test_graph_gpu.py::test_graph_steps_equal_eager_steps)
# ---------------------------------------------------------------------------------------------
def _graph_setup(dropout, H=64, B=4):
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    from physics_informed_image_segmentation_amd.dataset import disc_sample
    g = torch.Generator().manual_seed(5)
    imgs, masks = zip(*[disc_sample(H, H, g) for _ in range(B)])
    x, t = torch.stack(imgs).cuda(), torch.stack(masks).cuda()
    torch.manual_seed(42)
    m = UNet(1, 1, 64, dropout=dropout).cuda().train()
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5, max_grad_norm=1e-3, skip_nonfinite=True)
    crit = DiceBCEPDELoss(pde_weight=1e-2, phase_field_weight=1e-2, diffusion_coeff=5.0, epsilon=0.05)
    return m, opt, crit, x, t


def test_graph_steps_equal_eager_steps_with_clipping(hip):
    """Two eager warm-up steps and three graph steps equal five eager steps, bit for bit, with a
    clipping optimizer (StepGraph calls opt.step() eagerly after each replay)."""
    from physics_informed_image_segmentation_amd.graph import StepGraph
    n = 5
    me, oe, crit, x, t = _graph_setup(0.2)
    torch.cuda.manual_seed(11)
    losses_e = []
    for _ in range(n):
        oe.zero_grad(set_to_none=True)
        loss = crit(me(x), t)
        loss.backward()
        oe.step()
        losses_e.append(loss.item())
    mg, og, crit, x, t = _graph_setup(0.2)
    torch.cuda.manual_seed(11)
    sg = StepGraph(mg, crit, og, x, t, warmup=2)
    losses_g = [sg.step().item() for _ in range(n - 2)]
    sg.close()
    torch.cuda.synchronize()
    ok = losses_g == losses_e[2:]
    diff = [k for (k, p), q in zip(me.named_parameters(), mg.parameters()) if not torch.equal(p, q)]
    pe, pg = oe.pop_grad_stats(), og.pop_grad_stats()
    del sg, me, mg, oe, og
    gc.collect()
    torch.cuda.synchronize()
    assert ok, (losses_g, losses_e[2:])
    assert not diff, diff
    assert pe == pg and pe["steps"] == n and pe["clipped_steps"] == n


# ---------------------------------------------------------------------------------------------
# Data parallel (after tests/test_distributed_gpu.py): two gloo ranks on the one GPU
# ---------------------------------------------------------------------------------------------
DP_B, DP_H, DP_W = 2, 64, 64


def _dp_shard(rank):
    from oracle import reference_torch as rt
    img, mask = rt.synthetic_batch(2 * DP_B, DP_H, DP_W, seed=21)
    sl = slice(rank * DP_B, (rank + 1) * DP_B)
    return img[sl].cuda(), mask[sl].cuda()


def _dp_model():
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(5)
    return UNet(1, 1, 64).cuda().eval()  # eval: no dropout draw, the shards are deterministic


def _dp_loss():
    from physics_informed_image_segmentation_amd import DiceBCEPDELoss
    return DiceBCEPDELoss(pde_weight=1e-2, phase_field_weight=1e-2, diffusion_coeff=5.0, epsilon=0.05)


def _dp_worker(rank, world, port, q, max_norm):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from physics_informed_image_segmentation_amd import AdamW
        from physics_informed_image_segmentation_amd.distributed import GradBucketer, broadcast_parameters
        net = _dp_model()
        broadcast_parameters(net)
        GradBucketer(net, bucket_bytes=4 << 20)
        opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, grad_scale=1.0 / world, max_grad_norm=max_norm,
                    skip_nonfinite=True)
        x, t = _dp_shard(rank)
        crit = _dp_loss()
        steps = []
        for step in range(3):
            if step == 2 and rank == 1:
                x = x.clone()
                x[0, 0, 0, 0] = float("nan")  # one rank's input only: the all-reduce carries it to both
            opt.zero_grad(set_to_none=True)
            crit(net(x), t).backward()
            opt.step()
            st = opt.grad_stats()
            torch.cuda.synchronize()
            # plain bytes and digests, no fd sharing; the gradients only where the test reads them
            steps.append((net.grad_arena().cpu().numpy().copy() if step < 2 else None,
                          hashlib.sha1(net.arena.cpu().numpy().tobytes()).hexdigest(),
                          st["total_norm"].cpu().numpy().copy(), st["clip_coef"].cpu().numpy().copy(),
                          int(st["applied"])))
        q.put((rank, steps, opt.pop_grad_stats()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_and_skip_together(hip):
    """Different data per rank at 2 x 64^2, two clipped steps and a third with a NaN in rank 1's
    input: the replicas stay bitwise identical, total_norm is the same bits on both ranks and is the
    float64 norm of the mean of the two ranks' gradients within N 2^-53, and on the NaN step both
    ranks skip and keep their weights. The mean is the one the ranks hold, the all-reduce's fp32 sum
    halved, recomputed here from the per-shard gradients: the norm of the two gradients' float64 mean
    differs from it by the all-reduce's own rounding (2.8e-8 relative on these shards, where a few
    large elements carry the norm), which no norm kernel behind the all-reduce can see."""
    import socket

    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    # the first step's per-shard gradients from the same kernels in this process (initial weights)
    net, crit = _dp_model(), _dp_loss()
    shard_grads = []
    for r in range(2):
        net.zero_grad(set_to_none=True)
        x, t = _dp_shard(r)
        crit(net(x), t).backward()
        shard_grads.append(net.grad_arena().cpu().numpy().copy())
    segs = [(o, n) for _, o, n in net.arena_entries()]
    N = sum(n for _, n in segs)
    w0 = hashlib.sha1(net.arena.cpu().numpy().tobytes()).hexdigest()
    # the mean as the ranks hold it: the all-reduce's fp32 sum of the two gradients, halved (exact)
    mean0 = (shard_grads[0] + shard_grads[1]).astype(np.float64) / 2
    norm0 = math.sqrt(math.fsum(float(np.square(mean0[o:o + n]).sum()) for o, n in segs))
    mean64 = (shard_grads[0].astype(np.float64) + shard_grads[1].astype(np.float64)) / 2
    norm64 = math.sqrt(math.fsum(float(np.square(mean64[o:o + n]).sum()) for o, n in segs))
    max_norm = 0.5 * norm0
    del net
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, max_norm)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (steps, pop) for r, steps, pop in (q.get(timeout=300) for _ in procs)}
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs)
    for step in range(3):
        (g0, w_0, n0, c0, a0), (g1, w_1, n1, c1, a1) = res[0][0][step], res[1][0][step]
        assert w_0 == w_1, "replicas diverged"
        assert n0.tobytes() == n1.tobytes() and c0.tobytes() == c1.tobytes() and a0 == a1
        if step < 2:
            # what each rank holds after the all-reduce is the sum; AdamW applies half of it
            held = math.sqrt(math.fsum(float(np.square(g0[o:o + n].astype(np.float64) * 0.5).sum())
                                       for o, n in segs))
            assert abs(float(n0) - held) <= N * U64 * held
            assert a0 == 1 and float(c0) < 1.0
        else:
            assert a0 == 0 and math.isnan(float(n0))
            assert w_0 == res[0][0][1][1], "a skipped step changed the weights"
    print(f"total_norm {float(res[0][0][0][2])!r}; float64 norm of the fp32 mean {norm0!r}, of the two gradients' "
          f"float64 mean {norm64!r} (the all-reduce's own fp32 rounding: {abs(norm64 - norm0) / norm64:.2e} relative)")
    assert abs(float(res[0][0][0][2]) - norm0) <= N * U64 * norm0
    assert float(res[0][0][0][3]) == pytest.approx(max_norm / (norm0 + 1e-6), rel=1e-6)
    assert res[0][0][0][1] != w0 and res[0][0][1][1] != res[0][0][0][1]
    for r in range(2):
        pop = res[r][1]
        assert (pop["steps"], pop["clipped_steps"], pop["skipped_steps"], pop["finite_steps"]) == (3, 2, 1, 2)
