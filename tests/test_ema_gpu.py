"""EMA weight averaging on the GPU: pis_adamw_step_ema and pis_arena_exchange (csrc/ema.hip),
optim.AdamW(ema_decay=), train_stage / train() on the averaged weights.

What is bitwise: p, m and v against pis_adamw_step (no record) and pis_adamw_step_clipped (record);
the average at w = 0 and w = 1; a skipped step; the exchange. What is bounded: the average at any
other weight, against the float64 recurrence e64 <- e64 + w (p_k - e64) fed the kernel's own read-back
p_k (which isolates the averaging arithmetic from AdamW's). The bound is measured, not chosen:
ADAMW_MARGIN x the max-abs error, per step, of a CPU fp32 ``e.lerp_(p_k, w)`` run against that same
float64 recurrence over the 1003-element data set; the small sizes run the first n elements and are
held to the 1003-element bound (the error of a handful of elements is no yardstick of its own, as in
tests/test_small_kernels_gpu.py::test_adamw_against_float64). ADAMW_MARGIN is the project's allowance
for FMA contraction against torch's two-rounding form. Every kernel test keeps sentinel guard
elements behind all five buffers and checks them.
"""
import copy
import gc

import numpy as np
import pytest
import torch

from test_small_kernels_gpu import arena_grads, make_arena, optim_inputs  # the gapped arena of ARENA_LAYOUT
from test_small_kernels_host import (ADAMW_CONFIGS, ADAMW_MARGIN, ADAMW_N, BETA1, BETA2, adamw_inputs,
                                     adamw_scalars)

pytestmark = pytest.mark.gpu

GUARD = 8
SENT = 3.0e7
SIZES = [1, 2, 3, 4, 5, 7, 8, ADAMW_N]
BIG = 8192 * 256 * 4 + 4099  # more float4 items than the capped grid has threads, and a scalar tail
WEIGHTS = {"9/11": 9.0 / 11.0, "0.5": 0.5, "0.001": 0.001}


def s():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def dev(a, n):
    t = torch.full((n + GUARD,), SENT, device="cuda")
    t[:n].copy_(torch.tensor(a[:n]))  # a copy: the shared inputs are read-only
    return t


def guards_intact(bufs, n):
    return all(bool(torch.all(t[n:] == SENT)) for t in bufs)


def make_record(coef, apply):
    """pis_grad_sumsq's record {float coef; int apply; double norm} with the given decision."""
    rec = torch.zeros(2, dtype=torch.float64, device="cuda")
    rec[:1].view(torch.float32)[0] = coef
    rec[:1].view(torch.int32)[1] = apply
    return rec


_inputs = {}


def inputs_of(name, n=ADAMW_N):
    """(p0, m0, v0, grads, e0) of a configuration, computed once and read-only; e0 is its own draw."""
    if (name, n) not in _inputs:
        cfg = ADAMW_CONFIGS[name]
        p0, m0, v0, grads = adamw_inputs(cfg, n)
        e0 = np.random.default_rng(1000 + cfg["seed"]).standard_normal(n).astype(np.float32)
        for arr in (p0, m0, v0, e0) + tuple(grads):
            arr.setflags(write=False)
        _inputs[(name, n)] = (p0, m0, v0, grads, e0)
    return _inputs[(name, n)]


def ema_call(hip, cfg, step, p, g, m, v, e, n, w, record=None):
    step_size, bc2_sqrt = adamw_scalars(cfg, step)
    rc = hip.pis_adamw_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, cfg["lr"],
                                BETA1, BETA2, cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"], w,
                                0 if record is None else record.data_ptr(), s())
    assert rc == 0, hip.pis_last_error()


def plain_call(hip, cfg, step, p, g, m, v, n, record=None):
    step_size, bc2_sqrt = adamw_scalars(cfg, step)
    if record is None:
        rc = hip.pis_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, cfg["lr"], BETA1, BETA2,
                                cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"], s())
    else:
        rc = hip.pis_adamw_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, cfg["lr"], BETA1,
                                        BETA2, cfg["eps"], cfg["wd"], step_size, bc2_sqrt, cfg["grad_scale"],
                                        record.data_ptr(), s())
    assert rc == 0, hip.pis_last_error()


def run_ema(hip, name, n, w, record=None, against_plain=False, inputs=None):
    """pis_adamw_step_ema over the first n elements, every step of the configuration; returns
    [(p, m, v, e)] per step (numpy). Checks the guards behind all five buffers after every step and,
    with against_plain, p, m and v bitwise against the launch it stands in for."""
    cfg = ADAMW_CONFIGS[name]
    p0, m0, v0, grads, e0 = inputs or inputs_of(name)
    p, m, v, e = dev(p0, n), dev(m0, n), dev(v0, n), dev(e0, n)
    q = [dev(a, n) for a in (p0, m0, v0)] if against_plain else None
    out = []
    for i, g in enumerate(grads):
        gd = dev(g, n)
        ema_call(hip, cfg, cfg["first_step"] + i, p, gd, m, v, e, n, w, record)
        if against_plain:
            plain_call(hip, cfg, cfg["first_step"] + i, q[0], gd, q[1], q[2], n, record)
        torch.cuda.synchronize()
        assert guards_intact((p, gd, m, v, e), n)
        if against_plain:
            for a, b, what in zip((p, m, v), q, "pmv"):
                assert same_bits(a, b), (what, i)
        out.append(tuple(t[:n].cpu().numpy() for t in (p, m, v, e)))
    if against_plain:
        assert not np.array_equal(out[-1][0], p0[:n])
    return out


# ---------------------------------------------------------------------------------------------
# The float64 recurrence and the measured bound
# ---------------------------------------------------------------------------------------------
def recurrence64(e0, ps, ws):
    e = np.asarray(e0, np.float64).copy()
    out = []
    for p, w in zip(ps, ws):
        e = e + w * (np.asarray(p, np.float64) - e)
        out.append(e.copy())
    return out


def torch_lerp_errors(e0, ps, ws):
    """Max-abs error per step of torch's fp32 ``e.lerp_(p_k, w)`` on the CPU against recurrence64."""
    ref = recurrence64(e0, ps, ws)
    e = torch.from_numpy(np.array(e0, np.float32))
    errs = []
    for p, w, r in zip(ps, ws, ref):
        e.lerp_(torch.from_numpy(np.array(p, np.float32)), w)
        errs.append(float(np.abs(e.numpy().astype(np.float64) - r).max()))
    return errs


def worst_ratio(e0, ps, es, ws, terr):
    """Worst error of the averages `es` against recurrence64 relative to torch's (per step)."""
    worst = 0.0
    for e, r, t in zip(es, recurrence64(e0, ps, ws), terr):
        err = float(np.abs(np.asarray(e, np.float64) - r).max())
        assert np.isfinite(err)
        assert t > 0.0  # torch's fp32 run is never exact on these inputs
        worst = max(worst, err / t)
    return worst


_yardstick = {}


def yardstick(hip, name, wname):
    """torch's per-step error over the 1003-element data set, fed the kernel's own p_k at that size."""
    if (name, wname) not in _yardstick:
        w = WEIGHTS[wname]
        states = run_ema(hip, name, ADAMW_N, w)
        ps = [st[0] for st in states]
        _yardstick[(name, wname)] = torch_lerp_errors(inputs_of(name)[4], ps, [w] * len(ps))
    return _yardstick[(name, wname)]


# ---------------------------------------------------------------------------------------------
# pis_adamw_step_ema
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["all_terms", "late"])
@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "record"])
def test_p_m_v_bitwise(hip, name, n, clipped):
    """p, m and v after every step are bit for bit pis_adamw_step's (no record) and, with a record
    {coef 0.37, apply 1}, pis_adamw_step_clipped's."""
    record = make_record(0.37, 1) if clipped else None
    run_ema(hip, name, n, 0.1, record=record, against_plain=True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["all_terms", "late"])
@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_average_against_float64(hip, name, n, wname):
    w = WEIGHTS[wname]
    terr = yardstick(hip, name, wname)
    states = run_ema(hip, name, n, w)
    ps, es = [st[0] for st in states], [st[3] for st in states]
    ratio = worst_ratio(inputs_of(name)[4][:n], ps, es, [w] * len(ps), terr)
    print(f"ema kernel / torch lerp error, {name}, w = {wname}, n = {n}: {ratio:.2f}")
    assert ratio <= ADAMW_MARGIN
    assert not np.array_equal(es[-1], inputs_of(name)[4][:n])


@pytest.mark.parametrize("n", SIZES)
def test_exact_weights(hip, n):
    """w = 1 gives e == p_new and w = 0 leaves e as it was, bit for bit, on every step."""
    e0 = inputs_of("late")[4][:n]
    for st in run_ema(hip, "late", n, 1.0, against_plain=True):
        assert st[3].tobytes() == st[0].tobytes()
    for st in run_ema(hip, "late", n, 0.0, against_plain=True):
        assert st[3].tobytes() == e0.tobytes()


def test_grid_stride_and_tail(hip):
    """n = 8192 x 256 x 4 + 4099, one step: p, m and v bitwise pis_adamw_step's, every element of
    the average moved once, within the bound of a 1003-element data set (this one's first 1003)."""
    w = WEIGHTS["9/11"]
    inputs = inputs_of("one_step", BIG)
    (p, _, _, e), = run_ema(hip, "one_step", BIG, w, against_plain=True, inputs=inputs)
    e0 = inputs[4]
    terr = torch_lerp_errors(e0[:ADAMW_N], [p[:ADAMW_N]], [w])
    ratio = worst_ratio(e0, [p], [e], [w], terr)
    print(f"ema kernel / torch lerp error, one_step, n = {BIG}: {ratio:.2f}")
    assert ratio <= ADAMW_MARGIN
    far = np.abs(p - e0) > 1e-5  # all but a handful of 8.4 M independent draws
    assert far.mean() > 0.999 and np.all(e[far] != e0[far])


@pytest.mark.parametrize("n", [5, ADAMW_N])
def test_skipped_step_writes_nothing(hip, n):
    """A record with apply == 0: all five buffers keep their bits."""
    cfg = ADAMW_CONFIGS["late"]
    p0, m0, v0, grads, e0 = inputs_of("late")
    bufs = [dev(a, n) for a in (p0, grads[0], m0, v0, e0)]
    before = [bits(t) for t in bufs]
    p, g, m, v, e = bufs
    ema_call(hip, cfg, 1000, p, g, m, v, e, n, 0.5, make_record(0.37, 0))
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(bits(t), b)
    ema_call(hip, cfg, 1000, p, g, m, v, e, n, 0.5, make_record(0.37, 1))  # the same call applies with apply == 1
    torch.cuda.synchronize()
    assert not torch.equal(bits(p), before[0]) and not torch.equal(bits(e), before[4])
    assert guards_intact(bufs, n)


def test_of_nothing_touches_nothing(hip):
    bufs = [torch.full((GUARD,), SENT, device="cuda") for _ in range(5)]
    rc = hip.pis_adamw_step_ema(*[b.data_ptr() for b in bufs], 0, 1e-3, BETA1, BETA2, 1e-8, 1e-2, 1e-3, 1.0, 1.0,
                                0.5, 0, s())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(bufs, 0)


# ---------------------------------------------------------------------------------------------
# pis_arena_exchange
# ---------------------------------------------------------------------------------------------
IGUARD = 0x5A5A5A5A
PLANTS = [0x7FC00001, 0x7FC12345, 0x7F800123, -0x00400000 + 7, -0x80000000]  # quiet / signalling NaNs, -0.0


def word_buffer(n, seed):
    """n random 32-bit words (every class of float among them) with NaNs of distinct payloads and
    -0.0 planted, GUARD sentinel words behind; an int32 device tensor."""
    w = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    for k, pl in enumerate(PLANTS):
        # payloads differ per buffer; -0.0 in the first buffer faces the smallest negative denormal
        w[(k * 3 + seed) % n] = np.int32(pl + seed) if pl != -0x80000000 else np.int32(pl + seed - 1)
    full = np.concatenate([w, np.full(GUARD, IGUARD, np.int32)])
    return torch.from_numpy(full).cuda(), torch.from_numpy(w)


@pytest.mark.parametrize("n", SIZES + [BIG])
def test_exchange(hip, n):
    a, a0 = word_buffer(n, 1)
    b, b0 = word_buffer(n, 2)
    assert not torch.equal(a0, b0)
    if n >= 16:
        assert torch.isnan(a0.view(torch.float32)).any() and (a0 == -2 ** 31).any()
    for want_a, want_b in ((b0, a0), (a0, b0)):  # two calls restore both arrays
        rc = hip.pis_arena_exchange(a.view(torch.float32).data_ptr(), b.view(torch.float32).data_ptr(), n, s())
        assert rc == 0, hip.pis_last_error()
        torch.cuda.synchronize()
        assert torch.equal(a[:n].cpu(), want_a) and torch.equal(b[:n].cpu(), want_b)
        assert torch.all(a[n:] == IGUARD) and torch.all(b[n:] == IGUARD)


def test_exchange_refuses_overlap_and_nothing(hip):
    buf, w0 = word_buffer(64, 3)
    base = buf.data_ptr()
    for a, b, n in ((base, base, 16), (base, base + 16, 8), (base + 32, base, 9), (base, base, 0)):
        assert hip.pis_arena_exchange(a, b, n, s()) == -1
        assert b"pis_arena_exchange" in hip.pis_last_error()
    assert hip.pis_arena_exchange(base, base + 128, 0, s()) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(buf[:64].cpu(), w0) and torch.all(buf[64:] == IGUARD)


# ---------------------------------------------------------------------------------------------
# optim.AdamW over a gapped arena
# ---------------------------------------------------------------------------------------------
class _Names:
    """_hip tracer that keeps the names of the C-ABI calls."""

    def __init__(self):
        self.names = []

    def begin(self, name, args):
        self.names.append(name)

    def end(self, tok):
        pass


def traced_step(opt):
    from physics_informed_image_segmentation_amd import _hip
    tracer = _Names()
    _hip.set_tracer(tracer)
    try:
        opt.step()
    finally:
        _hip.set_tracer(None)
    return tracer.names


def _arena_opt(p0, cfg, **kw):
    from physics_informed_image_segmentation_amd import AdamW
    arena, params = make_arena(p0)
    return arena, params, AdamW(params, lr=cfg["lr"], eps=cfg["eps"], weight_decay=cfg["wd"],
                                grad_scale=cfg["grad_scale"], **kw)


def test_optim_flat_equals_per_tensor(hip):
    """AdamW(ema_decay=0.99) through three steps: the single flat launch and the per-parameter
    launches are bitwise equal in p, m, v and e on the live elements; the gaps belong to nobody."""
    cfg, (p0, grads), _, _, live = optim_inputs()
    lv = torch.from_numpy(live)
    runs = []
    for flat in (True, False):
        arena, params, opt = _arena_opt(p0, cfg, ema_decay=0.99)
        for g in grads:
            arena_grads(params, g, flat)
            names = traced_step(opt)
            assert names == (["pis_adamw_step_ema"] if flat else ["pis_adamw_step_ema"] * len(params))
        torch.cuda.synchronize()
        st = opt._flat[0]
        for p in params:
            assert opt.state[p]["ema"].shape == p.shape
            assert opt.state[p]["ema"].shape == opt.state[p]["exp_avg"].shape
        assert opt.ema_arena() is st["ema"] and st["ema"].shape == arena.shape
        runs.append([bits(t.cpu()[lv]) for t in (arena, st["m"], st["v"], st["ema"])])
        if not flat:
            for t in (arena, st["ema"]):  # the average started as a copy of the arena, gaps included
                assert torch.equal(t.cpu()[~lv], torch.from_numpy(p0[~live]))
            for t in (st["m"], st["v"]):
                assert torch.all(t.cpu()[~lv] == 0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][3], bits(torch.from_numpy(p0[live])))
    assert not torch.equal(runs[0][3], runs[0][0])


def test_optim_param_without_grad_keeps_its_average(hip):
    cfg, (p0, grads), _, _, _ = optim_inputs()
    arena, params, opt = _arena_opt(p0, cfg, ema_decay=0.99)
    arena_grads(params, grads[0], flat=False)
    opt.step()
    before = [bits(opt.state[p]["ema"]) for p in params]
    arena_grads(params, grads[1], flat=False)
    params[1].grad = None
    opt.step()
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        assert torch.equal(bits(opt.state[p]["ema"]), before[i]) == (i == 1), i


def test_optim_launch_sequence(hip):
    cfg, (p0, grads), _, _, _ = optim_inputs()
    for kw, want in ((dict(ema_decay=0.99), ["pis_adamw_step_ema"]),
                     (dict(ema_decay=0.99, max_grad_norm=1.0), ["pis_grad_sumsq", "pis_adamw_step_ema"]),
                     (dict(ema_decay=None), ["pis_adamw_step"])):
        arena, params, opt = _arena_opt(p0, cfg, **kw)
        for g in grads[:2]:
            arena_grads(params, g, flat=True)
            assert traced_step(opt) == want
        torch.cuda.synchronize()
        has = ["ema" in opt.state[p] for p in params]
        assert all(has) if kw["ema_decay"] else not any(has)
        assert ("ema" in opt._flat[0]) == bool(kw["ema_decay"])


def test_optim_skip_guard_freezes_the_average(hip):
    """skip_nonfinite with one Inf in the gradient arena: p, m, v and e keep their bits; the next
    clean step moves e with the weight of ITS step number (2: w = 1 - 3/12), not of step 1."""
    cfg, (p0, grads), _, _, live = optim_inputs()
    arena, params, opt = _arena_opt(p0, cfg, ema_decay=0.99, skip_nonfinite=True)
    arena_grads(params, grads[0], flat=True)
    params[3].grad.view(-1)[17] = float("inf")
    assert traced_step(opt) == ["pis_grad_sumsq", "pis_adamw_step_ema"]
    torch.cuda.synchronize()
    st0 = opt._flat[0]
    assert torch.equal(arena.cpu(), torch.tensor(p0))
    assert same_bits(st0["ema"].cpu(), torch.tensor(p0))
    assert torch.all(st0["m"] == 0) and torch.all(st0["v"] == 0)
    assert int(opt.grad_stats()["applied"]) == 0
    arena_grads(params, grads[1], flat=True)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.grad_stats()["applied"]) == 1
    p2, e2 = arena.cpu().numpy()[live], st0["ema"].cpu().numpy()[live]
    assert opt.ema_weight(2) == 0.75
    terr = torch_lerp_errors(p0[live], [p2], [0.75])
    ratio = worst_ratio(p0[live], [p2], [e2], [0.75], terr)
    print(f"average after a skipped step / torch lerp error: {ratio:.2f}")
    assert ratio <= ADAMW_MARGIN
    assert worst_ratio(p0[live], [p2], [e2], [opt.ema_weight(1)], terr) > 100  # step 1's weight is another average


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def _stage2_loss():
    from physics_informed_image_segmentation_amd import DiceBCEPDELoss
    return DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0, epsilon=0.05)


def _unet(seed=42, **kw):
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(seed)
    return UNet(1, 1, 64, **kw).cuda()


def _batch(B=2, H=64, seed=42):
    from oracle import reference_torch as rt
    img, mask = rt.synthetic_batch(B, H, H, seed=seed)
    return img.cuda(), mask.cuda()


def _train_step(net, opt, crit, x, t):
    opt.zero_grad()
    crit(net(x), t).backward()
    opt.step()


def test_model_end_to_end(hip):
    """Three training steps of the U-Net at 2 x 64^2 with the Stage-II loss and ema_decay = 0.9: the
    average follows the float64 recurrence over the read-back weights (weights 9/11, 9/12, 9/13);
    averaged_weights() puts it into the model and takes it out again, bit for bit, also when the
    body raises; step() and a nested entry raise inside."""
    from physics_informed_image_segmentation_amd import AdamW
    net = _unet(42).train()
    x, t = _batch()
    crit = _stage2_loss()
    opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, ema_decay=0.9)
    e0 = net.arena.cpu().numpy().copy()
    ps, es = [], []
    for _ in range(3):
        _train_step(net, opt, crit, x, t)
        torch.cuda.synchronize()
        ps.append(net.arena.cpu().numpy().copy())
        es.append(opt.ema_arena().cpu().numpy().copy())
    ws = [opt.ema_weight(k) for k in (1, 2, 3)]
    assert ws == [1 - 2 / 11, 1 - 3 / 12, 1 - 4 / 13]
    ratio = worst_ratio(e0, ps, es, ws, torch_lerp_errors(e0, ps, ws))
    print(f"model average / torch lerp error over three steps: {ratio:.2f}")
    assert ratio <= ADAMW_MARGIN

    raw, avg = bits(net.arena), bits(opt.ema_arena())
    assert not torch.equal(raw, avg)
    want = opt.ema_state_dict(net)
    raw_sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert list(want) == list(raw_sd) and all(want[k].shape == raw_sd[k].shape for k in want)
    assert all(want[k].data_ptr() != net.state_dict()[k].data_ptr() for k in want)
    assert any(not torch.equal(want[k], raw_sd[k]) for k in want)

    def inside():
        sd, esd = net.state_dict(), opt.ema_state_dict(net)
        for k in want:
            assert same_bits(sd[k], want[k]) and same_bits(esd[k], want[k]), k
        assert torch.equal(bits(net.arena), avg) and torch.equal(bits(opt.ema_arena()), raw)

    with opt.averaged_weights():
        inside()
        with torch.no_grad():
            u = net.eval()(x)
        assert u.shape == (2, 1, 64, 64) and bool(torch.isfinite(u).all())
        with pytest.raises(RuntimeError, match="averaged_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="averaged_weights"):
            with opt.averaged_weights():
                pass
        inside()  # the refused calls exchanged nothing
    assert torch.equal(bits(net.arena), raw) and torch.equal(bits(opt.ema_arena()), avg)
    with pytest.raises(KeyError):
        with opt.averaged_weights():
            inside()
            raise KeyError("body")
    assert torch.equal(bits(net.arena), raw) and torch.equal(bits(opt.ema_arena()), avg)
    for k in want:
        assert same_bits(opt.ema_state_dict(net)[k], want[k])
    _train_step(net.train(), opt, crit, x, t)  # and training goes on
    torch.cuda.synchronize()
    assert not torch.equal(bits(net.arena), raw)


def test_ema_state_dict_loads_into_both_models(hip):
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, UNet
    net = _unet(7).eval()
    x, t = _batch()
    opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, ema_decay=0.5, ema_warmup=False)
    _train_step(net, opt, _stage2_loss(), x, t)
    sd = {k: v.cpu() for k, v in opt.ema_state_dict(net).items()}
    other = UNet(1, 1, 64)
    other.load_state_dict(sd)
    ref = rt.UNetRef(1, 1, 64)
    ref.load_state_dict(sd)
    with opt.averaged_weights():
        for (k, a), b, c in zip(net.state_dict().items(), other.state_dict().values(), ref.state_dict().values()):
            assert same_bits(a.cpu(), b) and same_bits(a.cpu(), c), k


def test_state_dict_round_trip(hip):
    """Two steps, save both state dicts, a third step; fresh objects that load them and take the third
    step on the same batch and dropout scales end bitwise where the uninterrupted run ends."""
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, UNet
    x, t = _batch()
    crit = _stage2_loss()
    scales = [rt.make_drop_scales(rt.UNetRef(1, 1, 64), 2, torch.Generator().manual_seed(50 + k)) for k in range(3)]
    kw = dict(lr=1e-3, weight_decay=1e-5, ema_decay=0.9)
    net = _unet(42).train()
    opt = AdamW(net.parameters(), **kw)
    for k in range(2):
        net.set_dropout_scales(scales[k])
        _train_step(net, opt, crit, x, t)
    torch.cuda.synchronize()
    model_sd = copy.deepcopy(net.state_dict())
    opt_sd = copy.deepcopy(opt.state_dict())
    assert all("ema" in st for st in opt_sd["state"].values())
    saved = [{k: bits(st[k]) for k in ("exp_avg", "exp_avg_sq", "ema")} for st in opt_sd["state"].values()]
    net.set_dropout_scales(scales[2])
    _train_step(net, opt, crit, x, t)
    torch.cuda.synchronize()
    end = [bits(a) for a in (net.arena, opt._flat[0]["m"], opt._flat[0]["v"], opt.ema_arena())]

    fresh = UNet(1, 1, 64).cuda().train()  # other initial weights: what it ends with was loaded
    fopt = AdamW(fresh.parameters(), **kw)
    fresh.load_state_dict(model_sd)
    fopt.load_state_dict(opt_sd)
    for p, sv in zip(fresh.parameters(), saved):  # loaded, not re-initialised
        for k in sv:
            assert torch.equal(bits(fopt.state[p][k]), sv[k]), k
    lv = torch.zeros(fresh.arena.numel(), dtype=torch.bool)
    for (_, o, n), p, sv in zip(fresh.arena_entries(), fresh.parameters(), saved):
        lv[o:o + n] = True
        assert torch.equal(bits(fopt.ema_arena()[o:o + n]), sv["ema"].reshape(-1))  # adopted into the flat state
    assert float(fopt.state[next(iter(fresh.parameters()))]["step"]) == 2.0
    fresh.set_dropout_scales(scales[2])
    _train_step(fresh, fopt, crit, x, t)
    torch.cuda.synchronize()
    assert float(fopt.state[next(iter(fresh.parameters()))]["step"]) == 3.0
    got = [bits(a) for a in (fresh.arena, fopt._flat[0]["m"], fopt._flat[0]["v"], fopt.ema_arena())]
    lv = lv.cuda()
    for a, b, what in zip(got, end, "pmve"):
        assert torch.equal(a[lv], b[lv]), what
    assert not torch.equal(end[3], end[0])


def test_step_graph(hip):
    """StepGraph runs AdamW eagerly after each replay: over two graph steps (steps 3 and 4 after the
    two warm-up steps) the average follows the recurrence over the read-back weights."""
    from physics_informed_image_segmentation_amd import AdamW
    from physics_informed_image_segmentation_amd.graph import StepGraph
    net = _unet(42, dropout=0.2).train()
    x, t = _batch(4)
    opt = AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5, ema_decay=0.9)
    sg = StepGraph(net, _stage2_loss(), opt, x, t, warmup=2)
    torch.cuda.synchronize()
    e0 = opt.ema_arena().cpu().numpy().copy()
    ps, es = [], []
    for _ in range(2):
        sg.step()
        torch.cuda.synchronize()
        ps.append(net.arena.cpu().numpy().copy())
        es.append(opt.ema_arena().cpu().numpy().copy())
    with opt.averaged_weights():  # between two steps, outside any capture: the graph's addresses hold
        held = bits(net.arena)
    sg.step()
    sg.close()
    torch.cuda.synchronize()
    moved = not torch.equal(bits(net.arena), bits(torch.from_numpy(ps[-1]).cuda()))
    ws = [opt.ema_weight(3), opt.ema_weight(4)]
    terr = torch_lerp_errors(e0, ps, ws)
    ratio = worst_ratio(e0, ps, es, ws, terr)
    held_ok = torch.equal(held.cpu(), bits(torch.from_numpy(es[-1])))
    del sg, net, opt
    gc.collect()
    torch.cuda.synchronize()
    print(f"graph steps: average / torch lerp error {ratio:.2f}")
    assert ws == [1 - 4 / 13, 1 - 5 / 14]
    assert ratio <= ADAMW_MARGIN and held_ok and moved


# ---------------------------------------------------------------------------------------------
# train_epoch and train()
# ---------------------------------------------------------------------------------------------
def test_train_epoch_keys_do_not_change(hip):
    from torch.utils.data import DataLoader

    from physics_informed_image_segmentation_amd import AdamW, SyntheticDiscDataset, train_epoch
    dl = DataLoader(SyntheticDiscDataset(4, (64, 64), seed=1), batch_size=2)
    crit = _stage2_loss()
    keys = []
    for kw in (dict(ema_decay=0.9), {}):
        net = _unet(3, dropout=0.0)
        out = train_epoch(net, dl, crit, AdamW(net.parameters(), lr=1e-4, weight_decay=1e-5, **kw),
                          torch.device("cuda"), return_components=True, compute_metrics=False)
        keys.append(set(out))
    assert keys[0] == keys[1] == {"loss", "dice_loss", "bce_loss", "pde_loss", "phase_field_loss"}


def test_train_writes_the_averaged_models(hip, tmp_path):
    import csv

    from physics_informed_image_segmentation_amd import UNet
    from physics_informed_image_segmentation_amd.train import CSV_FIELDS, train
    model, result = train(synthetic=(4, 2, 64, 64), stage1_epochs=1, stage2_epochs=1, ema_decay=0.9,
                          base_dir=str(tmp_path))
    torch.cuda.synchronize()
    models = tmp_path / "models"
    assert sorted(p.name for p in models.iterdir()) == ["unet_baseline.pth", "unet_baseline_ema.pth",
                                                        "unet_pde_regularized.pth", "unet_pde_regularized_ema.pth"]
    for stem in ("unet_baseline", "unet_pde_regularized"):
        raw = torch.load(models / f"{stem}.pth", map_location="cpu", weights_only=True)
        avg = torch.load(models / f"{stem}_ema.pth", map_location="cpu", weights_only=True)
        assert list(raw) == list(avg) and all(raw[k].shape == avg[k].shape for k in raw)
        assert any(not torch.equal(raw[k], avg[k]) for k in raw)
        assert all(bool(torch.isfinite(v).all()) for v in avg.values())
        UNet(1, 1, 64).load_state_dict(avg)
    final = torch.load(models / "unet_pde_regularized.pth", map_location="cpu", weights_only=True)
    for k, v in model.state_dict().items():  # the model is left with its raw weights
        assert torch.equal(v.cpu(), final[k]), k
    files = sorted((tmp_path / "output").glob("metrics_stage*.csv"))
    assert len(files) == 2
    for f in files:
        with open(f, newline="") as fh:
            rows = list(csv.reader(fh))
        assert rows[0] == CSV_FIELDS and len(rows) == 2
    assert set(result) == {"stage1", "stage2"}
