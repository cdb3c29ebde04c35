"""The unrolled PDE layer, the host side (pde.py): ``unroll_vjp_np``, the definition of
``unroll``'s backward, against float64 torch autograd of the eager restatement of the same steps;
its bitwise properties; argument validation in numpy, in Python and through the loaded library (no
compute call: every refused call returns before its launch); the prefixed command-line flags."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from physics_informed_image_segmentation_amd import _hip, pde

f32 = np.float32

# max-norm relative disagreement allowed between the float32 definition and float64 autograd. Both
# sides are deterministic CPU arithmetic; the worst value over the whole grid below, measured, is
# 1.8e-6 (at 1 x 70 x 130; the test prints each shape's), so the bound is about 5 x that.
VJP_RTOL = 1e-5

SHAPES = [(1, 2, 2), (1, 3, 5), (2, 17, 33), (1, 33, 65), (1, 70, 130)]
PRESETS = {"rd": dict(D=1.5, k=1.0, a=0.4), "pf": dict(D=0.05, k=4.0 / 0.05, a=0.5)}


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and bool((bits(x) == bits(y)).all())


def eager_unroll(u, steps, D, k, a, mu, dt, clamp, u0=None, pre=None):
    """The steps of ``evolve_np`` in eager torch, in ``u``'s dtype: what autograd differentiates.
    ``pre`` collects every step's update before the clamp."""
    c, z = u, (u if u0 is None else u0)
    for _ in range(steps):
        p = F.pad(c[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
        up, dn, lf, rt = p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]
        lap = ((up + dn) + (lf + rt)) - 4 * c
        t = D * lap + k * ((c * (1 - c)) * (c - a))
        if mu != 0:
            t = t + mu * (z - c)
        n = c + dt * t
        if pre is not None:
            pre.append(n.detach())
        c = n.clamp(0, 1) if clamp else n
    return c


def pre_clamp_np(u, steps, D, k, a, mu, dt, clamp, u0):
    """Every step's float32 update before the clamp, from one-step ``evolve_np`` calls."""
    c, z, out = u, (u if u0 is None else u0), []
    for _ in range(steps):
        n = pde.evolve_np(c, 1, D, k, a, mu=mu, dt=dt, clamp=False, u0=z)
        out.append(n)
        c = np.clip(n, f32(0), f32(1)) if clamp else n
    return out


def rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def inputs(shape, wide, seed):
    rng = np.random.default_rng(seed)
    u, u0, g = (rng.random(shape, dtype=f32) for _ in range(3))
    if wide:
        u, u0 = f32(1.4) * u - f32(0.2), f32(1.4) * u0 - f32(0.2)
    return u, u0, g - f32(0.5)


def both_sides(u, u0, g, z, steps, kw, mu, dt, clamp):
    """``unroll_vjp_np`` and float64 autograd on one case: the two results, and for a clamped case
    whether both runs clamp the same pixels at every step and the first step's float32 block mask."""
    s64 = {n: float(f32(v)) for n, v in kw.items()}
    got = pde.unroll_vjp_np(u, g, steps, mu=mu, clamp=clamp, u0=z, **kw)
    tu = torch.from_numpy(u.astype(np.float64)).requires_grad_()
    tz = None if z is None else torch.from_numpy(z.astype(np.float64)).requires_grad_()
    pre64 = []
    out = eager_unroll(tu, steps, s64["D"], s64["k"], s64["a"], float(f32(mu)), float(dt), clamp, tz, pre64)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    want = (tu.grad.numpy(), None if tz is None or tz.grad is None else tz.grad.numpy())
    if not clamp:
        return got, want, True, None
    pre32 = pre_clamp_np(u, steps, kw["D"], kw["k"], kw["a"], mu, dt, clamp, z)
    same = all((((n32 < 0) | (n32 > 1)) == ((n64.numpy() < 0) | (n64.numpy() > 1))).all()
               for n32, n64 in zip(pre32, pre64))
    return got, want, same, (pre32[0] < 0) | (pre32[0] > 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vjp_against_float64_autograd(shape):
    """The seeds are chosen here, on the CPU: the first of a case's seeds whose wide input has a first
    step that clamps some pixels and not all, and on which no pre-clamp value falls on different
    sides of 0 or 1 in the two precisions (a tie there means the two runs differentiate different
    functions; it says nothing about the formula). At most TIES seeds may be passed over for a tie:
    a definition whose masks disagreed with autograd's as a rule would still fail the assertion."""
    TIES = 3
    worst = 0.0
    grid = itertools.product(PRESETS, (0.0, 0.5), (True, False), (1, 5, 19), (False, True))
    for case, (preset, mu, clamp, steps, wide) in enumerate(grid):
        kw = dict(PRESETS[preset])
        dt = pde._check_evolve(steps, kw["D"], kw["k"], kw["a"], mu, None)[-1]
        ties = 0
        for seed in range(1000 * (case + 1), 1000 * (case + 2)):
            u, u0, g = inputs(shape, wide, seed)
            runs = [both_sides(u, u0, g, z, steps, kw, mu, dt, clamp) for z in (None, u0)]
            if clamp and wide and not all(0 < r[3].sum() < r[3].size for r in runs):
                continue
            if all(r[2] for r in runs) or ties == TIES:
                break
            ties += 1
        for (got, want, same, blocked), z in zip(runs, (None, u0)):
            tag = (shape, preset, mu, clamp, steps, wide, z is not None, seed)
            assert same, tag
            if clamp and wide:
                assert blocked.any() and not blocked.all(), tag
            e = rel(got[0], want[0])
            assert e <= VJP_RTOL, (tag, e)
            worst = max(worst, e)
            if z is None:
                assert got[1] is None
            elif mu == 0:
                assert not got[1].any() and want[1] is None
            else:
                e = rel(got[1], want[1])
                assert e <= VJP_RTOL, (tag, e)
                worst = max(worst, e)
    print(f"worst max-norm relative disagreement at {shape}: {worst:.3g}")


# ---------------------------------------------------------------------------- bitwise properties

KW = dict(D=0.8, k=2.0, a=0.4)


def test_zero_steps_is_the_identity():
    u, u0, g = inputs((2, 5, 7), True, 3)
    for mu in (0.0, 0.5):
        g_u, g_z = pde.unroll_vjp_np(u, g, 0, mu=mu, **KW)
        assert same_bits(g_u, g) and g_z is None
        g_u, g_z = pde.unroll_vjp_np(u, g, 0, mu=mu, u0=u0, **KW)
        assert same_bits(g_u, g) and same_bits(g_z, np.zeros_like(g))
    g4, _ = pde.unroll_vjp_np(u[:, None], g[:, None], 0, **KW)
    assert g4.shape == (2, 1, 5, 7)


@pytest.mark.parametrize("mu", [0.0, 0.25])
@pytest.mark.parametrize("clamp", [True, False])
def test_flip_and_transpose_equivariance(mu, clamp):
    u, u0, g = inputs((2, 5, 7), True, 4)
    kw = dict(steps=6, mu=mu, clamp=clamp, **KW)
    base = pde.unroll_vjp_np(u, g, u0=u0, **kw)
    for op in (lambda x: x[:, ::-1].copy(), lambda x: x[:, :, ::-1].copy(), lambda x: x.transpose(0, 2, 1).copy()):
        got = pde.unroll_vjp_np(op(u), op(g), u0=op(u0), **kw)
        assert same_bits(got[0], op(base[0])) and same_bits(got[1], op(base[1]))
        alone = pde.unroll_vjp_np(op(u), op(g), **kw)
        assert same_bits(alone[0], op(pde.unroll_vjp_np(u, g, **kw)[0])) and alone[1] is None


@pytest.mark.parametrize("mu", [0.0, 0.5])
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 5, 7)])
def test_defaulted_u0_is_the_sum(mu, shape):
    u, _, g = inputs(shape, True, 5)
    for steps in (1, 4):
        g_u, g_z = pde.unroll_vjp_np(u, g, steps, mu=mu, u0=u.copy(), **KW)
        alone, none = pde.unroll_vjp_np(u, g, steps, mu=mu, **KW)
        assert none is None and same_bits(alone, g_u + g_z)


def test_one_step_by_hand():
    """H = W = 2, D = 1/4, k = 0, dt = 1/4, clamp off: d = 1 + dt (-4 D) = 3/4 everywhere, and every
    pixel receives 2 q from its one vertical and 2 q from its one horizontal neighbour (the reflect
    padding reads each of them twice), weighted dt D = 1/16."""
    u = np.array([[[0.25, 0.5], [0.75, 1.0]]], f32)
    g = np.array([[[1.0, 2.0], [4.0, 8.0]]], f32)
    want = 0.75 * g + (2 * g[:, ::-1] + 2 * g[:, :, ::-1]) / 16
    got, none = pde.unroll_vjp_np(u, g, 1, 0.25, 0.0, 0.5, dt=0.25, clamp=False)
    assert none is None and same_bits(got, want.astype(f32))
    # a clamped pixel passes nothing on: u = 1.5 with D = 0, k = 1 moves to 1.3125 > 1 before the clamp
    hot = np.array([[[1.5, 0.5], [0.5, 0.5]]], f32)
    got, _ = pde.unroll_vjp_np(hot, g, 1, 0.0, 1.0, 0.5, dt=0.25, clamp=True, u0=hot)
    assert got[0, 0, 0] == 0 and (got[0].ravel()[1:] != 0).all()


# ---------------------------------------------------------------------------- arguments

MAP = np.full((1, 4, 4), 0.5, f32)


@pytest.mark.parametrize("args, kw", [
    ((MAP, MAP, 1, 1.0, 1.0, 0.5), dict(dt=0.21)),
    ((MAP, MAP, pde.UNROLL_MAX_STEPS + 1, 1.0, 1.0, 0.5), {}),
    ((MAP, MAP, -1, 1.0, 1.0, 0.5), {}),
    ((MAP, MAP, 1, 1.0, 1.0, 1.0), {}),
    ((MAP, MAP, 1, 1.0, 1.0, 0.5), dict(mu=-1.0)),
    ((MAP, MAP[:, :2], 1, 1.0, 1.0, 0.5), {}),
    ((MAP, MAP, 1, 1.0, 1.0, 0.5), dict(u0=MAP[:, :, :2])),
    ((MAP[:, :1], MAP[:, :1], 1, 1.0, 1.0, 0.5), {}),
])
def test_vjp_bad_arguments_raise(args, kw):
    with pytest.raises(ValueError):
        pde.unroll_vjp_np(*args, **kw)


def test_unroll_refuses_before_any_work():
    """Bad arguments raise ValueError on a host without a GPU: nothing has touched the device yet."""
    u = torch.full((1, 4, 4), 0.5, requires_grad=True)
    for kw in (dict(steps=pde.UNROLL_MAX_STEPS + 1, D=1.0, k=1.0, a=0.5), dict(steps=1, D=1.0, k=1.0, a=0.5, dt=0.5),
               dict(steps=1, D=1.0, k=1.0), dict(steps=1, D=-1.0, k=1.0, a=0.5)):
        with pytest.raises(ValueError):
            pde.unroll(u, **kw)
    r = pde.PDERefine.reaction_diffusion(3)
    with pytest.raises(ValueError):
        pde.unroll(u, r, steps=3)
    with pytest.raises(TypeError):
        pde.unroll(u, object())
    with pytest.raises(TypeError):
        pde.PDELayer(dict(steps=3))
    with pytest.raises(ValueError):
        pde.PDELayer(pde.PDERefine.reaction_diffusion(pde.UNROLL_MAX_STEPS + 1))
    layer = pde.PDELayer(r)
    assert list(layer.parameters()) == [] and layer.refine is r
    net = pde.RefinedModel(torch.nn.Conv2d(1, 1, 1), r)
    assert not hasattr(net, "forward_with_loss") and isinstance(net.model, torch.nn.Conv2d)
    assert [n for n, _ in net.named_parameters()] == ["model.weight", "model.bias"]
    import physics_informed_image_segmentation_amd as pkg
    for name in ("unroll", "unroll_vjp_np", "PDELayer", "RefinedModel"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pde, name)


def test_temporal_block_key():
    lib = _hip.lib()
    shipped = pde.unroll_temporal_block()
    assert shipped in pde.UNROLL_TB_VALUES == (1, 2, 4)
    try:
        assert pde.unroll_temporal_block(1) == shipped and pde.unroll_temporal_block() == 1
        assert lib.pis_tune(_hip.PIS_TUNE_UNROLL_TB, 8) == -1 and pde.unroll_temporal_block() == 1
        with pytest.raises(ValueError):
            pde.unroll_temporal_block(3)
    finally:
        pde.unroll_temporal_block(shipped)


def test_workspace_queries():
    lib = _hip.lib()
    m = (2 * 17 * 33 * 4 + 15) // 16 * 16
    assert lib.pis_pde_unroll_ws(2, 17, 33, 11, 4) == 2 * m and lib.pis_pde_unroll_ws(2, 17, 33, 11, 1) == 10 * m
    assert lib.pis_pde_unroll_ws(2, 17, 33, 4, 4) == 0 and lib.pis_pde_unroll_ws(2, 17, 33, 0, 2) == 0
    assert lib.pis_pde_unroll_ws(2, 17, 33, 11, 0) == lib.pis_pde_unroll_ws(2, 17, 33, 11, pde.unroll_temporal_block())
    assert lib.pis_pde_unroll_bwd_ws(2, 17, 33) == 3 * m
    for bad in ((2, 17, 33, pde.UNROLL_MAX_STEPS + 1, 4), (2, 17, 33, 8, 3), (2, 1, 33, 8, 4)):
        assert lib.pis_pde_unroll_ws(*bad) == 0 and b"pis_pde_unroll_ws" in lib.pis_last_error()
    assert lib.pis_pde_unroll_bwd_ws(1, 8, 4097) == 0


def _fwd(lib, u=0x10000, u0=0, out=0x20000, ckpt=0, ckpt_bytes=0, H=8, W=8, steps=1, dt=0.1, flags=1, a=0.5, tb=4):
    f = ctypes.c_float
    return lib.pis_pde_unroll_fwd(u, u0, out, ckpt, ckpt_bytes, 1, H, W, f(1.0), f(1.0), f(a), f(0.0), f(dt), steps,
                                  flags, tb, 0)


def _bwd(lib, u=0x10000, u0=0, ckpt=0, g_out=0x20000, g_u=0x30000, g_u0=0, H=8, W=8, steps=1, dt=0.1, flags=1, a=0.5,
         tb=4, ws=0x40000, ws_bytes=1 << 16):
    f = ctypes.c_float
    return lib.pis_pde_unroll_bwd(u, u0, ckpt, g_out, g_u, g_u0, 1, H, W, f(1.0), f(1.0), f(a), f(0.0), f(dt), steps,
                                  flags, tb, ws, ws_bytes, 0)


@pytest.mark.parametrize("call, kw, word", [
    (_fwd, dict(H=1), b"H = 1"),
    (_fwd, dict(out=0x10000), b"overlaps"),
    (_fwd, dict(steps=9), b"checkpoint"),
    (_fwd, dict(steps=9, ckpt=0x40000, ckpt_bytes=256), b"checkpoint"),
    (_fwd, dict(steps=9, ckpt=0x20000, ckpt_bytes=1 << 12), b"overlaps"),
    (_fwd, dict(steps=pde.UNROLL_MAX_STEPS + 1), b"steps"),
    (_fwd, dict(dt=0.3), b"exceeds 1"),
    (_fwd, dict(a=1.0), b"0 < a < 1"),
    (_fwd, dict(flags=2), b"flags"),
    (_fwd, dict(tb=8), b"temporal block"),
    (_fwd, dict(u=0x10004), b"aligned"),
    (_bwd, dict(W=4097), b"W = 4097"),
    (_bwd, dict(g_u=0), b"NULL"),
    (_bwd, dict(g_u0=0x50000), b"g_u0 without u0"),
    (_bwd, dict(g_u=0x20000), b"overlaps"),
    (_bwd, dict(u0=0x50000, g_u0=0x30000), b"overlaps"),
    (_bwd, dict(steps=9, ckpt=0x60000, ws=0x30000), b"overlaps"),
    (_bwd, dict(steps=9), b"ckpt is NULL"),
    (_bwd, dict(steps=9, ckpt=0x60000, ws_bytes=256), b"workspace"),
    (_bwd, dict(steps=-1), b"steps"),
    (_bwd, dict(tb=3), b"temporal block"),
    (_bwd, dict(dt=0.3), b"exceeds 1"),
    (_bwd, dict(g_out=0x20008), b"aligned"),
])
def test_entry_point_argument_errors(call, kw, word):
    lib = _hip.lib()
    assert call(lib, **kw) == -1
    msg = lib.pis_last_error()
    assert b"pis_pde_unroll_" in msg and word in msg, msg


# ---------------------------------------------------------------------------- the command-line flags

def test_cli_pde_layer_flags():
    import main
    import run_ablation
    for parse, head in ((main.parse_args, []), (run_ablation.parse_args, ["--ablation", "R1"])):
        assert parse(head).pde_layer_refine is None
        a = parse(head + ["--pde-layer", "pf", "--pde-layer-steps", "5", "--pde-layer-mu", "0.25",
                          "--pde-layer-epsilon", "0.1"])
        assert a.pde_layer_refine == pde.PDERefine.phase_field(5, 0.1, mu=0.25)
        a = parse(head + ["--pde-layer", "rd", "--pde-layer-steps", "7", "--pde-layer-diffusion", "2.0",
                          "--pde-layer-threshold-a", "0.3", "--pde-layer-dt", "0.05"])
        assert a.pde_layer_refine == pde.PDERefine(steps=7, D=2.0, k=1.0, a=0.3, mu=0.0, dt=0.05)
        for bad in (["--pde-layer", "rd"], ["--pde-layer-steps", "3"], ["--pde-layer", "pf", "--pde-layer-steps", "-1"],
                    ["--pde-layer", "rd", "--pde-layer-steps", str(pde.UNROLL_MAX_STEPS + 1)],
                    ["--pde-layer", "rd", "--pde-layer-steps", "3", "--pde-layer-dt", "1.0"],
                    ["--pde-layer", "rd", "--pde-layer-steps", "3", "--pde-layer-threshold-a", "1.0"],
                    ["--pde-layer", "pf", "--pde-layer-steps", "3", "--pde-layer-epsilon", "0"],
                    ["--refine", "rd", "--refine-steps", "3"]):  # the inference flags stay with predict / evaluate
            with pytest.raises(SystemExit):
                parse(head + bad)


def test_refine_flags_round_trip():
    import argparse
    for r in (pde.PDERefine.reaction_diffusion(7, 2.0, 0.3, mu=0.25, dt=0.05), pde.PDERefine.phase_field(5, 0.1),
              pde.PDERefine.reaction_diffusion(3)):
        for prefix in ("refine", "pde-layer"):
            ap = argparse.ArgumentParser()
            pde.add_refine_flags(ap, prefix=prefix)
            args = ap.parse_args(pde.refine_flags(r, prefix=prefix).split())
            assert pde.refine_from_args(ap, args, prefix=prefix) == r
    with pytest.raises(ValueError):
        pde.refine_flags(pde.PDERefine(steps=1, D=1.0, k=3.0, a=0.3))
