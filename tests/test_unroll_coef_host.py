"""Learnable PDE coefficients, the host side (pde.py): ``unroll_coef_vjp_np``, the
definition of the coefficient gradient, against float64 torch autograd of an eager restatement of
the steps with the five coefficients as leaves; its special cases; ``LearnablePDELayer.coefficients``
on CPU tensors; the command-line flags; the argument checks of the ``_dev`` entry points through the
loaded library (fake pointers: every refused call returns before its launch)."""
import ctypes
import itertools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from physics_informed_image_segmentation_amd import _hip, pde

f32 = np.float32

# |float32 definition - float64 autograd| / abs_sums, per image and column. Both sides are
# deterministic CPU arithmetic; the worst value over the whole grid below, measured, is 2.9e-6 (at
# 1 x 2 x 2, 19 steps of the pf preset, where the float32 states have drifted furthest and four
# pixels average nothing out; 1.1e-7 at 2 x 17 x 33, 2.5e-8 at 1 x 70 x 130; the test prints each
# shape's), so the bound is that times 10 rounded up to one digit, the margin being for other
# seeds: under the project's float32 parity bar of 1e-4.
COEF_RTOL = 3e-5

SHAPES = [(1, 2, 2), (1, 3, 5), (2, 17, 33), (1, 33, 65), (1, 70, 130)]
PRESETS = {"rd": dict(D=1.5, k=1.0, a=0.4), "pf": dict(D=0.05, k=4.0 / 0.05, a=0.5)}


def inputs(shape, wide, seed):
    rng = np.random.default_rng(seed)
    u, u0, g = (rng.random(shape, dtype=f32) for _ in range(3))
    if wide:
        u, u0 = f32(1.4) * u - f32(0.2), f32(1.4) * u0 - f32(0.2)
    return u, u0, g - f32(0.5)


def eager_unroll(u, steps, coef, clamp, with_mu, u0=None, pre=None):
    """The steps of ``evolve_np`` in eager torch with the coefficients as (B, 1, 1) tensors, one row
    per image, so that autograd gives the per-image gradient. ``pre`` collects every step's update
    before the clamp."""
    D, k, a, mu, dt = coef
    c, z = u, (u if u0 is None else u0)
    for _ in range(steps):
        p = F.pad(c[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
        up, dn, lf, rt = p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]
        lap = ((up + dn) + (lf + rt)) - 4 * c
        t = D * lap + k * ((c * (1 - c)) * (c - a))
        if with_mu:
            t = t + mu * (z - c)
        n = c + dt * t
        if pre is not None:
            pre.append(n.detach())
        c = n.clamp(0, 1) if clamp else n
    return c


def pre_clamp_np(u, steps, D, k, a, mu, dt, clamp, u0):
    c, z, out = u, (u if u0 is None else u0), []
    for _ in range(steps):
        n = pde.evolve_np(c, 1, D, k, a, mu=mu, dt=dt, clamp=False, u0=z)
        out.append(n)
        c = np.clip(n, f32(0), f32(1)) if clamp else n
    return out


def autograd64(u, u0, g, steps, vals, clamp, with_mu, pre=None):
    """(B, 5) float64: d sum(g * evolved) / d (D, k, a, mu, dt) per image, the five as independent leaves."""
    B = u.shape[0]
    leaves = [torch.full((B, 1, 1), float(f32(v)), dtype=torch.float64, requires_grad=True) for v in vals]
    tu = torch.from_numpy(u.astype(np.float64))
    tz = None if u0 is None else torch.from_numpy(u0.astype(np.float64))
    out = eager_unroll(tu, steps, leaves, clamp, with_mu, tz, pre)
    (out * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return np.stack([np.zeros(B) if v.grad is None else v.grad.reshape(B).numpy() for v in leaves], axis=1)


def both_sides(u, z, g, steps, kw, mu, dt, clamp):
    sums, abs_sums = pde.unroll_coef_vjp_np(u, g, steps, mu=mu, dt=dt, clamp=clamp, u0=z, **kw)
    pre64 = []
    want = autograd64(u, z, g, steps, (kw["D"], kw["k"], kw["a"], mu, dt), clamp, mu != 0, pre64)
    same = True
    if clamp:
        pre32 = pre_clamp_np(u, steps, kw["D"], kw["k"], kw["a"], mu, dt, clamp, z)
        same = all((((n32 < 0) | (n32 > 1)) == ((n64.numpy() < 0) | (n64.numpy() > 1))).all()
                   for n32, n64 in zip(pre32, pre64))
    return sums, abs_sums, want, same


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_coef_vjp_against_float64_autograd(shape):
    """The case matrix of tests/test_unroll_host.py::test_vjp_against_float64_autograd. A clamped case
    is compared only on a seed where both precisions clamp the same pixels at every step (a tie means
    the two runs differentiate different functions); at most TIES seeds may be passed over for one."""
    TIES = 3
    worst = 0.0
    grid = itertools.product(PRESETS, (0.0, 0.5), (True, False), (1, 5, 19), (False, True))
    for case, (preset, mu, clamp, steps, wide) in enumerate(grid):
        kw = dict(PRESETS[preset])
        dt = pde._check_evolve(steps, kw["D"], kw["k"], kw["a"], mu, None)[-1]
        ties = 0
        for seed in range(1000 * (case + 1), 1000 * (case + 2)):
            u, u0, g = inputs(shape, wide, seed)
            runs = [both_sides(u, z, g, steps, kw, mu, dt, clamp) for z in (None, u0)]
            if all(r[3] for r in runs) or ties == TIES:
                break
            ties += 1
        for (sums, abs_sums, want, same), z in zip(runs, (None, u0)):
            # the mu column is in use with the mu term, except over one step from u0 = u, where z - c = 0
            cols = [0, 1, 2, 4] + ([3] if mu and (steps > 1 or z is not None) else [])
            tag = (shape, preset, mu, clamp, steps, wide, z is not None, seed)
            assert same, tag
            assert sums.shape == abs_sums.shape == (shape[0], 5) and sums.dtype == abs_sums.dtype == np.float64
            assert (abs_sums[:, cols] > 0).all(), tag
            e = float((np.abs(sums - want)[:, cols] / abs_sums[:, cols]).max())
            assert e <= COEF_RTOL, (tag, e)
            worst = max(worst, e)
            if 3 not in cols:
                assert not sums[:, 3].any() and not abs_sums[:, 3].any() and not want[:, 3].any()
    print(f"worst disagreement relative to abs_sums at {shape}: {worst:.3g}")


def test_one_step_by_hand():
    """H = W = 2, one step, clamp off, D = 1/4, k = 2, a = 1/2, dt = 1/8, every value a small dyadic
    rational so that float32 is exact. c = [[1/4, 1/2], [3/4, 1]]; with reflect padding each pixel reads
    its vertical and its horizontal neighbour twice: lap = 2 v + 2 h - 4 c."""
    c = np.array([[[0.25, 0.5], [0.75, 1.0]]], np.float64)
    g = np.array([[[1.0, 2.0], [4.0, 8.0]]], np.float64)
    D, k, a, dt = 0.25, 2.0, 0.5, 0.125
    lap = 2 * c[:, ::-1] + 2 * c[:, :, ::-1] - 4 * c
    cc = c * (1 - c)
    r = cc * (c - a)
    t = D * lap + k * r
    want = [(g * dt * lap).sum(), (g * dt * r).sum(), (g * dt * k * -cc).sum(), 0.0, (g * t).sum()]
    sums, abs_sums = pde.unroll_coef_vjp_np(c.astype(f32), g.astype(f32), 1, D, k, a, dt=dt, clamp=False)
    assert sums.tolist() == [want] and (abs_sums >= np.abs(sums)).all()
    assert abs_sums[0, 0] == np.abs(g * dt * lap).sum()
    # the four-dimensional form, and a pixel the clamp stops adds nothing: u = 1.5 moves past 1
    s4, _ = pde.unroll_coef_vjp_np(c.astype(f32)[:, None], g.astype(f32)[:, None], 1, D, k, a, dt=dt, clamp=False)
    assert (s4 == sums).all()
    hot = np.array([[[1.5, 0.5], [0.5, 0.5]]], f32)
    one = np.array([[[1.0, 0.0], [0.0, 0.0]]], f32)
    sums, abs_sums = pde.unroll_coef_vjp_np(hot, one, 1, 0.0, 1.0, 0.5, dt=0.25, clamp=True)
    assert not sums.any() and not abs_sums.any()


KW = dict(D=0.8, k=2.0, a=0.4)


def test_zero_steps_and_the_mu_column():
    u, u0, g = inputs((2, 5, 7), True, 3)
    for mu, z in itertools.product((0.0, 0.5), (None, u0)):
        sums, abs_sums = pde.unroll_coef_vjp_np(u, g, 0, mu=mu, u0=z, **KW)
        assert sums.shape == (2, 5) and not sums.any() and not abs_sums.any()
    # the mu path off: the column is 0
    sums, abs_sums = pde.unroll_coef_vjp_np(u, g, 4, u0=u0, **KW)
    assert not sums[:, 3].any() and not abs_sums[:, 3].any() and sums[:, [0, 1, 2, 4]].all()
    # kept at mu = 0: the derivative at 0. With u its own u0 the first step has z = c, so one step gives 0
    one, _ = pde.unroll_coef_vjp_np(u, g, 1, with_mu=True, **KW)
    assert not one[:, 3].any()
    two, abs_two = pde.unroll_coef_vjp_np(u, g, 2, with_mu=True, **KW)
    assert two[:, 3].all() and abs_two[:, 3].all()
    off, _ = pde.unroll_coef_vjp_np(u, g, 2, **KW)
    assert (two[:, [0, 1, 2, 4]] == off[:, [0, 1, 2, 4]]).all()  # the kept term adds zeros
    want = autograd64(u, None, g, 2, (KW["D"], KW["k"], KW["a"], 0.0, pde._check_evolve(2, **KW, mu=0.0, dt=None)[-1]),
                      True, True)
    assert (np.abs(two - want) <= COEF_RTOL * abs_two).all()
    # with_mu=False drops the term whatever mu is
    none, _ = pde.unroll_coef_vjp_np(u, g, 2, mu=0.5, dt=0.05, with_mu=False, **KW)
    assert not none[:, 3].any()


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
def test_coef_vjp_bad_arguments_raise(args, kw):
    with pytest.raises(ValueError):
        pde.unroll_coef_vjp_np(*args, **kw)


def test_unroll_coef_refuses_before_any_work():
    u = torch.full((1, 4, 4), 0.5, requires_grad=True)
    coef = torch.tensor([1.0, 1.0, 0.5, 0.0, 0.1])
    r = pde.PDERefine.reaction_diffusion(3)
    for kw in (dict(coef=coef, steps=3), dict(with_mu=False, steps=3), dict(coef=coef, steps=3, with_mu=1),
               dict(coef=coef, with_mu=False), dict(coef=coef, steps=pde.UNROLL_MAX_STEPS + 1, with_mu=False),
               dict(coef=coef, steps=3, with_mu=False, D=1.0), dict(coef=coef, steps=3, with_mu=False, dt=0.1),
               dict(coef=coef, steps=3, with_mu=True, mu=0.5), dict(coef=coef[:4], steps=3, with_mu=False),
               dict(coef=coef.double(), steps=3, with_mu=False), dict(coef=[1.0] * 5, steps=3, with_mu=False)):
        with pytest.raises(ValueError):
            pde.unroll(u, **kw)
    with pytest.raises(ValueError):
        pde.unroll(u, r, coef=coef, with_mu=False)
    assert pde.COEF_NAMES == ("D", "k", "a", "mu", "dt")
    import physics_informed_image_segmentation_amd as pkg
    for name in ("LearnablePDELayer", "unroll_coef_vjp_np"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pde, name)


# ---------------------------------------------------------------------------- LearnablePDELayer

def ulp_apart(x, y):
    return abs(int(np.asarray(x, f32).view(np.int32)) - int(np.asarray(y, f32).view(np.int32)))


@pytest.mark.parametrize("refine", [
    pde.PDERefine.reaction_diffusion(5, 1.5, 0.4, mu=0.25),
    pde.PDERefine.reaction_diffusion(5, 5.0, 0.3, mu=0.5, dt=0.03),
    pde.PDERefine.phase_field(7, 0.05, mu=0.1),
    pde.PDERefine(steps=3, D=0.7, k=2.0, a=0.9, mu=1.0, dt=0.17),
])
def test_layer_initial_values(refine):
    layer = pde.LearnablePDELayer(refine, learn=("D", "k", "a", "mu"))
    assert sorted(n for n, _ in layer.named_parameters()) == ["theta.D", "theta.a", "theta.k", "theta.mu"]
    assert all(p.dim() == 0 and p.item() == 0 and p.dtype == torch.float32 for p in layer.parameters())
    assert sorted(layer.state_dict()) == ["theta.D", "theta.a", "theta.k", "theta.mu"]  # the constants are not saved
    c = layer.coefficients()
    assert c.shape == (5,) and c.dtype == torch.float32 and c.requires_grad
    D, k, a, mu, dt = c.detach().numpy()
    assert D == f32(refine.D) and k == f32(refine.k) and mu == f32(refine.mu)
    assert ulp_apart(a, f32(refine.a)) <= 1
    want_dt = pde._check_evolve(refine.steps, refine.D, refine.k, refine.a, refine.mu, refine.dt)[-1]
    assert ulp_apart(dt, want_dt) <= 2  # dt0 (4 D0 + k0 + mu0) / (4 D0 + k0 + mu0): two more roundings
    if refine.dt is None:
        assert dt == want_dt
    snap = layer.snapshot()
    assert isinstance(snap, pde.PDERefine) and snap.steps == refine.steps and snap.clamp == refine.clamp
    assert snap.D == float(D) and snap.dt == float(dt)
    # what is not learned is the initial value, exactly
    fixed = pde.LearnablePDELayer(refine, learn=("D",)).coefficients().detach().numpy()
    assert fixed[2] == f32(refine.a) and fixed[1] == f32(refine.k) and fixed[3] == f32(refine.mu)


def test_layer_constraints_hold_for_any_theta():
    rng = np.random.default_rng(11)
    for refine, learn, frac in ((pde.PDERefine.reaction_diffusion(5, 1.5, 0.4, mu=0.25), ("D", "k", "a", "mu"), None),
                                (pde.PDERefine.phase_field(7, 0.05), ("eps", "a"), 1.0),
                                (pde.PDERefine.reaction_diffusion(2, 5.0, 0.5, dt=0.0476), ("D", "a"), None),
                                (pde.PDERefine(steps=2, D=0.5, k=1.0, a=0.5, mu=1.0, dt=0.25), ("D", "k", "mu"), None),
                                (pde.PDERefine.reaction_diffusion(2, 0.0, 0.5, mu=0.5), ("k", "mu"), 0.75)):
        layer = pde.LearnablePDELayer(refine, learn=learn, step_fraction=frac)
        for scale in (0.1, 3.0, 40.0, 1e4):
            for _ in range(20):
                with torch.no_grad():
                    for p in layer.parameters():
                        p.fill_(float(rng.uniform(-scale, scale)))
                D, k, a, mu, dt = (float(v) for v in layer.coefficients().detach().numpy())
                got = pde._check_evolve(refine.steps, D, k, a, mu, dt)  # raises when a constraint is broken
                assert np.isfinite(got[1:]).all()
                snap = layer.snapshot()
                assert (snap.D, snap.k, snap.a, snap.mu, snap.dt) == (D, k, a, mu, dt)
                if "D" not in learn and "eps" not in learn:
                    assert D == float(f32(refine.D))


def test_layer_eps_tie_and_gradients():
    r = pde.PDERefine.phase_field(7, 0.05, mu=0.1)
    layer = pde.LearnablePDELayer(r, learn=("eps",))
    assert [n for n, _ in layer.named_parameters()] == ["theta.eps"]
    with torch.no_grad():
        layer.theta["eps"].fill_(0.5)
    D, k, a, mu, dt = layer.coefficients().detach().numpy()
    e = np.exp(f32(0.5))
    assert np.isclose(D, 0.05 * e, rtol=1e-6) and np.isclose(k, 80.0 / e, rtol=1e-6) and np.isclose(D * k, 4.0, rtol=1e-6)
    assert a == f32(0.5) and mu == f32(0.1) and np.isclose(dt, 0.5 / (4 * D + k + mu), rtol=1e-6)
    # autograd reaches theta through dt too: d dt / d theta = -dt (4 D - k) / (4 D + k + mu)
    layer.coefficients()[4].backward()
    want = -dt * (4 * D - k) / (4 * D + k + mu)
    assert np.isclose(layer.theta["eps"].grad.item(), want, rtol=1e-5)
    # RefinedModel takes the layer as it is
    net = pde.RefinedModel(torch.nn.Conv2d(1, 1, 1), layer)
    assert net.layer is layer and [n for n, _ in net.named_parameters()] == ["model.weight", "model.bias",
                                                                           "layer.theta.eps"]


def test_layer_refusals():
    rd = pde.PDERefine.reaction_diffusion(5, 1.5, 0.4)
    for kw in (dict(learn=("D", "q")), dict(learn=("eps", "D")), dict(learn=("eps", "k")), dict(learn=("mu",)),
               dict(learn=("D", "D")), dict(learn=()), dict(step_fraction=0.0), dict(step_fraction=1.5)):
        with pytest.raises(ValueError):
            pde.LearnablePDELayer(rd, **kw)
    with pytest.raises(ValueError):
        pde.LearnablePDELayer(pde.PDERefine.reaction_diffusion(5, 0.0, 0.4), learn=("D",))
    with pytest.raises(ValueError):
        pde.LearnablePDELayer(pde.PDERefine(steps=2, D=1.0, k=0.0, a=0.5), learn=("eps",))
    with pytest.raises(ValueError):
        pde.LearnablePDELayer(pde.PDERefine(steps=pde.UNROLL_MAX_STEPS + 1, D=1.0, k=1.0, a=0.5))
    with pytest.raises(TypeError):
        pde.LearnablePDELayer(dict(steps=3))
    assert pde.LearnablePDELayer(rd).learn == ("D", "k", "a")


def test_train_refuses_before_any_work():
    import importlib
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    rd = pde.PDERefine.reaction_diffusion(3)
    for kw in (dict(pde_layer_learn=("D",)), dict(pde_layer=rd, pde_layer_learn=("mu",)),
               dict(pde_layer=rd, pde_layer_lr=0.1), dict(pde_layer=rd, pde_layer_learn=("D",), pde_layer_lr=0.0)):
        with pytest.raises(ValueError):
            tr.train(synthetic=(4, 2, 32, 32), **kw)


# ---------------------------------------------------------------------------- the command-line flags

def test_cli_learn_flags():
    import main
    head = ["--pde-layer", "rd", "--pde-layer-steps", "5", "--pde-layer-mu", "0.25"]
    a = main.parse_args(head)
    assert a.pde_layer_learn is None and a.pde_layer_lr is None
    a = main.parse_args(head + ["--pde-layer-learn", "D", "a", "mu", "--pde-layer-lr", "0.01"])
    assert a.pde_layer_learn == ("D", "a", "mu") and a.pde_layer_lr == 0.01
    assert a.pde_layer_refine == pde.PDERefine.reaction_diffusion(5, mu=0.25)
    assert main.parse_args(head + ["--pde-layer-learn", "eps"]).pde_layer_learn == ("eps",)
    for bad in (["--pde-layer-learn", "D"], ["--pde-layer-lr", "0.1"], head + ["--pde-layer-lr", "0.1"],
                head + ["--pde-layer-learn"], head + ["--pde-layer-learn", "dt"], head + ["--pde-layer-learn", "eps", "D"],
                head + ["--pde-layer-learn", "D", "--pde-layer-lr", "0"],
                ["--pde-layer", "rd", "--pde-layer-steps", "5", "--pde-layer-learn", "mu"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)


def test_cli_refine_file_round_trip(tmp_path):
    import argparse
    learned = pde.PDERefine(steps=6, D=1.25, k=3.0, a=0.375, mu=0.5, dt=0.0625, clamp=False)
    with pytest.raises(ValueError):
        pde.refine_flags(learned)  # no preset gives k = 3: the reason for the file
    path = tmp_path / "pde_layer.json"
    path.write_text(json.dumps(learned.kwargs(), indent=2))
    assert pde.refine_from_file(path) == learned

    def parse(argv, prefix="refine"):
        ap = argparse.ArgumentParser()
        pde.add_refine_flags(ap, prefix=prefix)
        return pde.refine_from_args(ap, ap.parse_args(argv), prefix=prefix)

    assert parse(["--refine-file", str(path)]) == learned and parse([]) is None
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(dict(learned.kwargs(), dt=1.0)))
    keys = tmp_path / "keys.json"
    keys.write_text(json.dumps(dict(steps=3, D=1.0)))
    for argv in (["--refine-file", str(path), "--refine", "rd", "--refine-steps", "3"],
                 ["--refine-file", str(path), "--refine-steps", "3"], ["--refine-file", str(tmp_path / "none.json")],
                 ["--refine-file", str(bad)], ["--refine-file", str(keys)]):
        with pytest.raises(SystemExit):
            parse(argv)
    with pytest.raises(SystemExit):  # the layer's flags have no file form
        parse(["--pde-layer-file", str(path)], prefix="pde-layer")
    import evaluate as eval_cli
    import predict as predict_cli
    (tmp_path / "m.pth").write_bytes(b"")
    (tmp_path / "a.png").write_bytes(b"")
    base = ["--model", str(tmp_path / "m.pth"), "--input", str(tmp_path / "a.png"), "--output", str(tmp_path / "o")]
    ev = ["--baseline", "b.pth", "--pde", "p.pth"]
    for cli, head in ((predict_cli.parse_args, base), (eval_cli.parse_args, ev)):
        assert cli(head + ["--refine-file", str(path)]).refine_preset == learned
        with pytest.raises(SystemExit):
            cli(head + ["--refine-file", str(path), "--refine", "rd", "--refine-steps", "3"])
    import main
    with pytest.raises(SystemExit):  # the inference flags stay with predict / evaluate
        main.parse_args(["--refine-file", str(path)])


# ---------------------------------------------------------------------------- the entry points

def test_dev_workspace_query():
    lib = _hip.lib()
    m = (2 * 70 * 130 * 4 + 15) // 16 * 16
    tiles = 2 * 3 * 3  # 70 x 130 on 32 x 64 tiles
    assert lib.pis_pde_unroll_bwd_dev_ws(2, 70, 130) == 3 * m + tiles * 8 * 8
    assert lib.pis_pde_unroll_bwd_dev_ws(2, 70, 130) == lib.pis_pde_unroll_bwd_ws(2, 70, 130) + tiles * 64
    assert lib.pis_pde_unroll_bwd_dev_ws(1, 8, 4097) == 0 and b"pis_pde_unroll_bwd_dev_ws" in lib.pis_last_error()
    assert _hip.PIS_EVOLVE_MU == 2


def _fwd(lib, u=0x10000, u0=0, out=0x20000, ckpt=0, ckpt_bytes=0, H=8, W=8, coef=0x70000, steps=1, flags=3, tb=4):
    return lib.pis_pde_unroll_fwd_dev(u, u0, out, ckpt, ckpt_bytes, 1, H, W, coef, steps, flags, tb, 0)


def _bwd(lib, u=0x10000, u0=0, ckpt=0, g_out=0x20000, g_u=0x30000, g_u0=0, g_coef=0x80000, H=8, W=8, coef=0x70000,
         steps=1, flags=3, tb=4, ws=0x40000, ws_bytes=1 << 16):
    return lib.pis_pde_unroll_bwd_dev(u, u0, ckpt, g_out, g_u, g_u0, g_coef, 1, H, W, coef, steps, flags, tb, ws,
                                      ws_bytes, 0)


@pytest.mark.parametrize("call, kw, word", [
    (_fwd, dict(H=1), b"H = 1"),
    (_fwd, dict(coef=0), b"NULL"),
    (_fwd, dict(out=0), b"NULL"),
    (_fwd, dict(coef=0x70002), b"aligned"),
    (_fwd, dict(u=0x10004), b"aligned"),
    (_fwd, dict(out=0x10000), b"overlaps"),
    (_fwd, dict(coef=0x20010), b"overlaps coef"),
    (_fwd, dict(steps=9, ckpt=0x6fff0, ckpt_bytes=1 << 12), b"overlaps coef"),
    (_fwd, dict(steps=9), b"checkpoint"),
    (_fwd, dict(steps=9, ckpt=0x40000, ckpt_bytes=256), b"checkpoint"),
    (_fwd, dict(steps=pde.UNROLL_MAX_STEPS + 1), b"steps"),
    (_fwd, dict(flags=4), b"flags"),
    (_fwd, dict(tb=8), b"temporal block"),
    (_bwd, dict(W=4097), b"W = 4097"),
    (_bwd, dict(g_u=0), b"NULL"),
    (_bwd, dict(coef=0), b"NULL"),
    (_bwd, dict(g_u0=0x50000), b"g_u0 without u0"),
    (_bwd, dict(coef=0x70001), b"aligned"),
    (_bwd, dict(g_coef=0x80004), b"aligned"),
    (_bwd, dict(g_out=0x20008), b"aligned"),
    (_bwd, dict(g_u=0x20000), b"overlaps"),
    (_bwd, dict(g_coef=0x30000), b"overlaps"),
    (_bwd, dict(g_coef=0x70008), b"overlaps"),
    (_bwd, dict(coef=0x300f0), b"overlaps"),
    (_bwd, dict(g_coef=0x40100), b"overlaps"),
    (_bwd, dict(steps=9), b"ckpt is NULL"),
    (_bwd, dict(steps=9, ckpt=0x60000, ws_bytes=3 * 256 + 63), b"workspace"),
    (_bwd, dict(steps=-1), b"steps"),
    (_bwd, dict(flags=8), b"flags"),
    (_bwd, dict(tb=3), b"temporal block"),
])
def test_dev_entry_point_argument_errors(call, kw, word):
    lib = _hip.lib()
    assert call(lib, **kw) == -1
    msg = lib.pis_last_error()
    assert b"pis_pde_unroll_" in msg and b"_dev" in msg and word in msg, msg


def test_by_value_entry_points_refuse_the_mu_flag():
    """PIS_EVOLVE_MU belongs to the _dev entry points: the by-value ones read mu themselves."""
    lib = _hip.lib()
    f = ctypes.c_float
    assert lib.pis_pde_unroll_fwd(0x10000, 0, 0x20000, 0, 0, 1, 8, 8, f(1.0), f(1.0), f(0.5), f(0.0), f(0.1), 1,
                                  _hip.PIS_EVOLVE_CLAMP | _hip.PIS_EVOLVE_MU, 4, 0) == -1
    assert b"flags" in lib.pis_last_error()
    assert lib.pis_pde_unroll_bwd(0x10000, 0, 0, 0x20000, 0x30000, 0, 1, 8, 8, f(1.0), f(1.0), f(0.5), f(0.0), f(0.1), 1,
                                  _hip.PIS_EVOLVE_MU, 4, 0x40000, 1 << 16, 0) == -1
    assert b"flags" in lib.pis_last_error()
