"""PDE evolution and per-image energies, the host side (pde.py): the numpy definitions against
hand-computed 3 x 3 cases (every value a dyadic rational, exact in float32), their fixed points
and symmetries, the stability check, the presets, and the PIS_ERR_ARG cases of the two entry
points through the loaded library (no compute call: every refused call returns before its launch,
and the pointers it is given are never dereferenced)."""
import ctypes

import numpy as np
import pytest

from physics_informed_image_segmentation_amd import _hip, pde

F = np.float32
MAP3 = np.array([[[0.0, 0.5, 1.0], [0.25, 0.5, 0.75], [1.0, 0.5, 0.0]]], F)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


# ---------------------------------------------------------------------------- evolve_np

def test_one_step_by_hand():
    """D = 1/4, k = 1, a = 1/2, dt = 1/4. Corner (0, 0): c = 0, up = dn = 1/4, lf = rt = 1/2, so
    lap = (1/2 + 1) - 0 = 3/2, r = 0, t = 3/8, c' = 3/32. Edge (1, 0): c = 1/4, up = 0, dn = 1,
    lf = rt = 1/2: lap = (1 + 1) - 1 = 1, r = (1/4 * 3/4) * (-1/4) = -3/64, t = 1/4 - 3/64 = 13/64,
    c' = 1/4 + 13/256 = 77/256. The others likewise."""
    want = np.array([[[0.09375, 0.5, 0.90625], [0.30078125, 0.5, 0.69921875], [0.84375, 0.5, 0.15625]]], F)
    got = pde.evolve_np(MAP3, 1, 0.25, 1.0, 0.5, dt=0.25)
    assert got.dtype == np.float32 and (bits(got) == bits(want)).all()
    assert (bits(pde.evolve_np(MAP3[:, None], 1, 0.25, 1.0, 0.5, dt=0.25)) == bits(want[:, None])).all()
    assert (bits(pde.evolve_np(MAP3, 0, 0.25, 1.0, 0.5, dt=0.25)) == bits(MAP3)).all()


@pytest.mark.parametrize("value", [0.0, 1.0, 0.3])
def test_constants_are_fixed_points(value):
    u = np.full((2, 4, 5), value, F)
    for clamp in (True, False):
        got = pde.evolve_np(u, 7, 0.7, 3.0, 0.3, clamp=clamp)
        assert (bits(got) == bits(u)).all()


def test_flip_and_transpose_equivariance():
    u = np.random.default_rng(0).random((1, 5, 7), dtype=F)
    kw = dict(steps=6, D=0.8, k=2.0, a=0.4, mu=0.25)
    base = pde.evolve_np(u, **kw)
    assert (bits(pde.evolve_np(u[:, ::-1].copy(), **kw)) == bits(base[:, ::-1])).all()
    assert (bits(pde.evolve_np(u[:, :, ::-1].copy(), **kw)) == bits(base[:, :, ::-1])).all()
    assert (bits(pde.evolve_np(u.transpose(0, 2, 1).copy(), **kw)) == bits(base.transpose(0, 2, 1))).all()


def test_mu_pulls_towards_u0():
    rng = np.random.default_rng(1)
    u, u0 = rng.random((1, 9, 11), dtype=F), rng.random((1, 9, 11), dtype=F)
    free = pde.evolve_np(u, 200, 1.0, 1.0, 0.5, mu=0.0, u0=u0)
    tied = pde.evolve_np(u, 200, 1.0, 1.0, 0.5, mu=5.0, u0=u0)
    assert np.abs(tied - u0).mean() < 0.5 * np.abs(free - u0).mean()
    # u0 defaults to the initial map
    assert (bits(pde.evolve_np(u, 5, 1.0, 1.0, 0.5, mu=0.5)) == bits(pde.evolve_np(u, 5, 1.0, 1.0, 0.5, mu=0.5, u0=u))).all()


def test_default_dt_is_half_the_bound():
    got = pde.evolve_np(MAP3, 1, 0.25, 1.0, 0.5, mu=0.5)             # 4 D + k + mu = 2.5, dt = 0.2
    want = pde.evolve_np(MAP3, 1, 0.25, 1.0, 0.5, mu=0.5, dt=F(0.5) / F(2.5))
    assert (bits(got) == bits(want)).all()


@pytest.mark.parametrize("args, kw", [
    ((MAP3, 1, 1.0, 1.0, 0.5), dict(dt=0.21)),                # dt (4 D + k + mu) = 1.05
    ((MAP3, 1, 1.0, 1.0, 0.5), dict(dt=0.19, mu=0.5)),        # 0.19 * 5.5 = 1.045
    ((MAP3[:, :1], 1, 1.0, 1.0, 0.5), {}),                    # H = 1
    ((MAP3[:, :, :1], 1, 1.0, 1.0, 0.5), {}),                 # W = 1
    ((MAP3, 1, 1.0, 1.0, 0.0), {}),                           # a = 0
    ((MAP3, 1, 1.0, 1.0, 1.0), {}),                           # a = 1
    ((MAP3, -1, 1.0, 1.0, 0.5), {}),                          # negative steps
    ((MAP3, 1, -1.0, 1.0, 0.5), {}),
    ((MAP3, 1, 1.0, -1.0, 0.5), {}),
    ((MAP3, 1, 1.0, 1.0, 0.5), dict(mu=-0.1)),
    ((MAP3, 1, 1.0, 1.0, 0.5), dict(dt=0.0)),
    ((MAP3, 1, 0.0, 0.0, 0.5), {}),                           # dt=None without a rate
])
def test_bad_arguments_raise(args, kw):
    with pytest.raises(ValueError):
        pde.evolve_np(*args, **kw)


def test_the_bound_itself_is_allowed():
    pde.evolve_np(MAP3, 1, 1.75, 1.0, 0.5, dt=0.125)   # 0.125 * 8 == 1
    with pytest.raises(TypeError):
        pde.evolve_np(MAP3.astype(np.float64), 1, 1.0, 1.0, 0.5)


# ---------------------------------------------------------------------------- presets

def test_presets():
    r = pde.PDERefine.reaction_diffusion(12, diffusion_coeff=2.0, reaction_threshold=0.3, mu=0.1)
    assert (r.steps, r.D, r.k, r.a, r.mu, r.dt, r.clamp) == (12, 2.0, 1.0, 0.3, 0.1, None, True)
    r = pde.PDERefine.reaction_diffusion(3)
    assert (r.D, r.k, r.a, r.mu) == (1.0, 1.0, 0.5, 0.0)
    p = pde.PDERefine.phase_field(5, epsilon=0.05, mu=0.5)
    assert (p.steps, p.D, p.k, p.a, p.mu) == (5, 0.05, 4.0 / 0.05, 0.5, 0.5)
    assert p.kwargs() == dict(steps=5, D=0.05, k=80.0, a=0.5, mu=0.5, dt=None, clamp=True)
    with pytest.raises(ValueError):
        pde.PDERefine(steps=1, D=1.0, k=1.0, a=0.5, dt=0.5)
    with pytest.raises(ValueError):
        pde.PDERefine.phase_field(5, epsilon=0.0)
    import physics_informed_image_segmentation_amd as pkg
    for name in ("PDERefine", "evolve", "evolve_np", "energies", "energies_np"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pde, name)


# ---------------------------------------------------------------------------- energies_np

def test_energies_by_hand():
    """D = 1/4, a = 1/2, eps = 1/2 (he = 1/4, ie = 2) on MAP3. Residuals, row by row: 3/8, 0, -3/8;
    13/64, 0, -13/64; -5/8, 0, 5/8: squares sum to 2 (9/64) + 2 (169/4096) + 2 (25/64) = 4690/4096.
    Energy densities: 0, 3/16, 0; 17/128, 9/64, 17/128; 0, 3/16, 0 (e.g. (1, 1): gx = 1/4, gy = 0,
    w = 1/16, e = 1/64 + 1/8), summing to 25/32. Five pixels lie strictly between 0.1 and 0.9."""
    out, n = pde.energies_np(MAP3, 0.25, 0.5, 0.5)
    assert out.dtype == np.float64 and out.shape == (1, 2) and n.dtype == np.int64
    assert out[0, 0] == (4690.0 / 4096.0) / 9.0
    assert out[0, 1] == (25.0 / 32.0) / 9.0
    assert n.tolist() == [5]
    two = np.concatenate([MAP3, np.full((1, 3, 3), 0.5, F)])
    out, n = pde.energies_np(two, 0.25, 0.5, 0.5)
    assert out[1].tolist() == [0.0, 2.0 * 0.0625] and n.tolist() == [5, 9]
    for bad in ((-1.0, 0.5, 0.5), (1.0, 0.0, 0.5), (1.0, 0.5, 0.0)):
        with pytest.raises(ValueError):
            pde.energies_np(MAP3, *bad)


# ---------------------------------------------------------------------------- the C-ABI on a GPU-less host

def _evolve(lib, u, out, H=8, W=8, steps=1, dt=0.1, ws=0, ws_bytes=0, flags=1, a=0.5):
    f = ctypes.c_float
    return lib.pis_pde_evolve(u, 0, out, 0, 1, H, W, f(1.0), f(1.0), f(a), f(0.0), f(dt), steps, flags, f(0.5), ws,
                              ws_bytes, 0)


def test_workspace_queries():
    lib = _hip.lib()
    assert lib.pis_pde_evolve_ws(2, 17, 33, 64) >= 2 * 2 * 17 * 33 * 4
    assert lib.pis_pde_energies_ws(2, 17, 33) > 0
    assert lib.pis_pde_evolve_ws(1, 1, 8, 1) == 0 and b"pis_pde_evolve_ws" in lib.pis_last_error()
    assert lib.pis_pde_evolve_ws(1, 8, 4097, 1) == 0
    assert lib.pis_pde_energies_ws(0, 8, 8) == 0 and b"pis_pde_energies_ws" in lib.pis_last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(H=1), b"H = 1"),
    (dict(out=0x10000), b"overlaps"),                      # out == u
    (dict(steps=64), b"workspace"),                        # several launches and no workspace
    (dict(steps=64, ws=0x40000, ws_bytes=16), b"workspace"),
    (dict(steps=-1), b"steps"),
    (dict(dt=0.3), b"exceeds 1"),
    (dict(a=0.0), b"0 < a < 1"),
    (dict(flags=2), b"flags"),
    (dict(u=0x10004), b"aligned"),
])
def test_evolve_argument_errors(kw, word):
    lib = _hip.lib()
    args = dict(u=0x10000, out=0x20000)
    args.update(kw)
    assert _evolve(lib, **args) == -1
    msg = lib.pis_last_error()
    assert b"pis_pde_evolve" in msg and word in msg, msg


def test_energies_argument_errors():
    lib = _hip.lib()
    f = ctypes.c_float
    need = lib.pis_pde_energies_ws(1, 8, 8)
    for args in ((0x10000, 1, 1, 8, f(1.0), f(0.5), f(0.05), 0x20000, 0x30000, 0x40000, need, 0),
                 (0x10000, 1, 8, 8, f(1.0), f(0.5), f(0.0), 0x20000, 0x30000, 0x40000, need, 0),
                 (0x10000, 1, 8, 8, f(1.0), f(0.5), f(0.05), 0x20000, 0x30000, 0x40000, need - 1, 0),
                 (0x10000, 1, 8, 8, f(1.0), f(0.5), f(0.05), 0, 0x30000, 0x40000, need, 0)):
        assert lib.pis_pde_energies(*args) == -1
        assert b"pis_pde_energies" in lib.pis_last_error()


def test_temporal_block_key():
    lib = _hip.lib()
    shipped = pde.evolve_temporal_block()
    assert shipped in pde.EVOLVE_T_VALUES and pde.EVOLVE_TILE == (32, 64)
    try:
        assert pde.evolve_temporal_block(1) == shipped and pde.evolve_temporal_block() == 1
        assert lib.pis_tune(_hip.PIS_TUNE_EVOLVE_T, 3) == -1 and pde.evolve_temporal_block() == 1
        with pytest.raises(ValueError):
            pde.evolve_temporal_block(3)
    finally:
        pde.evolve_temporal_block(shipped)


# ---------------------------------------------------------------------------- the command-line flags

def test_cli_refine_flags(tmp_path):
    import evaluate as eval_cli
    import predict as predict_cli
    (tmp_path / "m.pth").write_bytes(b"")
    (tmp_path / "a.png").write_bytes(b"")
    base = ["--model", str(tmp_path / "m.pth"), "--input", str(tmp_path / "a.png"), "--output", str(tmp_path / "o")]
    assert predict_cli.parse_args(base).refine_preset is None
    a = predict_cli.parse_args(base + ["--refine", "pf", "--refine-steps", "5", "--refine-mu", "0.25",
                                       "--refine-epsilon", "0.1"])
    assert a.refine_preset == pde.PDERefine.phase_field(5, 0.1, mu=0.25)
    a = predict_cli.parse_args(base + ["--refine", "rd", "--refine-steps", "7", "--refine-diffusion", "2.0",
                                       "--refine-threshold-a", "0.3", "--refine-dt", "0.05"])
    assert a.refine_preset == pde.PDERefine(steps=7, D=2.0, k=1.0, a=0.3, mu=0.0, dt=0.05)
    ev = ["--baseline", "b.pth", "--pde", "p.pth"]
    a = eval_cli.parse_args(ev)
    assert a.refine_preset is None and a.physics_metrics is False
    a = eval_cli.parse_args(ev + ["--refine", "rd", "--refine-steps", "3", "--physics-metrics",
                                  "--physics-diffusion", "2.0", "--physics-threshold-a", "0.4", "--physics-epsilon", "0.1"])
    assert a.refine_preset == pde.PDERefine.reaction_diffusion(3)
    assert (a.physics_metrics, a.physics_diffusion, a.physics_threshold_a, a.physics_epsilon) == (True, 2.0, 0.4, 0.1)
    for parse, head in ((predict_cli.parse_args, base), (eval_cli.parse_args, ev)):
        for bad in (["--refine", "rd"], ["--refine-steps", "3"], ["--refine", "pf", "--refine-steps", "-1"],
                    ["--refine", "rd", "--refine-steps", "3", "--refine-dt", "1.0"],
                    ["--refine", "rd", "--refine-steps", "3", "--refine-threshold-a", "1.0"],
                    ["--refine", "pf", "--refine-steps", "3", "--refine-epsilon", "0"]):
            with pytest.raises(SystemExit):
                parse(head + bad)
    with pytest.raises(SystemExit):
        eval_cli.parse_args(ev + ["--physics-metrics", "--physics-epsilon", "0"])
