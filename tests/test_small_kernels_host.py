"""Host-side checks of the bandwidth-bound kernels' C-ABI (csrc/pointwise.hip, pis_colsum in
csrc/wgrad.hip) that need no GPU:

* the argument contract: on a GPU-less host a call rejected by validation returns PIS_ERR_ARG
  (-1) and a call that passes it reaches the launch and returns PIS_ERR_LAUNCH (-2), so the
  return code says exactly which bad calls get through. Pointers are never dereferenced on the
  host, so made-up addresses serve.
* the AdamW test inputs of tests/test_small_kernels_gpu.py can tell the update's terms apart:
  a numpy fp32 transcription of adamw_kernel stays inside the GPU test's bound in every
  configuration, and the transcription with any one term removed lands at least 10x outside
  it in at least one. The configurations, the float64 reference and the torch-derived bound
  live here and are imported by the GPU file.
"""
import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

PIS_OK, PIS_ERR_ARG, PIS_ERR_LAUNCH = 0, -1, -2

# ---------------------------------------------------------------------------------------------
# AdamW: configurations, float64 reference, torch fp32 run, fp32 transcription of adamw_kernel
# ---------------------------------------------------------------------------------------------
BETA1, BETA2 = 0.9, 0.999
ADAMW_MARGIN = 4.0  # kernel error <= 4 x torch's own fp32 error (FMA contraction, lerp vs m + w (g - m))
ADAMW_N = 1003      # elements of the shared data set (the small sizes run its first n)

ADAMW_CONFIGS = {
    # the configuration of test_kernels_gpu.py::test_adamw_matches_torch
    "existing": dict(lr=1e-3, wd=1e-5, eps=1e-8, grad_scale=1.0, gmag=1.0, steps=3, first_step=1, seed=9),
    # data-parallel 1/world folded into the kernel
    "scaled": dict(lr=1e-3, wd=1e-2, eps=1e-8, grad_scale=0.125, gmag=1.0, steps=3, first_step=1, seed=10),
    # every term matters: small gradients against a large eps, strong decay, many steps
    "all_terms": dict(lr=1e-2, wd=0.1, eps=1e-3, grad_scale=0.125, gmag=1e-3, steps=50, first_step=1, seed=11),
    # late in training: non-zero moments, bias corrections close to 1
    "late": dict(lr=1e-3, wd=1e-2, eps=1e-8, grad_scale=1.0, gmag=1.0, steps=3, first_step=1000, seed=12),
    # one step, for the size that runs the grid-stride loop; and the optim.AdamW run (grad_scale = 1/4)
    "one_step": dict(lr=1e-3, wd=1e-2, eps=1e-8, grad_scale=0.125, gmag=1.0, steps=1, first_step=1, seed=13),
    "optim": dict(lr=1e-3, wd=1e-2, eps=1e-8, grad_scale=0.25, gmag=1.0, steps=3, first_step=1, seed=14),
}


def adamw_inputs(cfg, n=ADAMW_N):
    """p0, m0, v0 and the per-step gradients (fp32 numpy), fixed by the configuration's seed."""
    rng = np.random.default_rng(cfg["seed"])
    p0 = rng.standard_normal(n).astype(np.float32)
    if cfg["first_step"] > 1:
        m0 = (0.1 * cfg["gmag"] * cfg["grad_scale"] * rng.standard_normal(n)).astype(np.float32)
        v0 = ((cfg["gmag"] * cfg["grad_scale"]) ** 2 * (0.5 + rng.random(n))).astype(np.float32)
    else:
        m0 = np.zeros(n, np.float32)
        v0 = np.zeros(n, np.float32)
    grads = [(cfg["gmag"] * rng.standard_normal(n)).astype(np.float32) for _ in range(cfg["steps"])]
    return p0, m0, v0, grads


def adamw_scalars(cfg, step):
    """The host-side scalars optim.AdamW passes to pis_adamw_step at step number `step`."""
    bc1 = 1.0 - BETA1 ** step
    bc2 = 1.0 - BETA2 ** step
    return cfg["lr"] / bc1, bc2 ** 0.5


def adamw_float64(cfg, p0, m0, v0, grads):
    """The formula of include/pis_capi.h in float64; [(p, m, v)] after every step."""
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    out = []
    for i, g in enumerate(grads):
        step_size, bc2_sqrt = adamw_scalars(cfg, cfg["first_step"] + i)
        g = g.astype(np.float64) * cfg["grad_scale"]
        p = p * (1.0 - cfg["lr"] * cfg["wd"])
        m = m + (1.0 - BETA1) * (g - m)
        v = BETA2 * v + (1.0 - BETA2) * g * g
        p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + cfg["eps"])
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def adamw_torch_fp32(cfg, p0, m0, v0, grads):
    """torch.optim.AdamW (single-tensor path, fp32, CPU) on grad_scale * g; [(p, m, v)] per step."""
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=cfg["lr"], betas=(BETA1, BETA2), eps=cfg["eps"], weight_decay=cfg["wd"],
                            foreach=False)
    if cfg["first_step"] > 1:
        opt.state[p] = {"step": torch.tensor(float(cfg["first_step"] - 1)),
                        "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g) * cfg["grad_scale"]
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


def adamw_kernel_fp32(cfg, p0, m0, v0, grads, drop=None):
    """adamw_kernel (csrc/pointwise.hip) and pis_adamw_step's scalar rounding, in numpy fp32.
    drop removes one term: 'wd', 'eps', 'grad_scale', 'bc2_sqrt' or 'omb1' (the (1 - b1) factor)."""
    f = np.float32
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, g in enumerate(grads):
            step_size, bc2_sqrt = adamw_scalars(cfg, cfg["first_step"] + i)
            decay = f(1.0) if drop == "wd" else f(1.0 - cfg["lr"] * cfg["wd"])
            omb1 = f(1.0) if drop == "omb1" else f(1.0 - BETA1)
            omb2, beta2 = f(1.0 - BETA2), f(BETA2)
            gj = g if drop == "grad_scale" else g * f(cfg["grad_scale"])
            p = p * decay
            m = m + omb1 * (gj - m)
            v = v * beta2 + omb2 * gj * gj
            denom = np.sqrt(v) if drop == "bc2_sqrt" else np.sqrt(v) / f(bc2_sqrt)
            if drop != "eps":
                denom = denom + f(cfg["eps"])
            p = p + (-f(step_size)) * (m / denom)
            assert p.dtype == m.dtype == v.dtype == np.float32
            out.append((p.copy(), m.copy(), v.copy()))
    return out


_reference_cache = {}


def adamw_reference(name, n=ADAMW_N):
    """(inputs, float64 states per step, torch's max-abs error per step and quantity): computed once
    per configuration and size, shared and never modified."""
    key = (name, n)
    if key not in _reference_cache:
        cfg = ADAMW_CONFIGS[name]
        inputs = adamw_inputs(cfg, n)
        ref = adamw_float64(cfg, *inputs)
        tor = adamw_torch_fp32(cfg, *inputs)
        terr = [tuple(float(np.abs(t[q] - r[q]).max()) for q in range(3)) for t, r in zip(tor, ref)]
        for arr in inputs[:3] + tuple(inputs[3]) + tuple(a for r in ref for a in r):
            arr.setflags(write=False)
        _reference_cache[key] = (inputs, ref, terr)
    return _reference_cache[key]


def adamw_ratios(states, ref, terr, n=None):
    """Worst error of `states` relative to torch's, per quantity (p, m, v), over all steps. With n the
    states hold only the first n elements (their error is still measured against torch's error over the
    whole shared data set: the maximum over a handful of elements is not a stable yardstick)."""
    worst = [0.0, 0.0, 0.0]
    for s, r, t in zip(states, ref, terr):
        for q in range(3):
            e = float(np.abs(np.asarray(s[q], np.float64) - (r[q] if n is None else r[q][:n])).max())
            if not np.isfinite(e):
                e = float("inf")
            assert t[q] > 0.0  # torch's fp32 run is never exact on these inputs
            worst[q] = max(worst[q], e / t[q])
    return worst


@pytest.mark.parametrize("name", list(ADAMW_CONFIGS))
def test_adamw_transcription_within_bound(name):
    """The faithful fp32 transcription of the kernel is inside the GPU test's bound everywhere."""
    inputs, ref, terr = adamw_reference(name)
    ratios = adamw_ratios(adamw_kernel_fp32(ADAMW_CONFIGS[name], *inputs), ref, terr)
    print(f"adamw transcription / torch error, {name}: p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")
    assert max(ratios) <= ADAMW_MARGIN


@pytest.mark.parametrize("drop", ["wd", "eps", "grad_scale", "bc2_sqrt", "omb1"])
def test_adamw_inputs_expose_each_term(drop):
    """With any one term removed, some configuration puts the transcription at least 10x above the
    bound: the GPU test's inputs cannot pass a kernel that lost that term."""
    worst = {}
    for name, cfg in ADAMW_CONFIGS.items():
        inputs, ref, terr = adamw_reference(name)
        worst[name] = max(adamw_ratios(adamw_kernel_fp32(cfg, *inputs, drop=drop), ref, terr))
    print(f"adamw without {drop}: error / torch error = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) >= 10 * ADAMW_MARGIN


# ---------------------------------------------------------------------------------------------
# Argument contract
# ---------------------------------------------------------------------------------------------
# made-up device addresses, 16-byte aligned and far apart; OFF is one float past a boundary
A, B_, C_, D_, E_, F_, G_, WS = (0x10000000 * (k + 1) for k in range(8))
OFF = 4
BIG = 1 << 30

# every function's arguments by name; GOOD reaches the launch
ORDER = {
    "pis_maxpool2x2_fwd": ["x", "ldx", "y", "B", "H", "W", "C", "stream"],
    "pis_maxpool2x2_bwd": ["x", "ldx", "dy", "dskip", "ldskip", "dx", "lddx", "B", "H", "W", "C", "stream"],
    "pis_head_fwd": ["x", "ldx", "w", "b", "z", "u", "npix", "C", "stream"],
    "pis_head_bwd": ["x", "ldx", "w", "g", "u", "dx", "lddx", "dw", "db", "npix", "C", "flags", "ws", "ws_bytes",
                     "stream"],
    "pis_colsum": ["src", "ld", "npix", "C", "out", "flags", "ws", "ws_bytes", "stream"],
    "pis_adamw_step": ["p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "step_size",
                       "bc2_sqrt", "grad_scale", "stream"],
}
GOOD = {
    "pis_maxpool2x2_fwd": dict(x=A, ldx=16, y=B_, B=1, H=2, W=2, C=8, stream=0),
    "pis_maxpool2x2_bwd": dict(x=A, ldx=16, dy=B_, dskip=C_, ldskip=16, dx=D_, lddx=16, B=1, H=2, W=2, C=8,
                               stream=0),
    "pis_head_fwd": dict(x=A, ldx=16, w=B_, b=C_, z=D_, u=E_, npix=5, C=8, stream=0),
    "pis_head_bwd": dict(x=A, ldx=16, w=B_, g=C_, u=D_, dx=E_, lddx=16, dw=F_, db=G_, npix=5, C=8, flags=0,
                         ws=WS, ws_bytes=None, stream=0),  # ws_bytes: the function's own query
    "pis_colsum": dict(src=A, ld=16, npix=5, C=8, out=B_, flags=0, ws=WS, ws_bytes=None, stream=0),
    "pis_adamw_step": dict(p=A, g=B_, m=C_, v=D_, n=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                           weight_decay=1e-2, step_size=1e-3, bc2_sqrt=1.0, grad_scale=1.0, stream=0),
}


def _ws_query(lib, fn, a):
    if fn == "pis_head_bwd":
        return lib.pis_head_bwd_ws(a["npix"], a["C"])
    return lib.pis_colsum_ws(a["npix"], a["C"])


def _invoke(lib, fn, changes):
    a = dict(GOOD[fn], **{k: v for k, v in changes.items() if k != "ws_short"})
    if "ws_bytes" in a and a["ws_bytes"] is None:
        a["ws_bytes"] = _ws_query(lib, fn, a) - changes.get("ws_short", 0)
    return getattr(lib, fn)(*[a[k] for k in ORDER[fn]])


def _bad(fn, **changes):
    return pytest.param(fn, changes, id=fn[4:] + "-" + "-".join(f"{k}={v}" for k, v in changes.items()))


BAD_CALLS = [
    # ---- pis_maxpool2x2_fwd
    _bad("pis_maxpool2x2_fwd", x=0), _bad("pis_maxpool2x2_fwd", y=0), _bad("pis_maxpool2x2_fwd", B=0),
    _bad("pis_maxpool2x2_fwd", H=3), _bad("pis_maxpool2x2_fwd", W=3), _bad("pis_maxpool2x2_fwd", H=0),
    _bad("pis_maxpool2x2_fwd", C=0), _bad("pis_maxpool2x2_fwd", C=6), _bad("pis_maxpool2x2_fwd", ldx=18),
    _bad("pis_maxpool2x2_fwd", ldx=4),  # ldx < C: pixel rows overlap
    _bad("pis_maxpool2x2_fwd", x=A + OFF), _bad("pis_maxpool2x2_fwd", y=B_ + OFF),
    # ---- pis_maxpool2x2_bwd
    _bad("pis_maxpool2x2_bwd", x=0), _bad("pis_maxpool2x2_bwd", dy=0), _bad("pis_maxpool2x2_bwd", dx=0),
    _bad("pis_maxpool2x2_bwd", B=-1), _bad("pis_maxpool2x2_bwd", H=6, W=5), _bad("pis_maxpool2x2_bwd", H=5),
    _bad("pis_maxpool2x2_bwd", C=10), _bad("pis_maxpool2x2_bwd", C=0), _bad("pis_maxpool2x2_bwd", lddx=18),
    _bad("pis_maxpool2x2_bwd", ldskip=18),
    _bad("pis_maxpool2x2_bwd", ldx=4), _bad("pis_maxpool2x2_bwd", lddx=4), _bad("pis_maxpool2x2_bwd", ldskip=4),
    _bad("pis_maxpool2x2_bwd", x=A + OFF), _bad("pis_maxpool2x2_bwd", dy=B_ + OFF),
    _bad("pis_maxpool2x2_bwd", dskip=C_ + OFF), _bad("pis_maxpool2x2_bwd", dx=D_ + OFF),
    # ---- pis_head_fwd
    _bad("pis_head_fwd", x=0), _bad("pis_head_fwd", w=0), _bad("pis_head_fwd", b=0), _bad("pis_head_fwd", u=0),
    _bad("pis_head_fwd", npix=0), _bad("pis_head_fwd", npix=-3), _bad("pis_head_fwd", C=0),
    _bad("pis_head_fwd", C=6), _bad("pis_head_fwd", ldx=18),
    _bad("pis_head_fwd", ldx=4),
    _bad("pis_head_fwd", x=A + OFF), _bad("pis_head_fwd", w=B_ + OFF),
    # ---- pis_head_bwd
    _bad("pis_head_bwd", x=0), _bad("pis_head_bwd", w=0), _bad("pis_head_bwd", g=0), _bad("pis_head_bwd", dx=0),
    _bad("pis_head_bwd", dw=0), _bad("pis_head_bwd", npix=0), _bad("pis_head_bwd", npix=-1),
    _bad("pis_head_bwd", C=0, ws_bytes=BIG),  # 256 / (C / 4) on the device
    _bad("pis_head_bwd", C=6, ws_bytes=BIG), _bad("pis_head_bwd", C=1028, ldx=1028, lddx=1028, ws_bytes=BIG),
    _bad("pis_head_bwd", ldx=18), _bad("pis_head_bwd", lddx=18),
    _bad("pis_head_bwd", ldx=4), _bad("pis_head_bwd", lddx=4),  # rows overlap, the last one leaves dx
    _bad("pis_head_bwd", ws=0, ws_bytes=BIG),
    _bad("pis_head_bwd", ws_short=1),
    _bad("pis_head_bwd", ws_bytes=0),
    _bad("pis_head_bwd", x=A + OFF), _bad("pis_head_bwd", w=B_ + OFF), _bad("pis_head_bwd", dx=E_ + OFF),
    _bad("pis_head_bwd", ws=WS + OFF, ws_bytes=BIG),
    # ---- pis_colsum
    _bad("pis_colsum", src=0), _bad("pis_colsum", out=0), _bad("pis_colsum", npix=0), _bad("pis_colsum", npix=-5),
    _bad("pis_colsum", C=0, ws_bytes=BIG), _bad("pis_colsum", C=-4, ws_bytes=BIG), _bad("pis_colsum", ld=18),
    _bad("pis_colsum", ld=4), _bad("pis_colsum", C=3, ld=2),
    _bad("pis_colsum", ws=0, ws_bytes=BIG),
    _bad("pis_colsum", ws_short=1), _bad("pis_colsum", C=3, ws_short=1),
    _bad("pis_colsum", src=A + OFF), _bad("pis_colsum", ws=WS + OFF, ws_bytes=BIG),
    # ---- pis_adamw_step
    _bad("pis_adamw_step", p=0), _bad("pis_adamw_step", g=0), _bad("pis_adamw_step", m=0),
    _bad("pis_adamw_step", v=0), _bad("pis_adamw_step", n=-1),
    _bad("pis_adamw_step", p=A + OFF), _bad("pis_adamw_step", g=B_ + OFF), _bad("pis_adamw_step", m=C_ + OFF),
    _bad("pis_adamw_step", v=D_ + OFF),
]

# calls the contract allows: they must still reach the launch
LEGAL_CALLS = [
    _bad("pis_maxpool2x2_fwd"), _bad("pis_maxpool2x2_bwd"), _bad("pis_head_fwd"), _bad("pis_head_bwd"),
    _bad("pis_colsum"), _bad("pis_adamw_step"),
    _bad("pis_maxpool2x2_bwd", dskip=0, ldskip=0),           # no skip gradient: ldskip is unused
    _bad("pis_maxpool2x2_fwd", ldx=8), _bad("pis_head_fwd", ldx=8), _bad("pis_head_bwd", ldx=8, lddx=8),
    _bad("pis_head_fwd", z=0),                                # logits are optional
    _bad("pis_head_fwd", b=C_ + OFF, z=D_ + OFF, u=E_ + OFF),  # per-pixel scalars
    _bad("pis_head_bwd", u=0), _bad("pis_head_bwd", db=0),
    _bad("pis_head_bwd", g=C_ + OFF, u=D_ + OFF, dw=F_ + OFF, db=G_ + OFF),  # scalar reads; unaligned dw, db
    _bad("pis_head_bwd", C=1024, ldx=1024, lddx=1024),        # take the slab sum's scalar columns
    _bad("pis_colsum", out=B_ + OFF),                         # the slab sum's scalar fallback
    # unet.py's two calls: the head's dW, then its db one float past 64 channels (C = 1, ld = 1)
    _bad("pis_colsum", ld=64, npix=1, C=64),
    _bad("pis_colsum", src=A + 4 * 64, ld=1, npix=1, C=1, out=B_ + OFF),
    _bad("pis_colsum", src=A + OFF, ld=5, C=3, ws=WS + OFF),  # scalar kernel: nothing to align
    _bad("pis_colsum", C=1028, ld=1028),
]


@pytest.fixture(scope="module")
def hostlib():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a call that slips through validation would launch with these arguments")
    return _hip.lib()


@pytest.mark.parametrize("fn,changes", BAD_CALLS)
def test_bad_call_is_rejected_before_the_launch(hostlib, fn, changes):
    rc = _invoke(hostlib, fn, changes)
    msg = hostlib.pis_last_error() or b""
    assert rc == PIS_ERR_ARG, (rc, msg)
    assert fn.encode() in msg, msg


@pytest.mark.parametrize("fn,changes", LEGAL_CALLS)
def test_legal_call_reaches_the_launch(hostlib, fn, changes):
    """The baseline of every table row, and the edges the contract allows: validation passes, and on
    a host without a GPU the launch then fails. A bad row thus fails for its own change alone."""
    rc = _invoke(hostlib, fn, changes)
    assert rc == PIS_ERR_LAUNCH, (rc, hostlib.pis_last_error())


def test_adamw_of_nothing_is_a_no_op(hostlib):
    assert _invoke(hostlib, "pis_adamw_step", dict(n=0)) == PIS_OK


@pytest.mark.parametrize("npix,C", [(0, 8), (-1, 8), (5, 0), (5, 6), (5, 1028), (5, -4)])
def test_head_bwd_ws_rejects_bad_sizes(hostlib, npix, C):
    """A size query has no error code to return: it answers 0 bytes and names itself in
    pis_last_error(); pis_head_bwd with the same sizes is in the table above."""
    hostlib.pis_colsum(0, 0, 0, 0, 0, 0, 0, 0, 0)  # leaves another function's name in the message
    assert hostlib.pis_head_bwd_ws(npix, C) == 0
    assert b"pis_head_bwd_ws" in hostlib.pis_last_error()


def test_head_bwd_ws_size():
    """blocks x (C + 1) floats + 256 bytes at max(256, ceil(npix / 2048)) pixels per block."""
    lib = _hip.lib()
    assert lib.pis_head_bwd_ws(1, 4) == 1 * 5 * 4 + 256
    assert lib.pis_head_bwd_ws(257, 64) == 2 * 65 * 4 + 256
    assert lib.pis_head_bwd_ws(524293, 8) == 2041 * 9 * 4 + 256
    assert lib.pis_colsum_ws(65536, 4) == 1024 * 4 * 4
    assert lib.pis_colsum_ws(65537, 4) == 1009 * 4 * 4
