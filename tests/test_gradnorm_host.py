"""Host-side checks of global-norm gradient clipping and the non-finite step guard
(csrc/gradnorm.hip, optim.AdamW(max_grad_norm=, skip_nonfinite=)) that need no GPU:

* ``gradnorm_reference``: the contract of include/pis_capi.h in float64 on the host (segment sums
  of squares, total in segment order, norm, coefficient rounded once to fp32, apply, statistics).
  It is the yardstick of this file and of tests/test_gradnorm_gpu.py, and is itself pinned to
  ``torch.nn.utils.clip_grad_norm_`` on float64 CPU tensors.
* the argument contract of pis_grad_sumsq_ws / pis_grad_sumsq / pis_adamw_step_clipped, in the
  table style of tests/test_small_kernels_host.py: on a GPU-less host a rejected call returns
  PIS_ERR_ARG and names its function, a legal one reaches the launch and returns PIS_ERR_LAUNCH.
* optim.AdamW refuses a non-positive or NaN max_grad_norm, and both CLIs take the two flags, off
  by default.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip
from test_small_kernels_host import (A, ADAMW_MARGIN, B_, BIG, C_, D_, E_, F_, OFF, PIS_ERR_ARG, PIS_ERR_LAUNCH,
                                     PIS_OK, WS, adamw_float64, adamw_inputs, adamw_kernel_fp32, adamw_ratios,
                                     adamw_torch_fp32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53   # unit roundoff of float64
SLICE = 8192       # floats per work item of grad_sumsq_kernel (csrc/gradnorm.hip)
NSTATS = 8
STEPS, CLIPPED, SKIPPED, FINITE, NORM_SUM, NORM_MAX, LAST_NORM, LAST_COEF = range(NSTATS)


# ---------------------------------------------------------------------------------------------
# The contract in float64
# ---------------------------------------------------------------------------------------------
def seg_sumsq_float64(g, segs):
    """Per-segment sum of squares of the fp32 array g. Squares of fp32 values are exact in float64;
    the sum is math.fsum (correctly rounded) up to 2^16 elements and numpy's pairwise float64 sum
    beyond (error about log2(n) 2^-53, far below the n 2^-53 bound the tests allow the device)."""
    out = []
    for off, n in segs:
        sq = np.square(np.asarray(g[off:off + n], np.float64))
        out.append(math.fsum(sq) if n <= 1 << 16 else float(sq.sum()))
    return np.array(out, np.float64)


def gradnorm_reference(seg_sumsq, grad_scale=1.0, max_norm=None, skip_nonfinite=False, stats=None):
    """From the segment sums on: total in segment order, norm = sqrt(total) * grad_scale,
    c = max_norm / (norm + 1e-6) capped at 1 (a NaN stays a NaN), coef = fp32(c), apply, and the
    statistics after the step (a copy of ``stats`` updated; zeros when None)."""
    total = 0.0
    for s in seg_sumsq:
        total += float(s)
    norm = math.sqrt(total) * grad_scale if not math.isnan(total) else float("nan")
    finite = math.isfinite(total)
    c = 1.0
    if max_norm is not None:
        q = max_norm / (norm + 1e-6)
        c = 1.0 if q > 1.0 else q
    coef = np.float32(c)
    apply = 1 if (finite or not skip_nonfinite) else 0
    st = np.zeros(NSTATS) if stats is None else np.array(stats, np.float64)
    st[STEPS] += 1
    if apply and coef < np.float32(1.0):
        st[CLIPPED] += 1
    if not apply:
        st[SKIPPED] += 1
    if finite:
        st[FINITE] += 1
        st[NORM_SUM] += norm
        st[NORM_MAX] = max(st[NORM_MAX], norm)
    st[LAST_NORM] = norm
    st[LAST_COEF] = float(coef)
    return dict(total=total, norm=norm, coef64=c, coef=coef, apply=apply, finite=finite, stats=st)


ARENA_SEGS = [(0, 5), (8, 12), (20, 1), (24, 251)]  # tests/test_small_kernels_gpu.py:ARENA_LAYOUT


def _arena(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal(24 + 251)).astype(np.float32)


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_reference_is_clip_grad_norm(max_norm, grad_scale):
    """The float64 definition against torch.nn.utils.clip_grad_norm_ on float64 CPU tensors holding
    grad_scale * g: the same total norm, and the gradients after clipping are g * coef, both to
    1e-15 relative."""
    g = _arena(3)
    ref = gradnorm_reference(seg_sumsq_float64(g, ARENA_SEGS), grad_scale, max_norm)
    params = []
    for off, n in ARENA_SEGS:
        p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
        p.grad = torch.from_numpy(g[off:off + n].astype(np.float64)) * grad_scale
        params.append(p)
    before = [p.grad.clone() for p in params]
    norm_t = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert abs(norm_t - ref["norm"]) <= 1e-15 * ref["norm"]
    assert (ref["coef64"] < 1.0) == (norm_t + 1e-6 > max_norm)
    for p, b in zip(params, before):
        want = b.numpy() * ref["coef64"]
        assert np.all(np.abs(p.grad.numpy() - want) <= 1e-15 * np.abs(want))


def test_reference_nonfinite_and_stats():
    """Inf gives coef 0 and NaN gives coef NaN as torch's formula does; the guard decides apply;
    the statistics count steps, clipped (applied with coef < 1), skipped, and sum / max over the
    finite steps only."""
    inf, nan = float("inf"), float("nan")
    r = gradnorm_reference([1.0, inf], 1.0, 2.0, skip_nonfinite=False)
    assert r["coef"] == 0.0 and r["apply"] == 1 and r["stats"][CLIPPED] == 1
    t = torch.clamp(torch.tensor(2.0) / (torch.tensor(inf) + 1e-6), max=1.0)
    assert float(t) == 0.0
    r = gradnorm_reference([nan, 1.0], 1.0, 2.0, skip_nonfinite=False)
    assert math.isnan(r["coef"]) and r["apply"] == 1 and r["stats"][CLIPPED] == 0
    assert math.isnan(float(torch.clamp(torch.tensor(2.0) / (torch.tensor(nan) + 1e-6), max=1.0)))
    r = gradnorm_reference([nan, 1.0], 1.0, None, skip_nonfinite=True)
    assert r["coef"] == 1.0 and r["apply"] == 0
    st = None
    for sums, skip in (([9.0], True), ([inf], True), ([1.0], True), ([nan], False)):
        st = gradnorm_reference(sums, 0.5, 1.0, skip, st)["stats"]
    assert list(st[:4]) == [4, 1, 1, 2]
    assert st[NORM_SUM] == 1.5 + 0.5 and st[NORM_MAX] == 1.5 and math.isnan(st[LAST_NORM])
    # no threshold: the coefficient is 1 whatever the norm
    assert gradnorm_reference([4.0], 1.0, None)["coef"] == 1.0
    # exactly at the threshold the formula clips (norm / (norm + 1e-6) < 1), as torch does
    assert gradnorm_reference([4.0], 1.0, 2.0)["coef"] < 1.0


# ---------------------------------------------------------------------------------------------
# The clipped update's inputs can tell a kernel that ignores coef or apply from one that does not
# ---------------------------------------------------------------------------------------------
# the configuration of tests/test_gradnorm_gpu.py::test_clipped_update_against_float64
CLIP_CFG = dict(lr=1e-3, wd=1e-2, eps=1e-8, grad_scale=0.125, gmag=1.0, steps=3, first_step=1, seed=21)


def clip_yardstick(cfg, inputs, premult64, premult32, first_step=None):
    """float64 states and torch's fp32 max-abs error per step, both fed the same pre-multiplied
    gradients (so grad_scale = 1 inside)."""
    p0, m0, v0, _ = inputs
    c1 = dict(cfg, grad_scale=1.0, first_step=first_step or cfg["first_step"])
    ref = adamw_float64(c1, p0, m0, v0, premult64)
    tor = adamw_torch_fp32(c1, p0, m0, v0, premult32)
    terr = [tuple(float(np.abs(t[q] - r[q]).max()) for q in range(3)) for t, r in zip(tor, ref)]
    return ref, terr


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 1003])
def test_clipped_update_inputs_expose_coef(n):
    """A numpy fp32 transcription of adamw_clipped_kernel, g' = (g * grad_scale) * coef, on the GPU
    test's inputs and threshold: inside the GPU test's bound with coef, at least 10x outside it with
    coef ignored (g' = g * grad_scale). The GPU test cannot pass a kernel that drops the coefficient."""
    cfg = CLIP_CFG
    inputs = adamw_inputs(cfg)
    p0, m0, v0, grads = inputs
    gs = cfg["grad_scale"]
    max_norm = 0.25 * min(gs * math.sqrt(math.fsum(np.square(g[:n].astype(np.float64)))) for g in grads)
    coefs = [gradnorm_reference(seg_sumsq_float64(g, [(0, n)]), gs, max_norm)["coef"] for g in grads]
    assert all(c < 0.3 for c in coefs)
    pre64 = [g.astype(np.float64) * gs * float(c) for g, c in zip(grads, coefs)]
    pre32 = [(g * np.float32(gs)) * c for g, c in zip(grads, coefs)]
    ref, terr = clip_yardstick(cfg, inputs, pre64, pre32)
    c1 = dict(cfg, grad_scale=1.0)
    cut = lambda states: [tuple(a[:n] for a in st) for st in states]
    good = adamw_ratios(cut(adamw_kernel_fp32(c1, p0, m0, v0, pre32)), ref, terr, n=n)
    lost = adamw_ratios(cut(adamw_kernel_fp32(c1, p0, m0, v0, [g * np.float32(gs) for g in grads])), ref, terr, n=n)
    print(f"n = {n}: transcription / torch error {max(good):.2f}; with coef ignored {max(lost):.3g}")
    assert max(good) <= ADAMW_MARGIN
    assert max(lost) >= 10 * ADAMW_MARGIN


def test_guard_inputs_expose_apply():
    """The guard test's bad step through the same transcription with apply ignored: p, m and v all
    change bits (the NaN or Inf reaches them), so a kernel that ignores apply cannot keep them."""
    cfg = dict(CLIP_CFG, steps=1)
    p0, m0, v0, grads = adamw_inputs(cfg)
    for bad in (float("nan"), float("inf")):
        for spot in (0, 8, 12 + 250):
            g = grads[0][:263].copy()
            g[spot] = bad
            (p, m, v), = adamw_kernel_fp32(dict(cfg, grad_scale=1.0), p0[:263], m0[:263], v0[:263],
                                           [g * np.float32(cfg["grad_scale"])])
            assert p.tobytes() != p0[:263].tobytes() and not np.isfinite(m[spot]) and not np.isfinite(v[spot])


# ---------------------------------------------------------------------------------------------
# Argument contract
# ---------------------------------------------------------------------------------------------
ORDER = {
    "pis_grad_sumsq": ["g", "seg_off", "seg_len", "n_seg", "grad_scale", "max_norm", "flags", "seg_sumsq", "record",
                       "stats", "ws", "ws_bytes", "stream"],
    "pis_adamw_step_clipped": ["p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "step_size",
                               "bc2_sqrt", "grad_scale", "record", "stream"],
}
GOOD = {
    "pis_grad_sumsq": dict(g=A, seg_off=B_, seg_len=C_, n_seg=4, grad_scale=0.125, max_norm=1.0, flags=1,
                           seg_sumsq=D_, record=E_, stats=F_, ws=WS, ws_bytes=None, stream=0),  # None: the query
    "pis_adamw_step_clipped": dict(p=A, g=B_, m=C_, v=D_, n=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                                   weight_decay=1e-2, step_size=1e-3, bc2_sqrt=1.0, grad_scale=1.0, record=E_,
                                   stream=0),
}


def _invoke(lib, fn, changes):
    a = dict(GOOD[fn], **{k: v for k, v in changes.items() if k != "ws_short"})
    if a.get("ws_bytes", 0) is None:
        # the least any table of n_seg segments needs: all the host can check (the lengths are on the device)
        a["ws_bytes"] = lib.pis_grad_sumsq_ws(a["n_seg"], a["n_seg"]) - changes.get("ws_short", 0)
    return getattr(lib, fn)(*[a[k] for k in ORDER[fn]])


def _case(fn, **changes):
    return pytest.param(fn, changes, id=fn[4:] + "-" + "-".join(f"{k}={v}" for k, v in changes.items()))


BAD_CALLS = [
    _case("pis_grad_sumsq", g=0), _case("pis_grad_sumsq", seg_off=0), _case("pis_grad_sumsq", seg_len=0),
    _case("pis_grad_sumsq", seg_sumsq=0), _case("pis_grad_sumsq", record=0), _case("pis_grad_sumsq", stats=0),
    _case("pis_grad_sumsq", ws=0, ws_bytes=BIG),
    _case("pis_grad_sumsq", n_seg=0, ws_bytes=BIG), _case("pis_grad_sumsq", n_seg=-3, ws_bytes=BIG),
    _case("pis_grad_sumsq", g=A + OFF), _case("pis_grad_sumsq", ws=WS + OFF, ws_bytes=BIG),
    _case("pis_grad_sumsq", record=E_ + OFF), _case("pis_grad_sumsq", stats=F_ + OFF),
    _case("pis_grad_sumsq", seg_sumsq=D_ + OFF), _case("pis_grad_sumsq", seg_off=B_ + OFF),
    _case("pis_grad_sumsq", ws_short=1), _case("pis_grad_sumsq", ws_bytes=0),
    _case("pis_grad_sumsq", flags=2),
    _case("pis_adamw_step_clipped", p=0), _case("pis_adamw_step_clipped", g=0), _case("pis_adamw_step_clipped", m=0),
    _case("pis_adamw_step_clipped", v=0), _case("pis_adamw_step_clipped", record=0),
    _case("pis_adamw_step_clipped", n=-1),
    _case("pis_adamw_step_clipped", p=A + OFF), _case("pis_adamw_step_clipped", g=B_ + OFF),
    _case("pis_adamw_step_clipped", m=C_ + OFF), _case("pis_adamw_step_clipped", v=D_ + OFF),
    _case("pis_adamw_step_clipped", record=E_ + OFF),
]
LEGAL_CALLS = [
    _case("pis_grad_sumsq"), _case("pis_adamw_step_clipped"),
    _case("pis_grad_sumsq", max_norm=0.0, flags=0),   # telemetry only
    _case("pis_grad_sumsq", max_norm=-1.0),           # <= 0: no clipping
    _case("pis_grad_sumsq", n_seg=1), _case("pis_grad_sumsq", ws_bytes=BIG),
    _case("pis_grad_sumsq", g=A + 16),                # any 16-byte boundary
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
    rc = _invoke(hostlib, fn, changes)
    assert rc == PIS_ERR_LAUNCH, (rc, hostlib.pis_last_error())


def test_clipped_adamw_of_nothing_is_a_no_op(hostlib):
    assert _invoke(hostlib, "pis_adamw_step_clipped", dict(n=0)) == PIS_OK


@pytest.mark.parametrize("n_seg,n_total", [(0, 8), (-1, 8), (4, 3), (4, -1)])
def test_grad_sumsq_ws_rejects_bad_sizes(hostlib, n_seg, n_total):
    hostlib.pis_colsum(0, 0, 0, 0, 0, 0, 0, 0, 0)  # leaves another function's name in the message
    assert hostlib.pis_grad_sumsq_ws(n_seg, n_total) == 0
    assert b"pis_grad_sumsq_ws" in hostlib.pis_last_error()


def test_grad_sumsq_ws_size():
    """One float64 partial per (segment, 8192-float slice): at most n_seg + n_total / 8192 of them."""
    lib = _hip.lib()
    assert lib.pis_grad_sumsq_ws(4, 275) == 4 * 8
    assert lib.pis_grad_sumsq_ws(1, SLICE) == 2 * 8
    assert lib.pis_grad_sumsq_ws(46, 20_500_000) == (46 + 20_500_000 // SLICE) * 8
    for lens in ([1], [SLICE], [SLICE + 1, 3 * SLICE + 1], [7] * 300, [2 * SLICE - 1] * 5):
        items = sum(-(-n // SLICE) for n in lens)
        assert lib.pis_grad_sumsq_ws(len(lens), sum(lens)) >= items * 8


# ---------------------------------------------------------------------------------------------
# optim.AdamW arguments, CLI flags
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_adamw_rejects_bad_max_grad_norm(bad):
    from physics_informed_image_segmentation_amd import AdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        AdamW([torch.nn.Parameter(torch.zeros(4))], max_grad_norm=bad)


def test_adamw_options_are_attributes_not_group_entries():
    from physics_informed_image_segmentation_amd import AdamW
    plain = AdamW([torch.nn.Parameter(torch.zeros(4))])
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and not plain.norm_path
    opt = AdamW([torch.nn.Parameter(torch.zeros(4))], max_grad_norm=2.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True and opt.norm_path
    assert AdamW([torch.nn.Parameter(torch.zeros(4))], skip_nonfinite=True).norm_path
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])
    assert opt.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys()
    with pytest.raises(RuntimeError, match="grad_stats"):
        plain.grad_stats()


def test_cli_flags_default_off():
    sys.path.insert(0, ROOT)
    try:
        import main
        import run_ablation
    finally:
        sys.path.remove(ROOT)
    a = main.parse_args([])
    assert a.clip_grad_norm is None and a.skip_nonfinite is False
    a = main.parse_args(["--clip-grad-norm", "1.5", "--skip-nonfinite"])
    assert a.clip_grad_norm == 1.5 and a.skip_nonfinite is True
    a = run_ablation.parse_args(["--ablation", "R1"])
    assert a.clip_grad_norm is None and a.skip_nonfinite is False
    a = run_ablation.parse_args(["--ablation", "R1", "--clip-grad-norm", "0.25", "--skip-nonfinite"])
    assert a.clip_grad_norm == 0.25 and a.skip_nonfinite is True
    for mod in (main, run_ablation):
        with pytest.raises(SystemExit):
            mod.parse_args(["--ablation", "R1", "--clip-grad-norm", "0"] if mod is run_ablation
                           else ["--clip-grad-norm", "0"])
