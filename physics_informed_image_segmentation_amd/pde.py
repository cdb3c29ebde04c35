"""PDE regularisation of src/pde.py on the MI355X kernel path.

``PDERegularization`` keeps the reference's constructor checks, buffers and
method names (src/pde.py:6-212). The two losses the training step uses,
``compute_loss`` (reaction-diffusion residual, :124-145) and
``compute_phase_field_loss`` (:180-212), are the fused HIP kernel. The
per-pixel field helpers (``compute_laplacian``, ``reaction_term``,
``compute_residual``, ``compute_gradient_magnitude``, :49-178) are one HIP
stencil kernel each way (``pis_pde_fields`` / ``pis_pde_fields_bwd``) and are
differentiable, like the reference's F.pad + F.conv2d compositions.

Running the PDE (no reference counterpart): ``evolve`` advances a probability map
under ``u_t = D lap(u) + k u (1 - u) (u - a) + mu (u0 - u)`` by explicit Euler steps
(``pis_pde_evolve``: several steps per launch inside LDS), ``energies`` gives the per-image
residual, phase-field energy and interface pixel count (``pis_pde_energies``). ``evolve_np`` and
``energies_np`` are their definitions of record in float32 numpy, operation for operation; the
kernels agree with them bit for bit (tests/test_evolve_gpu.py).

The PDE as a layer: ``unroll`` is ``evolve`` with a backward (``pis_pde_unroll_fwd`` /
``pis_pde_unroll_bwd``: checkpoints every Tb steps, one reverse launch per Tb steps), ``PDELayer`` and
``RefinedModel`` wrap it for training, and ``unroll_vjp_np`` is the backward's definition of record,
again agreeing bit for bit (tests/test_unroll_gpu.py).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _hip
from .fused import LossConfig, fused_loss

_LAP, _RES, _GM = 0, 1, 2


# the output tile of a pis_pde_evolve block and the legal values of its temporal block T
EVOLVE_TILE = (_hip.PIS_EVOLVE_TILE_H, _hip.PIS_EVOLVE_TILE_W)
EVOLVE_T_VALUES = (1, 2, 4, 8)
EVOLVE_MAX_STEPS, EVOLVE_MAX_SIDE = _hip.PIS_EVOLVE_MAX_STEPS, 4096
_f32 = np.float32
# the legal temporal blocks Tb of pis_pde_unroll_fwd / _bwd and the bound on their step count
UNROLL_TB_VALUES = (1, 2, 4)
UNROLL_MAX_STEPS = _hip.PIS_UNROLL_MAX_STEPS
# the order of the coefficients wherever five of them travel together: the device tensor of
# ``unroll(coef=...)``, the columns of ``unroll_coef_vjp_np`` and of pis_pde_unroll_bwd_dev's g_coef
COEF_NAMES = ("D", "k", "a", "mu", "dt")


def evolve_temporal_block(value: Optional[int] = None) -> int:
    """The steps one ``pis_pde_evolve`` launch advances (pis_tune key ``PIS_TUNE_EVOLVE_T``); with
    ``value`` (one of ``EVOLVE_T_VALUES``) it is set, and the previous value returned. Every value
    gives the same bits."""
    if value is not None and value not in EVOLVE_T_VALUES:
        raise ValueError(f"temporal block {value!r}: one of {EVOLVE_T_VALUES} is needed")
    return int(_hip.lib().pis_tune(_hip.PIS_TUNE_EVOLVE_T, -1 if value is None else int(value)))


def unroll_temporal_block(value: Optional[int] = None) -> int:
    """The steps one checkpoint of ``unroll`` spans and one reverse launch sweeps back (pis_tune key
    ``PIS_TUNE_UNROLL_TB``); with ``value`` (one of ``UNROLL_TB_VALUES``) it is set, and the previous
    value returned. Every value gives the same bits; a forward keeps the value it ran with for its
    backward."""
    if value is not None and value not in UNROLL_TB_VALUES:
        raise ValueError(f"temporal block {value!r}: one of {UNROLL_TB_VALUES} is needed")
    return int(_hip.lib().pis_tune(_hip.PIS_TUNE_UNROLL_TB, -1 if value is None else int(value)))


def _check_evolve(steps, D, k, a, mu, dt) -> Tuple[int, np.float32, np.float32, np.float32, np.float32, np.float32]:
    """The stability check of ``pis_pde_evolve``, on the float32 scalars it receives; fills in
    ``dt=None``. Raises ValueError."""
    if isinstance(steps, bool) or int(steps) != steps or not 0 <= int(steps) <= EVOLVE_MAX_STEPS:
        raise ValueError(f"steps = {steps!r}: an integer in [0, {EVOLVE_MAX_STEPS}] is needed")
    D, k, a, mu = _f32(D), _f32(k), _f32(a), _f32(mu)
    if not (D >= 0 and k >= 0 and mu >= 0):
        raise ValueError(f"D = {D}, k = {k}, mu = {mu}: none may be negative")
    if not 0 < a < 1:
        raise ValueError(f"a = {a}: the reaction threshold must lie in (0, 1)")
    rate = float(4.0 * float(D) + float(k) + float(mu))
    if dt is None:
        if rate <= 0:
            raise ValueError("dt=None needs 4 D + k + mu > 0")
        dt = _f32(0.5) / _f32(_f32(_f32(4) * D + k) + mu)  # half the monotonicity bound: a choice
    dt = _f32(dt)
    if not dt > 0:
        raise ValueError(f"dt = {dt}: a positive step is needed")
    if not float(dt) * rate <= 1.0:
        raise ValueError(f"dt (4 D + k + mu) = {float(dt) * rate:g} exceeds 1: the explicit step is not monotone "
                         f"(dt <= {1.0 / rate:g} is needed)")
    return int(steps), D, k, a, mu, dt


def _maps_np(u, what: str) -> np.ndarray:
    u = np.asarray(u)
    if u.dtype != np.float32:
        raise TypeError(f"{what}: float32 maps expected, got {u.dtype}")
    if u.ndim == 4 and u.shape[1] == 1:
        u = u[:, 0]
    if u.ndim != 3:
        raise ValueError(f"{what}: (B, H, W) or (B, 1, H, W) expected, got {u.shape}")
    if u.shape[0] < 1 or not (2 <= u.shape[1] <= EVOLVE_MAX_SIDE and 2 <= u.shape[2] <= EVOLVE_MAX_SIDE):
        raise ValueError(f"{what}: B >= 1 and 2 <= H, W <= {EVOLVE_MAX_SIDE} are needed, got {u.shape}")
    return u


def _neighbours_np(c: np.ndarray):
    p = np.pad(c, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    return p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]  # up, dn, lf, rt


def evolve_np(u, steps: int, D, k, a, mu=0.0, dt=None, clamp: bool = True, u0=None) -> np.ndarray:
    """The definition of ``evolve``: ``steps`` explicit Euler steps of
    ``u_t = D lap(u) + k u (1 - u) (u - a) + mu (u0 - u)`` on float32 maps ``u`` ((B, H, W) or
    (B, 1, H, W), H, W >= 2), every scalar a float32 and every operation rounded on its own. Per
    step, with ``c`` the current map and up / dn / lf / rt its reflect-padded neighbours::

        lap = ((up + dn) + (lf + rt)) - 4 c
        r   = (c (1 - c)) (c - a)
        t   = D lap;  t = t + k r;  if mu != 0: t = t + mu (u0 - c)
        c'  = c + dt t;  if clamp: c' = min(max(c', 0), 1)

    ``u0`` is the initial map unless given. The pairing ``(up + dn) + (lf + rt)`` is part of the
    definition: each pair commutes, so a step commutes bit for bit with an H flip, a W flip and a
    transpose. ``dt=None`` is ``float32(0.5) / float32(4 D + k + mu)``. Refused with ValueError:
    negative D, k or mu, ``a`` outside (0, 1), ``dt <= 0`` and ``dt (4 D + k + mu) > 1``; under
    that bound the update is monotone in every argument (f' >= -1 on [0, 1] for
    f = u (1 - u) (u - a)), so [0, 1] is invariant in exact arithmetic and ``clamp`` only removes
    rounding excursions."""
    steps, D, k, a, mu, dt = _check_evolve(steps, D, k, a, mu, dt)
    shape = np.shape(u)
    c = _maps_np(u, "evolve_np").copy()
    z = c if u0 is None else _maps_np(u0, "evolve_np: u0")
    if z.shape != c.shape:
        raise ValueError(f"evolve_np: u0 {z.shape} does not match u {c.shape}")
    z = z.copy()
    one, four, zero = _f32(1), _f32(4), _f32(0)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            up, dn, lf, rt = _neighbours_np(c)
            lap = ((up + dn) + (lf + rt)) - four * c
            r = (c * (one - c)) * (c - a)
            t = D * lap
            t = t + k * r
            if mu != 0:
                t = t + mu * (z - c)
            n = c + dt * t
            if clamp:
                n = np.where(n < zero, zero, n)
                n = np.where(n > one, one, n)
            c = n.astype(np.float32, copy=False)
    return c.reshape(shape)


def _check_unroll(steps, D, k, a, mu, dt):
    """``_check_evolve`` under the smaller step bound of the checkpointed path."""
    out = _check_evolve(steps, D, k, a, mu, dt)
    if out[0] > UNROLL_MAX_STEPS:
        raise ValueError(f"steps = {steps!r}: an integer in [0, {UNROLL_MAX_STEPS}] is needed (the checkpoint stack is "
                         "bounded)")
    return out


def _adjoint_weights_np(n: int) -> Tuple[np.ndarray, np.ndarray]:
    """The transpose of reflect padding along an axis of n >= 2 pixels: pixel i receives
    ``wa[i] q[i - 1] + wb[i] q[i + 1]``. wa = 0, 2, 1, 1, ... from the start, wb the same from the end."""
    wa, wb = np.ones(n, np.float32), np.ones(n, np.float32)
    wa[1], wb[n - 2] = 2, 2  # before the zeros: n = 2 gives wa = [0, 2], wb = [2, 0]
    wa[0], wb[n - 1] = 0, 0
    return wa, wb


def unroll_vjp_np(u, g_out, steps: int, D, k, a, mu=0.0, dt=None, clamp: bool = True, u0=None
                  ) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The definition of ``unroll``'s backward: the vector-Jacobian product of ``evolve_np`` (same
    arguments, ``steps <= UNROLL_MAX_STEPS``) with ``g_out``, the gradient with respect to the evolved
    map, in float32 with every operation rounded on its own. Returns ``(g_u, g_u0)``.

    The forward steps are ``evolve_np``'s; with ``c`` a step's input and ``n = c + dt t`` its update
    before the clamp, the reverse step takes ``g'`` (gradient w.r.t. the step's output) to ``g``::

        pass = not (n < 0) and not (n > 1)        # clamp off: everywhere; equality passes, as torch.clamp
        q    = pass ? g' : 0
        nb   = (fu + fd) + (fl + fr)
          fu = wa_H[y] q[y-1, x]     fd = wb_H[y] q[y+1, x]
          fl = wa_W[x] q[y, x-1]     fr = wb_W[x] q[y, x+1]
        rp   = ((1 - 2 c) (c - a)) + (c (1 - c))
        s    = k rp;  s = s - (4 D);  if mu != 0: s = s - mu
        d    = 1 + dt s
        g    = d q + (dt D) nb
        if mu != 0:  gz = gz + (dt mu) q          # one running float32 sum, in reverse step order

    A ``q`` outside the image is 0; ``wa``, ``wb`` are the transpose of reflect padding
    (``_adjoint_weights_np``); ``4 D``, ``dt D`` and ``dt mu`` are float32 products formed once. The
    pairing ``(fu + fd) + (fl + fr)`` makes the product commute bit for bit with an H flip, a W flip
    and a transpose, as the forward does. ``g_u0 = gz`` (zeros when ``mu == 0``). With ``u0=None``
    the initial map is its own ``u0``: ``g_u + gz`` (one add, made for ``mu == 0`` too) and ``None``
    are returned. ``steps == 0`` is the identity: ``g_out``'s bits, and zeros or ``None``."""
    steps, D, k, a, mu, dt = _check_unroll(steps, D, k, a, mu, dt)
    shape = np.shape(u)
    c = _maps_np(u, "unroll_vjp_np").copy()
    g = _maps_np(g_out, "unroll_vjp_np: g_out")
    if g.shape != c.shape:
        raise ValueError(f"unroll_vjp_np: g_out {g.shape} does not match u {c.shape}")
    g = g.copy()
    z = c if u0 is None else _maps_np(u0, "unroll_vjp_np: u0")
    if z.shape != c.shape:
        raise ValueError(f"unroll_vjp_np: u0 {z.shape} does not match u {c.shape}")
    z = z.copy()
    one, two, four, zero = _f32(1), _f32(2), _f32(4), _f32(0)
    four_d, dt_d, dt_mu = four * D, dt * D, dt * mu
    (wa_h, wb_h), (wa_w, wb_w) = _adjoint_weights_np(c.shape[1]), _adjoint_weights_np(c.shape[2])
    wa_h, wb_h = wa_h[None, :, None], wb_h[None, :, None]
    wa_w, wb_w = wa_w[None, None, :], wb_w[None, None, :]
    states, passes = [], []
    gz = np.zeros_like(c)
    with np.errstate(all="ignore"):
        for _ in range(steps):  # evolve_np's step, keeping its input and its pass mask
            up, dn, lf, rt = _neighbours_np(c)
            lap = ((up + dn) + (lf + rt)) - four * c
            r = (c * (one - c)) * (c - a)
            t = D * lap
            t = t + k * r
            if mu != 0:
                t = t + mu * (z - c)
            n = c + dt * t
            states.append(c)
            passes.append(~(n < zero) & ~(n > one) if clamp else None)
            if clamp:
                n = np.where(n < zero, zero, n)
                n = np.where(n > one, one, n)
            c = n.astype(np.float32, copy=False)
        for c, ok in zip(reversed(states), reversed(passes)):
            q = g if ok is None else np.where(ok, g, zero)
            p = np.pad(q, ((0, 0), (1, 1), (1, 1)))
            fu, fd = wa_h * p[:, :-2, 1:-1], wb_h * p[:, 2:, 1:-1]
            fl, fr = wa_w * p[:, 1:-1, :-2], wb_w * p[:, 1:-1, 2:]
            nb = (fu + fd) + (fl + fr)
            rp = ((one - two * c) * (c - a)) + (c * (one - c))
            s = k * rp
            s = s - four_d
            if mu != 0:
                s = s - mu
            d = one + dt * s
            g = d * q + dt_d * nb
            if mu != 0:
                gz = gz + dt_mu * q
            assert g.dtype == np.float32 and gz.dtype == np.float32
    if steps == 0:
        return g.reshape(shape), (None if u0 is None else gz.reshape(shape))
    if u0 is None:
        return (g + gz).reshape(shape), None
    return g.reshape(shape), gz.reshape(shape)


def unroll_coef_vjp_np(u, g_out, steps: int, D, k, a, mu=0.0, dt=None, clamp: bool = True, u0=None,
                       with_mu: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of ``unroll``'s gradient with respect to the coefficients: per image
    the derivative of ``sum(g_out * evolve_np(u, ...))`` with respect to D, k, a, mu and dt (columns in
    the order of ``COEF_NAMES``), the five taken as independent. Returns ``(sums, abs_sums)``, both
    (B, 5) float64. With ``c`` a step's input, ``lap``, ``r``, ``t`` as ``evolve_np`` forms them from
    it and ``q`` the masked incoming gradient of ``unroll_vjp_np``, the step adds per pixel, in float32
    with every operation rounded on its own::

        eD  = q * (dt * lap)
        ek  = q * (dt * r)                           r = (c (1 - c)) (c - a)
        ea  = q * (dt * (k * (0 - (c (1 - c)))))
        emu = q * (dt * (z - c))                     with the mu term only, else 0
        edt = q * t

    ``sums`` is the float64 sum of those float32 terms over all pixels and steps, ``abs_sums`` the
    float64 sum of their magnitudes: the order of the sum is not part of the definition, and two
    correct sums differ by at most ``H W steps 2^-53 abs_sums``. ``with_mu=None``: the mu term is
    present when ``mu != 0``, as in ``evolve_np``; ``with_mu=True`` keeps ``t = t + mu (z - c)`` and
    ``s = s - mu`` for ``mu == 0`` too (they add zeros), which is what the device path does when mu is
    learnable: the mu column is then the derivative at ``mu = 0``. Arguments are checked as
    ``unroll_vjp_np`` checks them; ``steps == 0`` gives zeros."""
    steps, D, k, a, mu, dt = _check_unroll(steps, D, k, a, mu, dt)
    c = _maps_np(u, "unroll_coef_vjp_np").copy()
    g = _maps_np(g_out, "unroll_coef_vjp_np: g_out")
    if g.shape != c.shape:
        raise ValueError(f"unroll_coef_vjp_np: g_out {g.shape} does not match u {c.shape}")
    g = g.copy()
    z = c if u0 is None else _maps_np(u0, "unroll_coef_vjp_np: u0")
    if z.shape != c.shape:
        raise ValueError(f"unroll_coef_vjp_np: u0 {z.shape} does not match u {c.shape}")
    z = z.copy()
    with_mu = bool(mu != 0) if with_mu is None else bool(with_mu)
    one, two, four, zero = _f32(1), _f32(2), _f32(4), _f32(0)
    four_d, dt_d = four * D, dt * D
    (wa_h, wb_h), (wa_w, wb_w) = _adjoint_weights_np(c.shape[1]), _adjoint_weights_np(c.shape[2])
    wa_h, wb_h = wa_h[None, :, None], wb_h[None, :, None]
    wa_w, wb_w = wa_w[None, None, :], wb_w[None, None, :]
    steps_kept = []
    sums, abs_sums = np.zeros((c.shape[0], 5)), np.zeros((c.shape[0], 5))
    with np.errstate(all="ignore"):
        for _ in range(steps):
            up, dn, lf, rt = _neighbours_np(c)
            lap = ((up + dn) + (lf + rt)) - four * c
            cc = c * (one - c)
            r = cc * (c - a)
            t = D * lap
            t = t + k * r
            if with_mu:
                t = t + mu * (z - c)
            n = c + dt * t
            steps_kept.append((c, lap, cc, r, t, ~(n < zero) & ~(n > one) if clamp else None))
            if clamp:
                n = np.where(n < zero, zero, n)
                n = np.where(n > one, one, n)
            c = n.astype(np.float32, copy=False)
        for c, lap, cc, r, t, ok in reversed(steps_kept):
            q = g if ok is None else np.where(ok, g, zero)
            terms = [q * (dt * lap), q * (dt * r), q * (dt * (k * (zero - cc))),
                     q * (dt * (z - c)) if with_mu else np.zeros_like(q), q * t]
            for i, e in enumerate(terms):
                assert e.dtype == np.float32
                e = e.astype(np.float64)
                sums[:, i] += e.sum(axis=(1, 2))
                abs_sums[:, i] += np.abs(e).sum(axis=(1, 2))
            p = np.pad(q, ((0, 0), (1, 1), (1, 1)))
            fu, fd = wa_h * p[:, :-2, 1:-1], wb_h * p[:, 2:, 1:-1]
            fl, fr = wa_w * p[:, 1:-1, :-2], wb_w * p[:, 1:-1, 2:]
            nb = (fu + fd) + (fl + fr)
            rp = ((one - two * c) * (c - a)) + (c * (one - c))
            s = k * rp
            s = s - four_d
            if with_mu:
                s = s - mu
            d = one + dt * s
            g = d * q + dt_d * nb
            assert g.dtype == np.float32
    return sums, abs_sums


def energies_np(u, D, a, eps) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of ``energies``: per image of float32 maps ``u``, ``(out (B, 2) float64,
    interface (B,) int64)`` with ``out[:, 0]`` the mean of ``double(res)^2``,
    ``res = D lap + (c (1 - c)) (c - a)``, ``out[:, 1]`` the mean of ``double(e)``,
    ``e = he (gx gx + gy gy) + ie ((c c) ((1 - c) (1 - c)))`` with ``gx = 0.5 (rt - lf)``,
    ``gy = 0.5 (dn - up)``, ``he = float32(eps) / 2``, ``ie = 1 / float32(eps)``, and ``interface``
    the count of pixels with ``float32(0.1) < c < float32(0.9)``. The field arithmetic is float32,
    every operation rounded on its own; the sums are float64."""
    D, a, eps = _f32(D), _f32(a), _f32(eps)
    if not (D >= 0 and 0 < a < 1 and eps > 0):
        raise ValueError(f"D = {D}, a = {a}, eps = {eps}: D >= 0, 0 < a < 1 and eps > 0 are needed")
    c = _maps_np(u, "energies_np")
    one, four, half = _f32(1), _f32(4), _f32(0.5)
    he, ie = eps / _f32(2), one / eps
    with np.errstate(all="ignore"):
        up, dn, lf, rt = _neighbours_np(c)
        lap = ((up + dn) + (lf + rt)) - four * c
        res = D * lap + (c * (one - c)) * (c - a)
        gx, gy = half * (rt - lf), half * (dn - up)
        g = gx * gx + gy * gy
        w = (c * c) * ((one - c) * (one - c))
        e = he * g + ie * w
        assert res.dtype == np.float32 and e.dtype == np.float32
        out = np.stack([(res.astype(np.float64) ** 2).mean(axis=(1, 2)), e.astype(np.float64).mean(axis=(1, 2))], axis=1)
        interface = ((c > _f32(0.1)) & (c < _f32(0.9))).sum(axis=(1, 2)).astype(np.int64)
    return out, interface


@dataclass(frozen=True)
class PDERefine:
    """The arguments of one ``evolve`` call: a preset for ``Predictor(refine=...)`` and
    ``evaluate_model(refine=...)``. ``dt=None``: ``float32(0.5) / float32(4 D + k + mu)``."""
    steps: int
    D: float
    k: float
    a: float
    mu: float = 0.0
    dt: Optional[float] = None
    clamp: bool = True

    def __post_init__(self):
        _check_evolve(self.steps, self.D, self.k, self.a, self.mu, self.dt)

    @classmethod
    def reaction_diffusion(cls, steps: int, diffusion_coeff: float = 1.0, reaction_threshold: float = 0.5,
                           mu: float = 0.0, dt: Optional[float] = None) -> "PDERefine":
        """``u_t = D lap(u) + u (1 - u) (u - a)``: the PDE whose residual the loss penalises
        (``PDERegularization.compute_loss``): D = ``diffusion_coeff``, k = 1, a = ``reaction_threshold``."""
        return cls(steps=steps, D=diffusion_coeff, k=1.0, a=reaction_threshold, mu=mu, dt=dt)

    @classmethod
    def phase_field(cls, steps: int, epsilon: float = 0.05, mu: float = 0.0, dt: Optional[float] = None
                    ) -> "PDERefine":
        """The Allen-Cahn flow of the phase-field energy ``(eps / 2) |grad u|^2 + (1 / eps) u^2 (1 - u)^2``:
        ``u_t = eps lap(u) - (1 / eps) 2 u (1 - u) (1 - 2 u) = eps lap(u) + (4 / eps) u (1 - u) (u - 1/2)``,
        so D = eps, k = 4 / eps, a = 1/2. It is discretised with the 5-point Laplacian and is therefore
        NOT the exact discrete gradient of the loss's energy, whose gradient term uses central
        differences (their adjoint is a wider, 2-pixel-stride Laplacian)."""
        if not epsilon > 0:
            raise ValueError("epsilon must be positive")
        return cls(steps=steps, D=epsilon, k=4.0 / epsilon, a=0.5, mu=mu, dt=dt)

    def kwargs(self) -> dict:
        return dict(steps=self.steps, D=self.D, k=self.k, a=self.a, mu=self.mu, dt=self.dt, clamp=self.clamp)


def add_refine_flags(ap, prefix: str = "refine"):
    """--refine and its parameters on an argparse parser: shared by predict.py and evaluate.py. With
    ``prefix="pde-layer"`` the same set as --pde-layer, --pde-layer-steps, ...: the PDE layer of
    training (main.py, run_ablation.py), whose steps are bounded by ``UNROLL_MAX_STEPS``."""
    f = f"--{prefix}"
    layer = prefix != "refine"
    ap.add_argument(f, choices=["rd", "pf"], default=None,
                    help=("train the PDE stage through K unrolled steps of a PDE on the predicted probabilities: "
                          if layer else "evolve the predicted probabilities under a PDE before the threshold: ") +
                         "rd = the "
                         "reaction-diffusion equation the loss penalises, pf = the Allen-Cahn flow of the "
                         "phase-field energy (default: off)")
    ap.add_argument(f"{f}-steps", type=int, default=None, metavar="N",
                    help=f"explicit time steps of {f}, 0..{UNROLL_MAX_STEPS if layer else EVOLVE_MAX_STEPS} "
                         f"(required with {f})")
    ap.add_argument(f"{f}-dt", type=float, default=None, metavar="F",
                    help=f"time step of {f} (default: half the stability bound 1 / (4 D + k + mu))")
    ap.add_argument(f"{f}-mu", type=float, default=0.0, metavar="F",
                    help=f"fidelity weight of {f}: pulls the evolved map back to the prediction (default: 0)")
    ap.add_argument(f"{f}-diffusion", type=float, default=1.0, metavar="F",
                    help=f"diffusion coefficient of {f} rd (default: 1.0)")
    ap.add_argument(f"{f}-threshold-a", type=float, default=0.5, metavar="F",
                    help=f"reaction threshold a of {f} rd, in (0, 1) (default: 0.5)")
    ap.add_argument(f"{f}-epsilon", type=float, default=0.05, metavar="F",
                    help=f"interface width of {f} pf (default: 0.05)")
    if not layer:
        ap.add_argument(f"{f}-file", default=None, metavar="PATH",
                        help="a PDERefine written as JSON (steps, D, k, a, mu, dt, clamp), such as the "
                             "output/pde_layer_<stamp>.json of a training run with learned coefficients, which the "
                             f"presets of {f} may not be able to express; exclusive with {f}")


def refine_from_file(path) -> "PDERefine":
    """The PDERefine a JSON file holds (the keys of ``PDERefine.kwargs()``). Raises ValueError."""
    import json
    try:
        with open(path) as fh:
            kw = json.load(fh)
        if not isinstance(kw, dict):
            raise ValueError("a JSON object is needed")
        return PDERefine(**kw)
    except (OSError, TypeError, json.JSONDecodeError) as e:
        raise ValueError(f"{path}: {e}") from e


def refine_from_args(ap, args, prefix: str = "refine"):
    """The PDERefine of the parsed --refine (or --``prefix``) flags, or None; a bad combination ends
    in ap.error."""
    f, dest = f"--{prefix}", prefix.replace("-", "_")
    get = lambda name: getattr(args, f"{dest}_{name}")  # noqa: E731
    kind, steps = getattr(args, dest), get("steps")
    path = getattr(args, f"{dest}_file", None)
    if path is not None:
        if kind is not None or steps is not None:
            ap.error(f"{f}-file holds the whole refinement: give it without {f} and {f}-steps")
        try:
            return refine_from_file(path)
        except ValueError as e:
            ap.error(f"{f}-file: {e}")
    if kind is None:
        if steps is not None:
            ap.error(f"{f}-steps needs {f} {{rd,pf}}")
        return None
    if steps is None:
        ap.error(f"{f} needs {f}-steps N")
    try:
        if prefix != "refine":
            _check_unroll(steps, 0.0, 1.0, 0.5, 0.0, None)  # the step bound of the layer
        if kind == "rd":
            return PDERefine.reaction_diffusion(steps, get("diffusion"), get("threshold_a"), mu=get("mu"), dt=get("dt"))
        return PDERefine.phase_field(steps, get("epsilon"), mu=get("mu"), dt=get("dt"))
    except ValueError as e:
        ap.error(f"{f}: {e}")


def add_learn_flags(ap):
    """--pde-layer-learn and --pde-layer-lr on a parser that has the --pde-layer set (main.py)."""
    ap.add_argument("--pde-layer-learn", nargs="+", default=None, metavar="NAME", choices=list(LEARNABLE_NAMES),
                    help="train these coefficients of --pde-layer with the weights, from the values the other "
                         f"--pde-layer flags give: any of {', '.join(LEARNABLE_NAMES)} (eps ties D and k as "
                         "--pde-layer pf does and excludes both; a coefficient that starts at 0 cannot be "
                         "learned). dt follows as the same fraction of the stability bound (default: off)")
    ap.add_argument("--pde-layer-lr", type=float, default=None, metavar="F",
                    help="learning rate of the coefficients' Adam (default: the stage's learning rate)")


def learn_from_args(ap, args, refine: Optional["PDERefine"]):
    """``(learn, lr)`` of the parsed --pde-layer-learn / --pde-layer-lr, ``(None, None)`` when off; a bad
    combination ends in ap.error."""
    learn, lr = args.pde_layer_learn, args.pde_layer_lr
    if learn is None:
        if lr is not None:
            ap.error("--pde-layer-lr needs --pde-layer-learn")
        return None, None
    if refine is None:
        ap.error("--pde-layer-learn needs --pde-layer {rd,pf}")
    if lr is not None and not lr > 0:
        ap.error("--pde-layer-lr must be positive")
    try:
        LearnablePDELayer(refine, learn=tuple(learn))
    except ValueError as e:
        ap.error(f"--pde-layer-learn: {e}")
    return tuple(learn), lr


def refine_flags(refine: "PDERefine", kind: Optional[str] = None, prefix: str = "refine") -> str:
    """The command-line flags (``add_refine_flags``) that rebuild ``refine``: as ``rd`` when
    ``k == 1``, as ``pf`` when ``D = eps, k = 4 / eps, a = 1/2`` for some eps, unless ``kind`` says
    which. Raises ValueError for a PDERefine neither preset gives."""
    f = f"--{prefix}"
    if kind is None:
        kind = "rd" if refine.k == 1.0 else "pf"
    if kind == "rd" and refine.k == 1.0:
        out = f"{f} rd {f}-steps {refine.steps} {f}-diffusion {refine.D!r} {f}-threshold-a {refine.a!r}"
    elif kind == "pf" and refine.D > 0 and refine.k == 4.0 / refine.D and refine.a == 0.5:
        out = f"{f} pf {f}-steps {refine.steps} {f}-epsilon {refine.D!r}"
    else:
        raise ValueError(f"{refine}: neither the rd nor the pf preset")
    if refine.mu:
        out += f" {f}-mu {refine.mu!r}"
    if refine.dt is not None:
        out += f" {f}-dt {refine.dt!r}"
    return out


def _maps_cuda(u: torch.Tensor, what: str) -> torch.Tensor:
    _hip.require_cuda(u, what)
    if u.dtype != torch.float32:
        raise TypeError(f"{what}: float32 maps expected, got {u.dtype}")
    if not (u.dim() == 3 or (u.dim() == 4 and u.shape[1] == 1)):
        raise ValueError(f"{what}: (B, H, W) or (B, 1, H, W) expected, got {tuple(u.shape)}")
    B, H, W = u.shape[0], u.shape[-2], u.shape[-1]
    if B < 1 or not (2 <= H <= EVOLVE_MAX_SIDE and 2 <= W <= EVOLVE_MAX_SIDE):
        raise ValueError(f"{what}: B >= 1 and 2 <= H, W <= {EVOLVE_MAX_SIDE} are needed, got {tuple(u.shape)}")
    return u.detach().contiguous()


def evolve(u: torch.Tensor, refine: Optional[PDERefine] = None, *, steps: Optional[int] = None, D=None, k=None,
           a=None, mu=0.0, dt=None, clamp: bool = True, u0: Optional[torch.Tensor] = None,
           threshold: Optional[float] = None) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``evolve_np`` on the GPU, bit for bit: ``u`` ((B, H, W) or (B, 1, H, W) float32 CUDA) advanced
    by ``steps`` explicit steps, either under a ``PDERefine`` or under ``steps, D, k, a[, mu, dt, clamp]``.
    Returns a new tensor of ``u``'s shape (``u`` is left unchanged), or ``(tensor, mask)`` when
    ``threshold`` is given: ``mask = (evolved > threshold)`` as uint8, written by the same launch.
    ``ceil(steps / T)`` launches on the current stream, no host synchronisation. NOT differentiable:
    the input is detached and no gradient flows to it. Bad arguments raise ValueError before any
    GPU work."""
    if refine is not None:
        if not isinstance(refine, PDERefine):
            raise TypeError(f"evolve: refine must be a PDERefine, got {type(refine).__name__}")
        if steps is not None or D is not None or k is not None or a is not None:
            raise ValueError("evolve: give a PDERefine or steps, D, k, a, not both")
        steps, D, k, a, mu, dt, clamp = (refine.steps, refine.D, refine.k, refine.a, refine.mu, refine.dt,
                                         refine.clamp)
    elif steps is None or D is None or k is None or a is None:
        raise ValueError("evolve: a PDERefine, or steps, D, k and a, are needed")
    steps, D, k, a, mu, dt = _check_evolve(steps, D, k, a, mu, dt)
    if threshold is not None and not float(threshold) == float(threshold):
        raise ValueError("evolve: threshold is NaN")
    uc = _maps_cuda(u, "evolve")
    B, H, W = uc.shape[0], uc.shape[-2], uc.shape[-1]
    z = None
    if u0 is not None:
        z = _maps_cuda(u0, "evolve: u0")
        if z.shape[0] != B or tuple(z.shape[-2:]) != (H, W) or z.device != uc.device:
            raise ValueError(f"evolve: u0 {tuple(u0.shape)} does not match u {tuple(u.shape)}")
    out = torch.empty_like(uc)
    mask = torch.empty(uc.shape, dtype=torch.uint8, device=uc.device) if threshold is not None else None
    with torch.cuda.device(uc.device):
        nbytes = int(_hip.lib().pis_pde_evolve_ws(B, H, W, steps))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=uc.device)
        f = ctypes.c_float
        _hip.call("pis_pde_evolve", _hip.ptr(uc), _hip.ptr(z), _hip.ptr(out), _hip.ptr(mask), B, H, W, f(D), f(k), f(a),
                  f(mu), f(dt), steps, _hip.PIS_EVOLVE_CLAMP if clamp else 0,
                  f(0.0 if threshold is None else float(threshold)), _hip.ptr(ws), nbytes,
                  _hip.stream_handle(uc.device))
    out = out.reshape(u.shape)
    return out if mask is None else (out, mask.reshape(u.shape))


class _Unroll(torch.autograd.Function):
    """``pis_pde_unroll_fwd`` and its reverse sweep ``pis_pde_unroll_bwd``; ``z`` is None when the
    input is its own u0. The scalars are float32 already (``_check_unroll``)."""

    @staticmethod
    def forward(ctx, u, z, steps, D, k, a, mu, dt, clamp):
        uc = _maps_cuda(u, "unroll")
        zc = None if z is None else _maps_cuda(z, "unroll: u0")
        B, H, W = uc.shape[0], uc.shape[-2], uc.shape[-1]
        flags = _hip.PIS_EVOLVE_CLAMP if clamp else 0
        f = ctypes.c_float
        out = torch.empty_like(uc)
        with torch.cuda.device(uc.device):
            tb = int(_hip.lib().pis_tune(_hip.PIS_TUNE_UNROLL_TB, -1))  # read once: the backward runs with this one
            nbytes = int(_hip.lib().pis_pde_unroll_ws(B, H, W, steps, tb))
            ckpt = torch.empty(nbytes, dtype=torch.uint8, device=uc.device) if nbytes else None
            _hip.call("pis_pde_unroll_fwd", _hip.ptr(uc), _hip.ptr(zc), _hip.ptr(out), _hip.ptr(ckpt), nbytes, B, H, W,
                      f(D), f(k), f(a), f(mu), f(dt), steps, flags, tb, _hip.stream_handle(uc.device))
        ctx.save_for_backward(uc, zc, ckpt)
        ctx.args = (B, H, W, D, k, a, mu, dt, steps, flags, tb)
        ctx.shapes = (u.shape, None if z is None else z.shape)
        return out.reshape(u.shape)

    @staticmethod
    def backward(ctx, g_out):
        uc, zc, ckpt = ctx.saved_tensors
        B, H, W, D, k, a, mu, dt, steps, flags, tb = ctx.args
        if g_out.dtype != torch.float32:
            raise TypeError(f"unroll: float32 gradient expected, got {g_out.dtype}")
        g = g_out.contiguous()
        g_u = torch.empty_like(uc)
        g_z = torch.empty_like(uc) if zc is not None and ctx.needs_input_grad[1] else None
        f = ctypes.c_float
        with torch.cuda.device(uc.device):
            nbytes = int(_hip.lib().pis_pde_unroll_bwd_ws(B, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=uc.device)
            _hip.call("pis_pde_unroll_bwd", _hip.ptr(uc), _hip.ptr(zc), _hip.ptr(ckpt), _hip.ptr(g), _hip.ptr(g_u),
                      _hip.ptr(g_z), B, H, W, f(D), f(k), f(a), f(mu), f(dt), steps, flags, tb, _hip.ptr(ws), nbytes,
                      _hip.stream_handle(uc.device))
        return (g_u.reshape(ctx.shapes[0]), None if g_z is None else g_z.reshape(ctx.shapes[1]),
                None, None, None, None, None, None, None)


class _UnrollDev(torch.autograd.Function):
    """``pis_pde_unroll_fwd_dev`` / ``pis_pde_unroll_bwd_dev``: ``_Unroll`` with the five coefficients
    in a (5,) float32 CUDA tensor (``COEF_NAMES`` order) that the kernels read, and its gradient when
    it requires one: the per-image table of the reverse sweep, summed over the batch in float64."""

    @staticmethod
    def forward(ctx, u, z, coef, steps, clamp, with_mu):
        uc = _maps_cuda(u, "unroll")
        zc = None if z is None else _maps_cuda(z, "unroll: u0")
        cc = coef.detach().contiguous()
        B, H, W = uc.shape[0], uc.shape[-2], uc.shape[-1]
        flags = (_hip.PIS_EVOLVE_CLAMP if clamp else 0) | (_hip.PIS_EVOLVE_MU if with_mu else 0)
        out = torch.empty_like(uc)
        with torch.cuda.device(uc.device):
            tb = int(_hip.lib().pis_tune(_hip.PIS_TUNE_UNROLL_TB, -1))  # read once: the backward runs with this one
            nbytes = int(_hip.lib().pis_pde_unroll_ws(B, H, W, steps, tb))
            ckpt = torch.empty(nbytes, dtype=torch.uint8, device=uc.device) if nbytes else None
            _hip.call("pis_pde_unroll_fwd_dev", _hip.ptr(uc), _hip.ptr(zc), _hip.ptr(out), _hip.ptr(ckpt), nbytes, B, H,
                      W, _hip.ptr(cc), steps, flags, tb, _hip.stream_handle(uc.device))
        ctx.save_for_backward(uc, zc, ckpt, cc)
        ctx.args = (B, H, W, steps, flags, tb)
        ctx.shapes = (u.shape, None if z is None else z.shape)
        return out.reshape(u.shape)

    @staticmethod
    def backward(ctx, g_out):
        uc, zc, ckpt, cc = ctx.saved_tensors
        B, H, W, steps, flags, tb = ctx.args
        if g_out.dtype != torch.float32:
            raise TypeError(f"unroll: float32 gradient expected, got {g_out.dtype}")
        g = g_out.contiguous()
        g_u = torch.empty_like(uc)
        g_z = torch.empty_like(uc) if zc is not None and ctx.needs_input_grad[1] else None
        table = torch.empty((B, len(COEF_NAMES)), dtype=torch.float64, device=uc.device) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(uc.device):
            nbytes = int(_hip.lib().pis_pde_unroll_bwd_dev_ws(B, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=uc.device)
            _hip.call("pis_pde_unroll_bwd_dev", _hip.ptr(uc), _hip.ptr(zc), _hip.ptr(ckpt), _hip.ptr(g), _hip.ptr(g_u),
                      _hip.ptr(g_z), _hip.ptr(table), B, H, W, _hip.ptr(cc), steps, flags, tb, _hip.ptr(ws), nbytes,
                      _hip.stream_handle(uc.device))
        return (g_u.reshape(ctx.shapes[0]), None if g_z is None else g_z.reshape(ctx.shapes[1]),
                None if table is None else table.sum(0).to(torch.float32), None, None, None)


def _unroll_dev(u, u0, coef, steps, clamp, with_mu, refine, scalars_given) -> torch.Tensor:
    """``unroll(coef=...)``: the argument checks, then ``_UnrollDev``."""
    if refine is not None or scalars_given:
        raise ValueError("unroll: coef stands in place of a PDERefine and of D, k, a, mu and dt: give steps, clamp and "
                         "with_mu beside it, nothing else")
    if not isinstance(with_mu, bool):
        raise ValueError("unroll: with coef, with_mu=True or False is needed: the host does not read mu")
    if steps is None or isinstance(steps, bool) or int(steps) != steps or not 0 <= int(steps) <= UNROLL_MAX_STEPS:
        raise ValueError(f"unroll: steps = {steps!r}: an integer in [0, {UNROLL_MAX_STEPS}] is needed")
    if not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32 or tuple(coef.shape) != (len(COEF_NAMES),):
        raise ValueError(f"unroll: coef must be a float32 tensor of shape ({len(COEF_NAMES)},): {', '.join(COEF_NAMES)}")
    _maps_cuda(u, "unroll")
    if coef.device != u.device:
        raise ValueError(f"unroll: coef on {coef.device}, u on {u.device}")
    if u0 is not None:
        _maps_cuda(u0, "unroll: u0")
        if u0.shape[0] != u.shape[0] or tuple(u0.shape[-2:]) != tuple(u.shape[-2:]) or u0.device != u.device:
            raise ValueError(f"unroll: u0 {tuple(u0.shape)} does not match u {tuple(u.shape)}")
    return _UnrollDev.apply(u, u0, coef, int(steps), bool(clamp), with_mu)


def unroll(u: torch.Tensor, refine: Optional[PDERefine] = None, *, steps: Optional[int] = None, D=None, k=None,
           a=None, mu=0.0, dt=None, clamp: bool = True, u0: Optional[torch.Tensor] = None,
           coef: Optional[torch.Tensor] = None, with_mu: Optional[bool] = None) -> torch.Tensor:
    """``evolve`` as a differentiable layer: the same arguments without ``threshold``,
    the same bits in the result, ``steps <= UNROLL_MAX_STEPS``, and gradients with respect to ``u``
    and ``u0``: ``unroll_vjp_np`` on the GPU, bit for bit. The forward keeps the state after every
    Tb-th step (``unroll_temporal_block``; ``ceil(steps / Tb) - 1`` maps beside ``u``), the backward
    is one launch per block of Tb steps, last block first, each recomputing its states inside LDS.
    With grad disabled, or when neither ``u`` nor ``u0`` requires grad, it is exactly one ``evolve``
    call and keeps nothing. Given as Python scalars or a PDERefine, the PDE's coefficients take no
    gradient. No host synchronisation; bad arguments raise ValueError before any GPU work.

    ``coef``: the five coefficients as a (5,) float32 CUDA tensor in ``COEF_NAMES`` order,
    in place of ``refine`` and of ``D, k, a, mu, dt``; ``steps``, ``clamp`` and ``with_mu`` (whether the
    ``mu (u0 - c)`` term is formed: the host never reads the tensor) stay host arguments. The kernels
    read the values from device memory (``pis_pde_unroll_fwd_dev`` / ``_bwd_dev``), the result and the
    gradients with respect to ``u`` and ``u0`` are those of the same float32 values given as scalars,
    bit for bit, and ``coef`` receives its gradient when it requires one: ``unroll_coef_vjp_np``'s
    sums over the batch, to the order of a float64 sum, bitwise reproducible. The VALUES ARE NOT
    CHECKED, which would be a host synchronisation: no value can fault a kernel, but values outside
    the ranges ``evolve_np`` refuses give a map without meaning. ``LearnablePDELayer`` builds them in
    range."""
    if coef is not None or with_mu is not None:
        if coef is None:
            raise ValueError("unroll: with_mu belongs to coef")
        return _unroll_dev(u, u0, coef, steps, clamp, with_mu, refine,
                           D is not None or k is not None or a is not None or mu != 0.0 or dt is not None)
    if refine is not None:
        if not isinstance(refine, PDERefine):
            raise TypeError(f"unroll: refine must be a PDERefine, got {type(refine).__name__}")
        if steps is not None or D is not None or k is not None or a is not None:
            raise ValueError("unroll: give a PDERefine or steps, D, k, a, not both")
        steps, D, k, a, mu, dt, clamp = (refine.steps, refine.D, refine.k, refine.a, refine.mu, refine.dt,
                                         refine.clamp)
    elif steps is None or D is None or k is None or a is None:
        raise ValueError("unroll: a PDERefine, or steps, D, k and a, are needed")
    steps, D, k, a, mu, dt = _check_unroll(steps, D, k, a, mu, dt)
    needs_grad = torch.is_grad_enabled() and (u.requires_grad or (u0 is not None and u0.requires_grad))
    if not needs_grad:
        return evolve(u, steps=steps, D=D, k=k, a=a, mu=mu, dt=dt, clamp=clamp, u0=u0)
    _maps_cuda(u, "unroll")
    if u0 is not None:
        _maps_cuda(u0, "unroll: u0")
        if u0.shape[0] != u.shape[0] or tuple(u0.shape[-2:]) != tuple(u.shape[-2:]) or u0.device != u.device:
            raise ValueError(f"unroll: u0 {tuple(u0.shape)} does not match u {tuple(u.shape)}")
    return _Unroll.apply(u, u0, steps, float(D), float(k), float(a), float(mu), float(dt), bool(clamp))


class PDELayer(nn.Module):
    """``unroll`` under a fixed ``PDERefine`` as a parameter-free module: ``forward(u) = unroll(u, refine)``."""

    def __init__(self, refine: PDERefine):
        super().__init__()
        if not isinstance(refine, PDERefine):
            raise TypeError(f"PDELayer: a PDERefine is needed, got {type(refine).__name__}")
        _check_unroll(refine.steps, refine.D, refine.k, refine.a, refine.mu, refine.dt)
        self.refine = refine

    def forward(self, u: torch.Tensor) -> torch.Tensor:
        return unroll(u, self.refine)

    def extra_repr(self) -> str:
        return repr(self.refine)


LEARNABLE_NAMES = ("D", "k", "a", "mu", "eps")
_THETA_MAX = 30.0          # exp(+-30) keeps every product finite and positive in float32
_LOGIT_MAX = 15.0          # sigmoid(+-15) is the last float32 strictly inside (0, 1) by a margin: 3.1e-7 from the ends
_STEP_FRACTION_MAX = float(_f32(1.0 - 2.0 ** -21))


class LearnablePDELayer(nn.Module):
    """``unroll`` whose coefficients are trained: ``forward(u) = unroll(u, coef=
    self.coefficients(), steps=refine.steps, clamp=refine.clamp, with_mu=refine.mu != 0)``.

    ``refine`` gives the initial values D0, k0, a0, mu0 and the step count; ``learn`` names what is
    trained, each name one 0-dim parameter ``theta[name]`` that starts at 0::

        D  = D0 exp(theta_D)      k = k0 exp(theta_k)      mu = mu0 exp(theta_mu)
        a  = sigmoid(logit(a0) + theta_a)
        "eps" (instead of "D" and "k"): D = D0 exp(theta_eps), k = k0 exp(-theta_eps), the tie of the
                  phase-field preset D = eps, k = 4 / eps
        dt = s / ((4 D + k) + mu)

    in torch float32 operations on the parameters' device, a coefficient that is not learned being its
    initial value. ``s`` is the fraction of the monotonicity bound the step keeps: ``step_fraction``
    (in (0, 1]) when given, else ``dt0 (4 D0 + k0 + mu0)`` when ``refine.dt`` is given, else 0.5, and
    at most ``1 - 2^-21``, so that the three float32 roundings of ``dt`` cannot carry
    ``dt (4 D + k + mu)`` past 1. ``theta`` enters through ``clamp(theta, -30, 30)`` and the logit
    through ``clamp(., -15, 15)`` (no gradient beyond), so D, k, mu stay positive and finite, ``a``
    strictly inside (0, 1) and ``dt`` positive: every reachable value passes ``_check_evolve``. THIS
    CONSTRUCTION IS THE RANGE CHECK OF THE DEVICE PATH, which makes none of its own.

    Autograd takes the kernel's five gradients back to ``theta``, the dependence of ``dt`` on D, k
    and mu included. ValueError: an unknown or repeated name, "eps" beside "D" or "k", a name whose
    initial value is 0 (its exponential form cannot leave 0), ``a0`` within 3.1e-7 of 0 or 1 when
    "a" is learned, ``4 D0 + k0 + mu0 = 0``, a ``step_fraction`` outside (0, 1]."""

    def __init__(self, refine: PDERefine, learn=("D", "k", "a"), step_fraction: Optional[float] = None):
        super().__init__()
        if not isinstance(refine, PDERefine):
            raise TypeError(f"LearnablePDELayer: a PDERefine is needed, got {type(refine).__name__}")
        steps, D0, k0, a0, mu0, dt0 = _check_unroll(refine.steps, refine.D, refine.k, refine.a, refine.mu, refine.dt)
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for name in learn:
            if name not in LEARNABLE_NAMES:
                raise ValueError(f"LearnablePDELayer: cannot learn {name!r}: one of {LEARNABLE_NAMES} is needed")
        if len(set(learn)) != len(learn) or not learn:
            raise ValueError(f"LearnablePDELayer: learn = {learn!r}: at least one name, each once, is needed")
        if "eps" in learn and ("D" in learn or "k" in learn):
            raise ValueError('LearnablePDELayer: "eps" ties D and k: it cannot stand beside "D" or "k"')
        zero = [n for n, v in (("D", D0), ("k", k0), ("mu", mu0)) if v == 0 and (n in learn or (n != "mu" and "eps" in learn))]
        if zero:
            raise ValueError(f"LearnablePDELayer: {zero} start at 0 and cannot be learned: D0 exp(theta) stays 0")
        rate0 = 4.0 * float(D0) + float(k0) + float(mu0)
        if not rate0 > 0:
            raise ValueError("LearnablePDELayer: 4 D + k + mu > 0 is needed")
        logit0 = float(np.log(float(a0)) - np.log1p(-float(a0)))
        if "a" in learn and abs(logit0) > _LOGIT_MAX:
            raise ValueError(f"LearnablePDELayer: a = {a0} is too close to 0 or 1 to be learned")
        if step_fraction is not None:
            if not 0 < float(step_fraction) <= 1:
                raise ValueError(f"LearnablePDELayer: step_fraction = {step_fraction!r}: (0, 1] is needed")
            s = float(step_fraction)
        else:
            s = 0.5 if refine.dt is None else float(dt0) * rate0
        self.refine, self.learn = refine, learn
        self.step_fraction = min(s, _STEP_FRACTION_MAX)
        self.with_mu = bool(mu0 != 0)
        self.theta = nn.ParameterDict({name: nn.Parameter(torch.zeros((), dtype=torch.float32)) for name in learn})
        # D0, k0, a0, mu0, logit(a0), s: device constants, so that coefficients() copies nothing from the host
        self.register_buffer("_init", torch.tensor([float(D0), float(k0), float(a0), float(mu0), logit0,
                                                    self.step_fraction], dtype=torch.float32), persistent=False)

    def _scale(self, name: str, sign: float = 1.0) -> torch.Tensor:
        return torch.exp(sign * self.theta[name].clamp(-_THETA_MAX, _THETA_MAX))

    def coefficients(self) -> torch.Tensor:
        """The (5,) float32 tensor D, k, a, mu, dt (``COEF_NAMES``) of the current parameters, on their
        device and attached to them. No host synchronisation."""
        D0, k0, a0, mu0, logit0, s = self._init.unbind(0)
        D, k, a, mu = D0, k0, a0, mu0
        if "eps" in self.learn:
            D, k = D0 * self._scale("eps"), k0 * self._scale("eps", -1.0)
        if "D" in self.learn:
            D = D0 * self._scale("D")
        if "k" in self.learn:
            k = k0 * self._scale("k")
        if "mu" in self.learn:
            mu = mu0 * self._scale("mu")
        if "a" in self.learn:
            a = torch.sigmoid((logit0 + self.theta["a"]).clamp(-_LOGIT_MAX, _LOGIT_MAX))
        dt = s / ((4.0 * D + k) + mu)  # _check_evolve's order
        return torch.stack([D, k, a, mu, dt])

    def snapshot(self) -> PDERefine:
        """The current coefficients as a PDERefine with a concrete ``dt`` (one device-to-host copy: a
        synchronisation; meant for the end of training and for logs)."""
        D, k, a, mu, dt = (float(v) for v in self.coefficients().detach().cpu().tolist())
        return PDERefine(steps=self.refine.steps, D=D, k=k, a=a, mu=mu, dt=dt, clamp=self.refine.clamp)

    def forward(self, u: torch.Tensor) -> torch.Tensor:
        return unroll(u, coef=self.coefficients(), steps=self.refine.steps, clamp=self.refine.clamp, with_mu=self.with_mu)

    def extra_repr(self) -> str:
        return f"{self.refine!r}, learn={self.learn!r}, step_fraction={self.step_fraction!r}"


class RefinedModel(nn.Module):
    """``forward(x) = PDELayer(refine)(model(x))``: the network whose output is the evolved map, so a
    loss on it reaches the weights through the unrolled steps. The U-Net stays reachable (and
    checkpointed) as ``.model``. There is deliberately no ``forward_with_loss``: the training loop
    then takes the two calls, the model and the criterion on the evolved map, and the fused
    head + loss path is left only while the layer is on. Given a ``LearnablePDELayer`` instead of a
    PDERefine, that module is the layer and its parameters are ``layer.theta.*``."""

    def __init__(self, model: nn.Module, refine: Union[PDERefine, "LearnablePDELayer"]):
        super().__init__()
        self.model = model
        self.layer = refine if isinstance(refine, LearnablePDELayer) else PDELayer(refine)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.layer(self.model(x))


def energies(u: torch.Tensor, D=1.0, a=0.5, eps=0.05) -> Tuple[torch.Tensor, torch.Tensor]:
    """``energies_np`` on the GPU: ``((B, 2) float64, (B,) int64)`` on ``u``'s device, column 0 the
    mean squared reaction-diffusion residual, column 1 the mean phase-field energy density, and
    the count of interface pixels (0.1 < u < 0.9). The per-pixel float32 values are the
    definition's; the float64 sums run in a fixed order (no atomics), so two runs give the same
    bits. One ``pis_pde_energies`` call, no host synchronisation. Not differentiable."""
    D, a, eps = _f32(D), _f32(a), _f32(eps)
    if not (D >= 0 and 0 < a < 1 and eps > 0):
        raise ValueError(f"D = {D}, a = {a}, eps = {eps}: D >= 0, 0 < a < 1 and eps > 0 are needed")
    uc = _maps_cuda(u, "energies")
    B, H, W = uc.shape[0], uc.shape[-2], uc.shape[-1]
    out = torch.empty((B, 2), dtype=torch.float64, device=uc.device)
    cnt = torch.empty((B,), dtype=torch.int64, device=uc.device)
    with torch.cuda.device(uc.device):
        nbytes = int(_hip.lib().pis_pde_energies_ws(B, H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=uc.device)
        f = ctypes.c_float
        _hip.call("pis_pde_energies", _hip.ptr(uc), B, H, W, f(D), f(a), f(eps), _hip.ptr(out), _hip.ptr(cnt),
                  _hip.ptr(ws), nbytes, _hip.stream_handle(uc.device))
    return out, cnt


class _PDEField(torch.autograd.Function):
    """One reflect-padded stencil field of u and its exact adjoint."""

    @staticmethod
    def forward(ctx, u, which: int, D: float, a: float):
        _hip.require_cuda(u, "PDERegularization")
        if u.dtype != torch.float32:
            raise TypeError("PDERegularization: float32 input expected")
        uc = u.detach().contiguous()
        B, H, W = uc.shape[0], uc.shape[-2], uc.shape[-1]
        if uc.numel() != B * H * W:
            raise ValueError(f"single-channel maps expected, got {tuple(u.shape)}")
        out = torch.empty_like(uc)
        ptrs = [0, 0, 0]
        ptrs[which] = out.data_ptr()
        _hip.call("pis_pde_fields", uc.data_ptr(), B, H, W, float(D), float(a), *ptrs, _hip.stream_handle())
        ctx.save_for_backward(uc)
        ctx.which, ctx.D, ctx.a = which, float(D), float(a)
        return out

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        B, H, W = u.shape[0], u.shape[-2], u.shape[-1]
        g = g.to(torch.float32).contiguous()
        ptrs = [0, 0, 0]
        ptrs[ctx.which] = g.data_ptr()
        du = torch.empty_like(u)
        _hip.call("pis_pde_fields_bwd", u.data_ptr(), *ptrs, B, H, W, ctx.D, ctx.a, du.data_ptr(),
                  _hip.stream_handle())
        return du, None, None, None


class PDERegularization(nn.Module):
    def __init__(self, diffusion_coeff: float = 1.0, reaction_threshold: float = 0.5):
        super().__init__()
        if diffusion_coeff <= 0:
            raise ValueError("diffusion_coeff must be positive")
        if not (0 < reaction_threshold < 1):
            raise ValueError("reaction_threshold must be in (0,1)")
        self.diffusion_coeff = diffusion_coeff
        self.reaction_threshold = reaction_threshold
        # stencil coefficients kept as buffers for state_dict compatibility (src/pde.py:24-47);
        # the kernels hard-code the same 5-point / central-difference taps
        lap = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]])
        gx = torch.tensor([[0.0, 0.0, 0.0], [-0.5, 0.0, 0.5], [0.0, 0.0, 0.0]])
        self.register_buffer("laplacian_kernel", lap[None, None].clone())
        self.register_buffer("grad_x_kernel", gx[None, None].clone())
        self.register_buffer("grad_y_kernel", gx.t()[None, None].contiguous())

    # ---- per-pixel fields (differentiable) ----------------------------------------
    def compute_laplacian(self, u: torch.Tensor) -> torch.Tensor:
        """5-point Laplacian with reflect padding (src/pde.py:49-79)."""
        return _PDEField.apply(u, _LAP, 0.0, 0.0)

    def reaction_term(self, u: torch.Tensor) -> torch.Tensor:
        """u (1 - u) (u - a) (src/pde.py:81-99): the residual with D = 0."""
        return _PDEField.apply(u, _RES, 0.0, self.reaction_threshold)

    def compute_residual(self, u: torch.Tensor) -> torch.Tensor:
        """D Lap(u) + u (1 - u) (u - a) (src/pde.py:101-122)."""
        return _PDEField.apply(u, _RES, self.diffusion_coeff, self.reaction_threshold)

    def compute_gradient_magnitude(self, u: torch.Tensor) -> torch.Tensor:
        """gx^2 + gy^2 of the reflect-padded central differences (src/pde.py:147-178)."""
        return _PDEField.apply(u, _GM, 0.0, 0.0)

    # ---- losses (fused kernel, differentiable) ----------------------------------
    def compute_loss(self, u: torch.Tensor) -> torch.Tensor:
        cfg = LossConfig(dice_w=0.0, bce_w=0.0, rd_w=1.0, pf_w=0.0, D=self.diffusion_coeff,
                         a=self.reaction_threshold)
        return fused_loss(u, u.detach(), cfg)

    def compute_phase_field_loss(self, u: torch.Tensor, epsilon: float = 0.05) -> torch.Tensor:
        if epsilon <= 0:
            raise ValueError("epsilon must be positive")
        cfg = LossConfig(dice_w=0.0, bce_w=0.0, rd_w=0.0, pf_w=1.0, eps=epsilon, D=self.diffusion_coeff,
                         a=self.reaction_threshold)
        return fused_loss(u, u.detach(), cfg)


    # ---- running the PDE, and its per-image quantities (not differentiable) ----
    def evolve(self, u: torch.Tensor, steps: int, dt: Optional[float] = None, mu: float = 0.0,
               u0: Optional[torch.Tensor] = None, threshold: Optional[float] = None):
        """``evolve`` under this module's PDE: D = ``diffusion_coeff``, k = 1, a = ``reaction_threshold``."""
        return evolve(u, steps=steps, D=self.diffusion_coeff, k=1.0, a=self.reaction_threshold, mu=mu, dt=dt, u0=u0,
                      threshold=threshold)

    def energies(self, u: torch.Tensor, epsilon: float = 0.05) -> Tuple[torch.Tensor, torch.Tensor]:
        """``energies`` with this module's D and a: per image, the quantities whose batch means are
        ``compute_loss`` and ``compute_phase_field_loss``, and the interface pixel count."""
        return energies(u, self.diffusion_coeff, self.reaction_threshold, epsilon)


def create_pde_regularization(diffusion_coeff: float = 1.0, reaction_threshold: float = 0.5) -> PDERegularization:
    """src/pde.py:215-232."""
    return PDERegularization(diffusion_coeff=diffusion_coeff, reaction_threshold=reaction_threshold)


__all__ = ["PDERegularization", "create_pde_regularization", "PDERefine", "evolve", "evolve_np", "energies",
           "energies_np", "evolve_temporal_block", "EVOLVE_TILE", "EVOLVE_T_VALUES", "add_refine_flags",
           "refine_from_args", "refine_flags", "unroll", "unroll_vjp_np", "unroll_temporal_block", "PDELayer",
           "RefinedModel", "UNROLL_TB_VALUES", "UNROLL_MAX_STEPS", "COEF_NAMES", "unroll_coef_vjp_np",
           "LearnablePDELayer", "refine_from_file", "LEARNABLE_NAMES",
           "add_learn_flags", "learn_from_args"]
