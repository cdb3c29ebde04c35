"""Decoupled AdamW of src/train.py:658-662 (``optim.AdamW(params, lr,
weight_decay=1e-5)``) as ONE HIP kernel launch over the U-Net's flat
parameter arena.

Semantics are torch.optim.AdamW's single-tensor path (torch/optim/adam.py):
p *= 1 - lr*wd; m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2;
p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps), scalars rounded to fp32 as torch
rounds its Python floats. ``grad_scale`` multiplies the gradient inside the
kernel (data-parallel averaging without an extra pass).

``max_grad_norm`` (global L2 clipping, the ``clip_grad_norm_`` formula) and
``skip_nonfinite`` (skip the step when the gradient norm is Inf or NaN) turn on
the norm path: one deterministic float64 sum of squares over the gradient arena
(``pis_grad_sumsq``) leaves the clip coefficient and the skip decision on the
device, and the AdamW launch (``pis_adamw_step_clipped``) reads them there. No
host synchronisation, no second pass, and the gradient arena is not rescaled:
``p.grad`` after ``step()`` still holds the unclipped gradients. The norm is
that of ``grad_scale * g``, the gradient AdamW applies. With clipping on and
the guard off a non-finite norm behaves as torch's formula does (coefficient 0
for Inf, NaN for NaN; the NaN reaches the weights). A skipped step still
advances the step counter and so the bias corrections: the kernel's scalars
are rounded on the host exactly as torch rounds its Python floats, which a
device-side count (a device ``pow``) could not promise bit for bit.

``ema_decay`` keeps an exponential moving average of the weights in one more
arena-sized array that the same launch reads and writes
(``pis_adamw_step_ema``): ``e += w_k (p_new - e)`` with ``w_k = 1 - d_k``,
``d_k = min(ema_decay, (1 + k) / (10 + k))`` (``ema_warmup``) or ``ema_decay``,
``k`` the optimizer's 1-based step count. A skipped step counts in ``k`` but
does not move the average. ``averaged_weights()`` exchanges the CONTENTS of the
parameter arena and the average (``pis_arena_exchange``), never pointers:
parameter views, the engine's filter-job tables and a captured ``StepGraph`` all
hold addresses. Data parallel needs no communication: every rank holds the same
weights, hence the same average. Off by default; with ``ema_decay=None`` the
launches are the ones above and no EMA state exists.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import _hip


class AdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, grad_scale: float = 1.0,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True):
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        if max_grad_norm is not None and not max_grad_norm > 0:  # <= 0 and NaN
            raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:  # NaN too
            raise ValueError(f"ema_decay must be in (0, 1) or None, got {ema_decay!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = ema_decay
        self.ema_warmup = bool(ema_warmup)
        self._averaged = False  # inside averaged_weights(): the arenas' contents are exchanged
        self._flat = {}  # group index -> (arena tensor, m, v, offsets) when every param views one arena

    # ---- arena discovery ------------------------------------------------------
    @staticmethod
    def _storage(t: torch.Tensor) -> Tuple[int, int]:
        s = t.untyped_storage()
        return s.data_ptr(), s.nbytes()

    def _flat_state(self, gi: int, group):
        params: List[torch.Tensor] = group["params"]
        key = (gi, params[0].untyped_storage().data_ptr())
        st = self._flat.get(gi)
        if st is not None and st["key"] == key:
            return st
        base, nbytes = self._storage(params[0])
        if any(self._storage(p) != (base, nbytes) for p in params):
            return None
        arena = torch.empty(0, dtype=torch.float32, device=params[0].device).set_(
            params[0].untyped_storage(), 0, (nbytes // 4,), (1,))
        offs = [(p.data_ptr() - base) // 4 for p in params]
        # adopt moments a previous (per-tensor or older) state may hold
        m = torch.zeros_like(arena)
        v = torch.zeros_like(arena)
        # the average starts from the weights (padding included: the exchange moves whole arenas)
        ema = arena.clone() if self.ema_decay is not None else None
        step = 0
        for p, o in zip(params, offs):
            s = self.state.get(p)
            if s and "exp_avg" in s and s["exp_avg"].data_ptr() != m.data_ptr() + 4 * o:
                m.narrow(0, o, p.numel()).copy_(s["exp_avg"].reshape(-1))
                v.narrow(0, o, p.numel()).copy_(s["exp_avg_sq"].reshape(-1))
                step = int(s.get("step", 0))
            if ema is not None and s and "ema" in s:
                ema.narrow(0, o, p.numel()).copy_(s["ema"].reshape(-1))
        for p, o in zip(params, offs):
            self.state[p] = {"step": torch.tensor(float(step)),
                             "exp_avg": m.narrow(0, o, p.numel()).view(p.shape) if p.is_contiguous()
                             else m.narrow(0, o, p.numel()),
                             "exp_avg_sq": v.narrow(0, o, p.numel()).view(p.shape) if p.is_contiguous()
                             else v.narrow(0, o, p.numel())}
            if ema is not None:
                self.state[p]["ema"] = ema.narrow(0, o, p.numel()).view(p.shape) if p.is_contiguous() \
                    else ema.narrow(0, o, p.numel())
        st = {"key": key, "arena": arena, "m": m, "v": v, "offs": offs, "step": step}
        if ema is not None:
            st["ema"] = ema
        self._flat[gi] = st
        return st

    # ---- step -----------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        if self._averaged:
            raise RuntimeError("AdamW.step inside averaged_weights(): the model holds the averaged weights")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"]]
            if not params:
                continue
            _hip.require_cuda(params[0], "AdamW.step")
            st = self._flat_state(gi, group)
            if st is None:
                raise NotImplementedError("AdamW (MI355X) expects the parameters of one UNet (a single arena)")
            with_grad = [p.grad is not None for p in params]
            if not any(with_grad):
                continue
            st["step"] += 1
            step = st["step"]
            for p in params:
                self.state[p]["step"].fill_(float(step))
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            bc1 = 1.0 - b1 ** step
            bc2 = 1.0 - b2 ** step
            step_size, bc2_sqrt = lr / bc1, bc2 ** 0.5
            arena, m, v, offs = st["arena"], st["m"], st["v"], st["offs"]
            g_flat = self._grad_arena(params, offs, arena)
            stream = _hip.stream_handle()
            ema = st.get("ema")
            w = self.ema_weight(step) if ema is not None else None
            if self.norm_path:
                if g_flat is None or not all(with_grad):
                    raise NotImplementedError(
                        "AdamW(max_grad_norm / skip_nonfinite) needs the flat path: every parameter with a "
                        ".grad that views one gradient arena at its parameter's offset")
                nb = self._norm_buffers(st, params)
                _hip.call("pis_grad_sumsq", g_flat.data_ptr(), nb["off"].data_ptr(), nb["len"].data_ptr(),
                          len(params), self.grad_scale, self.max_grad_norm or 0.0,
                          _hip.PIS_GRADNORM_SKIP_NONFINITE if self.skip_nonfinite else 0,
                          nb["sumsq"].data_ptr(), nb["record"].data_ptr(), nb["stats"].data_ptr(),
                          nb["ws"].data_ptr(), nb["ws"].numel(), stream)
                if ema is not None:
                    _hip.call("pis_adamw_step_ema", arena.data_ptr(), g_flat.data_ptr(), m.data_ptr(),
                              v.data_ptr(), ema.data_ptr(), arena.numel(), lr, b1, b2, eps, wd, step_size,
                              bc2_sqrt, self.grad_scale, w, nb["record"].data_ptr(), stream)
                    continue
                _hip.call("pis_adamw_step_clipped", arena.data_ptr(), g_flat.data_ptr(), m.data_ptr(),
                          v.data_ptr(), arena.numel(), lr, b1, b2, eps, wd, step_size, bc2_sqrt,
                          self.grad_scale, nb["record"].data_ptr(), stream)
                continue
            if g_flat is not None and all(with_grad):
                if ema is not None:
                    _hip.call("pis_adamw_step_ema", arena.data_ptr(), g_flat.data_ptr(), m.data_ptr(),
                              v.data_ptr(), ema.data_ptr(), arena.numel(), lr, b1, b2, eps, wd, step_size,
                              bc2_sqrt, self.grad_scale, w, 0, stream)
                    continue
                _hip.call("pis_adamw_step", arena.data_ptr(), g_flat.data_ptr(), m.data_ptr(), v.data_ptr(),
                          arena.numel(), lr, b1, b2, eps, wd, step_size, bc2_sqrt, self.grad_scale, stream)
                continue
            for p, o in zip(params, offs):  # per-tensor launches (params without grad are skipped, as torch)
                if p.grad is None:
                    continue
                g = p.grad
                if g.stride() != p.stride():
                    g = torch.empty_strided(p.shape, p.stride(), device=p.device).copy_(g)
                if ema is not None:  # a parameter without .grad keeps its slice of the average
                    _hip.call("pis_adamw_step_ema", p.data_ptr(), g.data_ptr(), m.data_ptr() + 4 * o,
                              v.data_ptr() + 4 * o, ema.data_ptr() + 4 * o, p.numel(), lr, b1, b2, eps, wd,
                              step_size, bc2_sqrt, self.grad_scale, w, 0, stream)
                    continue
                _hip.call("pis_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr() + 4 * o, v.data_ptr() + 4 * o,
                          p.numel(), lr, b1, b2, eps, wd, step_size, bc2_sqrt, self.grad_scale, stream)
        return loss

    # ---- exponential moving average of the weights -----------------------------
    def ema_weight(self, step: int) -> float:
        """The weight ``w_k = 1 - d_k`` of step number ``step`` (1-based, skipped steps counted), in
        float64: ``d_k = min(ema_decay, (1 + k) / (10 + k))`` with ``ema_warmup``, else ``ema_decay``."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weight: the optimizer was built without ema_decay")
        d = min(self.ema_decay, (1.0 + step) / (10.0 + step)) if self.ema_warmup else self.ema_decay
        return 1.0 - d

    def _ema_state(self, what: str):
        if self.ema_decay is None:
            raise RuntimeError(f"{what}: the optimizer was built without ema_decay")
        groups = [(gi, g) for gi, g in enumerate(self.param_groups) if g["params"]]
        if len(groups) != 1:
            raise RuntimeError(f"{what}: one parameter group expected")
        gi, group = groups[0]
        _hip.require_cuda(group["params"][0], what)
        st = self._flat_state(gi, group)
        if st is None:
            raise NotImplementedError("AdamW (MI355X) expects the parameters of one UNet (a single arena)")
        return st

    def ema_arena(self) -> torch.Tensor:
        """The flat average, laid out like the parameter arena (created from the current weights, or
        adopted from a loaded state, when no step has been taken yet). Inside ``averaged_weights()``
        the contents are exchanged: this tensor then holds the raw weights."""
        return self._ema_state("ema_arena")["ema"]

    def ema_state_dict(self, model: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """``model.state_dict()``'s keys and shapes with the averaged values, as fresh tensors (entries
        that do not live in the parameter arena are copied as they are)."""
        st = self._ema_state("ema_state_dict")
        arena = st["arena"]
        src = arena if self._averaged else st["ema"]  # exchanged: the arena holds the average
        base, nbytes = self._storage(arena)
        out = {}
        for k, t in model.state_dict().items():
            if t.is_cuda and self._storage(t) == (base, nbytes) and t.dtype == torch.float32:
                out[k] = torch.as_strided(src, t.shape, t.stride(), (t.data_ptr() - base) // 4).clone()
            else:
                out[k] = t.clone()
        return out

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the ``with`` body the model holds the averaged weights: one ``pis_arena_exchange``
        of the parameter arena with the average on entry, one on exit (also when the body raises).
        ``step()`` and a nested entry raise inside it. No host synchronisation: the launches queue on
        the current stream. Not to be issued between the begin and the end of a graph capture."""
        st = self._ema_state("averaged_weights")
        if self._averaged:
            raise RuntimeError("averaged_weights: already inside averaged_weights()")
        arena, ema = st["arena"], st["ema"]
        _hip.call("pis_arena_exchange", arena.data_ptr(), ema.data_ptr(), arena.numel(), _hip.stream_handle())
        self._averaged = True
        try:
            yield self
        finally:
            _hip.call("pis_arena_exchange", arena.data_ptr(), ema.data_ptr(), arena.numel(), _hip.stream_handle())
            self._averaged = False

    # ---- gradient norm, clipping, step guard -----------------------------------
    @property
    def norm_path(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _norm_buffers(self, st, params):
        """Segment table, record, statistics and workspace of one flat state, allocated once."""
        nb = st.get("norm")
        if nb is None:
            dev = st["arena"].device
            lens = [p.numel() for p in params]
            ws_bytes = _hip.lib().pis_grad_sumsq_ws(len(params), sum(lens))
            nb = {"off": torch.tensor(st["offs"], dtype=torch.int64, device=dev),
                  "len": torch.tensor(lens, dtype=torch.int64, device=dev),
                  "sumsq": torch.zeros(len(params), dtype=torch.float64, device=dev),
                  "record": torch.zeros(2, dtype=torch.float64, device=dev),  # {float coef; int apply; double norm}
                  "stats": torch.zeros(_hip.PIS_GRADNORM_NSTATS, dtype=torch.float64, device=dev),
                  "ws": torch.empty((ws_bytes + 15) // 16 * 16, dtype=torch.uint8, device=dev)}
            st["norm"] = nb
        return nb

    def _norm_state(self):
        if not self.norm_path:
            raise RuntimeError("grad_stats: the optimizer was built without max_grad_norm or skip_nonfinite")
        sts = [st for st in self._flat.values() if "norm" in st]
        if len(sts) != 1:
            raise RuntimeError("grad_stats: one parameter group that has taken a step is needed" if not sts
                               else "grad_stats: one parameter group expected")
        return sts[0]["norm"]

    def grad_stats(self) -> Dict[str, torch.Tensor]:
        """Device tensors of the last step and the running counters; reading them is the caller's
        synchronisation, producing them is none. ``total_norm`` (float64 scalar) and ``per_tensor_norm``
        (float64 [n_params], in ``params`` order) are norms of ``grad_scale * g``; ``clip_coef`` is the
        fp32 coefficient the update used; ``applied`` is 0 when the step was skipped. ``steps``,
        ``clipped_steps``, ``skipped_steps``, ``finite_steps``, ``norm_sum`` and ``norm_max`` count
        since the last ``pop_grad_stats()`` (sums and maximum over the steps with a finite norm)."""
        nb = self._norm_state()
        stats = nb["stats"]
        return {"total_norm": nb["record"][1].clone(),
                "clip_coef": nb["record"][:1].view(torch.float32)[0].clone(),
                "applied": nb["record"][:1].view(torch.int32)[1].clone(),
                "per_tensor_norm": nb["sumsq"].sqrt() * self.grad_scale,
                "steps": stats[0].clone(), "clipped_steps": stats[1].clone(), "skipped_steps": stats[2].clone(),
                "finite_steps": stats[3].clone(), "norm_sum": stats[4].clone(), "norm_max": stats[5].clone()}

    def pop_grad_stats(self) -> Dict[str, float]:
        """The counters and sums as Python numbers, zeroed afterwards: one host synchronisation, meant
        for the end of an epoch. Before the first step everything is 0."""
        if not any("norm" in st for st in self._flat.values()):
            if not self.norm_path:
                raise RuntimeError("pop_grad_stats: the optimizer was built without max_grad_norm or skip_nonfinite")
            vals = [0.0] * _hip.PIS_GRADNORM_NSTATS
        else:
            stats = self._norm_state()["stats"]
            vals = stats.tolist()
            stats.zero_()
        return {"steps": int(vals[0]), "clipped_steps": int(vals[1]), "skipped_steps": int(vals[2]),
                "finite_steps": int(vals[3]), "norm_sum": vals[4], "norm_max": vals[5], "last_norm": vals[6]}

    @staticmethod
    def _grad_arena(params, offs, arena) -> Optional[torch.Tensor]:
        """The flat gradient arena when every .grad views one storage at its parameter's offset."""
        g0 = params[0].grad
        if g0 is None:
            return None
        gs = g0.untyped_storage()
        if gs.nbytes() != arena.numel() * 4:
            return None
        gbase = gs.data_ptr()
        for p, o in zip(params, offs):
            if p.grad is None or p.grad.untyped_storage().data_ptr() != gbase or \
                    p.grad.data_ptr() != gbase + 4 * o or p.grad.stride() != p.stride():
                return None
        return torch.empty(0, dtype=torch.float32, device=arena.device).set_(gs, 0, (arena.numel(),), (1,))
