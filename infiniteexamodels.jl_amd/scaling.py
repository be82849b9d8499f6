"""Gradient-based scaling of the NLP on the evaluator's own kernels.

Ipopt (``nlp_scaling_method = gradient-based``) and MadNLP (``scale_constraints!``) scale the problem they are handed: the
objective by ``min(1, max_gradient / ‖∇f(x0)‖∞)`` and every constraint row by ``min(1, max_gradient / max_j |∂c_r/∂x_j(x0)|)``,
then iterate on the scaled functions.  ``gradient_scaling`` computes the factors from ``grad`` and ``jac_row_maxabs`` alone —
no COO buffer, no structure download, no atomic scatter — and ``ScaledModel`` is the scaled problem behind the evaluation
surface of ``model.ExaModel``: ``cons`` and ``jac_coord`` come out of the scaled kernels (``cons_scaled`` /
``jac_coord_scaled``: the factor is applied in front of the store), the gradient and the Hessian out of ``grad_scaled`` (the
reverse sweep seeded with ``s_f``) and ``hess_coord_scaled`` (the row's multiplier ``y∘s`` formed in the kernel), and the
one-launch solver phases ``eval_trial`` / ``eval_accepted`` are the scaled phase kernels (``eval_trial_scaled`` /
``eval_accepted_scaled``): one launch per phase, as for the unscaled model.  A model that lacks the scaled gradient / Hessian
entry points (a host stand-in) gets the composed forms ``grad(x)·s_f`` and ``hess_coord(x, y∘s, obj_weight·s_f)``.

Not scaled here: the variables (x scaling).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


def gradient_scaling(model, x0, max_gradient: float = 100.0, min_value: float = 0.0):
    """``(obj_scale, con_scale)`` at the start point ``x0``: a float and a tensor of ``ncon`` factors on the model's device.

    ``obj_scale = min(1, max_gradient / ‖∇f(x0)‖∞)`` (1 where the gradient vanishes); ``con_scale[r] = max_gradient /
    rowmax[r]`` where the largest ``|∂c_r/∂x_j|`` of row ``r`` exceeds ``max_gradient``, else exactly 1.  Both are floored at
    ``min_value`` (Ipopt's ``nlp_scaling_min_value``; 0 = no floor)."""
    import torch
    g = model.grad(x0)
    gmax = float(g.abs().max().item()) if g.numel() else 0.0
    obj_scale = min(1.0, max_gradient / gmax) if gmax > 0.0 else 1.0
    m = int(model.meta.ncon)
    con_scale = torch.ones(m, dtype=torch.float64, device=model.device)
    if m and int(model.meta.nnzj):
        rowmax = model.jac_row_maxabs(x0)
        con_scale = torch.where(rowmax > max_gradient, max_gradient / rowmax, torch.ones_like(rowmax))
    if min_value > 0.0:
        obj_scale = max(obj_scale, float(min_value))
        con_scale = con_scale.clamp_min(float(min_value))
    return obj_scale, con_scale


class ScaledModel:
    """The problem ``min s_f·f(x)  s.t.  s∘lcon <= s∘c(x) <= s∘ucon`` behind the evaluation methods of ``ExaModel``.

    ``obj_scale`` is a float, ``con_scale`` a float64 tensor of ``ncon`` positive factors on the model's device.  Multipliers
    of the scaled problem go back to those of the model as stated through :meth:`unscale`."""

    def __init__(self, model, obj_scale: float, con_scale):
        self.inner, self.device = model, model.device
        self.obj_scale, self.con_scale = float(obj_scale), con_scale
        meta = model.meta
        if con_scale.numel() != int(meta.ncon):
            raise ValueError(f"con_scale must have ncon = {int(meta.ncon)} entries")
        s = con_scale.detach().cpu().numpy()
        fields = {k: getattr(meta, k) for k in ("nvar", "ncon", "npar", "nnzj", "nnzh", "x0", "lvar", "uvar", "y0", "n_templates", "n_kernels")
                  if hasattr(meta, k)}
        self.meta = SimpleNamespace(**fields, lcon=np.asarray(meta.lcon) * s, ucon=np.asarray(meta.ucon) * s,
                                    minimize=getattr(meta, "minimize", True))

    @classmethod
    def at(cls, model, x0, max_gradient: float = 100.0, min_value: float = 0.0):
        """The gradient-based scaling of ``model`` at ``x0`` (:func:`gradient_scaling`)."""
        return cls(model, *gradient_scaling(model, x0, max_gradient, min_value))

    # ---- evaluation ----------------------------------------------------------
    def obj(self, x) -> float:
        return self.obj_scale * self.inner.obj(x)

    def obj_device(self, x, out=None):
        return self.inner.obj_device(x, out).mul_(self.obj_scale)

    def grad(self, x, g=None):
        if hasattr(self.inner, "grad_scaled"):
            return self.inner.grad_scaled(x, self.obj_scale, g)
        return self.inner.grad(x, g).mul_(self.obj_scale)

    def cons(self, x, c=None):
        return self.inner.cons_scaled(x, self.con_scale, c)

    def jac_coord(self, x, vals=None):
        return self.inner.jac_coord_scaled(x, self.con_scale, vals)

    def hess_coord(self, x, y, vals=None, obj_weight: float = 1.0):
        if hasattr(self.inner, "hess_coord_scaled"):
            return self.inner.hess_coord_scaled(x, y, self.con_scale, vals, obj_weight=obj_weight * self.obj_scale)
        return self.inner.hess_coord(x, y * self.con_scale, vals, obj_weight=obj_weight * self.obj_scale)

    def eval_trial(self, x, c=None, defer_obj: bool = False):
        """``(s_f·f(x), s∘c(x))`` in ONE launch; ``defer_obj``: ``(None, c)`` at once, the model's ``obj_end`` collects the
        scaled value later."""
        return self.inner.eval_trial_scaled(x, self.con_scale, self.obj_scale, c, defer_obj)

    def eval_accepted(self, x, y, g=None, jac=None, hess=None, obj_weight: float = 1.0):
        """Gradient, Jacobian and Hessian of the scaled problem in ONE launch (``y``: the scaled problem's multipliers)."""
        return self.inner.eval_accepted_scaled(x, y, self.con_scale, self.obj_scale, g, jac, hess, obj_weight)

    def obj_end(self) -> float:
        return self.inner.obj_end()

    def jac_hess_coord(self, x, y, jac=None, hess=None, obj_weight: float = 1.0):
        return self.jac_coord(x, jac), self.hess_coord(x, y, hess, obj_weight)

    def jprod(self, x, v, Jv=None):
        return self.inner.jprod(x, v, Jv).mul_(self.con_scale)

    def jtprod(self, x, v, Jtv=None):
        return self.inner.jtprod(x, v * self.con_scale, Jtv)

    def hprod(self, x, y, v, Hv=None, obj_weight: float = 1.0):
        return self.inner.hprod(x, y * self.con_scale, v, Hv, obj_weight=obj_weight * self.obj_scale)

    def lagrangian_grad(self, x, y, obj_weight: float = 1.0, out=None):
        return self.inner.lagrangian_grad(x, y * self.con_scale if y is not None else None, obj_weight * self.obj_scale, out)

    # ---- structure (scaling does not move a position) -------------------------
    def jac_structure(self, base: int = 0):
        return self.inner.jac_structure(base)

    def hess_structure(self, base: int = 0):
        return self.inner.hess_structure(base)

    def jac_structure_device(self, base: int = 0):
        return self.inner.jac_structure_device(base)

    def hess_structure_device(self, base: int = 0):
        return self.inner.hess_structure_device(base)

    def unscale(self, y, zL, zU):
        """Multipliers of the scaled problem -> those of the model as stated."""
        return y * self.con_scale / self.obj_scale, zL / self.obj_scale, zU / self.obj_scale
