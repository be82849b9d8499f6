"""First-order parameter sensitivity of a solution: how (x, y) moves with θ.

At a solution the KKT conditions hold for every θ nearby, so

    K · [dx; dy] = −[∇²ₓθL · δθ ; ∂c/∂θ · δθ],      L = obj_weight·f + yᵀc,

with K the KKT matrix the solver has already assembled and factorised on the device.  The right-hand side is two
matrix-free products of the model (``ExaModel.hpprod`` / ``ExaModel.jpprod``); nothing here forms a matrix."""
from __future__ import annotations


def parameter_step(model, kkt, x, y, dtheta, obj_weight: float = 1.0):
    """``(dx, dy)`` for the parameter change ``dtheta`` (length ``npar``) at the primal-dual point ``(x, y)``.

    ``kkt`` is an ASSEMBLED AND FACTORISED system at that point — ``kkt_chain.ChainKKT``, ``kkt_chain.HubChainKKT``,
    ``kkt.KKTSystem``, or anything else with ``solve(rhs)`` over ``nvar + ncon`` entries."""
    import torch
    n, mc = model.meta.nvar, model.meta.ncon
    rhs = torch.empty(n + mc, dtype=x.dtype, device=x.device)
    model.hpprod(x, y, dtheta, obj_weight=obj_weight, out=rhs[:n])
    model.jpprod(x, dtheta, out=rhs[n:])
    rhs.neg_()
    sol = kkt.solve(rhs)
    return sol[:n], sol[n:]
