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


def parameter_steps(model, kkt, x, y, dthetas, obj_weight: float = 1.0):
    """``(dX, dY)``, shapes ``(nvar, K)`` and ``(ncon, K)``, for K parameter directions at once — the sensitivity matrix
    ``d(x, y)/dθ`` restricted to those directions.  ``dthetas`` is a ``(npar, K)`` tensor / array or a list of K directions
    of length ``npar``.  The right-hand sides are K pairs of matrix-free products into the columns of one buffer; the
    factorised system is then solved ONCE, with all K columns (``ChainKKT.solve`` reads its factors once per chunk of
    columns instead of once per column; every other ``kkt`` object loops)."""
    import torch
    n, mc = model.meta.nvar, model.meta.ncon
    if isinstance(dthetas, (list, tuple)):
        cols = [torch.as_tensor(d, dtype=x.dtype, device=x.device) for d in dthetas]
    else:
        D = torch.as_tensor(dthetas, dtype=x.dtype, device=x.device)
        if D.dim() != 2:
            raise ValueError("parameter_steps: dthetas must be (npar, K) or a list of K directions")
        cols = [D[:, j].contiguous() for j in range(D.shape[1])]
    K = len(cols)
    if K < 1:
        raise ValueError("parameter_steps: no direction")
    buf = torch.empty(K, n + mc, dtype=x.dtype, device=x.device)      # a direction per ROW: the products write contiguous slices
    for j, d in enumerate(cols):
        model.hpprod(x, y, d, obj_weight=obj_weight, out=buf[j, :n])
        model.jpprod(x, d, out=buf[j, n:])
    buf.neg_()
    sol = kkt.solve(buf.t())
    return sol[:n], sol[n:]
