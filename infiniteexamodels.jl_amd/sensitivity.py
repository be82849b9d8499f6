"""First-order parameter sensitivity of a solution: how (x, y) moves with θ.

At a solution the KKT conditions hold for every θ nearby, so

    K · [dx; dy] = −[∇²ₓθL · δθ ; ∂c/∂θ · δθ],      L = obj_weight·f + yᵀc,

with K the KKT matrix the solver has already assembled and factorised on the device.  The right-hand side is two
matrix-free products of the model (``ExaModel.hpprod`` / ``ExaModel.jpprod``); nothing here forms a matrix.

That is FORWARD mode: one solve per direction δθ.  The ADJOINT mode (``parameter_gradient(s)``) answers "how does one
quantity q of the solution react to every entry of θ" with one solve per quantity: with G = [∇²ₓθL ; ∂c/∂θ] the forward
step is [dx; dy] = −K⁻¹·G·δθ, so for g = [∂q/∂x; ∂q/∂y]

    dq/dθ = ∂q/∂θ + gᵀ·d[x; y]/dθ = ∂q/∂θ − Gᵀ·λ,      K·λ = g      (K symmetric),

and Gᵀ·λ = ``hptprod(x, y, λ_x)`` + ``jptprod(x, λ_y, obj_weight=0)`` — two matrix-free products again.

SECOND ORDER: the value function φ(θ) = L(x*(θ), y*(θ), θ) an outer problem optimises (parameter estimation, MPC tuning,
bilevel design).  At a KKT point its gradient is the partial one (envelope theorem): φ'(θ) = ``jptprod(x*, y*, σ)``
(``value_gradient``).  Differentiating once more along δθ, with [dx; dy] = −K⁻¹·G·δθ the forward step,

    φ''(θ)·δθ = L_θθ·δθ + Gᵀ·[dx; dy] = (L_θθ − Gᵀ·K⁻¹·G)·δθ
              = ``hppprod(x, y, δθ)`` + ``hptprod(x, y, dx)`` + ``jptprod(x, dy, obj_weight=0)``

(``value_hessian_product(s)``): one solve and three matrix-free products per direction.

THE FULL SENSITIVITY MATRIX over chosen entries of θ (``parameter_jacobian``): for unit directions the right-hand side of
the forward step is just ``−G[:, cols]``.  With G in COO (``ExaModel.hessp_coord`` / ``jacp_coord``: two launches, whatever K
is) the K columns are ONE deterministic segmented gather from a plan built once per ``(model, cols)`` — no product per
column, no loop over K on the host."""
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


class ParameterJacobianPlan:
    """Host-built gather plan of ``parameter_jacobian`` for one ``(model, theta_cols)``.

    The COO values of ``G = [∇²ₓθL ; ∂c/∂θ]`` live in ONE buffer — the ``nnz(Hxθ)`` values of ``hessp_coord`` first, the
    ``nnz(Jθ)`` values of ``jacp_coord`` behind them.  Every entry whose θ column is ``theta_cols[k]`` goes to position
    ``k·(nvar + ncon) + row`` (rows of Jθ behind those of Hxθ) of a ``(K, nvar + ncon)`` right-hand side: the selected
    entries are sorted by that destination — stable, so duplicates of a position keep their COO order — and ``dest``
    (the distinct destinations, ascending), ``seg`` (``len(dest) + 1`` boundaries) and ``perm`` (COO positions) are the
    ``seg`` / ``perm`` shape ``csr.build_plan`` makes and ``iem_csr_values`` consumes.  An index may repeat in
    ``theta_cols``: its column is produced once per occurrence."""

    def __init__(self, struct_xp, struct_jp, nvar: int, ncon: int, npar: int, theta_cols):
        import numpy as np
        cols = np.asarray(theta_cols)
        if cols.ndim != 1 or cols.size == 0:
            raise ValueError("parameter_jacobian: theta_cols must be a non-empty list of indices into θ")
        if not np.issubdtype(cols.dtype, np.integer):
            raise TypeError("parameter_jacobian: theta_cols must be integers")
        if cols.min() < 0 or cols.max() >= npar:
            raise IndexError(f"parameter_jacobian: theta_cols must lie in 0 .. {npar - 1}")
        (xr, xc), (jr, jc) = struct_xp, struct_jp
        self.nvar, self.ncon, self.K = int(nvar), int(ncon), int(cols.size)
        self.n_xp, self.n_jp = int(len(xr)), int(len(jr))
        rows = np.concatenate([np.asarray(xr, dtype=np.int64), np.asarray(jr, dtype=np.int64) + nvar])
        tcol = np.concatenate([np.asarray(xc, dtype=np.int64), np.asarray(jc, dtype=np.int64)])
        # the occurrences k of every θ index, ascending: entries fan out to each of them
        order = np.argsort(cols, kind="stable")
        first = np.searchsorted(cols[order], tcol, side="left")
        count = np.searchsorted(cols[order], tcol, side="right") - first
        pos = np.repeat(np.arange(rows.size, dtype=np.int64), count)
        within = np.arange(pos.size, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
        k = order[np.repeat(first, count) + within]
        dest = k.astype(np.int64) * (nvar + ncon) + rows[pos]
        by_dest = np.argsort(dest, kind="stable")
        sdest = dest[by_dest]
        self.perm = pos[by_dest]
        start = np.flatnonzero(np.concatenate([[True], sdest[1:] != sdest[:-1]])) if sdest.size else np.zeros(0, dtype=np.int64)
        self.dest = sdest[start].astype(np.int64)
        self.seg = np.concatenate([start, [sdest.size]]).astype(np.int64)
        self._dev = {}

    def on(self, device):
        """(dest, seg, perm) as int64 tensors on ``device`` (uploaded once)"""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.as_tensor(a, dtype=torch.int64).to(device) for a in (self.dest, self.seg, self.perm))
        return self._dev[key]

    def rhs(self, model, vals):
        """``−G[:, cols]`` as a ``(K, nvar + ncon)`` tensor from the COO buffer ``vals``: one segmented gather (fixed
        summation order, no atomics), negated, into zeros.  Device values go through ``iem_csr_values``; host tensors —
        a device-free model — through the same sums in the same order."""
        import torch
        dest, seg, perm = self.on(vals.device)
        buf = torch.zeros(self.K, self.nvar + self.ncon, dtype=vals.dtype, device=vals.device)
        n = int(dest.numel())
        if n == 0:
            return buf
        compact = torch.empty(n, dtype=vals.dtype, device=vals.device)
        if vals.is_cuda:
            from . import lib as _lib
            model._sync_stream()
            _lib.check(model._L.iem_csr_values(model._h, n, seg.data_ptr(), perm.data_ptr(), vals.data_ptr(), compact.data_ptr()))
        else:
            compact.zero_()
            compact.index_add_(0, torch.repeat_interleave(torch.arange(n), seg[1:] - seg[:-1]), vals[perm])
        buf.view(-1).index_copy_(0, dest, compact.neg_())
        return buf


def parameter_jacobian_plan(model, theta_cols) -> ParameterJacobianPlan:
    """The plan of ``parameter_jacobian`` for ``theta_cols``, built once per ``(model, theta_cols)`` and kept on the model."""
    import numpy as np
    cols = np.asarray(theta_cols)
    key = (cols.dtype.kind, tuple(cols.reshape(-1).tolist()))
    plans = model.__dict__.setdefault("_parameter_jacobian_plans", {})
    if key not in plans:
        plans[key] = ParameterJacobianPlan(model.hessxp_structure(), model.jacp_structure(), model.meta.nvar, model.meta.ncon,
                                           model.meta.npar, cols)
    return plans[key]


def parameter_jacobian(model, kkt, x, y, theta_cols, obj_weight: float = 1.0):
    """``(dX, dY)``, shapes ``(nvar, K)`` and ``(ncon, K)``: the columns of the sensitivity matrix ``d(x, y)/dθ`` for the K
    entries ``theta_cols`` of θ (indices into θ; ``ExaTranscriptionBackend.parameter_columns(p)`` has those of a parameter)
    at the primal-dual point ``(x, y)`` — what ``parameter_steps`` returns for the K unit directions, sign convention
    included (``K·[dx; dy] = −G·e_k``), from TWO launches and ONE gather instead of 2·K products and K copies:

        vals = [hessp_coord(x, y) ; jacp_coord(x)]      (G in COO)
        rhs  = −gather(plan, vals)                       (``(K, nvar + ncon)``, zeros where G has no entry)
        sol  = kkt.solve(rhsᵀ)                           (one solve with the 2-D right-hand side)

    ``kkt`` is an ASSEMBLED AND FACTORISED system at that point, as for ``parameter_step``."""
    import torch
    n = model.meta.nvar
    plan = parameter_jacobian_plan(model, theta_cols)
    vals = torch.empty(plan.n_xp + plan.n_jp, dtype=x.dtype, device=x.device)
    model.hessp_coord(x, y, obj_weight=obj_weight, vals_xp=vals[:plan.n_xp], vals_pp=False)      # (∂²L/∂θ² is not wanted here)
    model.jacp_coord(x, vals=vals[plan.n_xp:])
    sol = kkt.solve(plan.rhs(model, vals).t())
    return sol[:n], sol[n:]


def parameter_gradient(model, kkt, x, y, gx, gy=None, obj_weight: float = 1.0, dq_dtheta=None):
    """Total derivative ``dq/dθ`` (length ``npar``) of a quantity ``q(x, y, θ)`` of the solution at the primal-dual point
    ``(x, y)``, from ONE solve: ``gx = ∂q/∂x`` (length ``nvar``), ``gy = ∂q/∂y`` (length ``ncon``, ``None`` = zeros) and
    ``dq_dtheta = ∂q/∂θ`` at fixed ``(x, y)`` (``None`` = zeros).

    Sign convention: the one of ``parameter_step`` — ``K·[dx; dy] = −G·δθ`` with ``G = [∇²ₓθL ; ∂c/∂θ]`` — so that
    ``parameter_gradient(…)·δθ == ∂q/∂θ·δθ + gx·dx + gy·dy`` for the ``(dx, dy)`` of ``parameter_step(δθ)``:

        λ = kkt.solve([gx; gy]),      result = dq_dtheta − (hptprod(x, y, λ_x) + jptprod(x, λ_y, obj_weight=0)).

    ``kkt`` is an ASSEMBLED AND FACTORISED system at that point, as for ``parameter_step``; the formula solves with K where
    the derivation has Kᵀ, so K MUST BE THE SYMMETRIC SYSTEM the solver factorised (``[H + Σ + δw·I, Jᵀ; J, −δc·I]`` — what
    ``kkt.KKTSystem`` assembles and the chain solvers factorise), not an unsymmetric reduction of it."""
    import torch
    n, mc = model.meta.nvar, model.meta.ncon
    g = torch.zeros(n + mc, dtype=x.dtype, device=x.device)
    g[:n].copy_(torch.as_tensor(gx, dtype=x.dtype, device=x.device))
    if gy is not None:
        g[n:].copy_(torch.as_tensor(gy, dtype=x.dtype, device=x.device))
    lam = kkt.solve(g)
    out = model.hptprod(x, y, lam[:n].contiguous(), obj_weight=obj_weight)
    out += model.jptprod(x, lam[n:].contiguous(), obj_weight=0.0)
    out.neg_()
    if dq_dtheta is not None:
        out += torch.as_tensor(dq_dtheta, dtype=x.dtype, device=x.device)
    return out


def parameter_gradients(model, kkt, x, y, G, obj_weight: float = 1.0, dq_dtheta=None):
    """``(npar, K)``: ``parameter_gradient`` of K quantities at once.  ``G`` has shape ``(nvar + ncon, K)``, column j =
    ``[∂q_j/∂x; ∂q_j/∂y]``; ``dq_dtheta`` is ``None`` (zeros) or ``(npar, K)``.  The factorised system is solved ONCE with
    the 2-D right-hand side (``ChainKKT.solve`` reads its factors once per chunk of columns), then K pairs of matrix-free
    products write the rows of one buffer.  Sign convention and the symmetry K must have: see ``parameter_gradient``."""
    import torch
    n, mc, npar = model.meta.nvar, model.meta.ncon, model.meta.npar
    G = torch.as_tensor(G, dtype=x.dtype, device=x.device)
    if G.dim() != 2 or G.shape[0] != n + mc:
        raise ValueError("parameter_gradients: G must be (nvar + ncon, K)")
    K = G.shape[1]
    if K < 1:
        raise ValueError("parameter_gradients: no column")
    lam = kkt.solve(G).t().contiguous()          # a quantity per ROW: the products read contiguous slices
    buf = torch.empty(K, npar, dtype=x.dtype, device=x.device)
    tmp = torch.empty(npar, dtype=x.dtype, device=x.device)
    for j in range(K):
        model.hptprod(x, y, lam[j, :n], obj_weight=obj_weight, out=buf[j])
        model.jptprod(x, lam[j, n:], obj_weight=0.0, out=tmp)
        buf[j] += tmp
    buf.neg_()
    out = buf.t()
    if dq_dtheta is not None:
        out = out + torch.as_tensor(dq_dtheta, dtype=x.dtype, device=x.device)
    return out


def value_gradient(model, x, y, obj_weight: float = 1.0):
    """Gradient (length ``npar``) of the value function ``φ(θ) = L(x*(θ), y*(θ), θ)``, ``L = obj_weight·f + yᵀc``: an alias
    for ``model.jptprod(x, y, obj_weight)``.  That is the envelope theorem — the terms through ``dx*/dθ`` and ``dy*/dθ``
    vanish because ``∇ₓL = 0`` and ``c = 0`` — so it is the gradient of φ ONLY AT A KKT POINT ``(x*, y*)``; anywhere else
    it is just the partial derivative ``∂L/∂θ``."""
    return model.jptprod(x, y, obj_weight=obj_weight)


def value_hessian_product(model, kkt, x, y, dtheta, obj_weight: float = 1.0):
    """``φ''(θ)·dtheta`` (length ``npar``) for the value function ``φ(θ) = L(x*(θ), y*(θ), θ)`` at the KKT point ``(x, y)``:
    one ``parameter_step`` (ONE solve), then

        hppprod(x, y, dtheta) + hptprod(x, y, dx) + jptprod(x, dy, obj_weight=0).

    Sign convention: the one of ``parameter_step`` — ``K·[dx; dy] = −G·δθ`` with ``G = [∇²ₓθL ; ∂c/∂θ]`` — so the result is
    ``(L_θθ − Gᵀ·K⁻¹·G)·δθ``.  It is exactly that ONLY FOR THE K THAT WAS FACTORISED: the regularisation (δw, δc) and the
    barrier term Σ the solver put into ``kkt`` are part of it.  With the unregularised K of the reduced problem it is the
    Hessian of φ; with what an interior-point iteration left behind it is that of the barrier problem's regularised model.
    K must be the symmetric system (see ``parameter_gradient``) for the result to be symmetric in δθ."""
    dtheta = _as(dtheta, x)
    dx, dy = parameter_step(model, kkt, x, y, dtheta, obj_weight=obj_weight)
    out = model.hppprod(x, y, dtheta, obj_weight=obj_weight)
    out += model.hptprod(x, y, dx.contiguous(), obj_weight=obj_weight)
    out += model.jptprod(x, dy.contiguous(), obj_weight=0.0)
    return out


def value_hessian_products(model, kkt, x, y, dthetas, obj_weight: float = 1.0):
    """``(npar, K)``: ``value_hessian_product`` for K directions at once.  ``dthetas`` is what ``parameter_steps`` takes
    (``(npar, K)`` or a list of K directions); the factorised system is solved ONCE with the 2-D right-hand side, then K
    triples of matrix-free products write the rows of one buffer.  Exact only for the K that was factorised — its
    regularisation and Σ are part of the result; see ``value_hessian_product``."""
    import torch
    n, npar = model.meta.nvar, model.meta.npar
    if isinstance(dthetas, (list, tuple)):
        cols = [_as(d, x) for d in dthetas]
    else:
        D = _as(dthetas, x)
        if D.dim() != 2:
            raise ValueError("value_hessian_products: dthetas must be (npar, K) or a list of K directions")
        cols = [D[:, j].contiguous() for j in range(D.shape[1])]
    dX, dY = parameter_steps(model, kkt, x, y, cols, obj_weight=obj_weight)
    dX, dY = dX.t().contiguous(), dY.t().contiguous()      # a direction per ROW: the products read contiguous slices
    buf = torch.empty(len(cols), npar, dtype=x.dtype, device=x.device)
    tmp = torch.empty(npar, dtype=x.dtype, device=x.device)
    for j, d in enumerate(cols):
        model.hppprod(x, y, d, obj_weight=obj_weight, out=buf[j])
        model.hptprod(x, y, dX[j], obj_weight=obj_weight, out=tmp)
        buf[j] += tmp
        model.jptprod(x, dY[j], obj_weight=0.0, out=tmp)
        buf[j] += tmp
    return buf.t()


def _as(v, like):
    import torch
    return torch.as_tensor(v, dtype=like.dtype, device=like.device)
