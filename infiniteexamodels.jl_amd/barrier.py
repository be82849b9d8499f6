"""The interior-point barrier layer of the C-ABI (``iem_barrier_*``, ``csrc/iem_barrier_device.h``) held from Python: what a
primal-dual interior-point method computes between the evaluation calls and the KKT solver object — the barrier diagonal ``Σ``,
``Σs⁻¹``, the condensed right-hand side, the slack and bound-multiplier directions, the fraction-to-the-boundary step lengths, the
update with the multiplier safeguard, Ipopt's error terms — one launch per call, every scalar on the device.

Formulation (``include/iem.h`` has the per-entry contract): ``∇f + Jᵀy − zL + zU = 0``; rows with ``lcon == ucon`` are equalities,
every other row has an eliminated slack ``s``.  All vectors are full length: ``x, zL, zU`` have ``nvar`` entries, ``s, vL, vU`` (and
``ds, dvL, dvU``) have ``ncon`` entries of which those on equality rows are never read and never written.

    with BarrierLayer(model) as bar:
        state = bar.start(x0, model.cons(x0))                      # (x, s, y, zL, zU, vL, vU)
        _, c, r = model.eval_residual(state[0], state[2])
        sigma, dcon, rhs = bar.terms(state, r, c, mu)              # -> KKTObject.assemble(..., sigma, dw, dc, dcon=dcon), solve(rhs)
        dirs, alpha = bar.step(state, sol, mu, tau)                # (ds, dzL, dzU, dvL, dvU), device tensor of two
        bar.update(state, sol, dirs, alpha, mu)                    # in place
        out = bar.error(state, r, c, mu)                           # device tensor of eight

Nothing above reads a value back; :meth:`BarrierLayer.optimality_error` is the only place that does."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import lib as _lib

STATE = ("x", "s", "y", "zL", "zU", "vL", "vU")
DIRECTIONS = ("ds", "dzL", "dzU", "dvL", "dvU")


class BarrierLayer:
    """``BarrierLayer(model, relax=1e-8, bounds=None)``: ``bounds = (lvar, uvar, lcon, ucon)`` host arrays, any of them ``None`` for
    the model's own (a scaled solver passes its scaled row bounds).  Tensors are contiguous float64 CUDA tensors of the model's
    device; every method takes ``out=`` and allocates what is not given."""

    def __init__(self, model, relax: float = 1e-8, bounds=None):
        import torch
        self._torch = torch
        self.model = model
        self.nvar, self.ncon = int(model.meta.nvar), int(model.meta.ncon)
        self.n = self.nvar + self.ncon
        self._b = None
        arrs = []
        for a, n in zip(bounds if bounds is not None else (None,) * 4, (self.nvar, self.nvar, self.ncon, self.ncon)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (n,):
                    raise ValueError(f"bounds: an array of {n} entries expected, got shape {a.shape}")
            arrs.append(a)
        b = C.c_void_p()
        _lib.check(model._L.iem_barrier_create(model._h, *[a.ctypes.data if a is not None else None for a in arrs], float(relax), C.byref(b)))
        self._b = b
        info = _lib.BarrierInfo()
        info.struct_size = C.sizeof(_lib.BarrierInfo)
        _lib.check(model._L.iem_barrier_info(b, C.byref(info)))
        self.info = {name: int(getattr(info, name)) for name, _ in _lib.BarrierInfo._fields_ if name != "struct_size"}
        self.relax = float(relax)

    # ---- plumbing ----------------------------------------------------------------------------------------------
    def _handle(self):
        if self._b is None:
            raise _lib.IemError("BarrierLayer: closed")
        self.model._sync_stream()
        return self.model._L, self._b

    def _vec(self, t, n: int, name: str, optional: bool = False):
        if t is None:
            if optional or n == 0:
                return None
            raise ValueError(f"{name} is missing")
        self.model._chk(t, n, name)
        return C.c_void_p(t.data_ptr())

    def _state(self, state):
        if len(state) != 7:
            raise ValueError("state: (x, s, y, zL, zU, vL, vU)")
        sizes = (self.nvar, self.ncon, self.ncon, self.nvar, self.nvar, self.ncon, self.ncon)
        slack = self.info["n_ineq"] == 0
        return [self._vec(t, n, name, optional=slack and name in ("s", "vL", "vU")) for t, n, name in zip(state, sizes, STATE)]

    def _dirs(self, dirs):
        if len(dirs) != 5:
            raise ValueError("dirs: (ds, dzL, dzU, dvL, dvU)")
        sizes = (self.ncon, self.nvar, self.nvar, self.ncon, self.ncon)
        slack = self.info["n_ineq"] == 0
        return [self._vec(t, n, name, optional=slack and name in ("ds", "dvL", "dvU")) for t, n, name in zip(dirs, sizes, DIRECTIONS)]

    def _new(self, n: int):
        return self.model._new(n)

    # ---- the six calls -----------------------------------------------------------------------------------------
    def start(self, x, c, y=None, bound_push: float = 1e-2, bound_frac: float = 1e-2, out=None):
        """Ipopt's ``bound_push`` / ``bound_frac`` projection (``iem_barrier_start``): ``x`` is projected IN PLACE, ``s`` is the
        projection of ``c`` on inequality rows, the bound multipliers are 1 where their bound is present.  Returns the state
        ``(x, s, y, zL, zU, vL, vU)``; ``y`` (default: zeros) is passed through; ``out = (s, zL, zU, vL, vU)`` to reuse buffers.
        Entries of ``s, vL, vU`` on equality rows keep what the buffer held."""
        s, zL, zU, vL, vU = out if out is not None else (self._new(self.ncon), self._new(self.nvar), self._new(self.nvar), self._new(self.ncon), self._new(self.ncon))
        y = y if y is not None else self._torch.zeros(self.ncon, dtype=self._torch.float64, device=self.model.device)
        state = (x, s, y, zL, zU, vL, vU)
        p = self._state(state)
        pc = self._vec(c, self.ncon, "c")
        L, b = self._handle()
        _lib.check(L.iem_barrier_start(b, p[0], pc, p[1], p[3], p[4], p[5], p[6], float(bound_push), float(bound_frac)))
        return state

    def terms(self, state, r, c, mu: float, out=None):
        """``(sigma, dcon, rhs)`` (``iem_barrier_terms``): exactly the inputs of ``iem_kkt_assemble_diag`` /
        ``iem_kkt_solve_refined_diag``.  ``r = obj_weight·∇f + Jᵀy`` and ``c`` are what ``ExaModel.eval_residual`` writes."""
        sigma, dcon, rhs = out if out is not None else (self._new(self.nvar), self._new(self.ncon), self._new(self.n))
        p = self._state(state)
        args = (self._vec(r, self.nvar, "r"), self._vec(c, self.ncon, "c"), float(mu), self._vec(sigma, self.nvar, "sigma"), self._vec(dcon, self.ncon, "dcon"),
                self._vec(rhs, self.n, "rhs"))
        L, b = self._handle()
        _lib.check(L.iem_barrier_terms(b, *p, *args))
        return sigma, dcon, rhs

    def step(self, state, sol, mu: float, tau: float, out=None, alpha=None):
        """``((ds, dzL, dzU, dvL, dvU), alpha)`` from ``sol = [dx; dy]`` (``iem_barrier_step``).  ``alpha``: a DEVICE tensor
        ``(alpha_primal, alpha_dual)``; ``+0.0`` means the state or the direction was unusable."""
        dirs = out if out is not None else (self._new(self.ncon), self._new(self.nvar), self._new(self.nvar), self._new(self.ncon), self._new(self.ncon))
        alpha = alpha if alpha is not None else self._new(2)
        p, d = self._state(state), self._dirs(dirs)
        ps, pa = self._vec(sol, self.n, "sol"), self._vec(alpha, 2, "alpha")
        L, b = self._handle()
        _lib.check(L.iem_barrier_step(b, *p, ps, float(mu), float(tau), *d, pa))
        return dirs, alpha

    def update(self, state, sol, dirs, alpha, mu: float, kappa_sigma: float = 1e10):
        """The accepted step IN PLACE with the step lengths read from the device tensor ``alpha``, then the safeguard of the bound
        multipliers with the new gaps (``iem_barrier_update``).  A step length of ``+0.0`` moves nothing.  Returns ``state``."""
        p, d = self._state(state), self._dirs(dirs)
        ps, pa = self._vec(sol, self.n, "sol"), self._vec(alpha, 2, "alpha")
        L, b = self._handle()
        _lib.check(L.iem_barrier_update(b, *p, ps, *d, pa, float(mu), float(kappa_sigma)))
        return state

    def error(self, state, r, c, mu: float = 0.0, out=None):
        """The eight numbers of ``iem_barrier_error`` as a device tensor: max |r − zL + zU|, max |−y − vL + vU|, max |infeasibility|,
        max |gap·z − mu|, Σ|y|, Σ multipliers, θ = Σ|infeasibility|, Σ log gap.  ``r = None``: entry 0 is NaN."""
        out = out if out is not None else self._new(8)
        p = self._state(state)
        args = (self._vec(r, self.nvar, "r", optional=True), self._vec(c, self.ncon, "c"), float(mu), self._vec(out, 8, "out"))
        L, b = self._handle()
        _lib.check(L.iem_barrier_error(b, *p, *args))
        return out

    def merit(self, x, s, c, out=None):
        """``(θ, Σ log gap)`` at a trial point as a device tensor (``iem_barrier_merit``): the bits of ``error``'s entries 6, 7."""
        out = out if out is not None else self._new(2)
        args = (self._vec(x, self.nvar, "x"), self._vec(s, self.ncon, "s", optional=self.info["n_ineq"] == 0), self._vec(c, self.ncon, "c"), self._vec(out, 2, "out"))
        L, b = self._handle()
        _lib.check(L.iem_barrier_merit(b, *args))
        return out

    def bind_mu(self, param=None):
        """While bound to a :class:`BarrierParameter` (``iem_barrier_bind_mu``), :meth:`terms`, :meth:`step`, :meth:`update` and
        :meth:`error` read ``mu`` (and ``step`` its ``tau``) from the parameter's block on the device; their ``mu`` / ``tau``
        arguments are ignored.  ``None`` unbinds."""
        L, b = self._handle()
        _lib.check(L.iem_barrier_bind_mu(b, param._handle()[1] if param is not None else None))

    # ---- the one read-back -------------------------------------------------------------------------------------
    @staticmethod
    def optimality_error(out, mu_counts):
        """Ipopt's scaled optimality error ``E_μ`` from the eight numbers of :meth:`error` (a tensor: THIS is the read-back; or a
        sequence of floats) and the static counts ``mu_counts = (ncon, nz)`` (``info["ncon"]``, ``info["nz"]``):
        ``s_d = max(100, (Σ|y| + Σz)/(ncon + nz))/100``, ``s_c = max(100, Σz/nz)/100`` and
        ``(max(e_d, e_p, e_c), e_d, e_p, e_c)`` with ``e_d = max(out[0], out[1])/s_d``, ``e_p = out[2]``, ``e_c = out[3]/s_c``."""
        v = [float(a) for a in (out.tolist() if hasattr(out, "tolist") else out)]
        m, nz = int(mu_counts[0]), int(mu_counts[1])
        sd = max(100.0, (v[4] + v[5]) / max(1, m + nz)) / 100.0
        sc = max(100.0, v[5] / max(1, nz)) / 100.0
        ed = max(v[0], v[1]) / sd
        ep = v[2] if m else 0.0
        ec = v[3] / sc if nz else 0.0
        return max(ed, ep, ec), ed, ep, ec

    # ---- lifetime ----------------------------------------------------------------------------------------------
    def close(self):
        if self._b is not None:
            _lib.check(self.model._L.iem_barrier_destroy(self._b))
            self._b = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if getattr(self.model, "_h", None):
                self.close()
        except Exception:
            pass


class FilterSearch:
    """``FilterSearch(layer, **opts)``: the filter line search of the C-ABI (``iem_search_*``, ``csrc/iem_search_device.h``) beside a
    :class:`BarrierLayer` — the filter and a control block of sixteen words on the device, three one-launch calls, no read-back but
    :meth:`state`.  ``opts``: ``gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, alpha_floor, max_trials, filter_capacity``
    (Ipopt's defaults).  One rung of the ladder, with ``xt, st, ct, ft, m`` buffers of the caller:

        fs.begin(state, g, sol, dirs[0], obj, err, alpha, mu)          # obj: device tensor of one, err: bar.error(...) at this point
        fs.trial(state, sol, dirs[0], xt, st)
        model.obj_device(xt, out=ft); model.cons(xt, out=ct); bar.merit(xt, st, ct, out=m)
        fs.accept(ft, m, mu, alpha)                                    # alpha[0]: the accepted step length, or +0.0
        bar.update(state, sol, dirs, alpha, mu)

    Once a rung accepts, later rungs recompute the same trial point and change nothing; a search without a step leaves ``alpha[0] =
    +0.0``, for which ``update`` moves nothing.  ``reset()`` whenever ``mu`` changes."""

    def __init__(self, layer: BarrierLayer, **opts):
        self.layer = layer
        self._s = None
        o = _lib.SearchOpts.defaults(**opts)
        self.opts = {name: getattr(o, name) for name, _ in _lib.SearchOpts._fields_ if name != "struct_size"}
        L, b = layer._handle()
        s = C.c_void_p()
        _lib.check(L.iem_search_create(b, C.byref(o), C.byref(s)))
        self._s = s

    def _handle(self):
        if self._s is None:
            raise _lib.IemError("FilterSearch: closed")
        L, _ = self.layer._handle()
        return L, self._s

    def begin(self, state, grad, sol, ds, obj, err, alpha, mu: float, obj_weight: float = 1.0):
        """The slope of the barrier objective along ``sol = [dx; dy]``, ``ds`` and the control block of a new search
        (``iem_search_begin``): ``obj`` a device tensor of one (``f``), ``err`` the eight numbers of ``BarrierLayer.error`` at this
        point, ``alpha`` the device tensor of ``BarrierLayer.step``."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(grad, bar.nvar, "grad"), bar._vec(sol, bar.n, "sol"),
                bar._vec(ds, bar.ncon, "ds", optional=slack), bar._vec(obj, 1, "obj"), bar._vec(err, 8, "err"), bar._vec(alpha, 2, "alpha"))
        L, s = self._handle()
        _lib.check(L.iem_search_begin(s, *args, float(mu), float(obj_weight)))

    def trial(self, state, sol, ds, xt=None, st=None):
        """``(xt, st) = (x + α·dx, s + α·ds)`` with the block's ``α`` (``iem_search_trial``); entries of ``st`` on equality rows keep
        what the buffer held; nothing is stored once the search has failed."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        xt = xt if xt is not None else bar._new(bar.nvar)
        st = st if st is not None else bar._new(bar.ncon)
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(sol, bar.n, "sol"),
                bar._vec(ds, bar.ncon, "ds", optional=slack), bar._vec(xt, bar.nvar, "xt"), bar._vec(st, bar.ncon, "st", optional=slack))
        L, s = self._handle()
        _lib.check(L.iem_search_trial(s, *args))
        return xt, st

    def accept(self, ft, merit, mu: float, alpha, obj_weight: float = 1.0):
        """The decision (``iem_search_accept``): ``ft`` a device tensor of one (``f`` at the trial point), ``merit`` the two numbers of
        ``BarrierLayer.merit`` there; ``alpha[0]`` becomes the accepted step length or ``+0.0``.  Returns ``alpha``."""
        bar = self.layer
        args = (bar._vec(ft, 1, "ft"), bar._vec(merit, 2, "merit"), float(mu), float(obj_weight), bar._vec(alpha, 2, "alpha"))
        L, s = self._handle()
        _lib.check(L.iem_search_accept(s, *args))
        return alpha

    def reset(self):
        """A new barrier problem (``mu`` changed): the filter emptied, the flags cleared (``iem_search_reset``)."""
        L, s = self._handle()
        _lib.check(L.iem_search_reset(s))

    def bind_mu(self, param=None):
        """While bound to a :class:`BarrierParameter` (``iem_search_bind_mu``), :meth:`begin` and :meth:`accept` read ``mu`` from the
        parameter's block on the device; their ``mu`` argument is ignored.  ``None`` unbinds."""
        L, s = self._handle()
        _lib.check(L.iem_search_bind_mu(s, param._handle()[1] if param is not None else None))

    def state(self):
        """THE read-back (``iem_search_state``, synchronises): the control block as a dict, ``status`` also by name."""
        L, s = self._handle()
        v = _lib.SearchState()
        v.struct_size = C.sizeof(_lib.SearchState)
        _lib.check(L.iem_search_state(s, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.SearchState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.SEARCH_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.SEARCH_STATUS) else "?"
        return out

    def device(self):
        """``(control, filter)``: the addresses of the control block (16 words) and of the filter (``filter_capacity`` pairs) on the
        device (``iem_search_device``)."""
        L, s = self._handle()
        ctl, flt = C.c_void_p(), C.c_void_p()
        _lib.check(L.iem_search_device(s, C.byref(ctl), C.byref(flt)))
        return ctl.value, flt.value

    def close(self):
        if self._s is not None:
            _lib.check(self.layer.model._L.iem_search_destroy(self._s))
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class SecondOrderCorrection:
    """``SecondOrderCorrection(search, max_soc=4, kappa_soc=0.99)``: the second-order correction of the C-ABI (``iem_soc_*``,
    ``csrc/iem_soc_device.h``) beside a :class:`FilterSearch` — five one-launch calls gated on the device by words 13–15 of the
    search's control block, no read-back but :meth:`state`.  Between the first rung and the later ones, with buffers of the caller
    (``kkt``: the ``KKTObject`` holding this iteration's factors):

        soc.open()                                                     # behind the first rung's fs.accept
        for _ in range(P):                                             # P <= max_soc rounds; a round that does not apply stores nothing
            soc.rhs(state, c, ct, st, rhs, mu, out=rhs_soc)
            kkt.solve(rhs_soc, refine=1, out=sol_soc)
            bar.step(state, sol_soc, mu, tau, out=dirs_soc, alpha=alpha_soc)
            soc.trial(state, sol_soc, dirs_soc[0], alpha_soc, xt, st)
            model.obj_device(xt, out=ft); model.cons(xt, out=ct); bar.merit(xt, st, ct, out=m)
            soc.accept(ft, m, alpha_soc, mu, alpha)
        soc.select(sol_soc, dirs_soc, sol, dirs)                       # an accepted correction replaces the first-order direction

    The later rungs and ``bar.update(state, sol, dirs, alpha, mu)`` then take the corrected step with no host decision."""

    def __init__(self, search: FilterSearch, **opts):
        self.search = search
        self.layer = search.layer
        self._q = None
        o = _lib.SocOpts.defaults(**opts)
        self.opts = {name: getattr(o, name) for name, _ in _lib.SocOpts._fields_ if name != "struct_size"}
        L, s = search._handle()
        q = C.c_void_p()
        _lib.check(L.iem_soc_create(s, C.byref(o), C.byref(q)))
        self._q = q

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("SecondOrderCorrection: closed")
        L, _ = self.search._handle()
        return L, self._q

    def open(self):
        """The gate (``iem_soc_open``), behind the first rung's ``accept``: the correction becomes active iff that trial was rejected
        with a finite ``θ`` not below ``θ0``; a second call changes nothing."""
        L, q = self._handle()
        _lib.check(L.iem_soc_open(q))

    def rhs(self, state, c, ct, st, rhs, mu: float, out=None):
        """The accumulated constraint residual and the corrected right-hand side (``iem_soc_rhs``): ``c`` at the current point, ``ct`` /
        ``st`` at the latest trial point, ``rhs`` of ``BarrierLayer.terms``.  Returns ``out`` (``nvar + ncon``)."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        out = out if out is not None else bar._new(bar.n)
        args = (bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(state[2], bar.ncon, "y", optional=slack), bar._vec(state[5], bar.ncon, "vL", optional=slack),
                bar._vec(state[6], bar.ncon, "vU", optional=slack), bar._vec(c, bar.ncon, "c"), bar._vec(ct, bar.ncon, "ct"), bar._vec(st, bar.ncon, "st", optional=slack),
                bar._vec(rhs, bar.n, "rhs"), float(mu), bar._vec(out, bar.n, "rhs_soc"))
        L, q = self._handle()
        _lib.check(L.iem_soc_rhs(q, *args))
        return out

    def trial(self, state, sol_soc, ds_soc, alpha_soc, xt, st):
        """``(xt, st) = (x + α_soc·dx_soc, s + α_soc·ds_soc)`` with ``α_soc = alpha_soc[0]`` read on the device (``iem_soc_trial``);
        nothing is stored unless the correction is active and ``α_soc > 0``."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(sol_soc, bar.n, "sol_soc"),
                bar._vec(ds_soc, bar.ncon, "ds_soc", optional=slack), bar._vec(alpha_soc, 2, "alpha_soc"), bar._vec(xt, bar.nvar, "xt"),
                bar._vec(st, bar.ncon, "st", optional=slack))
        L, q = self._handle()
        _lib.check(L.iem_soc_trial(q, *args))
        return xt, st

    def accept(self, ft, merit, alpha_soc, mu: float, alpha, obj_weight: float = 1.0):
        """The decision on a corrected trial point (``iem_soc_accept``): accepted, ``alpha`` takes both step lengths of ``alpha_soc``;
        rejected, neither ``alpha`` nor the search's status, trials and step length change.  Returns ``alpha``."""
        bar = self.layer
        args = (bar._vec(ft, 1, "ft"), bar._vec(merit, 2, "merit"), bar._vec(alpha_soc, 2, "alpha_soc"), float(mu), float(obj_weight), bar._vec(alpha, 2, "alpha"))
        L, q = self._handle()
        _lib.check(L.iem_soc_accept(q, *args))
        return alpha

    def bind_mu(self, param=None):
        """While bound to a :class:`BarrierParameter` (``iem_soc_bind_mu``), :meth:`rhs` and :meth:`accept` read ``mu`` from the
        parameter's block on the device; their ``mu`` argument is ignored.  ``None`` unbinds."""
        L, q = self._handle()
        _lib.check(L.iem_soc_bind_mu(q, param._handle()[1] if param is not None else None))

    def select(self, sol_soc, dirs_soc, sol, dirs):
        """Iff the correction was accepted, ``sol_soc`` and ``dirs_soc = (ds, dzL, dzU, dvL, dvU)`` are copied over ``sol`` and
        ``dirs`` (``iem_soc_select``)."""
        bar = self.layer
        src, dst = bar._dirs(dirs_soc), bar._dirs(dirs)
        ps, pd = bar._vec(sol_soc, bar.n, "sol_soc"), bar._vec(sol, bar.n, "sol")
        L, q = self._handle()
        _lib.check(L.iem_soc_select(q, ps, *src, pd, *dst))
        return sol, dirs

    def state(self):
        """THE read-back (``iem_soc_state``, synchronises): the search's status word and words 13–15 of the block, ``state`` also by
        name."""
        L, q = self._handle()
        v = _lib.SocState()
        v.struct_size = C.sizeof(_lib.SocState)
        _lib.check(L.iem_soc_state(q, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.SocState._fields_ if name != "struct_size"}
        out["state_name"] = _lib.SOC_STATE[out["state"]] if 0 <= out["state"] < len(_lib.SOC_STATE) else "?"
        return out

    def device(self):
        """The address of the accumulated residual ``csoc`` (``ncon`` doubles) on the device (``iem_soc_device``)."""
        L, q = self._handle()
        p = C.c_void_p()
        _lib.check(L.iem_soc_device(q, C.byref(p)))
        return p.value

    def close(self):
        if self._q is not None:
            _lib.check(self.layer.model._L.iem_soc_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.search._s is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class BarrierParameter:
    """``BarrierParameter(layer, **opts)``: the barrier parameter of the C-ABI (``iem_mu_*``, ``csrc/iem_mu_device.h``) beside a
    :class:`BarrierLayer` — ``mu``, ``tau`` and the stopping test in a block of sixteen words on the device, two one-launch calls, no
    read-back but :meth:`state`.  ``opts``: ``mu_init, kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max`` (Ipopt's defaults;
    ``mu_floor = 0`` means ``max(1e-11, tol/10)``).  Per iteration, with the three objects bound (``bar.bind_mu(par)``,
    ``fs.bind_mu(par)``, ``soc.bind_mu(par)`` — their ``mu`` / ``tau`` arguments are then ignored):

        _, c, r = model.eval_residual(state[0], state[2])
        w = par.error(state, r, c, out=w)                              # twelve words; w[:8] is bar.error(state, r, c, 0.0)
        par.update(w, search=fs)                                       # the stopping test and the monotone rule; empties fs's filter iff mu moved
        ...                                                            # terms, solve, step, begin, rungs, update: one graph for every mu
        st = par.state()                                               # THE read-back: status, mu, the error terms"""

    def __init__(self, layer: BarrierLayer, **opts):
        self.layer = layer
        self._p = None
        o = _lib.MuOpts.defaults(**opts)
        L, b = layer._handle()
        p = C.c_void_p()
        _lib.check(L.iem_mu_create(b, C.byref(o), C.byref(p)))
        self._p = p
        self.opts = {name: getattr(o, name) for name, _ in _lib.MuOpts._fields_ if name != "struct_size"}
        if self.opts["mu_floor"] == 0.0:
            self.opts["mu_floor"] = max(1e-11, self.opts["tol"] / 10.0)

    def _handle(self):
        if self._p is None:
            raise _lib.IemError("BarrierParameter: closed")
        L, _ = self.layer._handle()
        return L, self._p

    def reset(self, mu0: float = None):
        """A new solve (``iem_mu_reset``, asynchronous): ``mu = mu0`` (default ``mu_init``), ``tau``, ``zeta`` from it, status
        iterating, flags and counters zero."""
        L, p = self._handle()
        _lib.check(L.iem_mu_reset(p, float(self.opts["mu_init"] if mu0 is None else mu0)))

    def error(self, state, r, c, out=None):
        """The twelve words of ``iem_mu_error`` as a device tensor: the eight numbers of ``BarrierLayer.error(state, r, c, 0.0)`` bit
        for bit, then the minimum of the complementarity products ``gap·z`` that are ``>= +0.0``, their sum, the count of the
        products that are not, and ``+0.0``.  ``r`` is required."""
        bar = self.layer
        out = out if out is not None else bar._new(12)
        ps = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(c, bar.ncon, "c"), bar._vec(out, 12, "out"))
        L, p = self._handle()
        _lib.check(L.iem_mu_error(p, *ps, *args))
        return out

    def update(self, out12, search: FilterSearch = None):
        """The stopping test and the monotone rule on the device (``iem_mu_update``) from the twelve words of :meth:`error`; a
        ``search`` has its filter emptied and its flags cleared exactly when ``mu`` moved."""
        bar = self.layer
        pw = bar._vec(out12, 12, "out12")
        ps = search._handle()[1] if search is not None else None
        L, p = self._handle()
        _lib.check(L.iem_mu_update(p, pw, ps))

    def state(self):
        """THE read-back (``iem_mu_state``, synchronises): words 0–11 of the block as a dict, ``status`` also by name, ``changed`` =
        flag bit 0."""
        L, p = self._handle()
        v = _lib.MuState()
        v.struct_size = C.sizeof(_lib.MuState)
        _lib.check(L.iem_mu_state(p, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.MuState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.MU_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.MU_STATUS) else "?"
        out["changed"] = bool(out["flags"] & 1)
        return out

    def device(self):
        """The address of the block (16 words) on the device (``iem_mu_device``)."""
        L, p = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_mu_device(p, C.byref(blk)))
        return blk.value

    def close(self):
        """Unbind (or close) the objects bound to this parameter first: they borrow its block."""
        if self._p is not None:
            _lib.check(self.layer.model._L.iem_mu_destroy(self._p))
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class AdaptiveBarrierParameter:
    """``AdaptiveBarrierParameter(par, **opts)``: the adaptive barrier parameter of the C-ABI (``iem_amu_*``,
    ``csrc/iem_amu_device.h``) ON a :class:`BarrierParameter` — Ipopt's free / fixed modes with the kkt-error progress test, the
    probing or the LOQO oracle, all in one launch that writes ``mu``, ``tau`` and the stopping test into ``par``'s block; the objects
    bound to ``par`` follow.  ``opts``: ``oracle`` (``"probing"`` / ``"loqo"`` or 0 / 1), ``sigma_max, mu_min, mu_max_fact,
    init_factor, red_fact, refs_max``.  Per iteration, in place of ``par.update``:

        w = par.error(state, r, c, out=w)
        with amu.affine(bar, fs):                                      # unbound inside: the calls take mu = 0, tau = 1
            _, _, rhs_a = bar.terms(state, r, c, 0.0, out=(sigma, dcon, rhs_a))
            sol_a = kkt.solve(rhs_a, refine=1)                         # one more back-solve on the iteration's factors
            dirs_a, alpha_a = bar.step(state, sol_a, 0.0, 1.0)
            q = amu.probe(state, sol_a, dirs_a, alpha_a, out=q)        # four words
        amu.update(w, q, search=fs)                                    # LOQO: amu.update(w, search=fs), no affine solve at all
        st = amu.state()                                               # THE read-back: both blocks"""

    def __init__(self, par: BarrierParameter, **opts):
        self.par = par
        self.layer = par.layer
        self._a = None
        o = _lib.AmuOpts.defaults(**opts)
        L, p = par._handle()
        a = C.c_void_p()
        _lib.check(L.iem_amu_create(p, C.byref(o), C.byref(a)))
        self._a = a
        self.opts = {name: getattr(o, name) for name, _ in _lib.AmuOpts._fields_ if name != "struct_size"}

    def _handle(self):
        if self._a is None:
            raise _lib.IemError("AdaptiveBarrierParameter: closed")
        L, _ = self.par._handle()
        return L, self._a

    def reset(self):
        """A new solve (``iem_amu_reset``, asynchronous): mode free, the ring of references empty, ``mu_max`` unset, counters zero.
        ``par.reset()`` is a call of its own."""
        L, a = self._handle()
        _lib.check(L.iem_amu_reset(a))

    def probe(self, state, sol_aff, dirs_aff, alpha_aff, out=None):
        """The four words of ``iem_amu_probe`` as a device tensor: the sum of the complementarity products after the affine step
        ``(alpha_aff[0], alpha_aff[1])`` along ``sol_aff = [dx; dy]``, ``dirs_aff = (ds, dzL, dzU, dvL, dvU)``; the count of the
        products that are NaN; the two step lengths.  ``y`` and ``dy`` are not read."""
        bar = self.layer
        out = out if out is not None else bar._new(4)
        ps, pd = bar._state(state), bar._dirs(dirs_aff)
        args = (bar._vec(sol_aff, bar.n, "sol_aff"), *pd, bar._vec(alpha_aff, 2, "alpha_aff"), bar._vec(out, 4, "out"))
        L, a = self._handle()
        _lib.check(L.iem_amu_probe(a, ps[0], ps[1], ps[3], ps[4], ps[5], ps[6], *args))
        return out

    def update(self, out12, probe4=None, force_fixed: bool = False, search: FilterSearch = None):
        """The stopping test and the adaptive rule on the device (``iem_amu_update``) from the twelve words of
        :meth:`BarrierParameter.error` and — probing oracle — the four of :meth:`probe`; a ``search`` has its filter emptied and its
        flags cleared exactly when the bits of ``mu`` changed.  ``force_fixed``: the last step was poor, leave the free mode."""
        bar = self.layer
        pw = bar._vec(out12, 12, "out12")
        pq = bar._vec(probe4, 4, "probe4", optional=True)
        ps = search._handle()[1] if search is not None else None
        L, a = self._handle()
        _lib.check(L.iem_amu_update(a, pw, pq, int(bool(force_fixed)), ps))

    def state(self):
        """THE read-back (``iem_amu_state``, synchronises once): the dict of :meth:`BarrierParameter.state` and, under the
        object's own names, ``mode`` / ``mode_name``, ``mu_max``, ``refs`` (oldest first), ``mu_oracle``, ``sigma``, ``avg``,
        ``m_aff``, ``to_fixed``, ``to_free``, ``oracle`` / ``oracle_name``."""
        L, a = self._handle()
        v, u = _lib.MuState(), _lib.AmuState()
        v.struct_size, u.struct_size = C.sizeof(_lib.MuState), C.sizeof(_lib.AmuState)
        _lib.check(L.iem_amu_state(a, C.byref(v), C.byref(u)))
        out = {name: getattr(v, name) for name, _ in _lib.MuState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.MU_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.MU_STATUS) else "?"
        out["changed"] = bool(out["flags"] & 1)
        out.update({name: getattr(u, name) for name, _ in _lib.AmuState._fields_ if name not in ("struct_size", "refs", "refs_count")})
        out["refs"] = [float(u.refs[i]) for i in range(max(0, min(4, int(u.refs_count))))]
        out["mode_name"] = _lib.AMU_MODE[out["mode"]] if 0 <= out["mode"] < len(_lib.AMU_MODE) else "?"
        out["oracle_name"] = _lib.AMU_ORACLE[out["oracle"]] if 0 <= out["oracle"] < len(_lib.AMU_ORACLE) else "?"
        return out

    def device(self):
        """The address of the object's own block (16 words) on the device (``iem_amu_device``); ``par.device()`` is the other."""
        L, a = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_amu_device(a, C.byref(blk)))
        return blk.value

    @contextlib.contextmanager
    def affine(self, layer: BarrierLayer, search: FilterSearch = None, soc: "SecondOrderCorrection" = None):
        """The affine-scaling calls of one iteration: ``layer`` (and ``search``, ``soc`` if given) — objects BOUND to ``par`` — are
        unbound inside the block, so ``terms`` / ``step`` take the host's ``mu = 0``, ``tau = 1``, and bound to ``par`` again
        afterwards.  No launch either way (the bound variant was loaded by the first bind): inside a capture each node keeps the
        variant it was captured with."""
        objs = [o for o in (layer, search, soc) if o is not None]
        for o in objs:
            o.bind_mu(None)
        try:
            yield self
        finally:
            for o in objs:
                o.bind_mu(self.par)

    def close(self):
        if self._a is not None:
            _lib.check(self.layer.model._L.iem_amu_destroy(self._a))
            self._a = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.par._p is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class QualityFunction:
    """``QualityFunction(amu, **opts)``: the quality-function oracle of the C-ABI (``iem_qf_*``, ``csrc/iem_qf_device.h``) ON an
    :class:`AdaptiveBarrierParameter` — Ipopt's default ``mu_oracle`` for ``mu_strategy = adaptive``: a golden-section search over
    ``sigma`` of the 2-norm-squared quality function, one launch for the step lengths and one for the value per candidate, the whole
    state machine on the device, and the adaptive rule with its result in one launch.  ``opts``: ``mu_ref, sigma_min, sigma_max``
    (0: ``amu``'s), ``section_sigma_tol, max_section_steps``.  Per iteration, in place of ``amu.update``:

        w = par.error(state, r, c, out=w)
        with amu.affine(bar, fs):                                      # unbound inside: the calls take the host's mu and tau = 1
            _, _, rhs0 = bar.terms(state, r, c, 0.0, out=(sigma, dcon, rhs2[0]))
            _, _, rhs1 = bar.terms(state, r, c, qf.opts["mu_ref"], out=(sigma, dcon, rhs2[1]))
            sol2 = kkt.solve(rhs2.t(), refine=1).t()                   # rhs2: (2, n).  ONE pass over the iteration's factors for both columns
            d0 = bar.step(state, sol2[0], 0.0, 1.0)[0]
            d1 = bar.step(state, sol2[1], qf.opts["mu_ref"], 1.0)[0]
        qf.begin(state, r, c, w)
        qf.section(state, (sol2[0], *d0), (sol2[1], *d1))              # max_section_steps + 4 alpha / value pairs, no decision between
        qf.update(w, search=fs)
        st = qf.state()                                                # THE read-back: the three blocks"""

    def __init__(self, amu: AdaptiveBarrierParameter, **opts):
        self.amu = amu
        self.par = amu.par
        self.layer = amu.layer
        self._q = None
        o = _lib.QfOpts.defaults(**opts)
        L, a = amu._handle()
        q = C.c_void_p()
        _lib.check(L.iem_qf_create(a, C.byref(o), C.byref(q)))
        self._q = q
        self.opts = {name: getattr(o, name) for name, _ in _lib.QfOpts._fields_ if name != "struct_size"}
        if self.opts["sigma_max"] == 0.0:
            self.opts["sigma_max"] = amu.opts["sigma_max"]
        self.pairs = int(self.opts["max_section_steps"]) + 4

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("QualityFunction: closed")
        L, _ = self.amu._handle()
        return L, self._q

    def reset(self):
        """A new solve (``iem_qf_reset``, asynchronous): the section idle, the block zero.  ``amu.reset()`` and ``par.reset()`` are
        calls of their own."""
        L, q = self._handle()
        _lib.check(L.iem_qf_reset(q))

    def begin(self, state, r, c, out12):
        """``iem_qf_begin``: the squared norms of the dual and the primal residual, and the section's first trial ``sigma`` from the
        twelve words of :meth:`BarrierParameter.error` — all into the object's block."""
        bar = self.layer
        ps = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(c, bar.ncon, "c"), bar._vec(out12, 12, "out12"))
        L, q = self._handle()
        _lib.check(L.iem_qf_begin(q, *ps, *args))

    def _pair_args(self, state, d0, d1):
        bar = self.layer
        ps = bar._state(state)
        if len(d0) != 6 or len(d1) != 6:
            raise ValueError("d0, d1: (sol, ds, dzL, dzU, dvL, dvU)")
        cols = []
        for d, tag in ((d0, "0"), (d1, "1")):
            cols += [bar._vec(d[0], bar.n, "sol" + tag), *bar._dirs(d[1:])]
        return (ps[0], ps[1], ps[3], ps[4], ps[5], ps[6], *cols)

    def alpha(self, state, d0, d1):
        """``iem_qf_alpha``: the fraction-to-the-boundary step lengths of the direction at the trial ``sigma`` into the block's two
        slots; ``d0 = (sol, ds, dzL, dzU, dvL, dvU)`` at ``mu = 0``, ``d1`` at ``mu = mu_ref``.  Nothing unless a section is open."""
        args = self._pair_args(state, d0, d1)
        L, q = self._handle()
        _lib.check(L.iem_qf_alpha(q, *args))

    def value(self, state, d0, d1):
        """``iem_qf_value``: the quality function at the trial ``sigma`` with the slots' step lengths, and one step of the section:
        the next trial, or the result.  Nothing unless a section is open."""
        args = self._pair_args(state, d0, d1)
        L, q = self._handle()
        _lib.check(L.iem_qf_value(q, *args))

    def section(self, state, d0, d1, pairs: int = None):
        """Every ``alpha`` / ``value`` pair of a section (``max_section_steps + 4``), with no decision in between: pairs behind the
        one that finishes the section do nothing on the device.  A model without any bound (``nz == 0``: ``begin`` leaves the section
        DONE) is issued no pair at all — a property of the model, not of the state."""
        args = self._pair_args(state, d0, d1)
        L, q = self._handle()
        if self.layer.info["nz"] == 0 and pairs is None:
            return
        for _ in range(self.pairs if pairs is None else int(pairs)):
            _lib.check(L.iem_qf_alpha(q, *args))
            _lib.check(L.iem_qf_value(q, *args))

    def update(self, out12, force_fixed: bool = False, search: FilterSearch = None):
        """The stopping test and the adaptive rule on the device (``iem_qf_update``) with the section's result as the oracle; a
        ``search`` has its filter emptied and its flags cleared exactly when the bits of ``mu`` changed."""
        bar = self.layer
        pw = bar._vec(out12, 12, "out12")
        ps = search._handle()[1] if search is not None else None
        L, q = self._handle()
        _lib.check(L.iem_qf_update(q, pw, int(bool(force_fixed)), ps))

    def state(self):
        """THE read-back (``iem_qf_state``, synchronises once): the dict of :meth:`AdaptiveBarrierParameter.state` and ``section``:
        the object's own words by the names of ``iem_qf_state_t`` (``status_name`` among them)."""
        L, q = self._handle()
        v, u, t = _lib.MuState(), _lib.AmuState(), _lib.QfState()
        v.struct_size, u.struct_size, t.struct_size = C.sizeof(_lib.MuState), C.sizeof(_lib.AmuState), C.sizeof(_lib.QfState)
        _lib.check(L.iem_qf_state(q, C.byref(v), C.byref(u), C.byref(t)))
        out = {name: getattr(v, name) for name, _ in _lib.MuState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.MU_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.MU_STATUS) else "?"
        out["changed"] = bool(out["flags"] & 1)
        out.update({name: getattr(u, name) for name, _ in _lib.AmuState._fields_ if name not in ("struct_size", "refs", "refs_count")})
        out["refs"] = [float(u.refs[i]) for i in range(max(0, min(4, int(u.refs_count))))]
        out["mode_name"] = _lib.AMU_MODE[out["mode"]] if 0 <= out["mode"] < len(_lib.AMU_MODE) else "?"
        sec = {name: getattr(t, name) for name, _ in _lib.QfState._fields_ if name not in ("struct_size", "alpha_slots")}
        sec["alpha_slots"] = [float(t.alpha_slots[0]), float(t.alpha_slots[1])]
        sec["status_name"] = _lib.QF_STATUS[sec["status"]] if 0 <= sec["status"] < len(_lib.QF_STATUS) else "?"
        out["section"] = sec
        return out

    def device(self):
        """The address of the object's own block (32 words) on the device (``iem_qf_device``)."""
        L, q = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_qf_device(q, C.byref(blk)))
        return blk.value

    def close(self):
        if self._q is not None:
            _lib.check(self.layer.model._L.iem_qf_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.amu._a is not None and self.par._p is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class MehrotraCorrector:
    """``MehrotraCorrector(amu, red_fact=1.0)``: Mehrotra's corrector of the C-ABI (``iem_mpc_*``, ``csrc/iem_mpc_device.h``) ON an
    :class:`AdaptiveBarrierParameter` — the second-order term ``Δgap_aff·Δz_aff`` of the complementarity equations on the right-hand
    side, for one more column of the iteration's refined solve; the safeguard's decision and the copy over the first-order direction
    on the device.  Per iteration, AFTER the rule's update, with the objects bound again (``mpc.bind_mu(par)`` once):

        amu.update(w, q, search=fs)                                    # (or qf.update; the affine direction is then its d0)
        rhs2 = mpc.terms(state, r, c, sol_a, dirs_a, out=rhs2)         # (2, n): column 0 is bar.terms(...)[2] at the new mu
        sol2 = kkt.solve(rhs2.t(), refine=1).t()                       # ONE pass over the iteration's factors for both columns
        dirs, alpha = bar.step(state, sol2[0], mu, tau)                # column 0: unchanged
        dirs_c, alpha_c = mpc.step(state, sol_a, dirs_a, sol2[1])
        q_c = amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c)      # the safeguard's measurement
        mpc.select(q_c, alpha_c, sol2[1], dirs_c, sol2[0], dirs, alpha)   # taken: the corrected direction over the first-order one
        ...                                                            # fs.begin, the rungs, soc, bar.update on (sol2[0], dirs, alpha)
        st = mpc.state()                                               # THE read-back"""

    def __init__(self, amu: AdaptiveBarrierParameter, **opts):
        self.amu = amu
        self.par = amu.par
        self.layer = amu.layer
        self._q = None
        o = _lib.MpcOpts.defaults(**opts)
        L, a = amu._handle()
        q = C.c_void_p()
        _lib.check(L.iem_mpc_create(a, C.byref(o), C.byref(q)))
        self._q = q
        self.opts = {name: getattr(o, name) for name, _ in _lib.MpcOpts._fields_ if name != "struct_size"}

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("MehrotraCorrector: closed")
        L, _ = self.amu._handle()
        return L, self._q

    def _affine(self, sol_aff, dirs_aff):
        bar = self.layer
        return (bar._vec(sol_aff, bar.n, "sol_aff"), *bar._dirs(dirs_aff))

    def reset(self):
        """A new solve (``iem_mpc_reset``, asynchronous): the block zero."""
        L, q = self._handle()
        _lib.check(L.iem_mpc_reset(q))

    def bind_mu(self, param=None):
        """While bound to the :class:`BarrierParameter` under ``amu`` (``iem_mpc_bind_mu``), :meth:`terms` and :meth:`step` read
        ``mu`` and ``tau`` from its block on the device; their ``mu`` / ``tau`` arguments are ignored.  ``None`` unbinds."""
        L, q = self._handle()
        _lib.check(L.iem_mpc_bind_mu(q, param._handle()[1] if param is not None else None))

    def terms(self, state, r, c, sol_aff, dirs_aff, mu: float = 0.0, out=None):
        """The two right-hand-side columns as one ``(2, n)`` device tensor (``iem_mpc_terms``): row 0 is ``BarrierLayer.terms``'s
        ``rhs`` at that ``mu`` bit for bit, row 1 has ``mu − Δgap_aff·Δz_aff`` per bound in the place of ``mu``.  ``sigma`` and
        ``dcon`` are not written: they are those of the affine ``terms`` call."""
        bar = self.layer
        out = out if out is not None else bar._torch.empty((2, bar.n), dtype=bar._torch.float64, device=bar.model.device)
        if tuple(out.shape) != (2, bar.n) or out.stride(1) != 1 or out.stride(0) < bar.n or out.dtype != bar._torch.float64:
            raise ValueError(f"out: a float64 tensor of shape (2, {bar.n}) with contiguous rows expected")
        ps = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(c, bar.ncon, "c"), *self._affine(sol_aff, dirs_aff), float(mu), C.c_void_p(out.data_ptr()), int(out.stride(0)))
        L, q = self._handle()
        _lib.check(L.iem_mpc_terms(q, *ps, *args))
        return out

    def step(self, state, sol_aff, dirs_aff, sol_c, mu: float = 0.0, tau: float = 1.0, out=None, alpha=None):
        """``((ds, dzL, dzU, dvL, dvU), alpha_c)`` of the corrected solution ``sol_c`` (``iem_mpc_step``): ``BarrierLayer.step`` with
        the per-bound target in the place of ``mu``."""
        bar = self.layer
        dirs = out if out is not None else (bar._new(bar.ncon), bar._new(bar.nvar), bar._new(bar.nvar), bar._new(bar.ncon), bar._new(bar.ncon))
        alpha = alpha if alpha is not None else bar._new(2)
        ps, d = bar._state(state), bar._dirs(dirs)
        args = (*self._affine(sol_aff, dirs_aff), bar._vec(sol_c, bar.n, "sol_c"), float(mu), float(tau), *d, bar._vec(alpha, 2, "alpha"))
        L, q = self._handle()
        _lib.check(L.iem_mpc_step(q, *ps, *args))
        return dirs, alpha

    def select(self, probe4, alpha_c, sol_c, dirs_c, sol, dirs, alpha):
        """The safeguard's decision on the device (``iem_mpc_select``) from the four words of ``amu.probe`` on the corrected
        direction: taken, ``sol_c``, ``dirs_c`` and ``alpha_c`` are copied over ``sol``, ``dirs`` and ``alpha``; refused, nothing
        moves.  Returns ``(sol, dirs, alpha)``."""
        bar = self.layer
        src, dst = bar._dirs(dirs_c), bar._dirs(dirs)
        args = (bar._vec(probe4, 4, "probe4"), bar._vec(alpha_c, 2, "alpha_c"), bar._vec(sol_c, bar.n, "sol_c"), *src, bar._vec(sol, bar.n, "sol"), *dst,
                bar._vec(alpha, 2, "alpha"))
        L, q = self._handle()
        _lib.check(L.iem_mpc_select(q, *args))
        return sol, dirs, alpha

    def state(self):
        """THE read-back (``iem_mpc_state``, synchronises once): ``taken`` (the last decision), ``n_taken``, ``n_refused``,
        ``predicted``, ``avg``, ``alpha_c``."""
        L, q = self._handle()
        v = _lib.MpcState()
        v.struct_size = C.sizeof(_lib.MpcState)
        _lib.check(L.iem_mpc_state(q, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.MpcState._fields_ if name not in ("struct_size", "alpha_c")}
        out["taken"] = bool(out["taken"])
        out["alpha_c"] = [float(v.alpha_c[0]), float(v.alpha_c[1])]
        return out

    def device(self):
        """The address of the object's own block (16 words) on the device (``iem_mpc_device``)."""
        L, q = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_mpc_device(q, C.byref(blk)))
        return blk.value

    def close(self):
        if self._q is not None:
            _lib.check(self.layer.model._L.iem_mpc_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.amu._a is not None and self.par._p is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class StartingPoint:
    """``StartingPoint(layer, **opts)``: the starting point of the C-ABI (``iem_init_*``, ``csrc/iem_init_device.h``) ON a
    :class:`BarrierLayer` — Ipopt's least-squares estimate of the row multipliers for a cold start, and for a warm start the
    projection of a given primal-dual point with a barrier parameter taken from its complementarity.  ``opts``: ``y_max, on_reject,
    warm_push, warm_frac, warm_z_push, warm_z_max, warm_y_max, mu_factor, mu_cap`` (``include/iem.h`` has ranges and defaults).

    A cold start, behind ``state = bar.start(x, model.cons(x))``, with ``r`` of ``model.eval_residual(x, y, 1.0)``:

        sigma, dcon, rhs = init.ls_terms(state, r)                     # sigma = 1; dcon = 1 on inequality rows
        kkt.assemble(zeros_h, jv, sigma, 0.0, delta_c, dcon=dcon, at=(x, zeros_y, 0.0))      # a ZERO Hessian: W = 0 at (y = 0, obj_weight = 0)
        kkt.factor(); sol = kkt.solve(rhs, refine=1)
        init.ls_apply(sol, state[2])                                   # y += sol[nvar:] where max |y| <= y_max, else y = 0

    A warm start from a previous solution (x, s, y, zL, zU, vL, vU), in the place of ``bar.start``:

        init.warm(state)                                               # in place: the push, the clamps
        w = par.error(state, r, c)                                     # r, c at the pushed point
        init.mu(w, par)                                                # mu0 into par's block: every bound object reads it

    Nothing above reads a value back; :meth:`state` is the only place that does."""

    def __init__(self, layer: BarrierLayer, **opts):
        self.layer = layer
        self._q = None
        o = _lib.InitOpts.defaults(**opts)
        L, b = layer._handle()
        q = C.c_void_p()
        _lib.check(L.iem_init_create(b, C.byref(o), C.byref(q)))
        self._q = q
        self.opts = {name: getattr(o, name) for name, _ in _lib.InitOpts._fields_ if name != "struct_size"}

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("StartingPoint: closed")
        L, _ = self.layer._handle()
        return L, self._q

    def reset(self):
        """A new solve (``iem_init_reset``, asynchronous): the block zero.  Returns ``self``."""
        L, q = self._handle()
        _lib.check(L.iem_init_reset(q))
        return self

    def ls_terms(self, state, r, out=None):
        """``(sigma, dcon, rhs)`` of the least-squares estimate at ``state`` (``iem_init_ls_terms``; ``x`` and ``s`` are not read):
        exactly the inputs of ``KKTObject.assemble`` with a zeroed Hessian value array and of ``solve``."""
        bar = self.layer
        sigma, dcon, rhs = out if out is not None else (bar._new(bar.nvar), bar._new(bar.ncon), bar._new(bar.n))
        p = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(sigma, bar.nvar, "sigma"), bar._vec(dcon, bar.ncon, "dcon"), bar._vec(rhs, bar.n, "rhs"))
        L, q = self._handle()
        _lib.check(L.iem_init_ls_terms(q, *p[2:], *args))
        return sigma, dcon, rhs

    def ls_apply(self, sol, y):
        """``y += sol[nvar:]`` IN PLACE where ``max |y + sol[nvar:]| <= y_max``; otherwise ``y = 0`` (``on_reject = 0``) or ``y`` as it
        was (``on_reject = 1``) — decided on the device (``iem_init_ls_apply``).  Returns ``y``."""
        bar = self.layer
        args = (bar._vec(sol, bar.n, "sol"), bar._vec(y, bar.ncon, "y"))
        L, q = self._handle()
        _lib.check(L.iem_init_ls_apply(q, *args))
        return y

    def warm(self, state):
        """The warm-start projection of ``state = (x, s, y, zL, zU, vL, vU)`` IN PLACE (``iem_init_warm``).  Returns ``state``."""
        p = self.layer._state(state)
        L, q = self._handle()
        _lib.check(L.iem_init_warm(q, *p))
        return state

    def mu(self, w12, par):
        """The barrier parameter of a warm start into the block of the :class:`BarrierParameter` ``par`` (``iem_init_mu``), from the
        twelve words ``w12 = par.error(state, r, c)`` at the warm state.  Returns ``self``."""
        pw = self.layer._vec(w12, 12, "w12")
        L, q = self._handle()
        _lib.check(L.iem_init_mu(q, pw, par._handle()[1]))
        return self

    def state(self):
        """THE read-back (``iem_init_state``, synchronises once): ``ynorm``, ``accepted`` (the last decision), ``n_accepted``,
        ``n_rejected``, ``mu0``, ``how`` and ``how_name``."""
        L, q = self._handle()
        v = _lib.InitState()
        v.struct_size = C.sizeof(_lib.InitState)
        _lib.check(L.iem_init_state(q, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.InitState._fields_ if name != "struct_size"}
        out["accepted"] = bool(out["accepted"])
        out["how_name"] = _lib.INIT_HOW[out["how"]] if 0 <= out["how"] < len(_lib.INIT_HOW) else "?"
        return out

    def device(self):
        """The address of the object's own block (16 words) on the device (``iem_init_device``)."""
        L, q = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_init_device(q, C.byref(blk)))
        return blk.value

    def close(self):
        if self._q is not None:
            _lib.check(self.layer.model._L.iem_init_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class ConvergenceCheck:
    """``ConvergenceCheck(par, **opts)``: the stopping test and the kept iterate of the C-ABI (``iem_conv_*``,
    ``csrc/iem_conv_device.h``) ON a :class:`BarrierParameter`, whose ``tol``, ``s_max``, ``mu_floor`` and block it reads — Ipopt's
    scaled error beside the unscaled tolerances, the acceptable level met ``acceptable_iter`` times in a row, ``max_iter``, diverging
    iterates, the invalid number, the tiny step; the best acceptable point is copied into the object's own buffers on the device's
    own decision.  ``opts``: ``dual_inf_tol, constr_viol_tol, compl_inf_tol, acceptable_tol, acceptable_iter,
    acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol, max_iter,
    diverging_iterates_tol, tiny_step_tol, tiny_step_y_tol`` (Ipopt's defaults; ``inf`` switches a tolerance off).  Per iteration:

        w = par.error(state, r, c, out=w)
        conv.check(w, f, state[0])                                     # the stopping test: status, keep
        conv.keep(state)                                               # copies iff the check asked for it
        par.update(w, search=fs)
        st = conv.state()                                              # THE read-back; st["status"] != 0: conv.restore(state) where st["kept"]
        ...                                                            # terms, assemble, factor, solve
        dirs, alpha = bar.step(state, sol, mu, tau)
        conv.step(state, sol, dirs[0])                                 # the tiny step: read with the next state()

    A status other than 0 is latched until :meth:`reset`."""

    def __init__(self, par: BarrierParameter, **opts):
        self.par = par
        self.layer = par.layer
        self._q = None
        o = _lib.ConvOpts.defaults(**opts)
        L, p = par._handle()
        q = C.c_void_p()
        _lib.check(L.iem_conv_create(p, C.byref(o), C.byref(q)))
        self._q = q
        self.opts = {name: getattr(o, name) for name, _ in _lib.ConvOpts._fields_ if name != "struct_size"}

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("ConvergenceCheck: closed")
        L, _ = self.par._handle()
        return L, self._q

    def reset(self):
        """A new solve (``iem_conv_reset``, asynchronous): the block zero; the kept buffers keep their bytes.  Returns ``self``."""
        L, q = self._handle()
        _lib.check(L.iem_conv_reset(q))
        return self

    def check(self, w12, f, x):
        """The stopping test on the device (``iem_conv_check``) from the twelve words of ``par.error``, the objective ``f`` (a device
        tensor of one) and ``x``.  Returns ``self``."""
        bar = self.layer
        args = (bar._vec(w12, 12, "w12"), bar._vec(f, 1, "f"), bar._vec(x, bar.nvar, "x"))
        L, q = self._handle()
        _lib.check(L.iem_conv_check(q, *args))
        return self

    def keep(self, state):
        """Copy ``state`` into the kept buffers iff the last :meth:`check` asked for it (``iem_conv_keep``).  Returns ``self``."""
        p = self.layer._state(state)
        L, q = self._handle()
        _lib.check(L.iem_conv_keep(q, *p))
        return self

    def restore(self, state):
        """The kept point into ``state`` IN PLACE iff one is held (``iem_conv_restore``): only the entries :meth:`keep` reads are
        written.  Returns ``state``."""
        p = self.layer._state(state)
        L, q = self._handle()
        _lib.check(L.iem_conv_restore(q, *p))
        return state

    def step(self, state, sol, ds):
        """The tiny-step test on the device (``iem_conv_step``) from ``x, s`` of ``state``, ``sol = [dx; dy]`` and the slack direction
        ``ds`` of ``BarrierLayer.step``.  Returns ``self``."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(sol, bar.n, "sol"), bar._vec(ds, bar.ncon, "ds", optional=slack))
        L, q = self._handle()
        _lib.check(L.iem_conv_step(q, *args))
        return self

    def kept(self):
        """The kept point ``(x, s, y, zL, zU, vL, vU)`` as device tensors that ALIAS the object's own buffers (``iem_conv_kept``):
        valid until :meth:`close`; absent bounds hold ``+0.0``, equality rows of ``s, vL, vU`` what create left (zero)."""
        import torch
        bar = self.layer
        L, q = self._handle()
        ptrs = [C.c_void_p() for _ in range(7)]
        _lib.check(L.iem_conv_kept(q, *[C.byref(p) for p in ptrs]))
        sizes = (bar.nvar, bar.ncon, bar.ncon, bar.nvar, bar.nvar, bar.ncon, bar.ncon)
        total = 3 * bar.nvar + 4 * bar.ncon

        class _Span:      # the whole allocation through the CUDA array interface: the tensors below are views of it
            __cuda_array_interface__ = dict(shape=(max(total, 1),), typestr="<f8", data=(ptrs[0].value, False), version=2)

        whole = torch.as_tensor(_Span(), device=bar.model.device)
        out, at = [], 0
        for p, k in zip(ptrs, sizes):
            assert (p.value or 0) == ptrs[0].value + 8 * at or k == 0
            out.append(whole[at:at + k])
            at += k
        return tuple(out)

    def state(self):
        """THE read-back (``iem_conv_state``, synchronises once): words 0–18 of the block as a dict, ``status_name``, and the flag bits
        as ``acceptable``, ``tiny``, ``tiny_above_floor``."""
        L, q = self._handle()
        v = _lib.ConvState()
        v.struct_size = C.sizeof(_lib.ConvState)
        _lib.check(L.iem_conv_state(q, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.ConvState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.CONV_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.CONV_STATUS) else "?"
        out["keep"], out["kept"] = bool(out["keep"]), bool(out["kept"])
        out.update(acceptable=bool(out["flags"] & 1), tiny=bool(out["flags"] & 2), tiny_above_floor=bool(out["flags"] & 4))
        return out

    def device(self):
        """The address of the object's own block (24 words) on the device (``iem_conv_device``)."""
        L, q = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_conv_device(q, C.byref(blk)))
        return blk.value

    def close(self):
        if self._q is not None:
            _lib.check(self.layer.model._L.iem_conv_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.par._p is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class Restoration:
    """``Restoration(search, rho=1000, kappa_resto=0.9, bound_mult_reset_threshold=1000)``: the feasibility restoration phase of the
    C-ABI (``iem_resto_*``, ``csrc/iem_resto_device.h``) beside the :class:`FilterSearch` of the ORIGINAL problem — the elastic
    variables ``p, n``, their multipliers and directions, the reference point and an INNER :class:`FilterSearch`-like object
    (:attr:`inner`) live on the device; no read-back but :meth:`state`.  When ``search.state()`` says ``failed``:

        resto.enter(state, c, max(mu, max|inf|))                       # err[2] of bar.error is max|inf|
        while resto.state()["state_name"] == "active":                 # one status read per iteration
            model.eval_residual(x, y, 0.0, c=c, out=r)                 # r = J'y
            resto.error(state, r, c, mu_R, zeta)                       # the restoration's own mu rule (inner.reset() on change)
            model.jac_hess_coord(x, y, jv, hv, obj_weight=0.0)
            sigma, dcon, rhs = resto.terms(state, r, c, mu_R, zeta)
            kkt.assemble(hv, jv, sigma, dw, dc, dcon=dcon); kkt.factor(); sol = kkt.solve(rhs, refine=1)
            dirs, alpha = resto.step(state, sol, mu_R, tau, zeta)
            m0 = resto.merit(0, x, s, c, zeta); resto.begin(state, sol, dirs[0], m0, alpha, mu_R, zeta)
            for _ in range(K):
                resto.trial(state, sol, dirs[0], xt, st); model.cons(xt, ct); mt = resto.merit(1, xt, st, ct, zeta)
                resto.inner.accept(mt[0:1], mt[1:3], mu_R, alpha)
            resto.update(state, sol, dirs, alpha, mu_R)
            model.obj_device(x, out=f); model.cons(x, c); bar.merit(x, s, c, out=m2); resto.check(f, m2, mu)
        resto.leave(state)

    ``zeta = sqrt(mu_R)``."""

    def __init__(self, search: FilterSearch, **opts):
        self.search = search
        self.layer = search.layer
        self._q = None
        self.inner = None
        o = _lib.RestoOpts.defaults(**opts)
        self.opts = {name: getattr(o, name) for name, _ in _lib.RestoOpts._fields_ if name != "struct_size"}
        L, s = search._handle()
        q = C.c_void_p()
        _lib.check(L.iem_resto_create(s, C.byref(o), C.byref(q)))
        self._q = q
        inner = C.c_void_p()
        _lib.check(L.iem_resto_search(q, C.byref(inner)))
        self.inner = _BorrowedSearch(self.layer, inner, search.opts)

    def _handle(self):
        if self._q is None:
            raise _lib.IemError("Restoration: closed")
        L, _ = self.search._handle()
        return L, self._q

    def enter(self, state, c, mu: float):
        """The elastic start, the reference point, ``y = 0``, the bound multipliers clipped at ``rho`` IN PLACE, and the current point
        into the ORIGINAL filter (``iem_resto_enter``); ``mu``: ``max(mu, max|inf|)``.  State ``active``."""
        bar = self.layer
        p = bar._state(state)
        pc = bar._vec(c, bar.ncon, "c")
        L, q = self._handle()
        _lib.check(L.iem_resto_enter(q, *p, pc, float(mu)))
        return state

    def terms(self, state, r, c, mu: float, zeta: float, out=None):
        """``(sigma, dcon, rhs)`` of the restoration's Newton system (``iem_resto_terms``); ``r = Jᵀy`` (``obj_weight = 0``)."""
        bar = self.layer
        sigma, dcon, rhs = out if out is not None else (bar._new(bar.nvar), bar._new(bar.ncon), bar._new(bar.n))
        p = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(c, bar.ncon, "c"), float(mu), float(zeta), bar._vec(sigma, bar.nvar, "sigma"), bar._vec(dcon, bar.ncon, "dcon"),
                bar._vec(rhs, bar.n, "rhs"))
        L, q = self._handle()
        _lib.check(L.iem_resto_terms(q, *p, *args))
        return sigma, dcon, rhs

    def step(self, state, sol, mu: float, tau: float, zeta: float, out=None, alpha=None):
        """``((ds, dzL, dzU, dvL, dvU), alpha)``; ``dp, dn, dzp, dzn`` stay in the object (``iem_resto_step``)."""
        bar = self.layer
        dirs = out if out is not None else (bar._new(bar.ncon), bar._new(bar.nvar), bar._new(bar.nvar), bar._new(bar.ncon), bar._new(bar.ncon))
        alpha = alpha if alpha is not None else bar._new(2)
        p, d = bar._state(state), bar._dirs(dirs)
        ps, pa = bar._vec(sol, bar.n, "sol"), bar._vec(alpha, 2, "alpha")
        L, q = self._handle()
        _lib.check(L.iem_resto_step(q, *p, ps, float(mu), float(tau), float(zeta), *d, pa))
        return dirs, alpha

    def merit(self, which: int, x, s, c, zeta: float, out=None):
        """``(rho·Σ(p + n) + zeta/2·proximity, θ_R, Σ log)`` as a device tensor (``iem_resto_merit``): at the state with ``(p, n)``
        (``which = 0``) or at a trial point with ``(pt, nt)`` (``which = 1``)."""
        bar = self.layer
        out = out if out is not None else bar._new(3)
        args = (bar._vec(x, bar.nvar, "x"), bar._vec(s, bar.ncon, "s", optional=bar.info["n_ineq"] == 0), bar._vec(c, bar.ncon, "c"), float(zeta), bar._vec(out, 3, "out"))
        L, q = self._handle()
        _lib.check(L.iem_resto_merit(q, int(which), *args))
        return out

    def begin(self, state, sol, ds, merit0, alpha, mu: float, zeta: float):
        """The slope of the restoration's barrier objective and the INNER block of a new search (``iem_resto_begin``)."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(sol, bar.n, "sol"),
                bar._vec(ds, bar.ncon, "ds", optional=slack), bar._vec(merit0, 3, "merit0"), bar._vec(alpha, 2, "alpha"))
        L, q = self._handle()
        _lib.check(L.iem_resto_begin(q, *args, float(mu), float(zeta)))

    def trial(self, state, sol, ds, xt=None, st=None):
        """``(xt, st)`` with the inner block's ``α``; ``pt, nt`` stay in the object (``iem_resto_trial``)."""
        bar = self.layer
        slack = bar.info["n_ineq"] == 0
        xt = xt if xt is not None else bar._new(bar.nvar)
        st = st if st is not None else bar._new(bar.ncon)
        args = (bar._vec(state[0], bar.nvar, "x"), bar._vec(state[1], bar.ncon, "s", optional=slack), bar._vec(sol, bar.n, "sol"),
                bar._vec(ds, bar.ncon, "ds", optional=slack), bar._vec(xt, bar.nvar, "xt"), bar._vec(st, bar.ncon, "st", optional=slack))
        L, q = self._handle()
        _lib.check(L.iem_resto_trial(q, *args))
        return xt, st

    def update(self, state, sol, dirs, alpha, mu: float, kappa_sigma: float = 1e10):
        """The accepted step IN PLACE, ``p, n, zp, zn`` included (``iem_resto_update``).  Returns ``state``."""
        bar = self.layer
        p, d = bar._state(state), bar._dirs(dirs)
        ps, pa = bar._vec(sol, bar.n, "sol"), bar._vec(alpha, 2, "alpha")
        L, q = self._handle()
        _lib.check(L.iem_resto_update(q, *p, ps, *d, pa, float(mu), float(kappa_sigma)))
        return state

    def error(self, state, r, c, mu: float, zeta: float, out=None):
        """The eight numbers of ``iem_resto_error`` (the layout of ``BarrierLayer.error``) as a device tensor;
        ``BarrierLayer.optimality_error`` applies with the counts ``(ncon, nz + 2·ncon)``."""
        bar = self.layer
        out = out if out is not None else bar._new(8)
        p = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r", optional=True), bar._vec(c, bar.ncon, "c"), float(mu), float(zeta), bar._vec(out, 8, "out"))
        L, q = self._handle()
        _lib.check(L.iem_resto_error(q, *p, *args))
        return out

    def check(self, f, merit, mu: float):
        """The return test against the ORIGINAL filter (``iem_resto_check``): ``f`` a device tensor of one, ``merit`` the two numbers of
        ``BarrierLayer.merit`` at the new iterate, ``mu`` the ORIGINAL problem's."""
        bar = self.layer
        args = (bar._vec(f, 1, "f"), bar._vec(merit, 2, "merit"), float(mu))
        L, q = self._handle()
        _lib.check(L.iem_resto_check(q, *args))

    def bind_mu(self, param=None):
        """While bound to a :class:`RestorationParameter` created on this object (``iem_resto_bind_mu``), every call above reads
        ``mu``, ``tau`` and ``zeta`` from the restoration block on the device — and :meth:`check` the ORIGINAL problem's ``mu`` from
        the original block where the parameter was given one; the host arguments are ignored.  ``None`` unbinds.  The first bind of
        a model loads a code object: bind outside a capture."""
        L, q = self._handle()
        _lib.check(L.iem_resto_bind_mu(q, param._handle()[1] if param is not None else None))

    def leave(self, state):
        """``y = 0``, the bound multipliers reset to 1 iff their maximum exceeds the threshold, state ``none`` (``iem_resto_leave``)."""
        p = self.layer._state(state)
        L, q = self._handle()
        _lib.check(L.iem_resto_leave(q, p[2], p[3], p[4], p[5], p[6]))
        return state

    def state(self):
        """THE read-back (``iem_resto_state``, synchronises): words 0–3 of the object's block, ``state`` also by name."""
        L, q = self._handle()
        v = _lib.RestoState()
        v.struct_size = C.sizeof(_lib.RestoState)
        _lib.check(L.iem_resto_state(q, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.RestoState._fields_ if name != "struct_size"}
        out["state_name"] = _lib.RESTO_STATE[out["state"]] if 0 <= out["state"] < len(_lib.RESTO_STATE) else "?"
        return out

    def device(self):
        """``dict(p, n, zp, zn, block)``: addresses on the device (``iem_resto_device``); the object's vectors are ONE allocation in
        the order of ``include/iem.h``, ``p`` first."""
        L, q = self._handle()
        ptr = [C.c_void_p() for _ in range(5)]
        _lib.check(L.iem_resto_device(q, *[C.byref(a) for a in ptr]))
        return dict(zip(("p", "n", "zp", "zn", "block"), (a.value for a in ptr)))

    def close(self):
        if self._q is not None:
            if self.inner is not None:
                self.inner._s = None      # owned by the object: destroyed with it
            _lib.check(self.layer.model._L.iem_resto_destroy(self._q))
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.search._s is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass


class _BorrowedSearch(FilterSearch):
    """the inner search of a :class:`Restoration`: every call of :class:`FilterSearch` on a handle the restoration object owns"""

    def __init__(self, layer: BarrierLayer, handle, opts):
        self.layer = layer
        self._s = handle
        self.opts = dict(opts)

    def close(self):
        self._s = None


class _BorrowedParameter(BarrierParameter):
    """the restoration block of a :class:`RestorationParameter`: :meth:`state`, :meth:`device` and ``FilterSearch.bind_mu`` of
    :class:`BarrierParameter` on a handle the restoration parameter owns"""

    def __init__(self, layer: BarrierLayer, handle, opts):
        self.layer = layer
        self._p = handle
        self.opts = dict(opts)

    def close(self):
        self._p = None


class RestorationParameter:
    """``RestorationParameter(resto, par_orig=None, **opts)``: the restoration problem's own barrier parameter of the C-ABI
    (``iem_rmu_*``, ``csrc/iem_rmu_device.h``) ON a :class:`Restoration` — the monotone rule over ``lib.RMU_K`` fixed candidates,
    the exit at a stationary point of the infeasibility, the start of a phase and Ipopt's ``alpha_min`` rule, every decision on the
    device.  ``par_orig``: the ORIGINAL problem's :class:`BarrierParameter`, whose ``mu`` :meth:`enter` and a bound
    ``Restoration.check`` then read from its block.  ``opts``: ``kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, gamma_alpha``.
    With ``resto.bind_mu(rp)`` and ``resto.inner.bind_mu(rp.inner_mu)`` the restoration iteration of :class:`Restoration` becomes

        rp.enter(err, mu); resto.enter(state, c, 0.0)                  # mu_R = max(mu, err[2]) on the device
        while True:
            model.eval_residual(x, y, 0.0, c=c, out=r)
            w = rp.error(state, r, c, out=w); rp.update(w)             # the rule; empties the inner filter iff mu moved
            ...                                                        # terms, solve, step, merit, begin: the scalars are ignored
            for _ in range(K):
                resto.trial(...); model.cons(xt, ct); mt = resto.merit(1, xt, st, ct, 0.0)
                resto.inner.accept(mt[0:1], mt[1:3], 0.0, alpha); rp.trigger(1, alpha)
            resto.update(...); ...; resto.check(f, m2, mu)
            st = rp.state()                                            # THE read-back: the rule, the block, the phase's state

    — one graph for every ``mu`` of the phase."""

    def __init__(self, resto: Restoration, par_orig: BarrierParameter = None, **opts):
        self.resto = resto
        self.layer = resto.layer
        self.par_orig = par_orig
        self._r = None
        self.inner_mu = None
        o = _lib.RmuOpts.defaults(**opts)
        self.opts = {name: getattr(o, name) for name, _ in _lib.RmuOpts._fields_ if name != "struct_size"}
        L, q = resto._handle()
        rp = C.c_void_p()
        _lib.check(L.iem_rmu_create(q, par_orig._handle()[1] if par_orig is not None else None, C.byref(o), C.byref(rp)))
        self._r = rp
        par = C.c_void_p()
        _lib.check(L.iem_rmu_mu(rp, C.byref(par)))
        self.inner_mu = _BorrowedParameter(self.layer, par, dict(self.opts, mu_init=0.1))

    def _handle(self):
        if self._r is None:
            raise _lib.IemError("RestorationParameter: closed")
        L, _ = self.resto._handle()
        return L, self._r

    def enter(self, err, mu: float = 0.0):
        """The start of a phase (``iem_rmu_enter``): ``mu_R = max(mu, err[2])`` into the restoration block, the own block zeroed, the
        inner filter emptied; ``err``: the eight words of ``BarrierLayer.error`` (or the first of ``BarrierParameter.error``) at this
        point; ``mu`` is ignored where a ``par_orig`` was given.  Issue it in front of ``Restoration.enter``."""
        bar = self.layer
        pe = bar._vec(err[:8], 8, "err")
        L, rp = self._handle()
        _lib.check(L.iem_rmu_enter(rp, pe, float(mu)))

    def error(self, state, r, c, out=None):
        """The 32 words of ``iem_rmu_error`` as a device tensor: ``Restoration.error(state, r, c, 0, zeta_0)`` bit for bit, the
        minimum, sum and unusable count of the complementarity products, then ``(mu_k, E[0], E[1])`` of each candidate."""
        bar = self.layer
        out = out if out is not None else bar._new(32)
        ps = bar._state(state)
        args = (bar._vec(r, bar.nvar, "r"), bar._vec(c, bar.ncon, "c"), bar._vec(out, 32, "out"))
        L, rp = self._handle()
        _lib.check(L.iem_rmu_error(rp, *ps, *args))
        return out

    def update(self, out32):
        """The rule on the device (``iem_rmu_update``) from the 32 words of :meth:`error`."""
        pw = self.layer._vec(out32, 32, "out32")
        L, rp = self._handle()
        _lib.check(L.iem_rmu_update(rp, pw))

    def trigger(self, which: int, alpha):
        """Ipopt's ``alpha_min`` rule (``iem_rmu_trigger``) behind an ``accept`` of the original search of the restoration
        (``which = 0``) or of its inner search (``which = 1``); ``alpha``: that search's step lengths."""
        pa = self.layer._vec(alpha, 2, "alpha")
        L, rp = self._handle()
        _lib.check(L.iem_rmu_trigger(rp, int(which), pa))

    def state(self):
        """THE read-back (``iem_rmu_state``, one copy, synchronises once): the own block, the restoration block (``mu, tau, zeta``,
        ``mu_*``) and the restoration's state, ``status`` and ``resto_state`` also by name, ``changed`` / ``truncated`` = flag bits."""
        L, rp = self._handle()
        v = _lib.RmuState()
        v.struct_size = C.sizeof(_lib.RmuState)
        _lib.check(L.iem_rmu_state(rp, C.byref(v)))
        out = {name: getattr(v, name) for name, _ in _lib.RmuState._fields_ if name != "struct_size"}
        out["status_name"] = _lib.RMU_STATUS[out["status"]] if 0 <= out["status"] < len(_lib.RMU_STATUS) else "?"
        out["resto_state_name"] = _lib.RESTO_STATE[out["resto_state"]] if 0 <= out["resto_state"] < len(_lib.RESTO_STATE) else "?"
        out.update(changed=bool(out["flags"] & 1), truncated=bool(out["flags"] & 2))
        return out

    def device(self):
        """The address of the object's own block (16 words) on the device (``iem_rmu_device``)."""
        L, rp = self._handle()
        blk = C.c_void_p()
        _lib.check(L.iem_rmu_device(rp, C.byref(blk)))
        return blk.value

    def close(self):
        """Unbinds the restoration object and its inner search where they still read the block."""
        if self._r is not None:
            if self.inner_mu is not None:
                self.inner_mu._p = None      # owned by the object: destroyed with it
            _lib.check(self.layer.model._L.iem_rmu_destroy(self._r))
            self._r = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            if self.resto._q is not None and self.resto.search._s is not None and self.layer._b is not None and getattr(self.layer.model, "_h", None):
                self.close()
        except Exception:
            pass
