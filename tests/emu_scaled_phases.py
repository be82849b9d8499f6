"""CPU emulation of the generated SCALED SOLVER PHASES (sp_cons / sp_jac / sp_hess / sp_obj / sp_grad and the two phase
kernels) — a test tool.

``emu.EmulatedModel`` compiled from the program the generator emits under ``scaled_phase_kinds = 1`` over the plain model: the
five kinds sit on the model's own table slots, the row factors ``s`` travel as ``v``, the multipliers as ``y``; the trial phase
(kind 9) writes ``c`` to ``out`` and the model's own ``f`` to ``aux``, the accepted phase (kind 10) the Jacobian to ``out``, the
Hessian to ``aux`` and the gradient to ``p2`` — its seed ``s_f`` rides on the head's word ``p4`` as the bits of a double, the
Hessian's objective weight is ``w``.  The factor of the objective meets the scalar on the host, as in the library."""
import ctypes as C

import numpy as np

from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib


class _Word:
    """a double whose bits travel as a pointer-sized word of the head (what ``_run`` passes for ``p4``)"""
    def __init__(self, value: float):
        self.ctypes = self
        self.data = C.c_void_p(int(np.float64(value).view(np.uint64)))


class EmulatedScaledPhases(EmulatedModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(scaled_phase_kinds=1, **opts):
            super().__init__(core, blob, store_mode)

    def set_theta(self, theta):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64) if len(theta) else np.zeros(1)

    def _s(self, s):
        return np.ascontiguousarray(s if s is not None and len(s) else np.zeros(1), dtype=np.float64)

    def cons_scaled(self, x, s):
        return self._run("cons", x, None, np.full(max(self.ncon, 1), np.nan), v=self._s(s))[:self.ncon]

    def jac_scaled(self, x, s, nnzj):
        return self._run("jac", x, None, np.full(max(nnzj, 1), np.nan), v=self._s(s))[:nnzj]

    def hess_scaled(self, x, y, s, w, nnzh):
        return self._run("hess", x, y, np.full(max(nnzh, 1), np.nan), w, v=self._s(s))[:nnzh]

    def grad_scaled(self, x, obj_scale):
        """Into a NaN-poisoned output: only the program's zero ranges are cleared beforehand."""
        return self._run("grad", x, None, self._scatter_out("grad"), obj_scale)[:self.nvar]

    def obj_scaled(self, x, obj_scale):
        return obj_scale * self.obj(x)

    def eval_trial_scaled(self, x, s, obj_scale):
        """One launch where the phase kernel exists, else the member launches — what ``iem_eval_trial_scaled`` does."""
        if not self.has("trial"):
            return self.obj_scaled(x, obj_scale), self.cons_scaled(x, s)
        c, f = np.full(max(self.ncon, 1), np.nan), np.full(1, np.nan)
        self._run("trial", x, None, c, v=self._s(s), aux=f, p2=np.zeros(self.n_partials + 2 + self.n_partials // 32))
        return obj_scale * float(f[0]), c[:self.ncon]

    def eval_accepted_scaled(self, x, y, s, obj_scale, obj_weight, nnzj, nnzh):
        w = obj_weight * obj_scale
        if not self.has("accepted"):
            return self.grad_scaled(x, obj_scale), self.jac_scaled(x, s, nnzj), self.hess_scaled(x, y, s, w, nnzh)
        jac, hess = np.full(max(nnzj, 1), np.nan), np.full(max(nnzh, 1), np.nan)
        g, ga = self._scatter_out("grad"), self._scatter_aux("grad")
        self._run("accepted", x, y, jac, w, v=self._s(s), aux=hess, p2=g, p3=ga, follow=("grad", g, ga), p4=_Word(obj_scale))
        return g[:self.nvar], jac[:nnzj], hess[:nnzh]
