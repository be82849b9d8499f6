"""CPU emulation of the generated RESIDUAL program (lagrad / cons / obj and their one-launch phase) — a test tool.

``emu.EmulatedModel`` compiled from the program the generator emits under ``param_kinds = 5`` over the plain model: lagrad
= σ·∇f + Jᵀ·y sits on the table slot of jtprod (kind 6) with jtprod's pointers (``v`` = y, ``w`` = σ, ``nvar`` entries out,
the same deterministic follow-ups), next to the model's own cons and obj; the phase launch is kind 9 with lagrad as its
third member (p3 = its output, p4 = its reduction buffer)."""
import numpy as np

from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib


class EmulatedLagradModel(EmulatedModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(param_kinds=5, **opts):
            super().__init__(core, blob, store_mode)

    def set_theta(self, theta):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64) if len(theta) else np.zeros(1)

    def _partials(self):
        return np.zeros(self.n_partials + 2 + self.n_partials // 32)      # partials + tickets

    def lagrad(self, x, y, obj_weight=1.0):
        """Into a NaN-poisoned output: only the program's zero_ranges are cleared beforehand (emu._scatter_out).
        ``y`` may be None on a model without constraints."""
        return self._run("jtprod", x, None, self._scatter_out("jtprod"), obj_weight, v=y)[:self.nvar]

    def eval_residual(self, x, y, obj_weight=1.0):
        """The phase launch: out = c, aux = the objective scalar, p2 = partials + tickets, p3 = the residual, p4 = its
        reduction buffer; lagrad's follow-ups run behind it.  Returns (f, c, r)."""
        assert self.has("trial"), "no phase kernel in this program"
        c, f = np.full(max(self.ncon, 1), np.nan), np.full(1, np.nan)
        r, ra = self._scatter_out("jtprod"), self._scatter_aux("jtprod")
        self._run("trial", x, None, c, obj_weight, v=y, aux=f, p2=self._partials(), p3=r, p4=ra, follow=("jtprod", r, ra))
        return float(f[0]), c[:self.ncon], r[:self.nvar]
