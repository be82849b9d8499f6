"""CPU emulation of the generated KKT OPERATOR (kktx / kkty / the one-launch kernel) — a test tool.

``emu.EmulatedModel`` compiled from the program the generator emits under ``kkt_kinds = 1`` over the plain model: kktx
(``W·u + Jᵀ·v``) sits on the table slot of hprod (kind 7, ``nvar`` entries out, scattered like hprod's), kkty (``J·u``) on that of
jprod (kind 5), and the phase slot trial (kind 9) holds both behind one dispatcher.  ``u`` travels as ``v``, the dual direction
as the head's last word ``p6``; the phase kernel writes kkty's rows through ``p2``."""
import numpy as np

from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib


class EmulatedKktModel(EmulatedModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(kkt_kinds=1, **opts):
            super().__init__(core, blob, store_mode)

    def set_theta(self, theta):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64) if len(theta) else np.zeros(1)

    def _dv(self, v):
        """``None`` is the C-ABI's NULL: a vector of zeros"""
        return np.ascontiguousarray(v if v is not None else np.zeros(max(self.ncon, 1)), dtype=np.float64)

    def kktx(self, x, y, u, v, w):
        """Into a NaN-poisoned output: only the program's zero ranges are cleared beforehand."""
        return self._run("hprod", x, y, self._scatter_out("hprod"), w, v=u, p6=self._dv(v))[:self.nvar]

    def kkty(self, x, u):
        return self._run("jprod", x, None, np.full(max(self.ncon, 1), np.nan), v=u)[:self.ncon]

    def kktprod(self, x, y, u, v, w):
        """One launch where the phase kernel exists, else the two member launches — what ``iem_kktprod`` does."""
        if not self.has("trial"):
            return self.kktx(x, y, u, v, w), self.kkty(x, u)
        ox, oy = self._scatter_out("hprod"), np.full(max(self.ncon, 1), np.nan)
        aux = self._scatter_aux("hprod")
        self._run("trial", x, y, ox, w, v=u, aux=aux, p2=oy, p6=self._dv(v), follow=("hprod", ox, aux))
        return ox[:self.nvar], oy[:self.ncon]
