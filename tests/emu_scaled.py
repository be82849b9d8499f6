"""CPU emulation of the generated SCALED program (rowmax / cons_scaled / jac_scaled) — a test tool.

``emu.EmulatedModel`` compiled from the program the generator emits under ``scaled_kinds = 1`` over the plain model: the row
maxima sit on the table slot of jprod (kind 5, ``ncon`` entries out, no tangent), the scaled constraints on that of cons
(kind 0) and the scaled Jacobian on that of jac (kind 1); the factors ``s`` travel as ``v``."""
import numpy as np

from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib


class EmulatedScaledModel(EmulatedModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(scaled_kinds=1, **opts):
            super().__init__(core, blob, store_mode)

    def set_theta(self, theta):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64) if len(theta) else np.zeros(1)

    def rowmax(self, x):
        """Into a NaN-poisoned output: every row must be written."""
        return self._run("jprod", x, None, np.full(max(self.ncon, 1), np.nan))[:self.ncon]

    def cons_scaled(self, x, s):
        return self._run("cons", x, None, np.full(max(self.ncon, 1), np.nan), v=s)[:self.ncon]

    def jac_scaled(self, x, s, nnzj):
        return self._run("jac", x, None, np.full(max(nnzj, 1), np.nan), v=s)[:nnzj]
