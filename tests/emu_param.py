"""CPU emulation of the generated PARAMETER kinds (jpprod / jptprod / hpprod) — a test tool.

``emu.EmulatedModel`` compiled from the program the generator emits under ``param_kinds = 1``: the three kinds sit on
the table slots of jprod / jtprod / hprod (kinds 5 / 6 / 7), with the same pointers and follow-ups; jptprod's output has
``npar`` entries and takes the objective weight."""
import numpy as np

from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib


class EmulatedParamModel(EmulatedModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(param_kinds=1, **opts):
            super().__init__(core, blob, store_mode)

    def set_theta(self, theta):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64) if len(theta) else np.zeros(1)

    def _out(self, kind: str, n: int):
        """NaN-poisoned output with exactly the runtime's memset ranges applied"""
        out = np.full(max(n, 1), np.nan)
        for k, lo, hi in self.zero_ranges:
            if k == self.KINDS[kind]:
                out[lo:hi] = 0.0
        return out

    def jpprod(self, x, w):
        return self._run("jprod", x, None, np.full(max(self.ncon, 1), np.nan), v=w)[:self.ncon]

    def jptprod(self, x, y, obj_weight=1.0):
        if self.npar == 0:
            return np.zeros(0)
        return self._run("jtprod", x, None, self._out("jtprod", self.npar), obj_weight, v=y)[:self.npar]

    def hpprod(self, x, y, w, obj_weight=1.0):
        return self._run("hprod", x, y, self._out("hprod", self.nvar), obj_weight, v=w)[:self.nvar]
