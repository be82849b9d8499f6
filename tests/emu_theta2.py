"""CPU emulation of the generated θθ parameter kind (hppprod) — a test tool.

``emu_param.EmulatedParamModel`` compiled from the program the generator emits under ``param_kinds = 3``: hppprod alone,
on the table slot of hprod (kind 7) with hprod's pointers (``v`` = the tangent w over θ) and jptprod's output (``npar``
entries, the same deterministic follow-ups)."""
import numpy as np

from emu import EmulatedModel
from emu_param import EmulatedParamModel
from infiniteexamodels.jl_amd import lib as iemlib


class EmulatedTheta2Model(EmulatedParamModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(param_kinds=3, **opts):
            EmulatedModel.__init__(self, core, blob, store_mode)

    def hppprod(self, x, y, w, obj_weight=1.0):
        if self.npar == 0:
            return np.zeros(0)
        return self._run("hprod", x, y, self._out("hprod", self.npar), obj_weight, v=w)[:self.npar]
