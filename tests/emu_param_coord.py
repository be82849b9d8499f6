"""CPU emulation of the explicit θ blocks in COO (jacp_coord / hessp_coord) — a test tool.

``emu_param.EmulatedParamModel`` compiled from the program the generator emits under ``param_kinds = 4``: jacp on the
table slot of jac_coord! (kind 1, ``out`` = the values of ∂c/∂θ) and hessp on that of hess_coord! (kind 2, ``out`` = the
values of ∂²L/∂x∂θ, ``aux`` = those of ∂²L/∂θ², both from one sweep).  Structures from the blob alone."""
import numpy as np

from emu import EmulatedModel
from emu_param import EmulatedParamModel
from infiniteexamodels.jl_amd import lib as iemlib

GUARD = 64      # doubles behind every output buffer that must stay NaN


class EmulatedParamCoordModel(EmulatedParamModel):
    def __init__(self, core, blob: bytes = None, store_mode: int = 2, **opts):
        with iemlib.options(param_kinds=4, **opts):
            EmulatedModel.__init__(self, core, blob, store_mode)
        self.structure = [iemlib.blob_param_coord_structure(self.blob, w) for w in range(3)]
        self.nnz = tuple(len(r) for r, _ in self.structure)

    def jacp_coord(self, x):
        """the whole buffer: ``nnz[0]`` values and the NaN guard behind them"""
        out = np.full(self.nnz[0] + GUARD, np.nan)
        if self.has("jac"):
            self._run("jac", x, None, out, aux=np.zeros(1))
        return out

    def hessp_coord(self, x, y, obj_weight=1.0):
        xp, pp = np.full(self.nnz[1] + GUARD, np.nan), np.full(self.nnz[2] + GUARD, np.nan)
        if self.has("hess"):
            self._run("hess", x, y, xp, obj_weight, aux=pp)
        return xp, pp
