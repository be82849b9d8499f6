"""Witness of the θθ parameter kind (hppprod), independent of the code under test: float64 torch autograd over the
Python restatement of the expression trees (param_witness.WitnessA._lag), θ a leaf, double backward —
``∇θ (w · ∇θL(x, y, σ, θ)) = (∂²L/∂θ²)·w``.  (On top of WitnessAdjoint, so that one object has every product of G too.)"""
import numpy as np
import torch

from adjoint_witness import WitnessAdjoint


class WitnessTheta2(WitnessAdjoint):
    def hppprod(self, x, y, w, sigma=1.0):
        th = torch.tensor(self.theta0, dtype=torch.float64, requires_grad=True)
        if th.numel() == 0:
            return np.zeros(0)
        xt = torch.tensor(np.asarray(x), dtype=torch.float64)
        yt = torch.tensor(np.asarray(y), dtype=torch.float64)
        L = self._lag(xt, th, yt, sigma)
        if not (isinstance(L, torch.Tensor) and L.requires_grad):
            return np.zeros(th.numel())
        (g,) = torch.autograd.grad(L, th, create_graph=True, allow_unused=True)
        if g is None or not g.requires_grad:      # θ absent, or entering linearly: the θθ block is zero
            return np.zeros(th.numel())
        (h,) = torch.autograd.grad((torch.tensor(np.asarray(w), dtype=torch.float64) * g).sum(), th, allow_unused=True)
        return np.zeros(th.numel()) if h is None else h.numpy()

    def theta2_matrix(self, x, y, sigma=1.0):
        """the dense ∂²L/∂θ² (npar × npar), a column per unit vector — small models only"""
        n = len(self.theta0)
        return np.stack([self.hppprod(x, y, np.eye(n)[j], sigma) for j in range(n)], axis=1)
