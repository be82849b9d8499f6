"""Witness of the adjoint parameter kind (hptprod), independent of the code under test: float64 torch autograd over the
Python restatement of the expression trees (param_witness.WitnessA), θ a leaf —
``∇θ (u · ∇ₓL(x, y, σ, θ)) = (∂²L/∂θ∂x)·u``."""
import numpy as np
import torch

from param_witness import WitnessA


class WitnessAdjoint(WitnessA):
    def hptprod(self, x, y, u, sigma=1.0):
        th = torch.tensor(self.theta0, dtype=torch.float64, requires_grad=True)
        if th.numel() == 0:
            return np.zeros(0)
        s = (torch.tensor(np.asarray(u), dtype=torch.float64) * self.grad_x_lag(x, y, sigma, th)).sum()
        if not s.requires_grad:
            return np.zeros(th.numel())
        (g,) = torch.autograd.grad(s, th, allow_unused=True)
        return np.zeros(th.numel()) if g is None else g.numpy()

    def gt_lambda(self, x, y, lam, sigma=1.0):
        """Gᵀλ with G = [∂²L/∂x∂θ ; ∂c/∂θ]: what the adjoint gradient subtracts, from autograd alone"""
        n = len(x)
        return self.hptprod(x, y, lam[:n], sigma) + self.jptprod(x, lam[n:], 0.0)
