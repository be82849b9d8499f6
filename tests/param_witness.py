"""Witnesses of the parameter sensitivities (jpprod / jptprod / hpprod), independent of the code under test.

A: float64 torch autograd over the Python restatement of the recorded expression trees (helpers.TorchModel), with θ a
leaf that requires grad.  B: the oracle under ``set_parameter`` — Richardson-extrapolated central differences of its
``cons`` / ``grad`` / ``jtprod`` along a direction of θ."""
import numpy as np
import torch

from helpers import TorchModel


class WitnessA:
    def __init__(self, core, theta=None):
        self.tm = TorchModel(core)
        self.theta0 = np.asarray(core.theta if theta is None else theta, dtype=np.float64)

    def _lag(self, xt, tht, yt, sigma):
        self.tm.theta = tht
        c = self.tm.cons(xt)
        return sigma * self.tm.obj(xt) + ((yt * c).sum() if c.numel() else 0.0)

    def jpprod(self, x, w):
        """(∂c/∂θ)·w by forward-over-reverse: d/dε c(x, θ + εw)"""
        xt = torch.tensor(np.asarray(x), dtype=torch.float64)
        wt = torch.tensor(np.asarray(w), dtype=torch.float64)

        def c_of(th):
            self.tm.theta = th
            return self.tm.cons(xt)
        th = torch.tensor(self.theta0, dtype=torch.float64)
        if th.numel() == 0:
            return np.zeros(c_of(th).numel())
        _, jv = torch.autograd.functional.jvp(c_of, th, wt)
        return jv.numpy()

    def jptprod(self, x, y, sigma=1.0):
        """σ ∂f/∂θ + (∂c/∂θ)ᵀ y = ∇θ L"""
        xt = torch.tensor(np.asarray(x), dtype=torch.float64)
        yt = torch.tensor(np.asarray(y), dtype=torch.float64)
        th = torch.tensor(self.theta0, dtype=torch.float64, requires_grad=True)
        if th.numel() == 0:
            return np.zeros(0)
        L = self._lag(xt, th, yt, sigma)
        if not (isinstance(L, torch.Tensor) and L.requires_grad):
            return np.zeros(th.numel())
        (g,) = torch.autograd.grad(L, th, allow_unused=True)
        return np.zeros(th.numel()) if g is None else g.numpy()

    def grad_x_lag(self, x, y, sigma, theta):
        """σ∇f + Jᵀy as a differentiable function of θ"""
        xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
        yt = torch.tensor(np.asarray(y), dtype=torch.float64)
        L = self._lag(xt, theta, yt, sigma)
        (g,) = torch.autograd.grad(L, xt, create_graph=True, allow_unused=True)
        return torch.zeros_like(xt) if g is None else g

    def hpprod(self, x, y, w, sigma=1.0):
        """(∂²L/∂x∂θ)·w: the directional derivative along w of ∇ₓL"""
        wt = torch.tensor(np.asarray(w), dtype=torch.float64)
        th = torch.tensor(self.theta0, dtype=torch.float64)
        if th.numel() == 0:
            return np.zeros(len(x))
        _, jv = torch.autograd.functional.jvp(lambda t: self.grad_x_lag(x, y, sigma, t), th, wt)
        return jv.numpy()

    def dfdtheta_dot(self, x, w):
        """∂f/∂θ · w"""
        return float(self.jptprod(x, np.zeros(self.tm.cons(torch.tensor(np.asarray(x), dtype=torch.float64)).numel()), 1.0) @ np.asarray(w)) if len(w) else 0.0


class WitnessB:
    """Richardson-extrapolated central differences of the oracle along w: D(h) = (F(θ+hw) − F(θ−hw)) / 2h,
    (4·D(h/2) − D(h)) / 3 — fourth-order in h."""

    def __init__(self, om, theta, h=1e-3):
        self.om, self.theta, self.h = om, np.asarray(theta, dtype=np.float64).copy(), h

    def _d(self, F, w):
        def D(h):
            self.om.set_parameter(0, self.theta + h * w)
            a = np.array(F(), dtype=np.float64)
            self.om.set_parameter(0, self.theta - h * w)
            b = np.array(F(), dtype=np.float64)
            return (a - b) / (2 * h)
        try:
            return (4.0 * D(self.h / 2) - D(self.h)) / 3.0
        finally:
            self.om.set_parameter(0, self.theta)

    def jpprod(self, x, w):
        return self._d(lambda: self.om.cons(x), np.asarray(w))

    def hpprod(self, x, y, w, sigma=1.0):
        return self._d(lambda: sigma * self.om.grad(x) + self.om.jtprod(x, y), np.asarray(w))
