"""Sphere-weighted training losses on the native kernels — mirror of the losses that
``MSFNO/Models/train.py:434-446`` builds from ``MSFNO/Models/losses.py`` (``L2Sphere``,
``L2Sphere_noSine``, ``CosineMSELoss``) and of the validation MSEs of ``train.py:553-564``.

All of them are, per (batch, channel),

    num = sum_h w[h] sum_x (prd - tar)^2,      den = sum_h w[h] sum_x tar^2

under different latitude weights ``w``: one pass over both fields (``msfno_loss_sums``)
and one for the gradient (``msfno_loss_backward``).  What remains (``relative``,
``squared``, the reductions) is plain torch on the (B, C) sums, so autograd gives it the
reference's semantics.  The target takes no gradient, as in the reference's training loop.

``weighted_sums(prd, tar, w)`` is the band-local entry: a latitude-band rank passes its
own rows and ``w[rows]`` and all-reduces the (B, C, 2) result.

The spectral losses of ``losses.py:158-232`` (``spectral_l2loss_sphere``,
``spectral_loss_sphere``, ``h1loss_sphere``) are at the end of this module: a
differentiable forward transform, the native per-degree power spectrum and torch ops on
the spectra; there the target may require grad.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _fields as F
from . import _native as N
from . import harmonics as _harmonics
from .harmonics import quadrature

KINDS = ("l2sphere", "l2sphere_nosine", "cosine", "uniform")


def sphere_weights(kind: str, nlat: int, eps: float = 1e-4) -> np.ndarray:
    """The latitude weights of one loss, float64 on the host, as the reference forms
    them (losses.py:16-19, 90-94, 129-132); ``eps`` is CosineMSELoss's pole weight."""
    if nlat < 1:
        raise ValueError(f"nlat must be >= 1, got {nlat}")
    if kind == "uniform":
        return np.ones(nlat, dtype=np.float64)
    if kind == "l2sphere_nosine":
        return np.asarray(quadrature.legendre_gauss_weights(nlat, -1, 1)[1], dtype=np.float64)
    lat = np.linspace(-np.pi / 2, np.pi / 2, nlat, dtype=np.float64)
    if kind == "l2sphere":
        w_quad = np.asarray(quadrature.legendre_gauss_weights(nlat, -1, 1)[1], dtype=np.float64)
        return np.abs(w_quad * np.cos(lat))
    if kind == "cosine":
        w = np.clip(np.cos(lat), 0.0, None) + eps
        return w / w.sum()
    raise ValueError(f"unknown weight kind {kind!r}; one of {KINDS}")


_weight_cache: dict = {}


def device_weights(kind: str, nlat: int, device, eps: float = 1e-4) -> torch.Tensor:
    """fp32 device copy of ``sphere_weights``, cached per (kind, nlat, eps, device)."""
    device = F.device_key(device)
    key = (kind, int(nlat), float(eps), device)
    w = _weight_cache.get(key)
    if w is None:
        w = torch.from_numpy(sphere_weights(kind, nlat, eps)).to(torch.float32).to(device)
        _weight_cache[key] = w
    return w


@N.on_input_device
def _native_sums(prd, tar, w):
    B, C, H, W = prd.shape
    lib = N.lib()
    sums = torch.empty(B, C, 2, dtype=torch.float32, device=prd.device)
    ws = torch.empty(lib.msfno_loss_workspace_size(B * C, H, W), dtype=torch.uint8,
                     device=prd.device)
    N.check(lib.msfno_loss_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), sums.data_ptr(),
                                B * C, H, W, ws.data_ptr(), ws.numel(),
                                N.stream_of(prd.device)), "msfno_loss_sums")
    return sums


@N.on_input_device
def _native_backward(prd, tar, w, gnum):
    B, C, H, W = prd.shape
    dprd = torch.empty_like(prd)
    N.check(N.lib().msfno_loss_backward(prd.data_ptr(), tar.data_ptr(), w.data_ptr(),
                                        gnum.data_ptr(), dprd.data_ptr(), B * C, H, W,
                                        N.stream_of(prd.device)), "msfno_loss_backward")
    return dprd


class _WeightedSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prd, tar, w):
        ctx.save_for_backward(prd, tar, w)
        return _native_sums(prd, tar, w)

    @staticmethod
    def backward(ctx, grad):
        prd, tar, w = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        gnum = N.require_device_f32(grad[..., 0], "grad")
        return _native_backward(prd, tar, w, gnum), None, None


def weighted_sums(prd: torch.Tensor, tar: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """(B, C, 2) = {num, den} of (B, C, H, W) fields under the latitude weights ``w``
    (any fp32 device vector of length H).  Differentiable in ``prd`` through ``num``."""
    F.check_pair(prd, tar)
    if tar.requires_grad:
        raise NotImplementedError(
            "the gradient with respect to the target is not implemented (the reference "
            "never differentiates it, train.py:162); pass tar.detach()")
    return _WeightedSums.apply(*F.check_fields(prd, tar, w, "prd"))


def _refuse_none(name, reduction):
    if reduction == "none":
        raise NotImplementedError(
            f"{name}(reduction='none') returns a full-size field and has no use in "
            "get_loss(...).backward() (train.py:162); not implemented natively")


class _L2SphereBase(nn.Module):
    kind = ""

    def __init__(self, relative=True, squared=False, reduction="sum", dampening=None):
        super().__init__()
        _refuse_none(type(self).__name__, reduction)
        self.relative = relative
        self.squared = squared
        self.reduction = reduction

    def forward(self, prd, tar):
        s = weighted_sums(prd, tar, device_weights(self.kind, prd.shape[2], prd.device))
        loss = s[..., 0]
        if self.relative:
            loss = loss / s[..., 1]
        if not self.squared:
            loss = torch.sqrt(loss)
        # "mean" is the sum too ("mean is done by weights", losses.py:110-113); any other
        # reduction string returns the (B, C) tensor (:116-117)
        if self.reduction in ("mean", "sum"):
            return loss.sum()
        return loss


class L2Sphere(_L2SphereBase):
    """losses.py:80-117: weights |Gauss-Legendre quadrature weight x cos(latitude)|."""
    kind = "l2sphere"


class L2Sphere_noSine(_L2SphereBase):
    """losses.py:119-155 (the default of --loss-fn): the quadrature weights alone."""
    kind = "l2sphere_nosine"


class CosineMSELoss(nn.Module):
    """losses.py:6-28: squared error under clamp(cos(latitude), 0) + eps, normalised to
    sum 1.  "mean" is sum / (B C H W), "sum" is sum / W, as the reference has them."""

    def __init__(self, reduction="mean", eps=1e-4):
        super().__init__()
        _refuse_none("CosineMSELoss", reduction)
        if reduction not in ("mean", "sum"):
            raise ValueError(f"CosineMSELoss: unknown reduction {reduction!r}")
        self.reduction = reduction
        self.eps = eps

    def forward(self, x, y):
        B, C, H, W = x.shape
        total = weighted_sums(x, y, device_weights("cosine", H, x.device, self.eps))[..., 0].sum()
        if self.reduction == "mean":
            return total / (B * C * H * W)
        return total / W


def mse(prd, tar):
    """torch.nn.MSELoss()(prd, tar) (train.py:553): a scalar."""
    B, C, H, W = prd.shape
    s = weighted_sums(prd, tar, device_weights("uniform", H, prd.device))
    return s[..., 0].sum() / (B * C * H * W)


def per_variable_mse(prd, tar):
    """MSELoss(reduction='none')(prd, tar).mean(dim=(0, 2, 3)) (train.py:564): (C,)."""
    B, C, H, W = prd.shape
    s = weighted_sums(prd, tar, device_weights("uniform", H, prd.device))
    return s[..., 0].sum(dim=0) / (B * H * W)


# ---- spectral losses (MSFNO/Models/losses.py:158-232) ---------------------------------
# Each is the forward transform of prd - tar (subtracted on the grid first, as the
# reference does: that keeps the conditioning when prd is close to tar), the per-degree
# power spectrum of the coefficients (harmonics.power_spectrum, csrc/spectrum.hip) and
# plain torch on the (..., C, lmax) spectra.  Both native steps are autograd ops, so the
# reference's semantics follow, a target that requires grad included.  As in the
# reference the sum runs over the last two dimensions of the spectra -- degree AND channel
# (losses.py:163: norm2 is (B, C, lmax)) -- before ``relative`` / ``squared``, and the
# result is the mean over what remains (the batch).

def _forward_transform(solver):
    """The transform of a reference-style solver (``solver.sht``) or the transform
    itself; one of another library (torch-harmonics) is adopted, its table shared."""
    return _harmonics.adopt(getattr(solver, "sht", solver), inverse=False)


def _degree_spectrum(sht, field):
    if not field.is_cuda:
        raise ValueError("prd and tar must be GPU (HIP) tensors; libmsfno has no CPU path")
    return _harmonics.power_spectrum(sht(field))


def _degree_weights(sht, device):
    ls = torch.arange(sht.lmax).float()  # l (l + 1) in fp32, as the reference forms it
    return (ls * (ls + 1)).to(device)


def _finish(loss, squared):
    if not squared:
        loss = torch.sqrt(loss)
    return loss.mean()


def spectral_l2loss_sphere(solver, prd, tar, relative=False, squared=True):
    """losses.py:158-176: the L2 norm of prd - tar from its spectrum."""
    sht = _forward_transform(solver)
    loss = _degree_spectrum(sht, prd - tar).sum(dim=(-1, -2))
    if relative:
        loss = loss / _degree_spectrum(sht, tar).sum(dim=(-1, -2))
    return _finish(loss, squared)


def spectral_loss_sphere(solver, prd, tar, relative=False, squared=True):
    """losses.py:178-203: the same under the weights l (l + 1) (the H1 seminorm)."""
    sht = _forward_transform(solver)
    w = _degree_weights(sht, prd.device)
    loss = (w * _degree_spectrum(sht, prd - tar)).sum(dim=(-1, -2))
    if relative:
        loss = loss / (w * _degree_spectrum(sht, tar)).sum(dim=(-1, -2))
    return _finish(loss, squared)


def h1loss_sphere(solver, prd, tar, relative=False, squared=True):
    """losses.py:205-232: seminorm + L2 norm (of the roots unless ``squared``: "strictly
    speaking this is not exactly h1 loss", :220)."""
    if relative:
        raise NotImplementedError("Relative H1 loss not implemented")
    sht = _forward_transform(solver)
    power = _degree_spectrum(sht, prd - tar)
    h1 = (_degree_weights(sht, prd.device) * power).sum(dim=(-1, -2))
    l2 = power.sum(dim=(-1, -2))
    if not squared:
        return (torch.sqrt(h1) + torch.sqrt(l2)).mean()
    return (h1 + l2).mean()
