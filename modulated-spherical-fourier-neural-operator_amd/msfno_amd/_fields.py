"""What the latitude-weighted field reductions (``losses``, ``verification``, ``ensemble``)
share: the device key of their caches, the latitude weights, the validation of fields against
them, the grid weight ``n = nlon sum(w)`` and the preallocated slots of a rollout's verifier."""
from __future__ import annotations

import torch

from . import _native as N


def device_key(device) -> torch.device:
    """``device`` with the index spelled out ("cuda" is the current device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def lat_weights(weights, nlat, device):
    """``weights`` as given, or the cached device vector of a ``losses.KINDS`` name."""
    if isinstance(weights, str):
        from . import losses
        return losses.device_weights(weights, nlat, device)
    return weights


def check_pair(prd, tar):
    if prd.dim() != 4 or prd.shape != tar.shape:
        raise ValueError(f"prd and tar must be (B, C, H, W) of one shape, got "
                         f"{tuple(prd.shape)} and {tuple(tar.shape)}")


def check_fields(x, tar, w, name, convert=N.require_device_f32, no_grad=None):
    """``x`` (through ``convert``), ``tar`` and ``w`` as fp32 device tensors on one device,
    ``w`` one weight per latitude row (dimension -2) of ``x``.  ``no_grad`` = (the sums that
    have no gradient, what to train with instead) refuses inputs that require one."""
    for n, t in ((name, x), ("tar", tar), ("w", w)) if no_grad else ():
        if t.requires_grad:
            raise ValueError(f"{n} requires grad: the {no_grad[0]} sums have no gradient; "
                             f"pass {n}.detach() (for training use {no_grad[1]})")
    x = convert(x, name)
    tar = N.require_device_f32(tar, "tar")
    w = N.require_device_f32(w, "w")
    nlat = x.shape[-2]
    if w.dim() != 1 or w.numel() != nlat:
        raise ValueError(f"w must hold one weight per latitude row ({nlat}), got "
                         f"{tuple(w.shape)}")
    if not (x.device == tar.device == w.device):
        raise ValueError(f"{name}, tar and w must be on one device")
    if x.numel() == 0:
        raise ValueError("empty fields")
    return x, tar, w


def grid_weight(w, nlon, device) -> torch.Tensor:
    """n = nlon * sum(w), in fp64 on ``device``."""
    return float(nlon) * torch.as_tensor(w).detach().double().sum().to(device)


class SlotVerifier:
    """Base of the rollout verifiers: the latitude weights ``w`` on ``device`` and, per
    result, one NaN-filled (n_scored, B, C, k) device tensor that ``update`` fills by slot."""

    def __init__(self, weights, nlat, nlon, n_scored, B, C, device):
        if min(nlat, nlon, n_scored, B, C) < 1:
            raise ValueError("nlat, nlon, n_scored, B and C must be >= 1")
        self.device = device_key(device)
        w = lat_weights(weights, nlat, self.device)
        w = N.require_device_f32(torch.as_tensor(w).detach().to(self.device), "weights")
        if w.dim() != 1 or w.numel() != nlat:
            raise ValueError(f"weights must hold one weight per latitude row ({nlat}), got "
                             f"{tuple(w.shape)}")
        self.w = w
        self._slots = (n_scored, B, C)

    def _alloc(self, k):
        return torch.full(self._slots + (k,), float("nan"), dtype=torch.float32,
                          device=self.device)

    def _check_slot(self, k, x, what):
        if not 0 <= k < self._slots[0]:
            raise IndexError(f"slot {k} of {self._slots[0]}")
        if tuple(x.shape) != self.shape:
            raise ValueError(f"expected {what} of shape {self.shape}, got {tuple(x.shape)}")

    def _on_device(self, t):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            return t.to(self.device, non_blocking=True)
        return t
