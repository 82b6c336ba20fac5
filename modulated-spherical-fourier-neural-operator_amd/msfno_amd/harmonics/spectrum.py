"""Per-degree power spectrum of spherical-harmonic coefficients on the native kernels
(csrc/spectrum.hip: ``msfno_spectrum_power`` and its gradient).

    power[..., l] = |c[..., l, 0]|^2 + 2 sum_{m >= 1} |c[..., l, m]|^2

This is the middle step of the reference's spectral losses (MSFNO/Models/losses.py:158-232,
mirrored in ``msfno_amd.losses``) and the diagnostic of a long rollout: spectral blow-up
or blurring shows per degree and lead time.  The weight 2 applies to every m >= 1 and all
m of a row are read, so any (..., lmax, mmax) coefficient tensor is accepted, not only a
transform's output.  The result is bitwise reproducible (no atomics).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _native as N


@N.on_input_device
def _native_power(c):
    lmax, mmax = c.shape[-2:]
    n = c.numel() // (lmax * mmax)
    power = torch.empty(c.shape[:-1], dtype=torch.float32, device=c.device)
    N.check(N.lib().msfno_spectrum_power(c.data_ptr(), power.data_ptr(), n, lmax, mmax,
                                         N.stream_of(c.device)), "msfno_spectrum_power")
    return power


@N.on_input_device
def _native_power_backward(c, g):
    lmax, mmax = c.shape[-2:]
    n = c.numel() // (lmax * mmax)
    dc = torch.empty_like(c)
    N.check(N.lib().msfno_spectrum_power_backward(c.data_ptr(), g.data_ptr(), dc.data_ptr(), n,
                                                  lmax, mmax, N.stream_of(c.device)),
            "msfno_spectrum_power_backward")
    return dc


class _PowerSpectrum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c):
        ctx.save_for_backward(c)
        return _native_power(c)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (c,) = ctx.saved_tensors
        # dL/dRe + i dL/dIm = 2 e_m g c, torch's convention for a complex input
        return _native_power_backward(c, N.require_device_f32(grad, "grad").resolve_neg())


def power_spectrum(coeffs: torch.Tensor) -> torch.Tensor:
    """(..., lmax, mmax) complex64 on the GPU -> (..., lmax) fp32, differentiable in
    ``coeffs`` (no double backward).  Another complex dtype or a non-contiguous tensor is
    converted by torch ops that autograd sees."""
    if not coeffs.is_cuda:
        raise ValueError("power_spectrum input must be a GPU (HIP) tensor; libmsfno has no "
                         "CPU path")
    if coeffs.dim() < 2:
        raise ValueError(f"power_spectrum input must be (..., lmax, mmax), got "
                         f"{tuple(coeffs.shape)}")
    if coeffs.numel() == 0:
        raise ValueError("empty coefficient tensor")
    if not coeffs.is_complex():
        raise ValueError(f"power_spectrum input must be complex, got {coeffs.dtype}")
    if coeffs.dtype != torch.complex64:
        coeffs = coeffs.to(torch.complex64)
    return _PowerSpectrum.apply(coeffs.resolve_conj().contiguous())
