"""Gaussian random fields on the sphere: the sibling of ``torch_harmonics``'
``GaussianRandomFieldS2`` on this package's ortho transforms, for perturbed initial
states and stochastic forcing of an ensemble.

A field is ``isht(sqrt_eig[l] xi[l, m])`` with complex Gaussian ``xi``: ``m = 0`` real with
unit variance, real and imaginary parts of ``1 <= m <= l`` with variance 1/2 each, zero above
the diagonal.  Under the ortho transforms this is isotropic: the pointwise variance is the
same at every latitude and equals ``field_variance(sqrt_eig) = sum_l (2l + 1) / (4 pi)
sqrt_eig[l]^2``.  The coefficients come from one native kernel (``msfno_noise_spectral``,
csrc/noise.hip), written directly in the layout the inverse transform reads.  Its stream
is a pure function of (seed, draw, field index, l, m) (a counter-based Philox4x32-10, see
DESIGN.md §9l): it does not depend on the launch geometry or on how the fields are split
over calls, and it does not touch torch's generator.

``SphericalAR1`` is the red-in-time process ``c <- phi c + sqrt(1 - phi^2) sqrt_eig xi``
with its draw counter in device memory: a ``step()`` captured into a HIP graph yields
fresh noise on every replay.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from .sht import InverseRealSHT

_U64 = (1 << 64) - 1


def matern_sqrt_eig(lmax, alpha=2.0, tau=3.0, sigma=None, radius=1.0):
    """fp64 (lmax,): ``sigma (l (l + 1) / radius^2 + tau^2)^(-alpha / 2)`` with entry 0 set
    to 0 (no mean), the square roots of the eigenvalues of the covariance
    ``sigma^2 (-Laplacian + tau^2)^(-alpha)``.  ``sigma`` defaults to ``tau^(alpha - 1)``
    (torch-harmonics' choice), which needs ``alpha > 1``."""
    if lmax < 1:
        raise ValueError(f"lmax must be >= 1, got {lmax}")
    if sigma is None:
        if not alpha > 1.0:
            raise ValueError(f"alpha must be greater than 1 when sigma is not given, got {alpha}")
        sigma = tau ** (alpha - 1.0)
    l = torch.arange(lmax, dtype=torch.float64)
    s = sigma * (l * (l + 1) / radius ** 2 + tau ** 2) ** (-alpha / 2.0)
    s[0] = 0.0
    return s


def field_variance(sqrt_eig):
    """The pointwise variance of the field of each row of ``sqrt_eig`` (..., lmax):
    ``sum_l (2l + 1) / (4 pi) sqrt_eig[l]^2``, in fp64."""
    s = torch.as_tensor(sqrt_eig).double()
    l = torch.arange(s.shape[-1], dtype=torch.float64, device=s.device)
    return ((2 * l + 1) / (4 * math.pi) * s * s).sum(-1)


def unit_variance(sqrt_eig):
    """``sqrt_eig`` with every row scaled to a field of pointwise variance 1 (fp64): an
    amplitude applied later is then a standard deviation in field units."""
    s = torch.as_tensor(sqrt_eig).double()
    return s / torch.sqrt(field_variance(s)).unsqueeze(-1)


def _require_device(t, what):
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the GPU (HIP); libmsfno has no CPU path")


def _fill(coeffs, prev, sqrt_eig, K, n, lmax, mmax, a, b, seed, draw, draw_dev):
    """One ``msfno_noise_spectral`` launch on the current stream of ``coeffs``' device."""
    with torch.cuda.device(coeffs.device):
        N.check(N.lib().msfno_noise_spectral(
            coeffs.data_ptr(), N.ptr(prev), sqrt_eig.data_ptr(), K, n, 0, lmax, mmax, a, b,
            seed & _U64, draw & _U64, N.ptr(draw_dev), N.stream_of(coeffs.device)),
            "msfno_noise_spectral")
    return coeffs


class GaussianRandomFieldS2(nn.Module):
    """Samples of a mean-free isotropic Gaussian random field on the (nlat, nlon) grid.

    ``nlon`` defaults to ``2 nlat``; ``lmax`` to ``min(nlat, nlon // 2)`` and ``mmax = lmax``,
    so the Nyquist bin, whose imaginary part the real FFT drops, is never populated (a
    larger ``lmax`` raises ValueError).  The spectrum is Matérn (``matern_sqrt_eig``) unless
    ``sqrt_eig`` is given: ``(lmax,)`` for one spectrum (samples are (N, nlat, nlon)) or
    ``(K, lmax)`` for one per channel (samples are (N, K, nlat, nlon)), for example a
    climatological spectrum from ``power_spectrum`` with per-channel amplitudes folded in.

    Persistent buffers: ``sqrt_eig`` (fp32) and ``rng_state`` (int64: seed, next draw), so a
    ``state_dict`` round trip continues the stream.  Every ``sample_coeffs`` consumes one
    draw.  Only this package's ortho normalisation and GPU tensors, as the transforms."""

    def __init__(self, nlat, nlon=None, lmax=None, alpha=2.0, tau=3.0, sigma=None, radius=1.0,
                 grid="equiangular", sqrt_eig=None, seed=0, norm="ortho"):
        super().__init__()
        nlon = 2 * nlat if nlon is None else nlon
        cap = min(nlat, nlon // 2)
        lmax = cap if lmax is None else lmax
        if lmax < 1 or lmax > cap:
            raise ValueError(f"lmax must be in 1 .. min(nlat, nlon // 2) = {cap}, got {lmax}: "
                             "the Nyquist bin of the longitude FFT cannot carry an isotropic "
                             "field")
        self.nlat, self.nlon, self.lmax, self.mmax, self.grid = nlat, nlon, lmax, lmax, grid
        if sqrt_eig is None:
            sqrt_eig = matern_sqrt_eig(lmax, alpha, tau, sigma, radius)
        sqrt_eig = torch.as_tensor(sqrt_eig).detach()
        if sqrt_eig.dim() not in (1, 2) or sqrt_eig.shape[-1] != lmax or sqrt_eig.numel() == 0:
            raise ValueError(f"sqrt_eig must be ({lmax},) or (K, {lmax}), got "
                             f"{tuple(sqrt_eig.shape)}")
        self.K = None if sqrt_eig.dim() == 1 else sqrt_eig.shape[0]
        self.isht = InverseRealSHT(nlat, nlon, lmax=lmax, mmax=lmax, grid=grid, norm=norm).float()
        self.register_buffer("sqrt_eig", sqrt_eig.float().contiguous().clone())
        self.register_buffer("rng_state", torch.zeros(2, dtype=torch.int64))
        self.reseed(seed)

    def reseed(self, seed, draw=0):
        """Restart the stream at (``seed``, ``draw``)."""
        self._rng = (int(seed) & _U64, int(draw) & _U64)
        self._store_rng()

    def _store_rng(self):
        s = [v - (1 << 64) if v >> 63 else v for v in self._rng]  # as int64 bit patterns
        self.rng_state.copy_(torch.tensor(s, dtype=torch.int64), non_blocking=True)

    @property
    def seed(self):
        return self._rng[0]

    @property
    def next_draw(self):
        return self._rng[1]

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._rng = tuple(int(v) & _U64 for v in self.rng_state.tolist())

    def table(self):
        """``sqrt_eig`` as the kernel reads it: fp32, contiguous, on the GPU."""
        return N.require_device_f32(self.sqrt_eig, "GaussianRandomFieldS2.sqrt_eig")

    @property
    def nrows(self):
        """Rows of the (K, lmax) table the kernel reads."""
        return 1 if self.K is None else self.K

    @torch.no_grad()
    def sample_coeffs(self, N_samples):
        """complex64 (N, [K,] lmax, mmax) coefficients of N fresh samples; the field index of
        the stream is the position in (N, K).  Consumes one draw."""
        if N_samples < 1:
            raise ValueError(f"N must be >= 1, got {N_samples}")
        table = self.table()
        lead = (N_samples,) if self.K is None else (N_samples, self.K)
        out = torch.empty(*lead, self.lmax, self.mmax, dtype=torch.complex64,
                          device=self.sqrt_eig.device)
        seed, draw = self._rng
        _fill(out, None, table, self.nrows, N_samples * self.nrows, self.lmax, self.mmax,
              0.0, 1.0, seed, draw, None)
        self._rng = (seed, (draw + 1) & _U64)
        self._store_rng()
        return out

    def forward(self, N_samples, xi=None):
        """(N, [K,] nlat, nlon) fp32 samples.  With ``xi`` (N, [K,] lmax, mmax) complex given,
        ``isht(xi * sqrt_eig)`` by torch ops: the deterministic form, which draws nothing."""
        if xi is None:
            return self.isht(self.sample_coeffs(N_samples))
        lead = (N_samples,) if self.K is None else (N_samples, self.K)
        if tuple(xi.shape) != lead + (self.lmax, self.mmax) or not xi.is_complex():
            raise ValueError(f"xi must be complex {lead + (self.lmax, self.mmax)}, got "
                             f"{xi.dtype} {tuple(xi.shape)}")
        _require_device(xi, "xi")
        return self.isht(xi * self.sqrt_eig.unsqueeze(-1))


class SphericalAR1:
    """A red-in-time Gaussian random field process for ``lead = (B, C)`` fields of ``grf``:

        c <- phi c + sqrt(1 - phi^2) sqrt_eig xi,     field = isht(c)

    stationary with the covariance of ``grf`` at every step and a lag-one correlation of
    ``phi = exp(-dt / tau_t)``.  C is ``grf``'s K, or ``grf`` has one spectrum, which then
    serves every channel.  The state is the (B, C, lmax, mmax) coefficient buffer ``coeffs``
    and the draw counter ``counter`` (a device uint64); ``step()`` reads the draw from the
    counter on the device and advances it there, allocates no state and synchronises
    nothing, so it records into a graph and every replay draws anew.  The Philox key is
    ``seed``, by default ``grf``'s seed with the top bit flipped, so that the process and
    ``grf.sample_coeffs`` never share a stream."""

    def __init__(self, grf, lead, phi=None, dt=None, tau_t=None, seed=None):
        if phi is None:
            if dt is None or tau_t is None or not tau_t > 0:
                raise ValueError("give phi, or dt and a positive tau_t (phi = exp(-dt / tau_t))")
            phi = math.exp(-dt / tau_t)
        if not 0.0 <= phi < 1.0:
            raise ValueError(f"phi must be in [0, 1), got {phi}")
        B, C = lead
        if B < 1 or C < 1 or (grf.nrows != 1 and grf.nrows != C):
            raise ValueError(f"lead = (B, C) = {tuple(lead)} needs C equal to the field's "
                             f"K = {grf.K}, or a field with one spectrum")
        _require_device(grf.sqrt_eig, "SphericalAR1's field")
        self.grf, self.lead, self.phi = grf, (B, C), float(phi)
        self.seed = (grf.seed ^ (1 << 63)) if seed is None else int(seed) & _U64
        # a, b in fp64 on the host, rounded once when they are passed
        self._a, self._b = float(phi), math.sqrt(1.0 - float(phi) ** 2)
        dev = grf.sqrt_eig.device
        self.coeffs = torch.zeros(B, C, grf.lmax, grf.mmax, dtype=torch.complex64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.uint64, device=dev)
        self.reset()

    @torch.no_grad()
    def reset(self, draw=0):
        """Draw the stationary state (draw number ``draw``); the next step uses ``draw + 1``."""
        g = self.grf
        _fill(self.coeffs, None, g.table(), g.nrows, self.lead[0] * self.lead[1], g.lmax,
              g.mmax, 0.0, 1.0, self.seed, draw, None)
        self.counter.copy_(torch.from_numpy(np.array([(draw + 1) & _U64], dtype=np.uint64)),
                           non_blocking=False)

    @torch.no_grad()
    def step(self):
        """Advance one step in place and return the grid field (B, C, nlat, nlon)."""
        g = self.grf
        _fill(self.coeffs, self.coeffs, g.table(), g.nrows, self.lead[0] * self.lead[1],
              g.lmax, g.mmax, self._a, self._b, self.seed, 0, self.counter)
        with torch.cuda.device(self.counter.device):
            N.check(N.lib().msfno_noise_advance(self.counter.data_ptr(), 1,
                                                N.stream_of(self.counter.device)),
                    "msfno_noise_advance")
        return g.isht(self.coeffs)

    def snapshot(self):
        """A copy of (coeffs, counter), for ``restore``."""
        return self.coeffs.clone(), self.counter.clone()

    def restore(self, snap):
        self.coeffs.copy_(snap[0])
        self.counter.copy_(snap[1])
