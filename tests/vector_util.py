"""fp64 reference of the vector spherical harmonic transforms, independent of the library's
route to its tables (which never divides by sin theta and never uses degree l - 1 at the
same order).

Tables from oracle.sht_ref.legpoly (P = the orthonormal associated Legendre function):

    Q_l^m = m P_l^m / sin(theta)
    D_l^m = dP_l^m/dtheta
          = [l cos(theta) P_l^m - sqrt((2l+1)/(2l-1) (l^2 - m^2)) P_{l-1}^m] / sin(theta)

at interior nodes.  At a pole only m = 1 is non-zero: at theta = 0,
D = Q = -1/2 sqrt((2l+1) l (l+1) / (4 pi)) with the Condon-Shortley phase, and at theta = pi
its parity image (D has the parity (-1)^(l-m+1), Q (-1)^(l-m)).  ``_confirm_pole_limit``
checks that closed form against the interior formula at theta = 1e-4 when the module is
imported.

Transforms: the einsums of the definitions (components (v_theta, v_phi), coefficients
(s, t), the scalar transforms' longitude step) on real tensors, complex numbers as a
trailing dim of 2, so that autograd through them gives reference gradients in torch's
convention dL/dRe + i dL/dIm without assuming it."""
import functools
import math

import numpy as np
import torch

from oracle import sht_ref as S


def _interior_dq(mmax, lmax, theta, csphase):
    """D, Q (mmax, lmax, len(theta)) by the interior formulas; theta strictly inside (0, pi)."""
    x, st = np.cos(theta), np.sin(theta)
    p = S.legpoly(mmax, lmax, x, csphase=csphase)
    m = np.arange(mmax, dtype=np.float64)[:, None, None]
    l = np.arange(lmax, dtype=np.float64)[None, :, None]
    pm1 = np.zeros_like(p)
    pm1[:, 1:] = p[:, :-1]
    c = np.sqrt((2 * l + 1) / np.maximum(2 * l - 1, 1) * np.maximum(l * l - m * m, 0))
    d = (l * x * p - c * pm1) / st
    q = m * p / st
    keep = l >= m
    return d * keep, q * keep


def _pole_value(lmax, csphase):
    """D_l^1 = Q_l^1 at theta = 0, l < lmax."""
    l = np.arange(lmax, dtype=np.float64)
    return (-0.5 if csphase else 0.5) * np.sqrt((2 * l + 1) * l * (l + 1) / (4 * math.pi))


def _confirm_pole_limit():
    """The closed form at the pole is one expression in l; the interior value at theta = 1e-4
    differs from its limit by the curvature term, about (3/8) l(l+1) theta^2 relative, which
    is below 3e-7 for l <= 8: there the two must agree to 1e-6 relative."""
    lmax = 9
    for cs in (True, False):
        d, q = _interior_dq(2, lmax, np.array([1e-4]), cs)
        want = _pole_value(lmax, cs)
        for got in (d[1, 1:, 0], q[1, 1:, 0]):
            rel = np.abs(got - want[1:]) / np.abs(want[1:])
            assert rel.max() < 1e-6, rel
        # every other order vanishes towards the pole
        assert np.abs(d[0, :, 0]).max() < 1e-2 and np.abs(q[0]).max() == 0


_confirm_pole_limit()


@functools.lru_cache(maxsize=None)
def dq_tables(grid, nlat, lmax, mmax, csphase=True):
    """(D, Q, w): the bare tables (mmax, lmax, nlat) at the grid's colatitudes north -> south
    and the quadrature weights (nlat), float64 numpy; shared, never modified."""
    theta, w = S.colatitudes(nlat, grid)
    pole = np.abs(np.cos(theta)) == 1.0
    d = np.zeros((mmax, lmax, nlat))
    q = np.zeros((mmax, lmax, nlat))
    d[:, :, ~pole], q[:, :, ~pole] = _interior_dq(mmax, lmax, theta[~pole], csphase)
    if mmax > 1:
        l = np.arange(lmax)
        v = _pole_value(lmax, csphase)
        for k in np.nonzero(pole)[0]:
            south = np.cos(theta[k]) < 0
            d[1, :, k] = v * ((-1.0) ** l if south else 1.0)         # (-1)^(l-1+1)
            q[1, :, k] = v * ((-1.0) ** (l + 1) if south else 1.0)   # (-1)^(l-1)
            d[1, 0, k] = q[1, 0, k] = 0.0
    for a in (d, q, w):
        a.setflags(write=False)
    return d, q, w


def analysis_tables(grid, nlat, lmax, mmax, csphase=True):
    """D, Q times w_k / (l(l+1)), the l = 0 row zero."""
    d, q, w = dq_tables(grid, nlat, lmax, mmax, csphase)
    l = np.arange(lmax, dtype=np.float64)
    f = np.zeros(lmax)
    f[1:] = 1.0 / (l[1:] * (l[1:] + 1))
    f = f[None, :, None] * w[None, None, :]
    return d * f, q * f


def _an(t, a):
    return torch.einsum("...km,mlk->...lm", a, t)


def _syn(t, a):
    return torch.einsum("...lm,mlk->...km", a, t)


def dense_analysis(v, dw, qw):
    """v (..., 2, nlat, nlon) float64 -> (..., 2, lmax, mmax, 2) float64 (re, im), with the
    weighted tables dw, qw (mmax, lmax, nlat) as float64 tensors:
        s = sum_k dw v_theta - i qw v_phi,    t = sum_k i qw v_theta + dw v_phi"""
    mmax = dw.shape[0]
    x = torch.view_as_real(2.0 * math.pi * torch.fft.rfft(v, dim=-1, norm="forward"))
    x = x[..., :mmax, :]
    tr, ti = x[..., 0, :, :, 0], x[..., 0, :, :, 1]
    pr, pi = x[..., 1, :, :, 0], x[..., 1, :, :, 1]
    s = torch.stack((_an(dw, tr) + _an(qw, pi), _an(dw, ti) - _an(qw, pr)), -1)
    t = torch.stack((_an(dw, pr) - _an(qw, ti), _an(dw, pi) + _an(qw, tr)), -1)
    return torch.stack((s, t), -4)


def dense_synthesis(st, d, q, nlon):
    """st (..., 2, lmax, mmax, 2) float64 (re, im) -> v (..., 2, nlat, nlon) float64:
        v_theta = sum_l d s - i q t,    v_phi = sum_l i q s + d t"""
    sr, si = st[..., 0, :, :, 0], st[..., 0, :, :, 1]
    tr, ti = st[..., 1, :, :, 0], st[..., 1, :, :, 1]
    vt = torch.stack((_syn(d, sr) + _syn(q, ti), _syn(d, si) - _syn(q, tr)), -1)
    vp = torch.stack((_syn(d, tr) - _syn(q, si), _syn(d, ti) + _syn(q, sr)), -1)
    x = torch.view_as_complex(torch.stack((vt, vp), -4).contiguous())
    return torch.fft.irfft(x, n=nlon, dim=-1, norm="forward")


def torch_tables(grid, nlat, lmax, mmax, inverse):
    d, q = (dq_tables(grid, nlat, lmax, mmax)[:2] if inverse
            else analysis_tables(grid, nlat, lmax, mmax))
    return torch.from_numpy(np.array(d)), torch.from_numpy(np.array(q))
