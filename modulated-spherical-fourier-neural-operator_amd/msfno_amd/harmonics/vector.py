"""Vector spherical harmonic transforms, the counterparts of ``torch_harmonics.RealVectorSHT``
/ ``InverseRealVectorSHT``, and the wind diagnostics built on them.

A tangent field on the sphere has the components ``(v_theta, v_phi)``, southward and
eastward, stacked in dim -3; for the model's ``u`` (eastward) and ``v`` (northward),
``v_theta = -v`` and ``v_phi = u`` (``uv_to_vector``).  Its coefficients are ``s``
(spheroidal, of grad Y_lm) and ``t`` (toroidal, of r x grad Y_lm), again stacked in dim -3.
With ``D = dP_l^m/dtheta`` and ``Q = m P_l^m / sin theta`` of the scalar transforms'
orthonormal P, and their longitude step, per m:

    synthesis   v_theta = sum_l D s - i Q t             v_phi = sum_l i Q s + D t
    analysis    s = 1/(l(l+1)) sum_k w_k [D v_theta - i Q v_phi]
                t = 1/(l(l+1)) sum_k w_k [i Q v_theta + D v_phi]

so the divergence has the coefficients ``-l(l+1) s`` and the vorticity ``-l(l+1) t``.

The tables are computed on the host in fp64 by libmsfno (``msfno_vector_legendre_table``)
and registered as the buffers ``weights`` / ``dpct`` of shape ``(2, mmax, lmax, nlat)``,
``[0] = D`` and ``[1] = Q``.  Each transform runs on two scalar plans of its direction
(``msfno_vsht_forward`` / ``msfno_vsht_inverse``): one of ``lmax + 1`` degrees holding ``D``
moved up one degree, which gives it the equatorial parity the hemisphere-folded Legendre
kernels need, and one holding ``Q``.  Plans are per device and re-laid out when the buffer
tensor changes, as for the scalar classes.

Both classes are autograd ops like the scalar ones: the adjoint of the analysis has the
structure of the synthesis and vice versa, so a backward is the opposite native transform on
two adjoint plans (``adjoint_table`` of each table), built on the first backward and never
under ``no_grad``.  Double backward is not supported.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from .sht import _SHTBase, _SHTFn, adjoint_table


def _vector_table(mmax, lmax, nlat, grid, inverse, csphase):
    t = np.zeros((2, mmax, lmax, nlat), dtype=np.float64)
    N.check(N.lib().msfno_vector_legendre_table(mmax, lmax, nlat, N.GRID[grid], int(inverse),
                                                int(csphase), t.ctypes.data),
            "vector_legendre_table")
    return torch.from_numpy(t)


class _PlanPair:
    """The two scalar plans of one vector transform: ``d`` (lmax + 1 degrees, D at row
    l + 1) and ``q`` (lmax degrees, Q)."""

    def __init__(self, mod, inverse, device):
        self.d = N.SHTPlan(mod.nlat, mod.nlon, mod.lmax + 1, mod.mmax, inverse, device)
        self.q = N.SHTPlan(mod.nlat, mod.nlon, mod.lmax, mod.mmax, inverse, device)
        self.key = None

    def load(self, table, key):
        """`table` (2, mmax, lmax, nlat) fp32 on the plans' device."""
        mmax, lmax, nlat = table.shape[1:]
        shifted = table.new_zeros(mmax, lmax + 1, nlat)
        shifted[:, 1:] = table[0]
        self.d.load(shifted, key)
        self.q.load(table[1].contiguous(), key)
        self.key = key


class _VectorSHTBase(_SHTBase):
    def _pair(self, store, device, inverse, adjoint):
        table = getattr(self, self._buffer_name)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        pair = store.get(idx)
        if pair is None:
            pair = store[idx] = _PlanPair(self, inverse, idx)
        key = N.tensor_key(table)
        if key != pair.key:  # (re)load only when the buffer tensor changed
            if adjoint:
                t = torch.stack([adjoint_table(table[i], self.nlon, self._inverse)
                                 for i in (0, 1)]).to(device)
            else:
                t = table.to(device=device, dtype=torch.float32)
            pair.load(t, key)
        return pair

    def _plan(self, device):
        return self._pair(self._plans, device, self._inverse, False)

    def _adjoint_plan(self, device):
        """The pair of the opposite direction that applies this transform's adjoint; made
        on the first backward, then kept per device under the key of ``_plan``."""
        return self._pair(self._adj_plans, device, not self._inverse, True)

    def _run(self, fn, pair, x, out_tail, dtype, what):
        lead = x.shape[:-3]
        bc = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(*lead, 2, *out_tail, dtype=dtype, device=x.device)
        ws = torch.empty(N.lib().msfno_vsht_workspace_size(pair.d.handle, pair.q.handle, bc),
                         dtype=torch.uint8, device=x.device)
        N.check(fn(pair.d.handle, pair.q.handle, x.data_ptr(), out.data_ptr(), bc,
                   ws.data_ptr(), ws.numel(), N.stream_of(x.device)), what)
        return out

    def _analysis(self, pair, x, what):
        """(..., 2, nlat, nlon) fp32 -> (..., 2, lmax, mmax) complex64 on a forward pair."""
        return self._run(N.lib().msfno_vsht_forward, pair, x, (self.lmax, self.mmax),
                         torch.complex64, what)

    def _synthesis(self, pair, x, what):
        """(..., 2, lmax, mmax) complex64 -> (..., 2, nlat, nlon) fp32 on an inverse pair."""
        return self._run(N.lib().msfno_vsht_inverse, pair, x, (self.nlat, self.nlon),
                         torch.float32, what)


class RealVectorSHT(_VectorSHTBase):
    """Forward vector SHT: (..., 2, nlat, nlon) fp32 -> (..., 2, lmax, mmax) complex64."""

    _buffer_name = "weights"
    _inverse = False

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho",
                 csphase=True):
        super().__init__()
        self._init_common(nlat, nlon, lmax, mmax, grid, norm, csphase)
        self.register_buffer("weights", _vector_table(self.mmax, self.lmax, nlat, grid, False,
                                                      csphase))

    @N.on_input_device
    def forward(self, x):
        assert x.shape[-3] == 2
        assert x.shape[-2] == self.nlat
        assert x.shape[-1] == self.nlon
        return self._call(N.require_device_f32(x, "RealVectorSHT input").resolve_neg())

    def _native(self, x):
        return self._analysis(self._plan(x.device), x, "RealVectorSHT.forward")

    @N.on_input_device
    def _native_adjoint(self, g):
        """dL/dx (..., 2, nlat, nlon) fp32 of g = dL/d(out), complex64."""
        return self._synthesis(self._adjoint_plan(g.device), g.resolve_conj().contiguous(),
                               "RealVectorSHT.backward")


class InverseRealVectorSHT(_VectorSHTBase):
    """Inverse vector SHT: (..., 2, lmax, mmax) complex64 -> (..., 2, nlat, nlon) fp32."""

    _buffer_name = "dpct"
    _inverse = True

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho",
                 csphase=True):
        super().__init__()
        self._init_common(nlat, nlon, lmax, mmax, grid, norm, csphase)
        self.register_buffer("dpct", _vector_table(self.mmax, self.lmax, nlat, grid, True,
                                                   csphase))

    @N.on_input_device
    def forward(self, x):
        assert x.shape[-3] == 2
        assert x.shape[-2] == self.lmax
        assert x.shape[-1] == self.mmax
        if not x.is_cuda:
            raise ValueError("InverseRealVectorSHT input must be a GPU (HIP) tensor")
        if x.dtype != torch.complex64:
            x = x.to(torch.complex64)
        return self._call(x.resolve_conj().contiguous())

    def _native(self, x):
        return self._synthesis(self._plan(x.device), x, "InverseRealVectorSHT.forward")

    @N.on_input_device
    def _native_adjoint(self, g):
        """dL/dx (..., 2, lmax, mmax) complex64, dL/dRe + i dL/dIm, of g = dL/d(out), fp32."""
        return self._analysis(self._adjoint_plan(g.device), g.resolve_neg().contiguous(),
                              "InverseRealVectorSHT.backward")


# ---- wind diagnostics: torch ops on the transforms' inputs and outputs, gradients flow ----
def uv_to_vector(u, v):
    """The model's eastward ``u`` and northward ``v`` (..., nlat, nlon) as the tangent field
    ``(v_theta, v_phi) = (-v, u)`` (..., 2, nlat, nlon)."""
    return torch.stack((-v, u), dim=-3)


def vector_to_uv(x):
    """``(u, v)`` of a tangent field (..., 2, nlat, nlon)."""
    return x[..., 1, :, :], -x[..., 0, :, :]


def _minus_ll1(lmax, like):
    l = torch.arange(lmax, device=like.device, dtype=torch.float32)
    return (-(l * (l + 1)))[:, None]


def divergence_vorticity_spectra(st):
    """``(delta, zeta)``, the scalar coefficients (..., lmax, mmax) of the divergence
    ``-l(l+1) s`` and the vorticity ``-l(l+1) t`` of ``st`` (..., 2, lmax, mmax)."""
    f = _minus_ll1(st.shape[-2], st)
    return st[..., 0, :, :] * f, st[..., 1, :, :] * f


def vorticity_divergence(u, v, vsht, isht):
    """The relative vorticity and the divergence (unit sphere) of the wind ``(u, v)`` on the
    grid of the scalar ``isht``, through ``vsht`` (a ``RealVectorSHT`` of the same lmax and
    mmax): ``(zeta, delta)``."""
    delta, zeta = divergence_vorticity_spectra(vsht(uv_to_vector(u, v)))
    return isht(zeta), isht(delta)


def wind_from_vorticity_divergence(zeta, delta, sht, ivsht):
    """``(u, v)`` on the grid of ``ivsht`` (an ``InverseRealVectorSHT``) from the vorticity
    and the divergence, analysed by the scalar ``sht``; degree 0 (a field with a non-zero
    mean is no vorticity or divergence) is dropped."""
    zc, dc = sht(zeta), sht(delta)
    f = _minus_ll1(zc.shape[-2], zc)
    inv = torch.zeros_like(f)
    inv[1:] = 1.0 / f[1:]
    return vector_to_uv(ivsht(torch.stack((dc * inv, zc * inv), dim=-3)))
