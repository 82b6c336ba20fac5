"""Drop-in replacements for ``torch_harmonics.RealSHT`` / ``InverseRealSHT``.

Reference usage: constructed at MSFNO/Models/sfno/sfnonet.py:537-548 with
``.float()``, the buffers ``.weights`` / ``.pct`` rescaled ×1e5 / ÷1e5 at
:551-555, and called as ``forward_transform(x)`` / ``inverse_transform(x)`` at
MSFNO/Models/sfno/layers.py:405,421,629,638.  Attributes read by the reference:
``nlat nlon lmax mmax`` (layers.py:361-365, 569-577).

The tables are computed on the host in fp64 by libmsfno (same recurrence as
torch-harmonics' ``legpoly``) and registered as buffers with the same names and
shapes ``(mmax, lmax, nlat)``; ``forward`` runs entirely on the GPU (HIP
longitude FFT + MFMA Legendre contraction).  Whenever the buffer tensor changes
(``.float()``, the ×1e5 rescale, ``.to(device)``) the device plan re-lays it out
on the next call, so the reference's construction recipe keeps working.

Both classes are ordinary autograd ops, as the torch-harmonics ones are: an input that
requires grad (with grad mode on) goes through a ``torch.autograd.Function`` whose
backward is one native transform on an *adjoint plan* -- a plan of the opposite
direction on the same grid whose table is this module's table rescaled per ``m``
(``adjoint_table``).  Adjoint plans are built on the first backward, cached per device
and rebuilt when the table buffer changes, exactly as the forward plans are.  They cost
a second device table per differentiated transform (375 MB at 721 x 1440 with lmax 360);
calls under ``no_grad`` or on inputs that do not require grad never build one.  Double
backward is not supported.
"""
from __future__ import annotations

import math
import weakref

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _native as N

_SUPPORTED_GRIDS = ("equiangular", "legendre-gauss")


def _legendre_table(mmax, lmax, nlat, grid, inverse, csphase):
    t = np.zeros((mmax, lmax, nlat), dtype=np.float64)
    N.check(N.lib().msfno_legendre_table(mmax, lmax, nlat, N.GRID[grid], int(inverse),
                                         int(csphase), t.ctypes.data), "legendre_table")
    return torch.from_numpy(t)


def adjoint_table(table, nlon, inverse):
    """The (mmax, lmax, nlat) table of the adjoint plan of a transform, formed in fp64 on
    the host and rounded to fp32 once.

    ``inverse=True``: `table` is an inverse transform's ``pct``; its adjoint is a forward
    plan with ``pct[m, l, k] c_m nlon / 2pi`` (irfft(norm="forward") weighs bin m by
    c_m = 2 but the DC and Nyquist bins, c_m = 1).  ``inverse=False``: `table` is a forward
    transform's ``weights``; its adjoint is an inverse plan with ``weights[m, l, k] d_m
    2pi / nlon`` (the adjoint of 2pi rfft(norm="forward"): d_m = 1/2 but DC and Nyquist,
    d_m = 1)."""
    mmax = table.shape[0]
    m = torch.arange(mmax, dtype=torch.float64)
    w = torch.full((mmax,), 2.0 if inverse else 0.5, dtype=torch.float64)
    w[(m == 0) | (2 * m == nlon)] = 1.0
    scale = nlon / (2 * math.pi) if inverse else 2 * math.pi / nlon
    return (table.detach().double().cpu() * w[:, None, None] * scale).float()


class _SHTFn(torch.autograd.Function):
    """A transform as an autograd op: forward is the module's native call, backward one
    native call on its adjoint plan."""

    @staticmethod
    def forward(ctx, x, mod):
        ctx.mod = mod
        return mod._native(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ctx.mod._native_adjoint(g), None


class _SHTBase(nn.Module):
    _buffer_name = "weights"
    _inverse = False

    def _init_common(self, nlat, nlon, lmax, mmax, grid, norm, csphase):
        if grid not in _SUPPORTED_GRIDS:
            raise NotImplementedError(f"Unknown quadrature mode {grid!r} (supported: {_SUPPORTED_GRIDS})")
        if norm != "ortho":
            raise NotImplementedError(f"Unsupported SHT normalisation {norm!r} (only 'ortho')")
        self.nlat, self.nlon, self.grid = nlat, nlon, grid
        self.norm, self.csphase = norm, csphase
        self.lmax = lmax or nlat
        self.mmax = mmax or nlon // 2 + 1
        self._plans = {}
        self._adj_plans = {}

    def _plan(self, device):
        table = getattr(self, self._buffer_name)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        plan = self._plans.get(idx)
        if plan is None:
            plan = N.SHTPlan(self.nlat, self.nlon, self.lmax, self.mmax, self._inverse, idx)
            self._plans[idx] = plan
        key = N.tensor_key(table)
        if key != plan.key:  # (re)load only when the buffer tensor changed
            t = table
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(device=device, dtype=torch.float32).contiguous()
            plan.load(t, key)
        return plan

    def _adjoint_plan(self, device):
        """The plan of the opposite direction that applies this transform's adjoint (the
        table: ``adjoint_table`` of the current buffer); created on the first backward,
        then kept per device under the key of ``_plan``."""
        table = getattr(self, self._buffer_name)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        plan = self._adj_plans.get(idx)
        if plan is None:
            plan = N.SHTPlan(self.nlat, self.nlon, self.lmax, self.mmax, not self._inverse, idx)
            self._adj_plans[idx] = plan
        key = N.tensor_key(table)
        if key != plan.key:
            plan.load(adjoint_table(table, self.nlon, self._inverse).to(device).contiguous(),
                      key)
        return plan

    def _analysis(self, plan, x, what):
        """(..., nlat, nlon) fp32 -> (..., lmax, mmax) complex64 on a forward plan."""
        lead = x.shape[:-2]
        bc = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(*lead, self.lmax, self.mmax, dtype=torch.complex64, device=x.device)
        ws = torch.empty(N.lib().msfno_sht_workspace_size(plan.handle, bc), dtype=torch.uint8,
                         device=x.device)
        N.check(N.lib().msfno_sht_forward(plan.handle, x.data_ptr(), out.data_ptr(), bc,
                                          ws.data_ptr(), ws.numel(), N.stream_of(x.device)),
                what)
        return out

    def _synthesis(self, plan, x, what):
        """(..., lmax, mmax) complex64 -> (..., nlat, nlon) fp32 on an inverse plan."""
        lead = x.shape[:-2]
        bc = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(*lead, self.nlat, self.nlon, dtype=torch.float32, device=x.device)
        ws = torch.empty(N.lib().msfno_sht_workspace_size(plan.handle, bc), dtype=torch.uint8,
                         device=x.device)
        N.check(N.lib().msfno_sht_inverse(plan.handle, x.data_ptr(), out.data_ptr(), bc,
                                          ws.data_ptr(), ws.numel(), N.stream_of(x.device)),
                what)
        return out

    def _call(self, x):
        """`x` is what the kernels take (device, fp32 / complex64, contiguous), made so by
        torch ops that autograd sees."""
        if torch.is_grad_enabled() and x.requires_grad:
            return _SHTFn.apply(x, self)
        return self._native(x)

    def __getstate__(self):
        s = self.__dict__.copy()
        s["_plans"] = {}
        s["_adj_plans"] = {}
        return s


class RealSHT(_SHTBase):
    """Forward real SHT: (..., nlat, nlon) fp32 -> (..., lmax, mmax) complex64."""

    _buffer_name = "weights"
    _inverse = False

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho",
                 csphase=True):
        super().__init__()
        self._init_common(nlat, nlon, lmax, mmax, grid, norm, csphase)
        self.register_buffer("weights", _legendre_table(self.mmax, self.lmax, nlat, grid, False,
                                                        csphase))

    @N.on_input_device
    def forward(self, x):
        assert x.shape[-2] == self.nlat
        assert x.shape[-1] == self.nlon
        # resolve_neg / resolve_conj: torch's lazy negation and conjugate bits survive
        # .contiguous(); the kernels read the memory as it lies
        return self._call(N.require_device_f32(x, "RealSHT input").resolve_neg())

    def _native(self, x):
        return self._analysis(self._plan(x.device), x, "RealSHT.forward")

    @N.on_input_device
    def _native_adjoint(self, g):
        """dL/dx (..., nlat, nlon) fp32 of g = dL/d(out), complex64."""
        return self._synthesis(self._adjoint_plan(g.device), g.resolve_conj().contiguous(),
                               "RealSHT.backward")


class InverseRealSHT(_SHTBase):
    """Inverse real SHT: (..., lmax, mmax) complex64 -> (..., nlat, nlon) fp32."""

    _buffer_name = "pct"
    _inverse = True

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho",
                 csphase=True):
        super().__init__()
        self._init_common(nlat, nlon, lmax, mmax, grid, norm, csphase)
        self.register_buffer("pct", _legendre_table(self.mmax, self.lmax, nlat, grid, True,
                                                    csphase))

    @N.on_input_device
    def forward(self, x):
        assert x.shape[-2] == self.lmax
        assert x.shape[-1] == self.mmax
        if not x.is_cuda:
            raise ValueError("InverseRealSHT input must be a GPU (HIP) tensor")
        if x.dtype != torch.complex64:
            x = x.to(torch.complex64)
        return self._call(x.resolve_conj().contiguous())

    def _native(self, x):
        return self._synthesis(self._plan(x.device), x, "InverseRealSHT.forward")

    @N.on_input_device
    def _native_adjoint(self, g):
        """dL/dx (..., lmax, mmax) complex64, dL/dRe + i dL/dIm, of g = dL/d(out), fp32."""
        return self._analysis(self._adjoint_plan(g.device), g.resolve_neg().contiguous(),
                              "InverseRealSHT.backward")


# ---- foreign transforms ------------------------------------------------------------
# A block built around torch_harmonics.RealSHT / InverseRealSHT objects (the reference's
# own, sfnonet.py:537-548) runs on the native plans too: adopt() wraps such an object in
# the matching class of this module WITHOUT copying its table.  The wrapper reads the
# foreign buffer (``weights`` / ``pct``) on every call, so the reference's later
# re-assignment of it (the x1e5 rescale, sfnonet.py:551-555, ``.to(device)``) is seen
# exactly as for the native classes.  Accepted: any object with nlat, nlon, lmax, mmax
# and a (mmax, lmax, nlat) table buffer, with norm "ortho" if it says.
_ADOPTED = weakref.WeakKeyDictionary()


class _AdoptedRealSHT(RealSHT):
    def __init__(self, src):
        nn.Module.__init__(self)
        object.__setattr__(self, "_src", src)
        self.nlat, self.nlon, self.lmax, self.mmax = src.nlat, src.nlon, src.lmax, src.mmax
        self.grid = getattr(src, "grid", "equiangular")
        self.norm, self.csphase = "ortho", getattr(src, "csphase", True)
        self._plans = {}
        self._adj_plans = {}

    @property
    def weights(self):
        return self._src.weights


class _AdoptedInverseRealSHT(InverseRealSHT):
    def __init__(self, src):
        nn.Module.__init__(self)
        object.__setattr__(self, "_src", src)
        self.nlat, self.nlon, self.lmax, self.mmax = src.nlat, src.nlon, src.lmax, src.mmax
        self.grid = getattr(src, "grid", "equiangular")
        self.norm, self.csphase = "ortho", getattr(src, "csphase", True)
        self._plans = {}
        self._adj_plans = {}

    @property
    def pct(self):
        return self._src.pct


def adopt(t, inverse: bool):
    """This module's transform for `t`: `t` itself when it already is one, else a
    table-sharing wrapper of a torch-harmonics-style transform (NotImplementedError
    when `t` does not look like one)."""
    ours = InverseRealSHT if inverse else RealSHT
    if isinstance(t, ours):
        return t
    name = "pct" if inverse else "weights"
    kind = "InverseRealSHT" if inverse else "RealSHT"
    tab = getattr(t, name, None)
    if not isinstance(tab, torch.Tensor) or not all(
            hasattr(t, a) for a in ("nlat", "nlon", "lmax", "mmax")):
        raise NotImplementedError(f"expected a {kind} (torch_harmonics or msfno_amd.harmonics), "
                                  f"got {type(t).__name__}")
    if getattr(t, "norm", "ortho") != "ortho":
        raise NotImplementedError(f"Unsupported SHT normalisation {t.norm!r} (only 'ortho')")
    if tuple(tab.shape) != (t.mmax, t.lmax, t.nlat):
        raise NotImplementedError(f"{kind}.{name} must have shape (mmax, lmax, nlat)")
    w = _ADOPTED.get(t)
    if w is None:
        w = (_AdoptedInverseRealSHT if inverse else _AdoptedRealSHT)(t)
        _ADOPTED[t] = w
    return w
