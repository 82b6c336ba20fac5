"""Regridding on the device: a separable, banded linear map over (lat, lon), optionally
normalised by the valid weight (``msfno_regrid``, csrc/regrid.hip).

* ``Grid`` is one of the package's two grids (north to south, first longitude 0) as cells:
  latitude edges in mu = cos(theta) and longitude cells of +-pi/nlon around each node.
* ``conservative``, ``bilinear`` and ``block_mean`` build the two fp64 matrices (Wlat
  (nlat_out, nlat_in), Wlon (nlon_out, nlon_in)) of ``y = Wlat @ x @ Wlon.T``;
  ``tables_from_dense`` turns any matrix whose rows are (cyclically) contiguous bands into
  the ELL table the kernel reads.
* ``Regridder`` applies them to (B, C, H, W) fp32 fields on the device, with a gradient in
  linear mode (the adjoint regridder ``.T``), and with a mask and / or NaN skipping in
  normalised mode: ``y = sum(w v x) / sum(w v)``.
* ``sst_input`` is the reference's generator input (MSFNO/Models/data.py:205-213,
  ``coarsen(latitude=4, longitude=4, boundary='trim').mean()`` with NaN over land skipped,
  then ``normalise_film``, sfno/model.py:281-287).

WeatherBench's 1.5 degree grid out of 0.25 degree is
``Regridder(Grid(721, 1440), Grid(121, 240))``: the cell mean, where the strided window
``export.Selection(lat=slice(None, None, 6), lon=slice(None, None, 6))`` is a point sample.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N

KINDS = ("equiangular", "legendre-gauss")
MAX_TAPS = N.REGRID_MAX_TAPS


class Grid:
    """``nlat`` x ``nlon`` nodes of ``kind`` with the cells around them.

    Latitude cell edges ``lat_edges`` (nlat + 1, from 1 down to -1, in mu = cos(theta)):
    equiangular, the midpoints between the nodes theta_k = pi k / (nlat - 1), so the pole rows
    are half cells; legendre-gauss, the cumulative quadrature weights mu_k = 1 - sum_{j<k} w_j,
    so a cell's area is exactly its quadrature weight and every node lies in its cell.
    ``lat_edges=`` (and ``lat_nodes=``, colatitudes in radians, for ``bilinear``) override
    them for other grids.  Longitude cells are +-pi/nlon around lambda_i = 2 pi i / nlon,
    periodic."""

    def __init__(self, nlat, nlon, kind="equiangular", lat_edges=None, lat_nodes=None):
        nlat, nlon = int(nlat), int(nlon)
        if nlat < 1 or nlon < 1:
            raise ValueError(f"a grid needs nlat and nlon >= 1, got {nlat} x {nlon}")
        if kind not in KINDS:
            raise NotImplementedError(f"grid kind {kind!r}; the package's grids are {KINDS}")
        self.nlat, self.nlon, self.kind = nlat, nlon, kind
        if lat_nodes is not None:
            theta = np.asarray(lat_nodes, dtype=np.float64)
        elif kind == "equiangular":
            theta = np.pi * np.arange(nlat) / max(nlat - 1, 1) if nlat > 1 else np.array([np.pi / 2])
        else:
            from .harmonics import quadrature as Q
            x, w = Q.legendre_gauss_weights(nlat)
            order = np.argsort(-x)                      # north to south
            theta, self._gauss_w = np.arccos(x[order]), w[order]
        if theta.shape != (nlat,) or np.any(np.diff(theta) <= 0):
            raise ValueError("lat_nodes must be nlat increasing colatitudes")
        self.theta = theta
        if lat_edges is not None:
            edges = np.asarray(lat_edges, dtype=np.float64)
        elif kind == "equiangular" or lat_nodes is not None:
            edges = np.concatenate([[1.0], np.cos(0.5 * (theta[1:] + theta[:-1])), [-1.0]])
        else:
            edges = 1.0 - np.concatenate([[0.0], np.cumsum(self._gauss_w)])
            edges[-1] = -1.0                            # the weights sum to 2
        if edges.shape != (nlat + 1,) or np.any(np.diff(edges) >= 0):
            raise ValueError("lat_edges must be nlat + 1 decreasing values of cos(theta)")
        self.lat_edges = edges

    @property
    def shape(self):
        return (self.nlat, self.nlon)

    def lat_area(self):
        """The cells' extents in mu (nlat); they sum to lat_edges[0] - lat_edges[-1]."""
        return self.lat_edges[:-1] - self.lat_edges[1:]

    def area(self):
        """Cell areas (nlat, nlon) on the unit sphere."""
        return np.repeat(self.lat_area()[:, None] * (2 * np.pi / self.nlon), self.nlon, axis=1)

    def __repr__(self):
        return f"Grid({self.nlat}, {self.nlon}, {self.kind!r})"


def _as_grid(g, like=None):
    if isinstance(g, Grid):
        return g
    nlat, nlon = g
    return Grid(nlat, nlon, like.kind if like is not None else "equiangular")


# ---- the builders: dense fp64 matrices ---------------------------------------------------------

def _overlap_lat(src_edges, dst_edges):
    """Overlap of decreasing edge sequences over the destination cell."""
    s_hi, s_lo = src_edges[None, :-1], src_edges[None, 1:]
    d_hi, d_lo = dst_edges[:-1, None], dst_edges[1:, None]
    ov = np.clip(np.minimum(s_hi, d_hi) - np.maximum(s_lo, d_lo), 0.0, None)
    return ov / (d_hi - d_lo)


def _overlap_lon(n_in, n_out):
    """Overlap of the periodic cells, in units of the circle, over the destination cell."""
    s_lo = (np.arange(n_in) - 0.5) / n_in
    d_lo = (np.arange(n_out) - 0.5) / n_out
    W = np.zeros((n_out, n_in))
    for shift in (-1.0, 0.0, 1.0):
        lo = np.maximum(s_lo[None, :] + shift, d_lo[:, None])
        hi = np.minimum(s_lo[None, :] + shift + 1.0 / n_in, d_lo[:, None] + 1.0 / n_out)
        W += np.clip(hi - lo, 0.0, None)
    W[W < 1e-15] = 0.0          # cells that only touch
    return W * n_out


def conservative(src, dst):
    """(Wlat, Wlon) of first-order conservative remapping: per axis, the overlap of a source
    cell with the destination cell over the destination cell.  Rows sum to 1 and
    ``sum(area_dst * (W x)) == sum(area_src * x)``."""
    src, dst = _as_grid(src), _as_grid(dst, src)
    Wlat = _overlap_lat(src.lat_edges, dst.lat_edges)
    Wlat[Wlat < 1e-15] = 0.0
    return Wlat / Wlat.sum(axis=1, keepdims=True), _overlap_lon(src.nlon, dst.nlon)


def bilinear(src, dst):
    """(Wlat, Wlon) of bilinear sampling at the destination nodes: two taps per axis, linear
    in theta and lambda, clamped at the source's first and last rows and wrapped in
    longitude."""
    src, dst = _as_grid(src), _as_grid(dst, src)
    Wlat = np.zeros((dst.nlat, src.nlat))
    for j, th in enumerate(dst.theta):
        k = int(np.searchsorted(src.theta, th, side="right")) - 1
        if k < 0:
            Wlat[j, 0] = 1.0
        elif k >= src.nlat - 1:
            Wlat[j, src.nlat - 1] = 1.0
        else:
            t = (th - src.theta[k]) / (src.theta[k + 1] - src.theta[k])
            Wlat[j, k], Wlat[j, k + 1] = 1.0 - t, t
    Wlon = np.zeros((dst.nlon, src.nlon))
    for i in range(dst.nlon):
        k, r = divmod(i * src.nlon, dst.nlon)           # the position i nlon_in / nlon_out, exact
        t = r / dst.nlon
        Wlon[i, k % src.nlon] += 1.0 - t
        Wlon[i, (k + 1) % src.nlon] += t
    return Wlat, Wlon


class BlockMean:
    """``block_mean``'s operator, resolved against a source shape by ``dense``."""

    def __init__(self, factor_lat, factor_lon):
        self.factor_lat, self.factor_lon = int(factor_lat), int(factor_lon)

    def dense(self, nlat, nlon):
        out = []
        for n, f in ((nlat, self.factor_lat), (nlon, self.factor_lon)):
            m = n // f
            if m < 1:
                raise ValueError(f"a block of {f} is longer than the axis of {n}")
            W = np.zeros((m, n))
            for j in range(m):
                W[j, j * f:(j + 1) * f] = 1.0 / f
            out.append(W)
        return tuple(out)


def block_mean(factor_lat, factor_lon, boundary="trim"):
    """The xarray ``coarsen(latitude=factor_lat, longitude=factor_lon, boundary='trim')
    .mean()`` operator: uniform weights over whole blocks, trailing rows and columns dropped.
    Pass it as a ``Regridder``'s ``method``."""
    if boundary != "trim":
        raise NotImplementedError(f"boundary={boundary!r}; only 'trim' is implemented")
    if min(factor_lat, factor_lon) < 1:
        raise ValueError("block factors must be >= 1")
    if max(factor_lat, factor_lon) > MAX_TAPS:
        raise NotImplementedError(f"a block wider than {MAX_TAPS}")
    return BlockMean(factor_lat, factor_lon)


def tables_from_dense(W, wrap):
    """(start int32 (n_out), count int32 (n_out), w fp32 (n_out, taps)) of an (n_out, n_in)
    matrix whose rows are contiguous bands (cyclically contiguous with ``wrap``): row j is
    ``W[j, (start[j] + a) % n_in]``, a < count[j].  ``NotImplementedError`` for a band wider
    than 32, ``ValueError`` for a row whose nonzeros have a gap."""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim != 2 or min(W.shape) < 1:
        raise ValueError(f"a regridding matrix is (n_out, n_in), got {W.shape}")
    if not np.isfinite(W).all():
        raise ValueError("a regridding matrix must be finite")
    n_out, n_in = W.shape
    start = np.zeros(n_out, dtype=np.int32)
    count = np.zeros(n_out, dtype=np.int32)
    for j in range(n_out):
        nz = W[j] != 0.0
        k = int(nz.sum())
        if k == 0:
            continue
        if wrap and k < n_in:
            # a cyclic run begins where a nonzero follows a zero
            begins = np.flatnonzero(nz & ~np.roll(nz, 1))
            if len(begins) != 1:
                raise ValueError(f"row {j} is not one cyclically contiguous band")
            start[j], count[j] = begins[0], k
        else:
            idx = np.flatnonzero(nz)
            if idx[-1] - idx[0] + 1 != k:
                raise ValueError(f"row {j} is not one contiguous band")
            start[j], count[j] = idx[0], k
    taps = max(int(count.max()), 1)
    if taps > MAX_TAPS:
        raise NotImplementedError(f"a band of {taps} taps; the kernel takes up to {MAX_TAPS}")
    w = np.zeros((n_out, taps), dtype=np.float32)
    for j in range(n_out):
        c = int(count[j])
        w[j, :c] = W[j, (int(start[j]) + np.arange(c)) % n_in]
    check_tables(start, count, w, n_in, wrap)
    return start, count, w


def check_tables(start, count, w, n_in, wrap):
    """``ValueError`` for a table the kernel would have to clamp or wrap: a count outside
    [0, taps], or an index that leaves the axis."""
    start, count = np.asarray(start), np.asarray(count)
    n_out, taps = w.shape
    if start.shape != (n_out,) or count.shape != (n_out,):
        raise ValueError("start and count hold one entry per output")
    if not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"taps must be 1..{MAX_TAPS}, got {taps}")
    if (count < 0).any() or (count > taps).any() or (count > n_in).any():
        raise ValueError("a count outside [0, taps]")
    if (start < 0).any() or (start >= n_in).any():
        raise ValueError("a band starts outside the axis")
    if not wrap and (start.astype(np.int64) + count > n_in).any():
        raise ValueError("a band leaves the axis")


# ---- the operator ------------------------------------------------------------------------------

class _Axis:
    def __init__(self, W, wrap):
        self.W = np.array(W, dtype=np.float64)
        self.wrap = bool(wrap)
        self.n_out, self.n_in = self.W.shape
        self.start, self.count, self.w = tables_from_dense(self.W, wrap)
        self.taps = self.w.shape[1]


class _Regrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, R):
        ctx.R = R
        return R._launch(x.detach(), None, None, False, 0.0, float("nan"), None)

    @staticmethod
    def backward(ctx, g):
        return ctx.R.T._launch(N.require_device_f32(g, "grad"), None, None, False, 0.0,
                               float("nan"), None), None


class Regridder:
    """``y = Wlat @ x @ Wlon.T`` per field on the device.

    ``src`` and ``dst`` are ``Grid`` (or (nlat, nlon), an equiangular grid / one of ``src``'s
    kind); ``method`` is ``"conservative"``, ``"bilinear"`` or a ``block_mean(...)`` (``dst`` is
    then not needed: the shape follows from the factors).  The tables are built and validated
    on the host once, and uploaded once per device.

    ``R(x, channels=None, mask=None, skip_nan=False, min_valid=0.0, fill=nan, out=None)``
    takes (B, C, H, W) fp32 on the device and returns (B, C', H', W'); ``channels`` picks and
    orders the channels (repeats allowed).  Without ``mask`` and ``skip_nan`` the map is
    linear, NaN propagates to the outputs whose taps cover it, and the call has a gradient
    (``R.T`` applied to the incoming one).  With a ``mask`` ((H, W) >= 0 on the device) and /
    or ``skip_nan`` the result is ``sum(w v x) / sum(w v)``, v = mask * (x is not NaN), where
    ``sum(w v) > 0`` and ``>= min_valid``, and ``fill`` elsewhere; this mode has no gradient.
    With ``out`` given, and after the first call on a device (and with a channel list),
    the call neither allocates nor synchronises and records into a graph.  Deterministic:
    results do not depend on the batch."""

    def __init__(self, src, dst=None, method="conservative", shape=None):
        if dst is None:
            dst = shape
        if isinstance(method, BlockMean):
            nlat, nlon = src.shape if isinstance(src, Grid) else src
            Wlat, Wlon = method.dense(int(nlat), int(nlon))
            if dst is not None and tuple(_as_grid(dst).shape) != (Wlat.shape[0], Wlon.shape[0]):
                raise ValueError(f"block_mean gives {(Wlat.shape[0], Wlon.shape[0])}, not "
                                 f"{tuple(_as_grid(dst).shape)}")
        elif method in ("conservative", "bilinear"):
            if dst is None:
                raise ValueError(f"{method} regridding needs a destination grid")
            Wlat, Wlon = (conservative if method == "conservative" else bilinear)(src, dst)
        else:
            raise ValueError(f"method must be 'conservative', 'bilinear' or a block_mean(...), "
                             f"got {method!r}")
        self._init(Wlat, Wlon, True)
        self.method = method

    def _init(self, Wlat, Wlon, wrap_lon):
        self.lat, self.lon = _Axis(Wlat, False), _Axis(Wlon, wrap_lon)
        if self.lon.n_in > 8188:
            raise NotImplementedError("source rows longer than 8188 (msfno_regrid stages a row "
                                      "in LDS)")
        self.in_shape = (self.lat.n_in, self.lon.n_in)
        self.out_shape = (self.lat.n_out, self.lon.n_out)
        self._dev, self._slabs, self._T = {}, {}, None

    @classmethod
    def from_dense(cls, Wlat, Wlon, wrap_lon=True):
        """A regridder of two matrices of your own ((nlat_out, nlat_in), (nlon_out, nlon_in))."""
        self = cls.__new__(cls)
        self._init(Wlat, Wlon, wrap_lon)
        self.method = "dense"
        return self

    def dense(self):
        """(Wlat, Wlon) in fp64, as built (the kernel reads their fp32 roundings)."""
        return self.lat.W.copy(), self.lon.W.copy()

    @property
    def T(self):
        """The adjoint regridder, built from the transposed matrices."""
        if self._T is None:
            self._T = Regridder.from_dense(self.lat.W.T, self.lon.W.T, self.lon.wrap)
            self._T._T = self
        return self._T

    def _tables(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            keep, axes = [], []
            for ax in (self.lat, self.lon):
                t = [torch.from_numpy(a).to(device) for a in (ax.start, ax.count, ax.w)]
                keep += t
                axes.append(N.RegridAxis(ax.n_in, ax.n_out, ax.taps, int(ax.wrap),
                                         t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()))
            self._dev[key] = (axes, keep)
        return self._dev[key][0]

    def _slab_tensor(self, B, C, channels, device):
        key = (B, C, tuple(channels), str(torch.device(device)))
        if key not in self._slabs:
            self._slabs[key] = torch.tensor([b * C + c for b in range(B) for c in channels],
                                            dtype=torch.int32, device=device)
        return self._slabs[key]

    def _launch(self, x, channels, mask, skip_nan, min_valid, fill, out):
        B, C = x.shape[:2]
        slab, Co = None, C
        if channels is not None:
            Co = len(channels)
            slab = self._slab_tensor(B, C, channels, x.device)
        shape = (B, Co) + self.out_shape
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or \
                not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"out must be contiguous fp32 {shape} on {x.device}")
        lat, lon = self._tables(x.device)
        with torch.cuda.device(x.device):
            N.check(N.lib().msfno_regrid(
                x.data_ptr(), B * C, N.ptr(slab), B * Co, ctypes.byref(lat), ctypes.byref(lon),
                N.ptr(mask), int(bool(skip_nan)), float(min_valid), float(fill),
                out.data_ptr(), N.stream_of(x.device)), "msfno_regrid")
        return out

    def __call__(self, x, channels=None, mask=None, skip_nan=False, min_valid=0.0,
                 fill=float("nan"), out=None):
        if x.dim() != 4:
            raise ValueError(f"x must be (B, C, H, W), got {tuple(x.shape)}")
        if tuple(x.shape[2:]) != self.in_shape:
            raise ValueError(f"this regridder maps {self.in_shape} fields, got "
                             f"{tuple(x.shape[2:])}")
        if not (min_valid >= 0.0 and math.isfinite(min_valid)):
            raise ValueError(f"min_valid must be finite and >= 0, got {min_valid}")
        normalised = mask is not None or skip_nan
        grad = x.requires_grad and torch.is_grad_enabled()
        if normalised and x.requires_grad:
            raise NotImplementedError(
                "the normalised mode (mask / skip_nan) has no gradient; pass x.detach()")
        if channels is not None:
            C = x.shape[1]
            channels = list(range(C))[channels] if isinstance(channels, slice) else \
                [int(c) for c in channels]
            if not channels or any(not -C <= c < C for c in channels):
                raise ValueError(f"channels {channels} of {C}")
            channels = [c % C for c in channels]
        if grad:
            if out is not None:
                raise ValueError("out= cannot be combined with a gradient")
            if channels is not None:    # torch selects (and scatters the gradient)
                x = x.index_select(1, torch.as_tensor(channels, device=x.device))
            return _Regrid.apply(N.require_device_f32(x, "x"), self)
        x = N.require_device_f32(x.detach(), "x")
        if x.numel() == 0:
            raise ValueError("empty fields")
        if mask is not None:
            mask = N.require_device_f32(mask.detach(), "mask")
            if tuple(mask.shape) != self.in_shape or mask.device != x.device:
                raise ValueError(f"mask must be {self.in_shape} on {x.device}")
        return self._launch(x, channels, mask, skip_nan, min_valid, fill, out)

    def __repr__(self):
        return (f"Regridder({self.in_shape} -> {self.out_shape}, {self.method!r}, taps "
                f"{self.lat.taps} x {self.lon.taps})")


_SST = {}


def sst_input(sst, factor=4, means=None, stds=None):
    """The FiLM generator's input from a fine SST field (B, T, H, W) with NaN over land:
    ``coarsen(latitude=factor, longitude=factor, boundary='trim').mean()`` with NaN skipped
    (MSFNO/Models/data.py:205-213), then ``(x - means) / stds`` (``normalise_film``,
    sfno/model.py:281-287; both or neither, broadcast against (B, T, H', W')).  A coarse cell
    without an ocean point stays NaN, so the reference's ``nan_mask`` selects the same
    cells."""
    if (means is None) != (stds is None):
        raise ValueError("means and stds come together")
    key = (tuple(sst.shape[2:]), int(factor))
    if key not in _SST:
        _SST[key] = Regridder(key[0], method=block_mean(factor, factor))
    y = _SST[key](sst, skip_nan=True)
    if means is not None:
        y = (y - means) / stds
    return y
