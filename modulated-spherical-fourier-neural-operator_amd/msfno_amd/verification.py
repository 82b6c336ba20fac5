"""Forecast verification on the device: RMSE, bias, MAE, the climatology skill score and
the anomaly correlation (ACC) of a rollout.

The reference scores a forecast on the host: ``evaluate_model``
(``MSFNO/Models/sfno/model.py:656-811``) and ``Trainer.validation`` (``train.py:533-583``)
copy every scored output off the device (``model.py:741,748``), denormalise it and form
per-variable MSEs and ``1 - MSE(prd, truth) / MSE(clim, truth)`` (``model.py:743-758``).
Here one native pass (``msfno_verify_sums``, csrc/verify.hip) over the forecast, the truth
and an optional climatology leaves six latitude-weighted sums per (batch, channel),

    se = sum w (p-t)^2    err = sum w (p-t)       ae = sum w |p-t|
    pa2 = sum w (p-c)^2   ta2 = sum w (t-c)^2     cross = sum w (p-c)(t-c)

and ``finish`` turns them into scores with plain torch on (B, C) numbers.  The sums are
additive over rows: a latitude-band rank calls ``field_sums`` on its own rows with
``w[rows]`` and ``clim[..., rows, :]``, all-reduces the (B, C, 6) result and finishes with
the whole grid's ``w``.

``Verifier`` is the preallocated form for a rollout (one launch per scored step into a
slot, nothing synchronises); ``Rollout.verify`` drives it.

Regional and masked scores: ``region_sums`` (``msfno_verify_region_sums``,
csrc/verify_regions.hip) takes a ``regions.Regions`` and leaves seven sums per (batch,
channel, region), ``n = sum w`` over the region's valid pixels and the six above over the
same pixels; ``finish_regions`` divides by that ``n``.  With ``skip_nan`` a pixel whose truth
(or climatology) is NaN is left out.  ``RegionalVerifier`` is the rollout form.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import _fields as F
from . import _native as N

NSUMS = 6
SE, ERR, AE, PA2, TA2, CROSS = range(NSUMS)
NRSUMS = 7   # per region: n, then the six

Scores = namedtuple("Scores", ["mse", "rmse", "bias", "mae", "skill", "acc"])

_slab_cache: dict = {}


def _default_slabs(clim_dim, B, C, device):
    """The slab map of a (C, H, W) climatology (broadcast over the batch) or a
    (B, C, H, W) one; built on the device (no host copy), cached per (kind, B, C, device)."""
    key = (clim_dim, B, C, F.device_key(device))
    m = _slab_cache.get(key)
    if m is None:
        if clim_dim == 3:
            m = torch.arange(C, dtype=torch.int32, device=device).repeat(B)
        else:
            m = torch.arange(B * C, dtype=torch.int32, device=device)
        _slab_cache[key] = m
    return m


def _check_fields(prd, tar, w):
    F.check_pair(prd, tar)
    return F.check_fields(prd, tar, w, "prd", no_grad=("verification", "msfno_amd.losses"))


def _check_clim(clim, clim_slab, shape, device):
    """(clim as (K, H, W), slab map as int32 (B C,)) on ``device``, or (None, None)."""
    B, C, H, W = shape
    if clim is None:
        if clim_slab is not None:
            raise ValueError("clim_slab without clim")
        return None, None
    if clim.requires_grad:
        raise ValueError("clim requires grad: the verification sums have no gradient")
    clim = N.require_device_f32(clim, "clim")
    if clim.device != device:
        raise ValueError("clim must be on the device of prd")
    if clim_slab is None:
        if tuple(clim.shape) not in ((C, H, W), (B, C, H, W)):
            raise ValueError(f"clim must be (C, H, W) = {(C, H, W)} or (B, C, H, W) = "
                             f"{(B, C, H, W)} without a clim_slab, got {tuple(clim.shape)}")
        return clim.reshape(-1, H, W), _default_slabs(clim.dim(), B, C, device)
    if clim.dim() != 3 or tuple(clim.shape[1:]) != (H, W) or clim.shape[0] < 1:
        raise ValueError(f"clim must be (K, H, W) with (H, W) = {(H, W)} under a clim_slab, "
                         f"got {tuple(clim.shape)}")
    if not isinstance(clim_slab, torch.Tensor) or not clim_slab.is_cuda:
        # a host map is range-checked here; a device map is trusted (checking it would
        # synchronise)
        host = torch.as_tensor(clim_slab, dtype=torch.int64).reshape(-1)
        if host.numel() and (host.min() < -1 or host.max() >= clim.shape[0]):
            raise ValueError(f"clim_slab entries must be -1 or in [0, {clim.shape[0]})")
        clim_slab = host.to(torch.int32).to(device, non_blocking=True)
    if clim_slab.dtype != torch.int32:
        clim_slab = clim_slab.to(torch.int32)
    clim_slab = clim_slab.reshape(-1).contiguous()
    if clim_slab.numel() != B * C or clim_slab.device != device:
        raise ValueError(f"clim_slab must hold B * C = {B * C} slab indices on the device of "
                         f"prd, got {tuple(clim_slab.shape)} on {clim_slab.device}")
    return clim, clim_slab


def workspace(B: int, C: int, nlat: int, nlon: int, device) -> torch.Tensor:
    """A workspace for ``msfno_verify_sums`` at this shape (contents do not matter)."""
    return torch.empty(N.lib().msfno_verify_workspace_size(B * C, nlat, nlon),
                       dtype=torch.uint8, device=device)


@N.on_input_device
def _launch(prd, tar, w, clim, clim_slab, out, ws):
    B, C, H, W = prd.shape
    N.check(N.lib().msfno_verify_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), N.ptr(clim),
                                      N.ptr(clim_slab), out.data_ptr(), B * C, H, W,
                                      ws.data_ptr(), ws.numel(), N.stream_of(prd.device)),
            "msfno_verify_sums")
    return out


@torch.no_grad()
def field_sums(prd, tar, w, clim=None, clim_slab=None) -> torch.Tensor:
    """(B, C, 6) fp32 = {se, err, ae, pa2, ta2, cross} of (B, C, H, W) fp32 device fields
    under the latitude weights ``w`` (any fp32 device vector of length H).

    ``clim`` is (C, H, W) (one climatology for every sample) or (B, C, H, W); or, with an
    explicit ``clim_slab`` (B * C slab indices, -1 for a slab without a climatology), a
    (K, H, W) stack.  A device ``clim_slab`` is not range-checked.  Slabs without a
    climatology get exact zeros in the last three sums.  No gradient."""
    prd, tar, w = _check_fields(prd, tar, w)
    clim, clim_slab = _check_clim(clim, clim_slab, prd.shape, prd.device)
    B, C, H, W = prd.shape
    out = torch.empty(B, C, NSUMS, dtype=torch.float32, device=prd.device)
    return _launch(prd, tar, w, clim, clim_slab, out, workspace(B, C, H, W, prd.device))


def finish(sums, w, nlon, batch_mean=False) -> Scores:
    """Scores from (..., B, C, 6) sums (device or host, any float dtype) taken under the
    weights ``w`` of the whole grid, with n = nlon * sum(w):

        mse = se / n, rmse = sqrt(mse), bias = err / n, mae = ae / n,
        skill = 1 - se / ta2  (model.py:757),  acc = cross / sqrt(pa2 ta2)

    each of shape (..., B, C); ``skill`` and ``acc`` are NaN where the slab had no
    climatology.  ``batch_mean`` adds the sums over B first and returns (..., C): with
    uniform weights ``mse`` is then the reference's ``.mean(dim=(0, 2, 3))``."""
    if sums.shape[-1] != NSUMS or sums.dim() < 3:
        raise ValueError(f"sums must be (..., B, C, {NSUMS}), got {tuple(sums.shape)}")
    n = F.grid_weight(w, nlon, sums.device)
    if batch_mean:
        n = n * sums.shape[-3]
        sums = sums.sum(dim=-3)
    n = n.to(sums.dtype)
    se, err, ae, pa2, ta2, cross = sums.unbind(-1)
    mse = se / n
    # no climatology: pa2 = ta2 = 0 exactly.  (With one, both vanish only where
    # prd = tar = clim everywhere, and 0 / 0 is NaN there too.)
    nan = torch.full_like(se, float("nan"))
    none = (pa2 == 0) & (ta2 == 0)
    skill = torch.where(none, nan, 1 - se / ta2)
    acc = torch.where(none, nan, cross / (torch.sqrt(pa2) * torch.sqrt(ta2)))
    return Scores(mse, torch.sqrt(mse), err / n, ae / n, skill, acc)


def regions_workspace(B: int, C: int, nlat: int, nlon: int, nregions: int, device) -> torch.Tensor:
    """A workspace for ``msfno_verify_region_sums`` at this shape (contents do not matter)."""
    return torch.empty(N.lib().msfno_verify_regions_workspace_size(B * C, nlat, nlon, nregions),
                       dtype=torch.uint8, device=device)


def _check_regions(regions, shape):
    from .regions import Regions
    if not isinstance(regions, Regions):
        raise ValueError(f"regions must be a regions.Regions, got {type(regions).__name__}")
    if tuple(regions.shape) != tuple(shape[2:]):
        raise ValueError(f"the regions are of a {regions.shape} grid, the fields are "
                         f"{tuple(shape[2:])}")
    return regions


@N.on_input_device
def _launch_regions(prd, tar, w, clim, clim_slab, regions, skip_nan, out, ws):
    B, C, H, W = prd.shape
    row, col, pix = regions.tables(prd.device)
    N.check(N.lib().msfno_verify_region_sums(
        prd.data_ptr(), tar.data_ptr(), w.data_ptr(), N.ptr(clim), N.ptr(clim_slab),
        row.data_ptr(), col.data_ptr(), N.ptr(pix), len(regions), int(bool(skip_nan)),
        out.data_ptr(), B * C, H, W, ws.data_ptr(), ws.numel(), N.stream_of(prd.device)),
        "msfno_verify_region_sums")
    return out


@torch.no_grad()
def region_sums(prd, tar, w, regions, clim=None, clim_slab=None, skip_nan=False) -> torch.Tensor:
    """(B, C, R, 7) fp32 = {n, se, err, ae, pa2, ta2, cross} per region of ``regions`` (a
    ``regions.Regions`` of the fields' grid): ``n = sum w`` over the region's valid pixels
    and the six sums of ``field_sums`` over the same pixels.  Fields, ``w``, ``clim`` and
    ``clim_slab`` as in ``field_sums``.  With ``skip_nan`` a pixel is left out where ``tar``
    is NaN or, for a slab with a climatology, ``clim`` is; a NaN in ``prd`` is never
    skipped.  A region's sums depend only on the values at its own valid pixels.  No
    gradient."""
    prd, tar, w = _check_fields(prd, tar, w)
    regions = _check_regions(regions, prd.shape)
    clim, clim_slab = _check_clim(clim, clim_slab, prd.shape, prd.device)
    B, C, H, W = prd.shape
    R = len(regions)
    out = torch.empty(B, C, R, NRSUMS, dtype=torch.float32, device=prd.device)
    return _launch_regions(prd, tar, w, clim, clim_slab, regions, skip_nan, out,
                           regions_workspace(B, C, H, W, R, prd.device))


def finish_regions(sums, batch_mean=False) -> Scores:
    """Scores from (..., B, C, R, 7) regional sums (device or host, any float dtype), each
    of shape (..., B, C, R): as ``finish`` with the region's own ``n`` (the first of its
    seven sums) in place of ``nlon * sum(w)``.  Every score of a region with ``n == 0``
    (empty, or all of it missing) is NaN; ``skill`` and ``acc`` are NaN too where the slab
    had no climatology.  ``batch_mean`` adds the sums over B first and returns (..., C, R)."""
    if sums.shape[-1] != NRSUMS or sums.dim() < 4:
        raise ValueError(f"sums must be (..., B, C, R, {NRSUMS}), got {tuple(sums.shape)}")
    if batch_mean:
        sums = sums.sum(dim=-4)
    n, se, err, ae, pa2, ta2, cross = sums.unbind(-1)
    nan = torch.full_like(se, float("nan"))
    empty = n == 0

    def per_n(x):
        return torch.where(empty, nan, x / n)

    mse = per_n(se)
    none = empty | ((pa2 == 0) & (ta2 == 0))
    skill = torch.where(none, nan, 1 - se / ta2)
    acc = torch.where(none, nan, cross / (torch.sqrt(pa2) * torch.sqrt(ta2)))
    return Scores(mse, torch.sqrt(mse), per_n(err), per_n(ae), skill, acc)


def mse_normalised(mse, stds):
    """The MSE in normalised space from the raw-space ``mse`` (..., C): mse / std^2, exact
    because the reference's normalisation is a per-channel affine (model.py:273-279)."""
    stds = torch.as_tensor(stds).to(mse).reshape(-1)
    if stds.numel() != mse.shape[-1]:
        raise ValueError(f"stds must hold one value per channel ({mse.shape[-1]}), got "
                         f"{stds.numel()}")
    return mse / stds ** 2


def kinetic_energy_spectrum(u, v, vsht):
    """Kinetic energy per degree (..., lmax) of the wind ``(u, v)`` (..., nlat, nlon),
    eastward and northward, on the unit sphere, through ``vsht``, a
    ``harmonics.RealVectorSHT`` of the fields' grid:

        KE_l = l(l+1) / (8 pi) [power(s)_l + power(t)_l]

    with ``power`` of ``harmonics.power_spectrum``; its sum over l is the global mean of
    ``|v|^2 / 2`` of the band-limited wind.  Differentiable in u and v, and bitwise
    reproducible like the power spectrum."""
    from .harmonics import power_spectrum, uv_to_vector
    p = power_spectrum(vsht(uv_to_vector(u, v)))  # (..., 2, lmax)
    l = torch.arange(p.shape[-1], device=p.device, dtype=torch.float32)
    return (p[..., 0, :] + p[..., 1, :]) * (l * (l + 1) / (8 * math.pi))


class Verifier(F.SlotVerifier):
    """The sums of ``n_scored`` scored steps of a rollout of (B, C, nlat, nlon) fields, in
    one preallocated (n_scored, B, C, 6) device tensor ``sums`` with one workspace.

    ``weights`` is one of ``losses.KINDS`` ("uniform" is the reference's ``MSELoss``,
    "cosine" the usual area weighting) or an fp32 vector of nlat weights.  ``update``
    launches into a slot and never synchronises, so it records into a graph; a slot that
    was never updated holds NaN."""

    def __init__(self, weights, nlat, nlon, n_scored, B, C, device="cuda"):
        super().__init__(weights, nlat, nlon, n_scored, B, C, device)
        self.shape = (B, C, nlat, nlon)
        self.sums = self._alloc(NSUMS)
        self._ws = workspace(B, C, nlat, nlon, self.device)

    @torch.no_grad()
    def update(self, k, y, tar, clim=None, clim_slab=None):
        """Score the forecast ``y`` against ``tar`` (and ``clim``, as in ``field_sums``)
        into slot ``k``.  A host ``tar`` or ``clim`` is copied with non_blocking=True."""
        self._check_slot(k, y, "fields")
        y, tar, w = _check_fields(y, self._on_device(tar), self.w)
        clim, clim_slab = _check_clim(self._on_device(clim), clim_slab, y.shape, y.device)
        _launch(y, tar, w, clim, clim_slab, self.sums[k], self._ws)

    def scores(self, batch_mean=False) -> Scores:
        """``finish`` of all slots: Scores of (n_scored, B, C) tensors, or (n_scored, C)."""
        return finish(self.sums, self.w, self.shape[3], batch_mean=batch_mean)


class RegionalVerifier(F.SlotVerifier):
    """``Verifier`` per region: the sums of ``n_scored`` scored steps of a rollout of
    (B, C, nlat, nlon) fields over the R regions of ``regions`` (a ``regions.Regions`` of
    that grid), in one preallocated (n_scored, B, C, R, 7) device tensor ``sums`` with one
    workspace.  ``skip_nan`` as in ``region_sums``.  ``update`` launches into a slot and
    never synchronises, so it records into a graph; a slot that was never updated holds
    NaN."""

    def __init__(self, weights, regions, n_scored, B, C, skip_nan=False, device="cuda"):
        from .regions import Regions
        if not isinstance(regions, Regions):
            raise ValueError(f"regions must be a regions.Regions, got {type(regions).__name__}")
        nlat, nlon = regions.shape
        super().__init__(weights, nlat, nlon, n_scored, B, C, device)
        self.shape = (B, C, nlat, nlon)
        self.regions, self.skip_nan = regions, bool(skip_nan)
        self.sums = torch.full((n_scored, B, C, len(regions), NRSUMS), float("nan"),
                               dtype=torch.float32, device=self.device)
        self._ws = regions_workspace(B, C, nlat, nlon, len(regions), self.device)
        regions.tables(self.device)

    @torch.no_grad()
    def update(self, k, y, tar, clim=None, clim_slab=None):
        """Score the forecast ``y`` against ``tar`` (and ``clim``, as in ``region_sums``)
        into slot ``k``.  A host ``tar`` or ``clim`` is copied with non_blocking=True."""
        self._check_slot(k, y, "fields")
        y, tar, w = _check_fields(y, self._on_device(tar), self.w)
        clim, clim_slab = _check_clim(self._on_device(clim), clim_slab, y.shape, y.device)
        _launch_regions(y, tar, w, clim, clim_slab, self.regions, self.skip_nan, self.sums[k],
                        self._ws)

    def scores(self, batch_mean=False) -> Scores:
        """``finish_regions`` of all slots: Scores of (n_scored, B, C, R) tensors, or
        (n_scored, C, R)."""
        return finish_regions(self.sums, batch_mean=batch_mean)
