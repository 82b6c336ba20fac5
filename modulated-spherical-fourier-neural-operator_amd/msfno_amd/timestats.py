"""Statistics over time at fixed pixel, on the device: climatologies, score maps and the
time mean and variability of a long rollout.

``verification`` reduces over space and ``ensemble`` over members; this module reduces over
time.  The reference forms its hour-of-year climatology on the host with xarray, one variable
per run (``data_process/climatology.py``: ``IterMean``, ``mean += (x - mean) / n`` over 40
years, 29 February dropped, saved every 4 years), and gets score maps by copying every output
to the host.  Here one streaming native call (``msfno_tstats_update``, csrc/timestats.hip)
folds a batch into per-pixel Welford moments, and ``msfno_tstats_merge`` combines two states
(other processes or devices, or neighbouring climatology bins).  Everything is formed from
differences against the running mean: ``sum x^2 - (sum x)^2 / n`` in fp32 is garbage on a
300 K field with 1 K of variability.

A state is a uint32 count (C, H, W) (kept in an int32 tensor: the same bits) and K fp32
planes (K, C, H, W):

    kind    flags    K  planes
    FIELD   0        2  mean, m2
    FIELD   MINMAX   4  mean, m2, lo, hi
    ERROR   0        3  mean_d, m2_d, mean_abs                            d = p - t
    ERROR   ANOM     8  ... mean_pa, m2_pa, mean_ta, m2_ta, c_pt          pa = p - c, ta = t - c

Memory: at 73 x 721 x 1440 a plane is 303 MB; an ``ErrorMaps`` with anomalies is 9 planes
(8 and the count), 2.7 GB per lead time.  ``regrid=`` to 1.5 degrees or a channel subset is the
intended way to keep 40 lead times.

Nothing here synchronises (but the range check of a caller's device ``clim_slab``, skipped
under a stream capture), so updates record into a graph; the count lives on the device.  This
module is plumbing: the arithmetic is in the kernels.
"""
from __future__ import annotations

import datetime as _dt

import torch

from . import _fields as F
from . import _native as N

FIELD, ERROR = 0, 1
MINMAX, ANOM = 1, 2
PLANE_NAMES = {
    (FIELD, 0): ("mean", "m2"),
    (FIELD, MINMAX): ("mean", "m2", "lo", "hi"),
    (ERROR, 0): ("mean_d", "m2_d", "mean_abs"),
    (ERROR, ANOM): ("mean_d", "m2_d", "mean_abs", "mean_pa", "m2_pa", "mean_ta", "m2_ta",
                    "c_pt"),
}


def planes(kind: int, flags: int) -> int:
    """K of a state (``msfno_tstats_planes``)."""
    if (kind, flags) not in PLANE_NAMES:
        raise ValueError(f"unknown kind / flags {(kind, flags)}")
    return N.lib().msfno_tstats_planes(kind, flags)


def _check_dims(*dims):
    if any((not isinstance(d, int)) or d < 1 for d in dims):
        raise ValueError(f"extents must be integers >= 1, got {dims}")


def _check_clim_slab_range(clim, clim_slab):
    """Every entry of a caller's ``clim_slab`` is in [0, K): the kernel reads a climatology
    for every (b, c).  A host map is checked on the host; a device map with one
    synchronising reduction, unless a stream capture is under way."""
    if clim is None or clim_slab is None:
        return
    K = clim.shape[0]
    if isinstance(clim_slab, torch.Tensor) and clim_slab.is_cuda:
        if torch.cuda.is_current_stream_capturing():
            return
        lo, hi = int(clim_slab.min()), int(clim_slab.max())
    else:
        host = torch.as_tensor(clim_slab, dtype=torch.int64).reshape(-1)
        if host.numel() == 0:
            return
        lo, hi = int(host.min()), int(host.max())
    if lo < 0 or hi >= K:
        raise ValueError(f"clim_slab entries must be in [0, {K}) here (no -1: every (b, c) "
                         f"needs its climatology), got {lo}..{hi}")


@N.on_input_device
def _launch_update(in0, in1, clim, clim_slab, kind, flags, skip_nan, count, state):
    B, C, H, W = in0.shape
    N.check(N.lib().msfno_tstats_update(
        kind, flags, in0.data_ptr(), N.ptr(in1), in0.stride(0) if B > 1 else C * H * W,
        0 if in1 is None else (in1.stride(0) if B > 1 else C * H * W), N.ptr(clim),
        N.ptr(clim_slab), B, C, H * W, int(bool(skip_nan)), count.data_ptr(), state.data_ptr(),
        state.stride(0), N.stream_of(in0.device)), "msfno_tstats_update")


@N.on_input_device
def _launch_merge(dcount, dstate, scount, sstate, kind, flags):
    N.check(N.lib().msfno_tstats_merge(
        kind, flags, dcount.data_ptr(), dstate.data_ptr(), dstate.stride(0), scount.data_ptr(),
        sstate.data_ptr(), sstate.stride(0), dcount.numel(), N.stream_of(dcount.device)),
        "msfno_tstats_merge")


def _batch_fields(x, name, shape, device):
    """``x`` (B, C, H, W) or (C, H, W) as an fp32 device tensor whose batch elements are
    dense (the batch stride is free)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or tuple(x.shape[1:]) != shape or x.shape[0] < 1:
        raise ValueError(f"{name} must be (B, C, H, W) or (C, H, W) with (C, H, W) = {shape}, "
                         f"got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{name} must be a GPU (HIP) tensor; libmsfno has no CPU path")
    if x.requires_grad:
        raise ValueError(f"{name} requires grad: the statistics have no gradient; pass "
                         f"{name}.detach()")
    if x.device != device:
        raise ValueError(f"{name} is on {x.device}, the state on {device}")
    if x.dtype != torch.float32:
        x = x.float()
    C, H, W = shape
    if tuple(x.stride()[1:]) != (H * W, W, 1) or (x.shape[0] > 1 and x.stride(0) < C * H * W):
        x = x.contiguous()
    return x


class _Stats:
    """A count and K planes of one kind over (C, nlat, nlon); the base of ``FieldStats`` and
    ``ErrorMaps``.  ``_views`` = (count (C, H, W) int32, planes (K, C, H, W) fp32 with any
    plane stride) makes it a window into a larger allocation.  A state may be built on the
    host (to hold or inspect a state dict); only a device state updates and merges."""

    kind = FIELD

    def __init__(self, C, nlat, nlon, flags, device="cuda", _views=None):
        _check_dims(C, nlat, nlon)
        self.shape = (C, nlat, nlon)
        self.flags = flags
        self.K = len(PLANE_NAMES[(self.kind, flags)])
        if _views is None:
            self.device = F.device_key(device)
            self._count = torch.empty(C, nlat, nlon, dtype=torch.int32, device=self.device)
            self._planes = torch.empty(self.K, C, nlat, nlon, dtype=torch.float32,
                                       device=self.device)
            self.reset()
        else:
            self._count, self._planes = _views
            self.device = self._count.device
            assert tuple(self._count.shape) == self.shape and self._count.is_contiguous()
            assert tuple(self._planes.shape) == (self.K,) + self.shape
            assert tuple(self._planes.stride()[1:]) == (nlat * nlon, nlon, 1)

    def reset(self):
        """The fresh state: count 0, planes 0, lo = +inf, hi = -inf."""
        self._count.zero_()
        self._planes.zero_()
        if self.kind == FIELD and self.flags & MINMAX:
            self._planes[2].fill_(float("inf"))
            self._planes[3].fill_(float("-inf"))
        return self

    @property
    def count(self) -> torch.Tensor:
        """(C, H, W) int64: the valid updates per pixel."""
        return self._count.to(torch.int64) & 0xFFFFFFFF

    def _plane(self, name):
        return self._planes[PLANE_NAMES[(self.kind, self.flags)].index(name)]

    def _where_counted(self, x, more_than=0):
        return torch.where(self.count > more_than, x, torch.full_like(x, float("nan")))

    def _per_n(self, name, ddof=0):
        n = (self.count - ddof).clamp(min=1).to(torch.float32)
        return self._where_counted(self._plane(name) / n, ddof)

    def _check_other(self, other):
        if type(other) is not type(self) or other.shape != self.shape or \
                other.flags != self.flags:
            raise ValueError("merge needs a state of the same class, shape and flags")
        if not self._count.is_cuda:
            raise ValueError("merge needs device states; libmsfno has no CPU path")
        if other.device != self.device:
            raise ValueError(f"merge: the other state is on {other.device}, this one on "
                             f"{self.device} (copy it over with state_dict / load_state_dict)")
        if other is self or other._count.data_ptr() == self._count.data_ptr():
            raise ValueError("merge of a state into itself")

    @torch.no_grad()
    def merge(self, other):
        """self <- self (+) other (``msfno_tstats_merge``): the accumulators of two
        processes or devices, each over its own initial dates.  ``other`` is unchanged."""
        self._check_other(other)
        _launch_merge(self._count, self._planes, other._count, other._planes, self.kind,
                      self.flags)
        return self

    def state_dict(self):
        """The raw count and planes (copies) with what identifies them: enough to save a long
        accumulation and resume it bit for bit."""
        return {"kind": self.kind, "flags": self.flags, "shape": self.shape,
                "count": self._count.clone(), "planes": self._planes.contiguous().clone()}

    def load_state_dict(self, sd):
        if (sd["kind"], sd["flags"], tuple(sd["shape"])) != (self.kind, self.flags, self.shape):
            raise ValueError(f"state dict of kind / flags / shape "
                             f"{(sd['kind'], sd['flags'], tuple(sd['shape']))}, this state is "
                             f"{(self.kind, self.flags, self.shape)}")
        self._count.copy_(sd["count"])
        self._planes.copy_(sd["planes"])
        return self

    def _clim_args(self, clim, clim_slab, B):
        from .verification import _check_clim
        if isinstance(clim, torch.Tensor) and not clim.is_cuda:
            clim = clim.to(self.device, non_blocking=True)
        clim, slab = _check_clim(clim, clim_slab, (B,) + self.shape, self.device)
        if clim_slab is not None:
            _check_clim_slab_range(clim, clim_slab)
        return clim, slab


class FieldStats(_Stats):
    """Per-pixel mean and variance (and, with ``minmax``, the range) of the fields it is
    updated with: the time mean and variability of a rollout, or one climatology bin.

    2 planes and the count, 4 with ``minmax``; at 73 x 721 x 1440 a plane is 303 MB."""

    kind = FIELD

    def __init__(self, C, nlat, nlon, minmax=False, device="cuda", _views=None):
        super().__init__(C, nlat, nlon, MINMAX if minmax else 0, device, _views)

    @torch.no_grad()
    def update(self, x, clim=None, clim_slab=None, skip_nan=False):
        """Fold ``x`` (B, C, H, W) or (C, H, W) in, batch elements in order; with a
        climatology (``clim`` / ``clim_slab`` as ``verification.field_sums`` takes them, every
        slab index >= 0) the statistics are those of ``x - clim``.  With ``skip_nan`` an
        update is left out where ``x`` or ``clim`` is NaN."""
        x = _batch_fields(x, "x", self.shape, self.device)
        clim, slab = self._clim_args(clim, clim_slab, x.shape[0])
        _launch_update(x, None, clim, slab, FIELD, self.flags, skip_nan, self._count,
                       self._planes)
        return self

    @property
    def mean(self):
        return self._where_counted(self._plane("mean"))

    def var(self, ddof=0):
        """m2 / (n - ddof); NaN where the count is at most ``ddof``."""
        return self._per_n("m2", ddof)

    @property
    def std(self):
        return torch.sqrt(self.var())

    def _range(self, name):
        if not self.flags & MINMAX:
            raise ValueError("built without minmax=True")
        return self._where_counted(self._plane(name))

    @property
    def min(self):
        return self._range("lo")

    @property
    def max(self):
        return self._range("hi")


class ErrorMaps(_Stats):
    """Per-pixel bias, RMSE, MAE and, with ``anomalies``, ACC of forecasts against truths,
    accumulated over many initial dates at one lead time.

    3 planes and the count; with ``anomalies`` 8 planes and the count: 9 x 303 MB = 2.7 GB at
    73 x 721 x 1440.  ``regrid=`` to 1.5 degrees or a channel subset keeps 40 lead times."""

    kind = ERROR

    def __init__(self, C, nlat, nlon, anomalies=False, device="cuda", _views=None):
        super().__init__(C, nlat, nlon, ANOM if anomalies else 0, device, _views)

    @property
    def anomalies(self):
        return bool(self.flags & ANOM)

    @torch.no_grad()
    def update(self, prd, tar, clim=None, clim_slab=None, skip_nan=False):
        """Fold the errors of ``prd`` against ``tar`` (both (B, C, H, W) or (C, H, W)) in.
        The anomaly planes need a climatology on every update, and only they take one
        (``clim`` / ``clim_slab`` as ``verification.field_sums`` takes them, every slab index
        >= 0).  With ``skip_nan`` an update is left out where ``tar`` or ``clim`` is NaN; a
        NaN in ``prd`` is never skipped.  A host ``tar`` is copied without blocking."""
        if clim is not None and not self.anomalies:
            raise ValueError("a climatology needs ErrorMaps(..., anomalies=True)")
        if clim is None and self.anomalies:
            raise ValueError("built with anomalies=True: every update needs a climatology")
        if clim is None and clim_slab is not None:
            raise ValueError("clim_slab without clim")
        prd = _batch_fields(prd, "prd", self.shape, self.device)
        if isinstance(tar, torch.Tensor) and not tar.is_cuda:
            tar = tar.to(self.device, non_blocking=True)
        tar = _batch_fields(tar, "tar", self.shape, self.device)
        if tar.shape != prd.shape:
            raise ValueError(f"prd and tar must be of one shape, got {tuple(prd.shape)} and "
                             f"{tuple(tar.shape)}")
        clim, slab = self._clim_args(clim, clim_slab, prd.shape[0])
        _launch_update(prd, tar, clim, slab, ERROR, self.flags, skip_nan, self._count,
                       self._planes)
        return self

    @property
    def bias(self):
        return self._where_counted(self._plane("mean_d"))

    @property
    def error_std(self):
        return torch.sqrt(self._per_n("m2_d"))

    @property
    def mae(self):
        return self._where_counted(self._plane("mean_abs"))

    @property
    def mse(self):
        """m2_d / n + mean_d^2."""
        return self._per_n("m2_d") + self.bias ** 2

    @property
    def rmse(self):
        return torch.sqrt(self.mse)

    def moments(self):
        """(pa2, ta2, cross) / n per pixel, the uncentred anomaly moments of
        ``verification``: m2_pa / n + mean_pa^2, likewise ta2, c_pt / n + mean_pa mean_ta."""
        if not self.anomalies:
            raise ValueError("built without anomalies=True")
        mpa = self._where_counted(self._plane("mean_pa"))
        mta = self._where_counted(self._plane("mean_ta"))
        return (self._per_n("m2_pa") + mpa ** 2, self._per_n("m2_ta") + mta ** 2,
                self._per_n("c_pt") + mpa * mta)

    def acc(self, centred=False):
        """The anomaly correlation over the cases, per pixel: ``verification``'s uncentred
        ``cross / sqrt(pa2 ta2)`` rebuilt from the moments, or with ``centred`` the Pearson
        form ``c_pt / sqrt(m2_pa m2_ta)``."""
        if centred:
            if not self.anomalies:
                raise ValueError("built without anomalies=True")
            return self._where_counted(self._plane("c_pt") / (
                torch.sqrt(self._plane("m2_pa")) * torch.sqrt(self._plane("m2_ta"))))
        pa2, ta2, cross = self.moments()
        return cross / (torch.sqrt(pa2) * torch.sqrt(ta2))


class _Stack:
    """``n`` states of one class over one allocation: the count (n, C, H, W) and the planes
    (K, n, C, H, W), so that every plane of a member has the stack's plane stride and a whole
    stack merges in one call."""

    def __init__(self, cls, n, C, nlat, nlon, device, **kw):
        _check_dims(n, C, nlat, nlon)
        self.device = F.device_key(device)
        flags = (MINMAX if kw.get("minmax") else 0) | (ANOM if kw.get("anomalies") else 0)
        K = len(PLANE_NAMES[(cls.kind, flags)])
        self.shape = (C, nlat, nlon)
        self._count = torch.empty(n, C, nlat, nlon, dtype=torch.int32, device=self.device)
        self._planes = torch.empty(K, n, C, nlat, nlon, dtype=torch.float32,
                                   device=self.device)
        self._items = [cls(C, nlat, nlon, _views=(self._count[i], self._planes[:, i]), **kw)
                       for i in range(n)]
        self.reset()

    def reset(self):
        for it in self._items:
            it.reset()
        return self

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        return self._items[i]

    def __iter__(self):
        return iter(self._items)

    @torch.no_grad()
    def merge(self, other):
        """Every member with ``other``'s member of the same index, in one call."""
        if type(other) is not type(self) or len(other) != len(self):
            raise ValueError("merge needs a stack of the same class and length")
        self._items[0]._check_other(other._items[0])
        it = self._items[0]
        _launch_merge(self._count, self._planes, other._count, other._planes, it.kind, it.flags)
        return self

    def state_dict(self):
        it = self._items[0]
        return {"kind": it.kind, "flags": it.flags, "shape": (len(self),) + self.shape,
                "count": self._count.clone(), "planes": self._planes.clone()}

    def load_state_dict(self, sd):
        it = self._items[0]
        want = (it.kind, it.flags, (len(self),) + self.shape)
        if (sd["kind"], sd["flags"], tuple(sd["shape"])) != want:
            raise ValueError(f"state dict of kind / flags / shape "
                             f"{(sd['kind'], sd['flags'], tuple(sd['shape']))}, this stack is "
                             f"{want}")
        self._count.copy_(sd["count"])
        self._planes.copy_(sd["planes"])
        return self


class LeadTimeMaps(_Stack):
    """``n_scored`` ``ErrorMaps`` over one allocation, indexed by scored step: what
    ``Rollout.verify_maps`` fills, batch of initial dates after batch.

    Memory: n_scored x (3 or 8 planes and the count); at 73 x 721 x 1440 with anomalies 2.7 GB
    per lead time.  ``regrid=`` to 1.5 degrees or a channel subset keeps 40 lead times."""

    def __init__(self, n_scored, C, nlat, nlon, anomalies=False, device="cuda"):
        super().__init__(ErrorMaps, n_scored, C, nlat, nlon, device, anomalies=anomalies)
        self.anomalies = bool(anomalies)


def hour_of_year_bin(when: _dt.datetime, step_hours: int = 6):
    """The climatology bin of ``when`` by the reference's rule (data_process/climatology.py):
    365 x (24 / step_hours) bins, 1460 at 6 h; 29 February has none (``None``: the reference
    drops indices 236-239 of a leap year) and every later date of a leap year shifts down by
    one day, so 1 March 00 UTC is bin 236 in every year."""
    if not isinstance(step_hours, int) or step_hours < 1 or 24 % step_hours:
        raise ValueError(f"step_hours must divide 24, got {step_hours}")
    if when.hour % step_hours or when.minute or when.second or when.microsecond:
        raise ValueError(f"{when} is not on a {step_hours} h step")
    day = when.timetuple().tm_yday - 1
    leap = when.year % 4 == 0 and (when.year % 100 != 0 or when.year % 400 == 0)
    if leap:
        if (when.month, when.day) == (2, 29):
            return None
        if day > 59:
            day -= 1
    return day * (24 // step_hours) + when.hour // step_hours


class Climatology(_Stack):
    """``nbins`` ``FieldStats`` over one allocation: a binned climatology built on the device
    (2 planes and the count per bin; a plane of 73 x 721 x 1440 is 303 MB, so 1460 bins want a
    channel subset or a coarser grid)."""

    hour_of_year_bin = staticmethod(hour_of_year_bin)

    def __init__(self, nbins, C, nlat, nlon, device="cuda"):
        super().__init__(FieldStats, nbins, C, nlat, nlon, device)

    def _check_bins(self, bins, n=None, allow_none=False):
        bins = list(bins)
        if n is not None and len(bins) != n:
            raise ValueError(f"bins must hold one entry per batch element ({n}), got "
                             f"{len(bins)}")
        for b in bins:
            if b is None and allow_none:
                continue
            if not isinstance(b, int) or not 0 <= b < len(self):
                raise ValueError(f"a bin must be an integer in [0, {len(self)})"
                                 f"{' or None' if allow_none else ''}, got {b!r}")
        return bins

    @torch.no_grad()
    def update(self, x, bins, skip_nan=False):
        """Fold batch element ``b`` of ``x`` (B, C, H, W) into bin ``bins[b]`` (a host
        integer, or None to leave the element out, as for 29 February).  One call where all
        the elements share a bin, otherwise one call per element: two elements of one call
        never write one state."""
        nb = x.shape[0] if isinstance(x, torch.Tensor) and x.dim() == 4 else 1
        bins = self._check_bins(bins, nb, allow_none=True)
        x = _batch_fields(x, "x", self.shape, self.device)
        if bins[0] is not None and all(b == bins[0] for b in bins):
            self[bins[0]].update(x, skip_nan=skip_nan)
        else:
            for b, j in enumerate(bins):
                if j is not None:
                    self[j].update(x[b], skip_nan=skip_nan)
        return self

    def mean(self, bins):
        """The means of ``bins`` (a sequence of bin indices), (len(bins), C, H, W); NaN where
        a bin has no update."""
        return torch.stack([self[j].mean for j in self._check_bins(bins)])

    def as_clim(self, bins):
        """``(clim, clim_slab)`` for a batch whose element ``b`` falls into ``bins[b]``,
        exactly as ``verification.field_sums``, ``ErrorMaps.update`` and ``Rollout.verify``
        take them: the (K, H, W) stack of the means of the distinct bins and the device int32
        map of the B * C slabs."""
        bins = self._check_bins(bins)
        C = self.shape[0]
        uniq = sorted(set(bins))
        clim = self.mean(uniq).reshape(len(uniq) * C, *self.shape[1:])
        slab = [uniq.index(j) * C + c for j in bins for c in range(C)]
        return clim, torch.tensor(slab, dtype=torch.int32).to(self.device, non_blocking=True)

    @torch.no_grad()
    def window(self, k):
        """A new ``Climatology`` whose bin ``j`` is the merge of bins ``j - k .. j + k``,
        periodic: bin ``j`` itself, then for d = 1 .. k bin ``j - d``, then bin ``j + d``."""
        if not isinstance(k, int) or k < 0 or 2 * k + 1 > len(self):
            raise ValueError(f"window half-width {k} with {len(self)} bins")
        C, H, W = self.shape
        out = Climatology(len(self), C, H, W, device=self.device)
        out._count.copy_(self._count)
        out._planes.copy_(self._planes)
        n = len(self)
        for j in range(n):
            for d in range(1, k + 1):
                out[j].merge(self[(j - d) % n])
                out[j].merge(self[(j + d) % n])
        return out
