"""Forecast export: 16-bit field packing on the device and an asynchronous host writer.

The reference copies every output to the host in full precision before it writes it
(train.py:996-998, ``output.cpu().numpy()`` then ``save_to_zarr_forecast``).  Here a step is
subset and packed on the device, copied on a stream of its own into pinned memory while the
next step runs, and handed to a sink in step order.

Encoding (``msfno_pack16``, csrc/pack.hip; GRIB simple packing with a binary scale, the
``scale_factor = 2^E`` / ``add_offset = R`` of netCDF and zarr).  Per (batch, channel) field,
over the selected points only, in fp32::

    lo = min x, hi = max x, d = hi - lo, R = lo
    E  = 0 where d == 0, else the smallest integer with d <= 65535 * 2^E, at least -126
    q  = uint16(rint((x - R) * 2^-E))        round to nearest even, clamped to [0, 65535]
    xhat = R + float32(q) * 2^E              |xhat - x| <= 2^(E-1) + ulp(d)/2 + ulp(xhat)/2

Inputs are finite, and so is ``hi - lo``: that is the caller's contract and is not checked.

``pack`` / ``unpack`` are the device calls, ``decode_numpy`` and ``Packed.numpy`` the same
decode on the host.  The public numpy dtype of ``q`` is ``uint16``.  On the torch side ``q`` is
a ``torch.uint16`` tensor: this torch's ``copy_``, ``.cpu()``, ``.numpy()`` and
``.view(torch.uint16)`` of a byte buffer support it (probed at import; were one of them
missing, ``Q_DTYPE`` falls back to ``torch.int16`` storage holding the same bits).  The pinned
host buffers of the writer are byte buffers viewed from numpy, so they do not depend on it.

``ForecastWriter`` is the ring of staging buffers, ``MemorySink`` and ``NpyArchive`` are
sinks, ``open_archive`` reads an archive back (on the host, or as the ``truths`` of
``Rollout.verify`` at half the host-to-device bytes), and ``Rollout.export`` drives a writer.
No zarr, netCDF or GRIB writer: a sink is any ``callable(step, host_packed)``.
"""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

from . import _native as N


def _probe_uint16():
    try:
        a = torch.zeros(4, dtype=torch.uint8).view(torch.uint16)
        b = torch.empty(2, dtype=torch.uint16)
        b.copy_(a)
        return b.numpy().dtype == np.uint16 and torch.from_numpy(
            np.zeros(2, np.uint16)).dtype == torch.uint16
    except Exception:
        return False


Q_DTYPE = torch.uint16 if hasattr(torch, "uint16") and _probe_uint16() else torch.int16


def _index(i, n, what):
    if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
        raise ValueError(f"{what} must be integers, got {i!r}")
    if not -n <= i < n:
        raise ValueError(f"{what} {i} is outside a dimension of {n}")
    return int(i) % n


def _axis(sel, n, what):
    """(origin, step, count) of a slice or an int along a dimension of n."""
    if isinstance(sel, (int, np.integer)) and not isinstance(sel, bool):
        return _index(sel, n, what), 1, 1
    if not isinstance(sel, slice):
        raise ValueError(f"{what} must be a slice or an int, got {sel!r}")
    if sel.step is not None and sel.step < 1:
        raise ValueError(f"{what} needs a step >= 1, got {sel.step}")
    start, stop, step = sel.indices(n)
    count = len(range(start, stop, step))
    if count < 1:
        raise ValueError(f"{what} {sel} selects nothing of a dimension of {n}")
    return start, step, count


class Resolved:
    """A ``Selection`` against one (B, C, H, W) shape: ``channels`` (the list), ``window``
    (lat0, lat_step, nlat_out, lon0, lon_step, nlon_out), ``out_shape`` (B, C_out, H_out,
    W_out), ``slabs`` (the source slab b * C + c of every output slab, or None for all in
    order) and ``whole`` (the window is the whole grid)."""

    def __init__(self, shape, channels, window):
        B, C, H, W = shape
        self.shape = tuple(int(v) for v in shape)
        self.channels = channels
        self.window = window
        self.out_shape = (B, len(channels), window[2], window[5])
        self.whole = window == (0, 1, H, 0, 1, W)
        identity = channels == list(range(C))
        self.slabs = None if identity else [b * C + c for b in range(B) for c in channels]
        self._dev = {}

    def slab_tensor(self, device):
        """The int32 slab list on ``device`` (uploaded once per device), or None."""
        if self.slabs is None:
            return None
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = torch.tensor(self.slabs, dtype=torch.int32, device=device)
        return self._dev[key]

    def c_window(self):
        return None if self.whole else N.Window(*self.window)

    def index(self, x):
        """The selected values of ``x`` (B, C, H, W) by torch indexing."""
        la0, las, nla, lo0, los, nlo = self.window
        if self.slabs is not None:
            x = x.index_select(1, torch.as_tensor(self.channels, device=x.device))
        return x[:, :, la0:la0 + (nla - 1) * las + 1:las, lo0:lo0 + (nlo - 1) * los + 1:los]


class Selection:
    """What of a (B, C, H, W) field is exported: ``channels`` (None for all, a slice, or a
    sequence of channel indices in any order, repeats allowed), and ``lat`` / ``lon`` (a slice
    with a step >= 1, or one index).  ``Selection(lat=slice(None, None, 6), lon=slice(None,
    None, 6))`` takes the 0.25 degree field at the nodes of the 1.5 degree grid: a point
    sample; the cell mean is ``regrid.Regridder`` (``Rollout.export(regrid=)``).  ``resolve(shape)``
    raises ``ValueError`` for a selection that is empty or leaves the field."""

    def __init__(self, channels=None, lat=slice(None), lon=slice(None)):
        self.channels, self.lat, self.lon = channels, lat, lon
        self._resolved = {}

    def resolve(self, shape) -> Resolved:
        shape = tuple(int(v) for v in shape)
        if len(shape) != 4 or min(shape) < 1:
            raise ValueError(f"a selection applies to a (B, C, H, W) shape, got {shape}")
        if shape not in self._resolved:
            B, C, H, W = shape
            ch = self.channels
            if ch is None:
                ch = list(range(C))
            elif isinstance(ch, slice):
                ch = list(range(C))[ch]
            else:
                try:
                    ch = [_index(c, C, "channel") for c in ch]
                except TypeError:
                    raise ValueError(f"channels must be None, a slice or a sequence of "
                                     f"indices, got {self.channels!r}") from None
            if not ch:
                raise ValueError("the selection has no channel")
            la = _axis(self.lat, H, "lat")
            lo = _axis(self.lon, W, "lon")
            self._resolved[shape] = Resolved(shape, ch, (la[0], la[1], la[2], lo[0], lo[1],
                                                         lo[2]))
        return self._resolved[shape]

    def describe(self):
        """JSON-able form (``NpyArchive`` keeps it in meta.json)."""
        def ax(s):
            return [s.start, s.stop, s.step] if isinstance(s, slice) else int(s)
        ch = self.channels
        return {"channels": None if ch is None else ax(ch) if isinstance(ch, slice)
                else [int(c) for c in ch], "lat": ax(self.lat), "lon": ax(self.lon)}

    def __repr__(self):
        return f"Selection(channels={self.channels!r}, lat={self.lat!r}, lon={self.lon!r})"


def decode_numpy(q, ref, exp2):
    """The decode on the host, in fp32 as on the device: ``ref + float32(q) * 2^exp2`` with
    ``ref`` and ``exp2`` of shape ``q.shape[:-2]``."""
    q = np.asarray(q)
    if q.dtype == np.int16:
        q = q.view(np.uint16)
    ref = np.asarray(ref, dtype=np.float32)[..., None, None]
    e = np.asarray(exp2, dtype=np.int32)[..., None, None]
    return (ref + np.ldexp(q.astype(np.float32), e).astype(np.float32)).astype(np.float32)


def _host(t):
    """A tensor as a numpy array on the host (int16 storage of q as the uint16 it holds)."""
    if not isinstance(t, torch.Tensor):
        return t
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


class Packed:
    """One packed field set: ``q`` (B, C_out, H_out, W_out) 16-bit, ``ref`` (B, C_out) fp32,
    ``exp2`` (B, C_out) int32, ``shape`` (that of ``q``) and the ``selection`` it was made
    with.  Device tensors from ``pack``, numpy arrays where a sink receives it.  With the
    writer's ``encoding="f32"`` only ``values`` (fp32) is set."""

    def __init__(self, q, ref, exp2, shape, selection=None, values=None):
        self.q, self.ref, self.exp2 = q, ref, exp2
        self.shape = tuple(shape)
        self.selection = selection
        self.values = values

    def numpy(self):
        """The decoded fields as a numpy fp32 array (copies device tensors to the host)."""
        if self.values is not None:
            return np.array(_host(self.values), dtype=np.float32)
        return decode_numpy(_host(self.q), _host(self.ref), _host(self.exp2))

    def copy(self):
        """A host copy that outlives the buffers this one views."""
        c = lambda a: None if a is None else np.array(_host(a))
        return Packed(c(self.q), c(self.ref), c(self.exp2), self.shape, self.selection,
                      c(self.values))


def _field(x, name="x"):
    if x.dim() != 4:
        raise ValueError(f"{name} must be (B, C, H, W), got {tuple(x.shape)}")
    if x.requires_grad:
        raise ValueError(f"{name} requires grad: packing has no gradient; pass "
                         f"{name}.detach()")
    x = N.require_device_f32(x, name)
    if x.numel() == 0:
        raise ValueError("empty fields")
    return x


def workspace(out_shape, device):
    """A workspace for ``pack`` into this output shape (contents do not matter)."""
    B, C, H, W = out_shape
    return torch.empty(N.lib().msfno_pack16_workspace_size(B * C, H, W), dtype=torch.uint8,
                       device=device)


def empty_packed(out_shape, device, selection=None):
    B, C, H, W = out_shape
    return Packed(torch.empty(B, C, H, W, dtype=Q_DTYPE, device=device),
                  torch.empty(B, C, dtype=torch.float32, device=device),
                  torch.empty(B, C, dtype=torch.int32, device=device), out_shape, selection)


@N.on_input_device
def pack(x, selection=None, out=None, ws=None):
    """``Packed`` of the fields ``x`` (B, C, H, W) fp32 on the device, or of the part that
    ``selection`` names; the range of a field is that of its selected points.  ``out`` is a
    ``Packed`` of the output shape to write into (``empty_packed``), ``ws`` a ``workspace``;
    both are made if absent.  With both given, and after the first call with a selection (its
    slab list is uploaded once), the call neither allocates nor synchronises and records into
    a graph.  Deterministic.  No gradient."""
    x = _field(x)
    B, C, H, W = x.shape
    r = (selection or _WHOLE).resolve(x.shape)
    So = r.out_shape[0] * r.out_shape[1]
    if out is None:
        out = empty_packed(r.out_shape, x.device, selection)
    elif tuple(out.q.shape) != r.out_shape or not out.q.is_contiguous():
        raise ValueError(f"out.q must be contiguous {r.out_shape}, got {tuple(out.q.shape)}")
    if ws is None:
        ws = workspace(r.out_shape, x.device)
    slab = r.slab_tensor(x.device)
    win = r.c_window()
    N.check(N.lib().msfno_pack16(
        x.data_ptr(), B * C, H, W, N.ptr(slab), So, None if win is None else ctypes.byref(win),
        out.ref.data_ptr(), out.exp2.data_ptr(), out.q.data_ptr(), ws.data_ptr(), ws.numel(),
        N.stream_of(x.device)), "msfno_pack16")
    return out


_WHOLE = Selection()


def unpack(packed, out=None):
    """The decoded fields (B, C_out, H_out, W_out) fp32 on the device (``msfno_unpack16``);
    ``out`` is a contiguous fp32 tensor of that shape to write into."""
    q = packed.q
    if not isinstance(q, torch.Tensor) or not q.is_cuda:
        raise ValueError("unpack takes a Packed of GPU (HIP) tensors; libmsfno has no CPU "
                         "path (decode_numpy is the host form)")
    B, C, H, W = q.shape
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != tuple(q.shape) or out.dtype != torch.float32 or \
            not out.is_contiguous() or out.device != q.device:
        raise ValueError(f"out must be contiguous fp32 {tuple(q.shape)} on {q.device}")
    q = q.contiguous()
    with torch.cuda.device(q.device):    # the kernel goes to the stream of q's device
        N.check(N.lib().msfno_unpack16(q.data_ptr(), packed.ref.data_ptr(),
                                       packed.exp2.data_ptr(), out.data_ptr(), H * W, B * C,
                                       N.stream_of(q.device)), "msfno_unpack16")
    return out


class _Slot:
    pass


class ForecastWriter:
    """A ring of ``depth`` staging slots between a rollout and a sink.

    ``shape`` is the (B, C, H, W) of the fields that ``put`` receives, ``selection`` what of
    them is exported, ``encoding`` ``"u16"`` (``pack``) or ``"f32"`` (the selected values
    themselves, by torch indexing).  A slot is one device buffer and one pinned host buffer
    that hold header (``ref``, ``exp2``) and payload contiguously, so a step is one
    device-to-host copy; the writer owns one copy stream and one event pair per slot.

    ``put(step, y)`` packs on the current stream into the next slot, lets the copy stream wait
    for that, copies without blocking and records the slot's done event; before a slot is
    packed into again the current stream waits (on the device) for its done event.  Then
    every finished slot is handed to ``sink(step, host_packed)`` in step order.  ``y`` may be
    overwritten as soon as ``put`` returns.  The host blocks only when the ring is full (on
    the oldest slot) and in ``flush()`` / ``__exit__``, which deliver what is left, in order.

    The arrays a sink receives (``host_packed.q``, ``.ref``, ``.exp2`` or ``.values``) are
    views of pinned memory that the ring reuses: they are valid only during the call.  Copy
    what is to be kept (``host_packed.copy()``)."""

    def __init__(self, shape, selection=None, encoding="u16", depth=2, sink=None, device=None):
        if encoding not in ("u16", "f32"):
            raise ValueError(f"encoding must be 'u16' or 'f32', got {encoding!r}")
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.selection = selection
        self.resolved = (selection or _WHOLE).resolve(shape)
        self.encoding = encoding
        self.sink = sink if sink is not None else MemorySink()
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise ValueError("ForecastWriter stages on a GPU (HIP) device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        B, C, H, W = self.resolved.out_shape
        S, n = B * C, B * C * H * W
        # header: ref (S fp32), exp2 (S int32), padded to the 16-byte grid; then the payload
        self._head = 0 if encoding == "f32" else (8 * S + 15) // 16 * 16
        nbytes = self._head + n * (4 if encoding == "f32" else 2)
        self.copy_stream = torch.cuda.Stream(self.device)
        self._slots = []
        for _ in range(depth):
            s = _Slot()
            s.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            s.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            s.ready = torch.cuda.Event()
            s.done = torch.cuda.Event()
            s.used = False
            s.step = None
            hv = s.host.numpy()
            if encoding == "u16":
                s.packed = Packed(s.dev[self._head:].view(Q_DTYPE).view(B, C, H, W),
                                  s.dev[:4 * S].view(torch.float32).view(B, C),
                                  s.dev[4 * S:8 * S].view(torch.int32).view(B, C),
                                  self.resolved.out_shape, selection)
                s.ws = workspace(self.resolved.out_shape, self.device)
                s.view = Packed(hv[self._head:].view(np.uint16).reshape(B, C, H, W),
                                hv[:4 * S].view(np.float32).reshape(B, C),
                                hv[4 * S:8 * S].view(np.int32).reshape(B, C),
                                self.resolved.out_shape, selection)
            else:
                s.values = s.dev.view(torch.float32).view(B, C, H, W)
                s.view = Packed(None, None, None, self.resolved.out_shape, selection,
                                values=hv.view(np.float32).reshape(B, C, H, W))
            self._slots.append(s)
        self.resolved.slab_tensor(self.device)  # uploaded here, not in the first put
        self._chan = None
        if encoding == "f32" and self.resolved.slabs is not None:
            self._chan = torch.tensor(self.resolved.channels, device=self.device)
        self._head_i = 0   # the oldest slot in flight
        self._count = 0    # slots in flight
        self.puts = 0

    def _deliver(self, block):
        """Hand finished slots to the sink, oldest first; with ``block`` wait for the oldest."""
        while self._count:
            s = self._slots[self._head_i]
            if block:
                s.done.synchronize()
                block = False
            elif not s.done.query():
                return
            self._head_i = (self._head_i + 1) % len(self._slots)
            self._count -= 1
            self.sink(s.step, s.view)

    @torch.no_grad()
    def put(self, step, y):
        if tuple(y.shape) != self.resolved.shape:
            raise ValueError(f"the writer was made for {self.resolved.shape}, got "
                             f"{tuple(y.shape)}")
        y = _field(y, "y")
        if y.device != self.device:
            raise ValueError(f"the writer stages on {self.device}, y is on {y.device}")
        if self._count == len(self._slots):
            self._deliver(block=True)      # the ring is full: wait for the oldest slot
        s = self._slots[(self._head_i + self._count) % len(self._slots)]
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if s.used:
                cur.wait_event(s.done)     # the slot's last copy has read the device buffer
            if self.encoding == "u16":
                pack(y, self.selection, out=s.packed, ws=s.ws)
            else:
                r = self.resolved
                la0, las, nla, lo0, los, nlo = r.window
                src = y if self._chan is None else y.index_select(1, self._chan)
                s.values.copy_(src[:, :, la0:la0 + (nla - 1) * las + 1:las,
                                   lo0:lo0 + (nlo - 1) * los + 1:los])
            s.ready.record(cur)
            self.copy_stream.wait_event(s.ready)
            with torch.cuda.stream(self.copy_stream):
                s.host.copy_(s.dev, non_blocking=True)
                s.done.record(self.copy_stream)
        s.used = True
        s.step = step
        self._count += 1
        self.puts += 1
        self._deliver(block=False)

    def flush(self):
        """Deliver every slot in flight, in order (blocks until their copies are done)."""
        while self._count:
            self._deliver(block=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.flush()
        return False


class MemorySink:
    """Keeps a host copy of everything delivered: ``steps`` and ``items`` (``Packed`` of numpy
    arrays), in delivery order."""

    def __init__(self):
        self.steps, self.items = [], []

    def __call__(self, step, host_packed):
        self.steps.append(step)
        self.items.append(host_packed.copy())


class NpyArchive:
    """A sink that writes a directory of plain numpy files: ``q.npy``, a
    ``numpy.lib.format.open_memmap`` of (n_steps, S, H_out, W_out) uint16 with S = B * C_out,
    ``ref.npy`` (n_steps, S) fp32, ``exp2.npy`` (n_steps, S) int32 and ``meta.json`` (the steps
    written, in order; the selection; the source and output shapes).  The k-th delivery goes
    to row k.  The files are created by the first delivery; ``close()`` (or leaving the
    ``with`` block) flushes them.  ``source_shape`` and ``selection`` are recorded as given."""

    def __init__(self, path, n_steps, source_shape=None, selection=None):
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        self.path, self.n_steps = path, int(n_steps)
        self.source_shape, self.selection = source_shape, selection
        self.steps = []
        self._q = self._ref = self._exp2 = None
        os.makedirs(path, exist_ok=True)

    def _open(self, shape):
        B, C, H, W = shape
        mm = np.lib.format.open_memmap
        self._shape = tuple(int(v) for v in shape)
        self._q = mm(os.path.join(self.path, "q.npy"), mode="w+", dtype=np.uint16,
                     shape=(self.n_steps, B * C, H, W))
        self._ref = mm(os.path.join(self.path, "ref.npy"), mode="w+", dtype=np.float32,
                       shape=(self.n_steps, B * C))
        self._exp2 = mm(os.path.join(self.path, "exp2.npy"), mode="w+", dtype=np.int32,
                        shape=(self.n_steps, B * C))

    def _meta(self):
        sel = self.selection
        meta = {"steps": [int(s) for s in self.steps], "n_steps": self.n_steps,
                "out_shape": list(self._shape),
                "source_shape": None if self.source_shape is None else
                [int(v) for v in self.source_shape],
                "selection": None if sel is None else sel.describe(), "encoding": "u16"}
        with open(os.path.join(self.path, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1)

    def __call__(self, step, host_packed):
        if host_packed.q is None:
            raise ValueError("NpyArchive stores the 16-bit encoding; the writer was made "
                             "with encoding='f32'")
        if self._q is None:
            self._open(host_packed.shape)
            if self.selection is None:
                self.selection = host_packed.selection
        k = len(self.steps)
        if k >= self.n_steps:
            raise ValueError(f"the archive holds {self.n_steps} steps")
        if tuple(host_packed.shape) != self._shape:
            raise ValueError(f"the archive holds {self._shape}, got {host_packed.shape}")
        S = self._shape[0] * self._shape[1]
        self._q[k] = np.asarray(_host(host_packed.q)).reshape(S, *self._shape[2:])
        self._ref[k] = np.asarray(_host(host_packed.ref)).reshape(S)
        self._exp2[k] = np.asarray(_host(host_packed.exp2)).reshape(S)
        self.steps.append(step)
        self._meta()

    def close(self):
        for m in (self._q, self._ref, self._exp2):
            if m is not None:
                m.flush()
        if self._q is not None:
            self._meta()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Archive:
    """An ``NpyArchive`` directory opened for reading: ``steps`` (the step numbers written),
    ``out_shape``, ``meta``; ``decode(k)`` is the k-th written step on the host,
    ``packed(k)`` its ``Packed`` of numpy views, ``truths(device)`` the replay on a device."""

    def __init__(self, path):
        with open(os.path.join(path, "meta.json")) as f:
            self.meta = json.load(f)
        self.steps = list(self.meta["steps"])
        self.out_shape = tuple(self.meta["out_shape"])
        self.q = np.load(os.path.join(path, "q.npy"), mmap_mode="r")
        self.ref = np.load(os.path.join(path, "ref.npy"), mmap_mode="r")
        self.exp2 = np.load(os.path.join(path, "exp2.npy"), mmap_mode="r")

    def __len__(self):
        return len(self.steps)

    def packed(self, k):
        if not 0 <= k < len(self.steps):
            raise IndexError(f"the archive holds {len(self.steps)} steps, asked for {k}")
        B, C, H, W = self.out_shape
        return Packed(self.q[k].reshape(B, C, H, W), self.ref[k].reshape(B, C),
                      self.exp2[k].reshape(B, C), self.out_shape)

    def decode(self, k):
        """(B, C_out, H_out, W_out) fp32 on the host."""
        return self.packed(k).numpy()

    def truths(self, device):
        """An iterator over the written steps as decoded fp32 device tensors (B, C_out,
        H_out, W_out): the 16-bit payload is uploaded and decoded by ``msfno_unpack16``, half
        the host-to-device bytes of the fields.  What ``Rollout.verify`` takes as
        ``truths``."""
        for k in range(len(self.steps)):
            p = self.packed(k)
            q = torch.from_numpy(np.array(p.q).view(np.int16)).to(device)   # a writable copy
            dev = Packed(q.view(Q_DTYPE) if Q_DTYPE != torch.int16 else q,
                         torch.from_numpy(np.array(p.ref, dtype=np.float32)).to(device),
                         torch.from_numpy(np.array(p.exp2, dtype=np.int32)).to(device),
                         self.out_shape)
            yield unpack(dev)


def open_archive(path) -> Archive:
    return Archive(path)
