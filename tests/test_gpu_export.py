"""Forecast export on the GPU (csrc/pack.hip through the C-ABI, msfno_amd/export.py and
Rollout.export) against the numpy fp32 restatement of the encoding (tests/export_util.py),
compared with ==.  ref is pre-filled with NaN, exp2 with a sentinel, q with 0xFFFF, y with NaN
and every workspace with NaN; one case runs behind a guarded workspace
(tests/workspace_guard.py).

Shapes (S, H, W), whole window: a single element, a row shorter than one 16-byte store, an odd
slab (the phase of the fp32 and of the 16-bit rows moves from row to row), nlon % 8 != 0, a
row wider than one sweep, more rows than one unit holds, more units than the grid cap, one
real row length and one real 721 x 1440 slab pair; each at base pointers 0..3 floats past the
16-byte grid.  Windows on (3, 121, 250) and (2, 7, 9) with a value below the window's minimum
and one above its maximum outside the window of every slab, the window's minimum in its first
element and its maximum in its last, so a range taken over the whole slab, or one that leaves
out the first or the last element, gives another ref or exp2.

Tolerances.  ref, exp2, q, the decode and everything the writer and the rollout driver deliver:
bit for bit.  The round trip: |unpack(pack(x)) - x| <= 2^(E-1) + ulp32(d)/2 +
ulp32(max |xhat|)/2 per slab, in fp64: the rounding of q (half a step of 2^E), of x - R (a
value of at most d) and of the decode's one add; the products with 2^-E and 2^E are exact.
Measured worst ratio to it: 0.886 (300 + N(0, 1)) and 0.996 (N(0, 1) 1e-3); the RMSE test
uses 0.02 of its tolerance.  The RMSE of a
rollout against truths replayed from an archive is within max over the slab of that bound
(the triangle inequality: RMSE is a weighted 2-norm over the points divided by its weight, and
every point of the truth moved by at most the bound) plus 1e-5 of the RMSE (the bound of
tests/test_gpu_verify.py on the kernel's se against fp64, 1e-5 relative, halved by the root,
for each of the two sides).

What the tests catch (edits of csrc/pack.hip on scratch builds, none of which can index out of
bounds; the failing tests of this file in brackets):
  - the range taken over the whole source slab instead of the window (the range pass sweeps
    all rows and columns of the slab): 6 tests [test_windows at both shapes,
    test_pack_captures_in_a_graph_and_does_not_synchronise,
    test_writer_delivers_in_order_what_a_synchronous_pack_gives and
    test_rollout_export_on_the_fixture_network in both modes: every test that packs a window];
  - truncation in place of rint: 19 tests [test_whole_window_shapes at every shape but
    (1, 1, 1), test_windows, test_edges_of_the_encoding, both round trips (the error leaves
    the bound), the two-calls test, the graph, the writer and both rollout tests];
  - E one too small at the 65535 2^k edge (the mantissa of d compared with <= 0x7fff01, so
    that nextafter(65535 2^k) still takes E = k): 1 test [test_edges_of_the_encoding; no
    random slab has its range on that one mantissa];
  - the elements after the aligned part of a row left out of the range pass: 6 tests
    [test_whole_window_shapes at (1, 1, 1), (6, 5, 12) and (2100, 1, 4), where an extreme of
    a slab falls into a tail; test_windows at both shapes, whose maximum sits in the window's
    last element; the graph test].
"""
import functools

import numpy as np
import pytest
import torch

import export_util as XU
from workspace_guard import guard_intact, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345

SHAPES = [(1, 1, 1), (1, 2, 8), (2, 7, 9), (6, 5, 12), (3, 121, 250), (1, 3, 4100),
          (2, 130, 12), (2100, 1, 4), (1, 3, 1440), (2, 721, 1440)]


def _u16(t):
    """A 16-bit device or host tensor as a numpy uint16 array."""
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _q_buffer(*shape):
    return torch.full(shape, -1, dtype=torch.int16, device=DEV)          # 0xFFFF


def _pack(xd, S_in, H, W, slab=None, win=None, ws=None):
    """msfno_pack16 on device pointers into pre-filled outputs and a NaN-filled workspace;
    (ref, exp2, q) as numpy arrays."""
    import ctypes
    from msfno_amd import _native as N
    lib = N.lib()
    S_out = S_in if slab is None else len(slab)
    Ho, Wo = (H, W) if win is None else (win[2], win[5])
    nbytes = lib.msfno_pack16_workspace_size(S_out, Ho, Wo)
    assert nbytes > 0 and nbytes % 4 == 0
    if ws is None:
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ref = torch.full((S_out,), float("nan"), dtype=torch.float32, device=DEV)
    exp2 = torch.full((S_out,), SENTINEL, dtype=torch.int32, device=DEV)
    q = _q_buffer(S_out + 1, Ho, Wo)                     # one slab more: stays 0xFFFF
    sl = None if slab is None else torch.tensor(slab, dtype=torch.int32, device=DEV)
    w = None if win is None else ctypes.byref(N.Window(*win))
    N.check(lib.msfno_pack16(xd.data_ptr(), S_in, H, W, N.ptr(sl), S_out, w, ref.data_ptr(),
                             exp2.data_ptr(), q.data_ptr(), ws.data_ptr(), nbytes,
                             N.stream_of(xd.device)), "msfno_pack16")
    qh = _u16(q)
    assert (qh[S_out] == 0xFFFF).all(), "written past q"
    return ref.cpu().numpy(), exp2.cpu().numpy(), qh[:S_out]


def _at_offset(x, k):
    """A device copy of the numpy array x that starts k floats past a 16-byte boundary."""
    buf = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + x.size].view(x.shape)
    v.copy_(torch.from_numpy(x))
    return v


def _same(tag, got, want):
    for name, g, w in zip(("ref", "exp2", "q"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (tag, name)


@functools.lru_cache(maxsize=None)
def _problem(shape):
    x = XU.slabs(shape, seed=sum(shape))
    return x, XU.encode(x)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_whole_window_shapes(shape):
    x, want = _problem(shape)
    S, H, W = shape
    for k in ((0, 1, 2, 3) if shape != (2, 721, 1440) else (0, 3)):
        _same(f"{shape} offset {k}", _pack(_at_offset(x, k), S, H, W), want)


def _windowed(shape, seed):
    """Slabs whose window carries its minimum in its first element and its maximum in its
    last; set by the caller per window."""
    g = np.random.default_rng(seed)
    return (300 + np.clip(g.standard_normal(shape), -3, 3)).astype(np.float32)


def _mark(x, win):
    """Put 290 / 310 into the first / last element of the window of every slab and 200 / 400
    at two points outside it."""
    S, H, W = x.shape
    la0, las, nla, lo0, los, nlo = win
    inside = np.zeros((H, W), bool)
    inside[la0:la0 + (nla - 1) * las + 1:las, lo0:lo0 + (nlo - 1) * los + 1:los] = True
    out = np.argwhere(~inside)
    assert len(out) >= 2
    x = x.copy()
    x[:, la0, lo0] = 290.0
    x[:, la0 + (nla - 1) * las, lo0 + (nlo - 1) * los] = 310.0
    x[:, out[0][0], out[0][1]] = 200.0
    x[:, out[-1][0], out[-1][1]] = 400.0
    return x


def _windows(H, W):
    return {
        "stride to the last admissible point": (1, 2, (H - 2) // 2 + 1, 3, 6, (W - 4) // 6 + 1),
        "a single point": (H // 2, 1, 1, W // 3, 1, 1),
        "the last row": (H - 1, 1, 1, 0, 1, W),
        "the last column": (0, 1, H, W - 1, 1, 1),
        "the last point": (H - 1, 1, 1, W - 1, 1, 1),
        "odd lon0, lon_step 1": (0, 1, H - 1, 1, 1, W - 2),
        "odd lon0 to the end": (2, 3, (H - 3) // 3 + 1, 3, 1, W - 3),
    }


@pytest.mark.parametrize("shape", [(3, 121, 250), (2, 7, 9)], ids=str)
def test_windows(shape):
    S, H, W = shape
    base = _windowed(shape, seed=5)
    for name, win in _windows(H, W).items():
        la0, las, nla, lo0, los, nlo = win
        assert la0 + (nla - 1) * las < H and lo0 + (nlo - 1) * los < W
        x = _mark(base, win)
        want = XU.pack(x, None, win)
        assert (want[0] == (290.0 if nla * nlo > 1 else 310.0)).all()
        if nla * nlo > 1:
            assert (want[1] == XU.exponent(np.float32(20.0))).all()
            assert (want[1] < XU.encode(x)[1]).all()               # the whole slab's E is larger
        for k in (0, 1):
            _same(f"{shape} {name} offset {k}", _pack(_at_offset(x, k), S, H, W, None, win), want)
    # a slab list with a repeat and a permutation, with and without a window
    slab = [S - 1, 0, S - 1, 1, 0]
    win = _windows(H, W)["stride to the last admissible point"]
    x = _mark(base, win) + np.arange(S, dtype=np.float32)[:, None, None]   # slabs differ
    for w in (win, None):
        want = XU.pack(x, slab, w)
        assert not np.array_equal(want[2][0], want[2][1])
        _same(f"{shape} slab list, window {w}", _pack(_at_offset(x, 2), S, H, W, slab, w), want)


def test_edges_of_the_encoding():
    for name, x, E_want, qmax_want in XU.edge_slabs():
        want = XU.encode(x)
        if E_want is not None:
            assert want[1][0] == E_want, name
        if qmax_want is not None:
            assert want[2].max() == qmax_want, name
        got = _pack(_at_offset(x, 0), 1, x.shape[1], x.shape[2])
        _same(name, got, want)
        if name == "constant":
            assert got[1][0] == 0 and not got[2].any()
        if name == "ties":
            assert got[2][0, 0].tolist() == [0, 0, 2, 2] and got[2][0, 1, 0] == 65534


def _unpack(q, ref, exp2, k=0):
    """msfno_unpack16 of numpy arrays into a NaN-filled y that starts k floats past the
    16-byte grid; numpy."""
    from msfno_amd import _native as N
    S, n = q.shape[0], q[0].size
    qd = torch.from_numpy(q.view(np.int16)).to(DEV)
    buf = torch.full((q.size + 8,), float("nan"), dtype=torch.float32, device=DEV)
    y = buf[k:k + q.size]
    rd, ed = torch.from_numpy(ref).to(DEV), torch.from_numpy(exp2).to(DEV)
    N.check(N.lib().msfno_unpack16(qd.data_ptr(), rd.data_ptr(), ed.data_ptr(), y.data_ptr(), n,
                                   S, N.stream_of(qd.device)), "msfno_unpack16")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:k]).all() and torch.isnan(buf[k + q.size:]).all()
    return y.view(q.shape).cpu().numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 9), (3, 121, 250), (1, 3, 4100),
                                   (2100, 1, 4), (2, 1, 4099)], ids=str)
def test_unpack_equals_decode_numpy(shape):
    from msfno_amd import export as X
    g = np.random.default_rng(4)
    q = g.integers(0, 65536, shape).astype(np.uint16)
    q.reshape(-1)[:2] = (0, 65535)[:q.size]
    ref = (300 * g.standard_normal(shape[0])).astype(np.float32)
    exp2 = g.integers(-30, 20, shape[0]).astype(np.int32)
    exp2[0] = -126
    want = X.decode_numpy(q, ref, exp2)
    assert np.array_equal(want, XU.decode(q, ref, exp2))
    for k in (0, 1, 2, 3):
        assert np.array_equal(_unpack(q, ref, exp2, k), want), (shape, k)


@pytest.mark.parametrize("kind", ["field", "small"])
def test_round_trip_is_within_the_derived_bound(kind):
    from msfno_amd import export as X
    shape = (3, 121, 250)
    x = XU.slabs(shape, seed=9, kind=kind)
    xd = torch.from_numpy(x).to(DEV).view(1, *shape)
    p = X.pack(xd)
    back = X.unpack(p).cpu().numpy()[0]
    ref, exp2 = p.ref.cpu().numpy()[0], p.exp2.cpu().numpy()[0]
    assert np.array_equal(back, p.numpy()[0])                       # device and host decode
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    b = XU.bound(x, ref, exp2, back)
    print(f"round trip {kind}: worst error / bound {(err / b).max():.3f}, E = {exp2.tolist()}")
    assert (err <= b).all()


def test_two_calls_are_bit_identical_and_nothing_is_written_past_the_workspace():
    from msfno_amd import _native as N
    shape = (3, 121, 250)
    x, want = _problem(shape)
    xd = _at_offset(x, 1)
    nbytes = N.lib().msfno_pack16_workspace_size(*shape)
    ws = guarded(nbytes, 0xFF)                                       # NaN words
    a = _pack(xd, *shape, ws=ws)
    guard_intact(ws, nbytes)
    ws2 = guarded(nbytes, 0x7B)                                      # 3e36 in every word
    b = _pack(xd, *shape, ws=ws2)
    guard_intact(ws2, nbytes)
    _same("first", a, want)
    _same("second", b, a)


def test_pack_captures_in_a_graph_and_does_not_synchronise():
    from msfno_amd import export as X
    B, C, H, W = 2, 3, 7, 9
    sel = X.Selection(channels=[2, 0], lat=slice(1, None, 2))
    x1, x2 = XU.slabs((B * C, H, W), seed=1), XU.slabs((B * C, H, W), seed=2, kind="small")
    xd = torch.from_numpy(x1).to(DEV).view(B, C, H, W)
    r = sel.resolve(xd.shape)
    out = X.empty_packed(r.out_shape, DEV, sel)
    ws = X.workspace(r.out_shape, DEV)
    X.pack(xd, sel, out=out, ws=ws)                 # the slab list is uploaded here, once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        X.pack(xd, sel, out=out, ws=ws)
    xd.copy_(torch.from_numpy(x2).view(B, C, H, W))
    out.ref.fill_(float("nan"))
    out.exp2.fill_(SENTINEL)
    out.q.view(torch.int16).fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    want = XU.pack(x2, r.slabs, r.window)
    _same("replay", (out.ref.cpu().numpy().ravel(), out.exp2.cpu().numpy().ravel(),
                     _u16(out.q).reshape(want[2].shape)), want)
    torch.cuda.set_sync_debug_mode("error")
    try:
        X.pack(xd, sel, out=out, ws=ws)
        X.unpack(out, out=torch.empty(r.out_shape, device=DEV))
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _host_tuple(p):
    S = p.shape[0] * p.shape[1]
    return (np.asarray(p.ref).reshape(S), np.asarray(p.exp2).reshape(S),
            np.asarray(p.q).reshape(S, *p.shape[2:]))


def test_writer_delivers_in_order_what_a_synchronous_pack_gives():
    from msfno_amd import export as X
    B, C, H, W = 2, 3, 31, 50
    sel = X.Selection(channels=[1, 2, 0, 1], lat=slice(1, None, 3), lon=slice(1, None))
    fields = [XU.slabs((B * C, H, W), seed=20 + i, kind="field" if i % 2 else "small")
              for i in range(5)]
    sink = X.MemorySink()
    wr = X.ForecastWriter((B, C, H, W), selection=sel, depth=2, sink=sink, device=DEV)
    y = torch.empty(B, C, H, W, device=DEV)
    pinned = [torch.from_numpy(f).view(B, C, H, W).pin_memory() for f in fields]
    torch.cuda.synchronize()
    for i, f in enumerate(pinned):
        y.copy_(f, non_blocking=True)
        if i < 2:                                   # a slot is free: put does not synchronise
            torch.cuda.set_sync_debug_mode("error")
        try:
            wr.put(10 + i, y)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        y.fill_(float("nan"))                       # the input is overwritten right after put
    assert sink.steps == sorted(sink.steps) and len(sink.steps) >= 3   # the ring was full thrice
    wr.flush()
    assert sink.steps == [10, 11, 12, 13, 14] and wr.puts == 5
    r = sel.resolve((B, C, H, W))
    for f, item in zip(fields, sink.items):
        assert item.shape == r.out_shape == (B, 4, 10, 49)
        assert item.q.dtype == np.uint16 and item.q.shape == r.out_shape
        _same("writer", _host_tuple(item), XU.pack(f, r.slabs, r.window))
        sync = X.pack(torch.from_numpy(f).to(DEV).view(B, C, H, W), sel)
        _same("synchronous pack", _host_tuple(sync.copy()), _host_tuple(item))
    with X.ForecastWriter((B, C, H, W), depth=3, sink=X.MemorySink(), device=DEV) as w2:
        w2.put(0, torch.from_numpy(fields[0]).to(DEV).view(B, C, H, W))
        assert w2.sink.steps in ([], [0])
    assert w2.sink.steps == [0]                     # __exit__ flushes
    _same("whole", _host_tuple(w2.sink.items[0]), XU.encode(fields[0]))
    with pytest.raises(ValueError, match="made for"):
        wr.put(0, y[:1])


def test_writer_f32_returns_the_selected_values_exactly():
    from msfno_amd import export as X
    B, C, H, W = 1, 4, 13, 22
    sel = X.Selection(channels=[3, 1], lat=slice(None, None, 6), lon=slice(2, None, 6))
    r = sel.resolve((B, C, H, W))
    fields = [XU.slabs((B * C, H, W), seed=40 + i) for i in range(3)]
    for s, depth in ((sel, 2), (None, 1)):
        wr = X.ForecastWriter((B, C, H, W), selection=s, encoding="f32", depth=depth, device=DEV)
        for i, f in enumerate(fields):
            wr.put(i, torch.from_numpy(f).to(DEV).view(B, C, H, W))
        wr.flush()
        assert wr.sink.steps == [0, 1, 2]
        for f, item in zip(fields, wr.sink.items):
            want = XU.select(f, r.slabs, r.window) if s else f
            assert item.q is None and item.values.dtype == np.float32
            assert np.array_equal(item.numpy().reshape(want.shape), want)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_rollout_export_on_the_fixture_network(graph, tmp_path):
    """3 steps with every = 2: the steps 0 and 2 are delivered, each the restatement of the
    very output of run() that the driver saw (recorded: a second run need not give the same
    bits); then an archive of truths replayed into Rollout.verify."""
    from test_gpu_ensemble import _rollout
    from msfno_amd import export as X
    from msfno_amd import verification as V
    r, x0, stds = _rollout(graph)
    B, C, H, W = x0.shape
    assert r.use_graph == graph
    rec, run = [], r.run

    def recording(*args, **kwargs):
        for i, y in run(*args, **kwargs):
            rec.append(y.clone())
            yield i, y

    r.run = recording
    sel = X.Selection(channels=list(range(C - 1, -1, -2)), lat=slice(1, None, 2),
                      lon=slice(0, None, 3))
    wr = X.ForecastWriter(x0.shape, selection=sel, depth=2, device=DEV)
    assert r.export(x0, 3, wr, every=2) == 2
    wr.flush()                                      # export itself does not flush
    assert wr.sink.steps == [0, 2] and len(rec) == 3
    res = sel.resolve(x0.shape)
    for step, item in zip(wr.sink.steps, wr.sink.items):
        out = rec[step].cpu().numpy().reshape(B * C, H, W)
        _same(f"step {step}", _host_tuple(item), XU.pack(out, res.slabs, res.window))
    # truths = the antipode of the recorded outputs plus a shift, archived in 16 bits
    truths = [(rec[i].flip(2).roll(W // 2, 3) + 0.25 * (k + 1) * stds).contiguous()
              for k, i in enumerate((0, 2))]
    del rec[:]
    path = str(tmp_path / "truths")
    with X.NpyArchive(path, 2, source_shape=x0.shape) as arc:
        with X.ForecastWriter(x0.shape, depth=1, sink=arc, device=DEV) as tw:
            for k, t in enumerate(truths):
                tw.put(2 * k, t)
    a = X.open_archive(path)
    assert a.steps == [0, 2] and a.out_shape == tuple(x0.shape)
    sc = r.verify(x0, a.truths(DEV), 3, every=2)
    w = torch.ones(H, device=DEV)
    for k, i in enumerate((0, 2)):
        want = V.finish(V.field_sums(rec[i], truths[k], w), w, W).rmse.cpu().double().numpy()
        got = sc.rmse[k].cpu().double().numpy()
        t = truths[k].cpu().numpy().reshape(B * C, H, W)
        ref, exp2, q = XU.encode(t)
        assert np.array_equal(a.decode(k).reshape(t.shape), XU.decode(q, ref, exp2))
        bound = XU.bound(t, ref, exp2, XU.decode(q, ref, exp2)).reshape(B, C)
        print(f"step {i}: rmse difference / bound {(np.abs(got - want) / (bound + 1e-5 * want)).max():.3f}")
        assert (np.abs(got - want) <= bound + 1e-5 * want).all()
        assert (want > 100 * bound).all()           # the comparison is not vacuous

    class Sharded:
        world = 2

    from msfno_amd.rollout import Rollout
    with pytest.raises(NotImplementedError, match="all-reduced"):
        Rollout(Sharded(), graph=False).export(x0, 1, wr)
    with pytest.raises(ValueError, match="steps"):
        r.export(x0, 0, wr)
