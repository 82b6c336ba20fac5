"""Host-side checks of the forecast export (msfno_amd/export.py, csrc/pack.hip through the
C-ABI): the entry points, every refusal before a launch (null and host pointers, never
dereferenced), the workspace size, ``Selection`` resolution, the properties of the numpy
restatement of the encoding (tests/export_util.py) on random and edge slabs, and an
``NpyArchive`` round trip from host arrays.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import export_util as XU
from conftest import REPO

SYMBOLS = ("msfno_pack16_workspace_size", "msfno_pack16", "msfno_unpack16")


def test_entry_points_are_declared_bound_and_exported():
    from msfno_amd import _native as N
    from msfno_amd import export as X
    header = open(os.path.join(REPO, "include", "msfno.h")).read()
    declared = set(re.findall(r"\b(msfno_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in SYMBOLS:
        assert s in declared and s in bound and hasattr(N.lib(), s), s
    assert N.lib().msfno_abi_version() == 6
    assert "typedef struct msfno_window" in header
    assert [f for f, _ in N.Window._fields_] == ["lat0", "lat_step", "nlat_out", "lon0",
                                                 "lon_step", "nlon_out"]
    for name in ("Selection", "pack", "unpack", "Packed", "decode_numpy", "ForecastWriter",
                 "MemorySink", "NpyArchive", "open_archive"):
        assert hasattr(X, name), name
    from msfno_amd.rollout import Rollout
    assert callable(Rollout.export)


def test_c_abi_refusals_come_before_any_launch():
    """Every refusal is decided on the arguments alone: the pointers here are never
    dereferenced (this test runs without a GPU)."""
    from msfno_amd import _native as N
    lib = N.lib()
    S, H, W = 3, 12, 20
    p = 4096                       # any non-null address
    size = lib.msfno_pack16_workspace_size(S, H, W)
    assert size > 0 and size % 4 == 0
    for bad in ((0, H, W), (S, 0, W), (S, H, 0), (-1, H, W)):
        assert lib.msfno_pack16_workspace_size(*bad) == 0
    # non-decreasing in each argument
    for a in ((1, 1, 1), (3, 12, 20), (73, 721, 1440), (2100, 1, 4), (5, 130, 7)):
        for k in range(3):
            prev = lib.msfno_pack16_workspace_size(*a)
            for step in (1, 2, 7, 64, 1000):
                b = list(a)
                b[k] += step
                cur = lib.msfno_pack16_workspace_size(*b)
                assert cur >= prev, (a, b)
                prev = cur

    def pack(x=p, S_in=S, H=H, W=W, slab=None, S_out=S, win=None, ref=p, exp2=p, q=p, ws=p,
             nbytes=None):
        w = None if win is None else ctypes.byref(N.Window(*win))
        if nbytes is None:
            nbytes = 1 << 30
        return lib.msfno_pack16(x, S_in, H, W, slab, S_out, w, ref, exp2, q, ws, nbytes, None)

    for kw in (dict(x=None), dict(ref=None), dict(exp2=None), dict(q=None), dict(ws=None),
               dict(S_in=0), dict(H=0), dict(W=0), dict(S_out=0), dict(S_out=-2),
               dict(S_out=S + 1),                                  # identity needs S_out <= S_in
               dict(win=(0, 0, 2, 0, 1, 2)), dict(win=(0, 1, 2, 0, 0, 2)),   # a step below 1
               dict(win=(0, 1, 0, 0, 1, 2)), dict(win=(0, 1, 2, 0, 1, 0)),   # an extent below 1
               dict(win=(0, -1, 2, 0, 1, 2)), dict(win=(0, 1, -3, 0, 1, 2)),
               dict(win=(-1, 1, 2, 0, 1, 2)), dict(win=(0, 1, 2, -1, 1, 2)),  # a negative origin
               dict(win=(0, 1, H + 1, 0, 1, W)), dict(win=(0, 1, H, 0, 1, W + 1)),
               dict(win=(1, 1, H, 0, 1, W)), dict(win=(0, 1, H, 1, 1, W)),
               dict(win=(1, 2, 7, 0, 1, W)),              # 1 + 6 * 2 = 13 >= 12
               dict(win=(0, 1, H, 3, 6, 4)),              # 3 + 3 * 6 = 21 >= 20
               dict(win=(H, 1, 1, 0, 1, 1)), dict(win=(0, 1, 1, W, 1, 1)),
               dict(win=(0, 2 ** 30, 3, 0, 1, 1))):       # no 32-bit wrap
        assert pack(**kw) == N.MSFNO_EINVAL, kw
    # the last admissible windows pass the checks and fail only on the workspace
    for win in ((1, 2, 6, 3, 6, 3), (H - 1, 1, 1, W - 1, 1, 1), (0, 1, H, 0, 1, W), None):
        need = size if win is None else lib.msfno_pack16_workspace_size(S, win[2], win[5])
        assert pack(win=win, nbytes=need - 1) == N.MSFNO_EWORKSPACE, win
    assert pack(slab=p, S_out=S + 5, nbytes=0) == N.MSFNO_EWORKSPACE   # a list lifts S_out <= S_in
    with pytest.raises(ValueError, match="workspace"):
        N.check(pack(nbytes=0), "msfno_pack16")
    with pytest.raises(ValueError, match="leaves the slab"):
        N.check(pack(win=(0, 1, H + 1, 0, 1, W)), "msfno_pack16")

    def unpack(q=p, ref=p, exp2=p, y=p, n=10, S=S):
        return lib.msfno_unpack16(q, ref, exp2, y, n, S, None)

    for kw in (dict(q=None), dict(ref=None), dict(exp2=None), dict(y=None), dict(n=0),
               dict(n=-1), dict(S=0)):
        assert unpack(**kw) == N.MSFNO_EINVAL, kw


def test_selection_resolution():
    from msfno_amd import export as X
    shape = (2, 5, 12, 20)
    r = X.Selection().resolve(shape)
    assert r.slabs is None and r.whole and r.out_shape == shape and r.c_window() is None
    r = X.Selection(channels=[3, 0, 3], lat=slice(1, None, 2), lon=slice(3, None, 6)).resolve(shape)
    assert r.slabs == [3, 0, 3, 8, 5, 8]
    assert r.window == (1, 2, 6, 3, 6, 3) and r.out_shape == (2, 3, 6, 3) and not r.whole
    w = r.c_window()
    assert (w.lat0, w.lat_step, w.nlat_out, w.lon0, w.lon_step, w.nlon_out) == r.window
    r = X.Selection(channels=slice(1, 4), lat=-1, lon=7).resolve(shape)
    assert r.slabs == [1, 2, 3, 6, 7, 8] and r.window == (11, 1, 1, 7, 1, 1)
    r = X.Selection(channels=[-1]).resolve(shape)
    assert r.slabs == [4, 9] and r.whole
    r = X.Selection(channels=range(5), lat=slice(0, 12), lon=slice(None)).resolve(shape)
    assert r.slabs is None and r.whole                        # all in order: the identity
    r = X.Selection(lat=slice(None, None, 6), lon=slice(None, None, 6)).resolve((1, 73, 721, 1440))
    assert r.out_shape == (1, 73, 121, 240) and r.slabs is None
    # the torch indexing of the f32 path selects the same points as the restatement
    import torch
    x = torch.arange(2 * 5 * 12 * 20, dtype=torch.float32).view(shape)
    sel = X.Selection(channels=[3, 0, 3], lat=slice(1, None, 2), lon=slice(3, None, 6))
    r = sel.resolve(shape)
    want = XU.select(x.view(10, 12, 20).numpy(), r.slabs, r.window)
    assert np.array_equal(r.index(x).reshape(6, 6, 3).numpy(), want)
    for bad in (dict(channels=[5]), dict(channels=[-6]), dict(channels=[]), dict(channels=[0.5]),
                dict(channels=slice(5, 9)), dict(channels=3), dict(lat=12), dict(lon=-21),
                dict(lat=slice(4, 4)), dict(lat=slice(None, None, -1)), dict(lon=slice(0, 5, 0)),
                dict(lat=[1, 2]), dict(lon="all")):
        with pytest.raises(ValueError):
            X.Selection(**bad).resolve(shape)
    with pytest.raises(ValueError, match="B, C, H, W"):
        X.Selection().resolve((5, 12, 20))
    d = sel.describe()
    assert json.loads(json.dumps(d)) == {"channels": [3, 0, 3], "lat": [1, None, 2],
                                         "lon": [3, None, 6]}


def test_python_refusals():
    import torch
    from msfno_amd import export as X
    from msfno_amd.rollout import Rollout
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(ValueError, match="GPU"):
        X.pack(x)                                                    # no CPU path
    with pytest.raises(ValueError, match="B, C, H, W"):
        X.pack(x[0])
    with pytest.raises(ValueError, match="requires grad"):
        X.pack(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="GPU"):
        X.unpack(X.Packed(torch.zeros(1, 2, 4, 8, dtype=torch.int16), torch.zeros(1, 2),
                          torch.zeros(1, 2, dtype=torch.int32), (1, 2, 4, 8)))
    with pytest.raises(ValueError, match="encoding"):
        X.ForecastWriter((1, 2, 4, 8), encoding="f16")
    with pytest.raises(ValueError, match="depth"):
        X.ForecastWriter((1, 2, 4, 8), depth=0)
    with pytest.raises(ValueError):
        X.ForecastWriter((1, 2, 4, 8), selection=X.Selection(lat=9))

    class Sharded:
        world = 2

    with pytest.raises(NotImplementedError, match="all-reduced"):
        Rollout(Sharded(), graph=False).export(x, 1, writer=None)


def _random_slab(g):
    H, W = int(g.integers(1, 9)), int(g.integers(1, 40))
    kind = int(g.integers(0, 6))
    n = g.standard_normal((1, H, W))
    if kind == 0:
        x = 300 + n
    elif kind == 1:
        x = n * 10.0 ** g.integers(-30, 30)
    elif kind == 2:
        x = g.standard_normal() * 10.0 ** g.integers(-5, 5) + n * 10.0 ** g.integers(-12, 3)
    elif kind == 3:
        x = np.round(n * 100) * 2.0 ** g.integers(-130, 100)       # many ties and exact values
    elif kind == 4:
        x = np.full((1, H, W), g.standard_normal() * 1e3)
    else:
        x = 2.0 ** -126 * g.integers(-40000, 40000, (1, H, W))
    return x.astype(np.float32)


def _properties(name, x, E_want=None, qmax_want=None):
    ref, exp2, q = XU.encode(x)
    xhat = XU.decode(q, ref, exp2)
    d = np.float32(x.max() - x.min())
    E = int(exp2[0])
    assert ref[0] == x.min() and -126 <= E <= 112, name
    assert int(q.max()) <= 65535 and int(q.min()) == 0, name
    if d > 0 and E > -126:
        assert int(q.max()) >= 32767, name
    if d == 0:
        assert E == 0 and not q.any(), name
    else:
        # the smallest E: d fits under 65535 2^E and, unless clamped, not under 65535 2^(E-1)
        assert float(d) <= 65535 * 2.0 ** E, name
        assert E == -126 or float(d) > 65535 * 2.0 ** (E - 1), name
    if E_want is not None:
        assert E == E_want, (name, E, E_want)
    if qmax_want is not None:
        assert int(q.max()) == qmax_want, (name, int(q.max()))
    err = np.abs(xhat.astype(np.float64) - x.astype(np.float64))
    b = XU.bound(x, ref, exp2, xhat)
    assert (err <= b).all(), (name, (err / b).max())
    return float((err / b).max())


def test_the_restatement_keeps_its_properties():
    """The issue's claims about the definition, on 2,000 random slabs and the edge slabs."""
    g = np.random.default_rng(7)
    worst = max(_properties(f"random {i}", _random_slab(g)) for i in range(2000))
    for name, x, E_want, qmax_want in XU.edge_slabs():
        worst = max(worst, _properties(name, x, E_want, qmax_want))
    print(f"restatement: worst round-trip error / bound {worst:.3f}")
    assert worst <= 1.0
    _, _, q = XU.encode(dict((n, x) for n, x, _, _ in XU.edge_slabs())["ties"])
    assert q[0, 0].tolist() == [0, 0, 2, 2] and q[0, 1].tolist() == [65534, 65535, 3, 7]
    # a subset takes the range of its own points
    x = XU.slabs((3, 7, 9), seed=1)
    x[:, 0, 0], x[:, 6, 8] = -1e4, 1e4
    ref, exp2, q = XU.pack(x, slab=[2, 0, 2], win=(1, 2, 3, 1, 3, 3))
    sub = x[[2, 0, 2]][:, 1:6:2, 1:8:3]
    assert q.shape == (3, 3, 3) and np.array_equal(ref, sub.min(axis=(1, 2)))
    assert (exp2 < XU.encode(x)[1][[2, 0, 2]]).all()


def test_decode_numpy_is_the_restatement():
    from msfno_amd import export as X
    g = np.random.default_rng(2)
    q = g.integers(0, 65536, (2, 3, 4, 5)).astype(np.uint16)
    ref = (300 * g.standard_normal((2, 3))).astype(np.float32)
    exp2 = g.integers(-20, 8, (2, 3)).astype(np.int32)
    got = X.decode_numpy(q, ref, exp2)
    assert got.dtype == np.float32 and np.array_equal(got, XU.decode(q, ref, exp2))
    assert np.array_equal(X.decode_numpy(q.view(np.int16), ref, exp2), got)   # the same bits
    p = X.Packed(q, ref, exp2, q.shape)
    assert np.array_equal(p.numpy(), got) and np.array_equal(p.copy().numpy(), got)


def test_npy_archive_round_trip_from_host_arrays(tmp_path):
    from msfno_amd import export as X
    B, C, H, W = 1, 3, 7, 9
    sel = X.Selection(channels=[2, 0, 1])
    path = str(tmp_path / "fc")
    steps, want = [0, 2, 4], []
    with X.NpyArchive(path, n_steps=4, source_shape=(B, C, H, W), selection=sel) as arc:
        for k, step in enumerate(steps):
            x = XU.slabs((C, H, W), seed=k)
            ref, exp2, q = XU.encode(x)
            want.append(XU.decode(q, ref, exp2).reshape(B, C, H, W))
            arc(step, X.Packed(q.reshape(B, C, H, W), ref.reshape(B, C), exp2.reshape(B, C),
                               (B, C, H, W), sel))
        with pytest.raises(ValueError, match="holds"):
            arc(6, X.Packed(q, ref, exp2, (B, C, H + 1, W)))          # another shape
    qf = np.load(os.path.join(path, "q.npy"))
    assert qf.dtype == np.uint16 and qf.shape == (4, C, H, W)
    assert np.load(os.path.join(path, "ref.npy")).shape == (4, C)
    assert np.load(os.path.join(path, "exp2.npy")).dtype == np.int32
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["steps"] == steps and meta["source_shape"] == [B, C, H, W]
    assert meta["selection"]["channels"] == [2, 0, 1] and meta["out_shape"] == [B, C, H, W]
    a = X.open_archive(path)
    assert a.steps == steps and len(a) == 3 and a.out_shape == (B, C, H, W)
    for k in range(3):
        got = a.decode(k)
        assert got.dtype == np.float32 and np.array_equal(got, want[k])
    with pytest.raises(IndexError):
        a.decode(3)
    with pytest.raises(ValueError, match="f32"):
        X.NpyArchive(str(tmp_path / "g"), 1)(0, X.Packed(None, None, None, (B, C, H, W),
                                                         values=want[0]))
