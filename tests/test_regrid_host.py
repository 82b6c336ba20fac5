"""Host-side checks of the regridder (msfno_amd/regrid.py, csrc/regrid.hip through the C-ABI):
the builders' rows, conservation in fp64, the band widths at the sizes that matter, the block
mean against a reshape-mean, the adjoint's tables, the refusals of ``tables_from_dense``, the
binding, every refusal of ``msfno_regrid`` before a launch (pointers never dereferenced), and
the margin the derived tolerance of tests/regrid_util.py leaves to an fp32 emulation.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import regrid_util as RU
from conftest import REPO

PAIRS = [((13, 26), (5, 10)), ((33, 64), (9, 16)), ((721, 1440), (121, 240))]


def _grids(src, dst, kind):
    from msfno_amd import regrid as G
    return G.Grid(*src), G.Grid(*dst, kind=kind)


def test_entry_point_is_declared_bound_and_exported():
    from msfno_amd import _native as N
    from msfno_amd import regrid as G
    header = open(os.path.join(REPO, "include", "msfno.h")).read()
    declared = set(re.findall(r"\b(msfno_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in N.SIGNATURES}
    assert "msfno_regrid" in declared and "msfno_regrid" in bound
    assert hasattr(N.lib(), "msfno_regrid")
    assert N.lib().msfno_abi_version() == 6
    assert "typedef struct msfno_regrid_axis" in header
    assert [f for f, _ in N.RegridAxis._fields_] == ["n_in", "n_out", "taps", "wrap", "start",
                                                     "count", "w"]
    # four ints, then three pointers
    assert ctypes.sizeof(N.RegridAxis) == 4 * 4 + 3 * 8
    assert N.RegridAxis.start.offset == 16 and N.RegridAxis.w.offset == 32
    assert N.REGRID_MAX_TAPS == 32 and "#define MSFNO_REGRID_MAX_TAPS 32" in header
    for name in ("Grid", "Regridder", "conservative", "bilinear", "block_mean",
                 "tables_from_dense", "sst_input"):
        assert hasattr(G, name), name
    import inspect
    from msfno_amd.rollout import Rollout
    for fn in (Rollout.verify, Rollout.verify_ensemble, Rollout.export):
        assert inspect.signature(fn).parameters["regrid"].default is None


def test_grid_cells():
    from msfno_amd import regrid as G
    from msfno_amd.harmonics import quadrature as Q
    g = G.Grid(13, 26)
    assert g.lat_edges[0] == 1.0 and g.lat_edges[-1] == -1.0
    assert np.isclose(g.lat_area()[0], 1 - np.cos(np.pi / 24)) and g.lat_area()[0] < g.lat_area()[1] / 1.9
    assert abs(g.area().sum() - 4 * np.pi) < 1e-12
    n = 120
    g = G.Grid(n, 240, "legendre-gauss")
    x, w = Q.legendre_gauss_weights(n)
    # a cell is its weight, up to the roundings of a cumulative sum of n terms below 2
    assert np.abs(np.sort(g.lat_area()) - np.sort(w)).max() < n * 2.0 ** -52
    mu = np.cos(g.theta)
    assert (np.diff(mu) < 0).all()                                    # north to south
    assert ((mu < g.lat_edges[:-1]) & (mu > g.lat_edges[1:])).all()   # every node in its cell
    e = np.linspace(1, -1, 6)
    assert np.array_equal(G.Grid(5, 8, lat_edges=e).lat_edges, e)
    for bad in (dict(lat_edges=e[::-1]), dict(lat_edges=e[:-1])):
        with pytest.raises(ValueError):
            G.Grid(5, 8, **bad)
    with pytest.raises(NotImplementedError):
        G.Grid(5, 8, "lobatto")


@pytest.mark.parametrize("kind", ["equiangular", "legendre-gauss"])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_rows_sum_to_one_and_the_map_conserves(src, dst, kind):
    from msfno_amd import regrid as G
    if kind == "legendre-gauss":
        dst = (dst[0] - 1, dst[1])
    gs, gd = _grids(src, dst, kind)
    for name, (Wlat, Wlon) in (("conservative", G.conservative(gs, gd)),
                               ("bilinear", G.bilinear(gs, gd)),
                               ("bilinear up", G.bilinear(gd, gs))):
        assert np.abs(Wlat.sum(1) - 1).max() < 1e-13, name
        assert np.abs(Wlon.sum(1) - 1).max() < 1e-13, name
        assert (Wlat >= 0).all() and (Wlon >= 0).all()
    Wlat, Wlon = G.conservative(gs, gd)
    g = np.random.default_rng(3)
    for k in range(3):
        x = g.standard_normal(src) + (300.0 if k else 0.0)
        a = (gd.area() * RU.apply64(Wlat, Wlon, x)).sum()
        b = (gs.area() * x).sum()
        scale = (gs.area() * np.abs(x)).sum()
        assert abs(a - b) <= 1e-12 * scale, (k, a, b)


def test_band_widths_at_the_sizes_that_matter():
    from msfno_amd import regrid as G
    R = G.Regridder(G.Grid(721, 1440), G.Grid(121, 240))
    assert (R.lat.taps, R.lon.taps) == (7, 7)
    assert R.lat.count[0] == 4 and R.lat.count[-1] == 4 and (R.lat.count[1:-1] == 7).all()
    assert (R.lon.count == 7).all() and R.lon.start[0] == 1437 and R.lon.start[1] == 3
    assert R.in_shape == (721, 1440) and R.out_shape == (121, 240)
    Rg = G.Regridder(G.Grid(721, 1440), G.Grid(120, 240, "legendre-gauss"))
    print("taps to the 120-row Gauss grid:", Rg.lat.taps, Rg.lon.taps)
    assert (Rg.lat.taps, Rg.lon.taps) == (8, 7)
    assert (R.T.lat.taps, R.T.lon.taps) == (2, 2)


def test_block_mean_is_a_reshape_mean():
    from msfno_amd import regrid as G
    H, W, fl, fo = 14, 23, 4, 5
    R = G.Regridder((H, W), method=G.block_mean(fl, fo))
    assert R.out_shape == (3, 4) and (R.lat.taps, R.lon.taps) == (4, 5)
    x = np.random.default_rng(0).standard_normal((2, H, W))
    want = x[:, :12, :20].reshape(2, 3, 4, 4, 5).mean(axis=(2, 4))
    Wlat, Wlon = R.dense()
    assert np.abs(RU.apply64(Wlat, Wlon, x) - want).max() < 1e-14
    assert np.array_equal(R.lat.start, 4 * np.arange(3)) and (R.lat.count == 4).all()
    assert np.array_equal(R.lon.w, np.full((4, 5), 0.2, dtype=np.float32))
    # the adjoint has empty rows where the source was trimmed
    assert R.T.lat.count.tolist() == [1] * 12 + [0, 0] and R.T.lon.count.tolist() == [1] * 20 + [0] * 3
    with pytest.raises(NotImplementedError):
        G.block_mean(4, 4, boundary="pad")
    with pytest.raises(NotImplementedError):
        G.block_mean(33, 1)
    with pytest.raises(ValueError):
        G.block_mean(0, 1)
    with pytest.raises(ValueError):
        G.Regridder((3, 8), method=G.block_mean(4, 4))


@pytest.mark.parametrize("method", ["conservative", "bilinear"])
def test_adjoint_tables_are_the_dense_transposes(method):
    from msfno_amd import regrid as G
    src, dst = ((13, 26), (5, 10)) if method == "conservative" else ((5, 10), (13, 26))
    R = G.Regridder(G.Grid(*src), G.Grid(*dst), method)
    T = R.T
    assert T.T is R and T.in_shape == R.out_shape and T.out_shape == R.in_shape
    for ax, fwd in ((T.lat, R.lat), (T.lon, R.lon)):
        W = RU.dense_from_tables(ax.start, ax.count, ax.w, ax.n_in)
        assert np.array_equal(W, fwd.W.T.astype(np.float32).astype(np.float64))
        assert np.array_equal(ax.W, fwd.W.T)
    # rows whose band wraps in longitude exist on both sides
    assert (R.lon.start + R.lon.count > R.lon.n_in).any()
    assert (T.lon.start + T.lon.count > T.lon.n_in).any()
    # the forward tables stand for the forward matrices too
    for ax in (R.lat, R.lon):
        W = RU.dense_from_tables(ax.start, ax.count, ax.w, ax.n_in)
        assert np.array_equal(W, ax.W.astype(np.float32).astype(np.float64))


def test_tables_from_dense_refusals():
    from msfno_amd import regrid as G
    W = np.zeros((2, 40))
    W[0, 3:36] = 1.0 / 33
    W[1, 0] = 1.0
    with pytest.raises(NotImplementedError):
        G.tables_from_dense(W, False)                      # a band of 33
    W[0] = 0
    W[0, 3:35] = 1.0 / 32
    s, c, w = G.tables_from_dense(W, False)                # 32 is the limit
    assert s.tolist() == [3, 0] and c.tolist() == [32, 1] and w.shape == (2, 32)
    assert s.dtype == np.int32 and c.dtype == np.int32 and w.dtype == np.float32
    W[0, 10] = 0
    with pytest.raises(ValueError, match="band"):
        G.tables_from_dense(W, False)                      # a gap
    V = np.zeros((1, 10))
    V[0, [8, 9, 0, 1]] = 0.25
    with pytest.raises(ValueError, match="band"):
        G.tables_from_dense(V, False)                      # contiguous only cyclically
    s, c, w = G.tables_from_dense(V, True)
    assert (s[0], c[0]) == (8, 4)
    V[0, 4] = 0.5
    with pytest.raises(ValueError, match="band"):
        G.tables_from_dense(V, True)                       # two runs on the circle
    s, c, w = G.tables_from_dense(np.full((2, 5), 0.2), True)   # the whole circle
    assert s.tolist() == [0, 0] and c.tolist() == [5, 5]
    for bad in (np.zeros((0, 3)), np.zeros(3), np.full((1, 3), np.nan)):
        with pytest.raises(ValueError):
            G.tables_from_dense(bad, False)
    w1 = np.ones((1, 2), dtype=np.float32)
    for start, count, wrap in (([4], [2], False), ([-1], [1], True), ([5], [1], True),
                               ([0], [3], True), ([0], [-1], True)):
        with pytest.raises(ValueError):
            G.check_tables(np.array(start), np.array(count), w1, 5, wrap)
    G.check_tables(np.array([4]), np.array([2]), w1, 5, True)


def test_c_abi_refusals_come_before_any_launch():
    """Every refusal is decided on the arguments alone: the pointers here are never
    dereferenced (this test runs without a GPU)."""
    from msfno_amd import _native as N
    lib = N.lib()
    p = 4096                       # any non-null address

    def axis(n_in=12, n_out=5, taps=7, wrap=0, start=p, count=p, w=p):
        return N.RegridAxis(n_in, n_out, taps, wrap, start, count, w)

    def call(x=p, S_in=3, slab=None, S_out=3, lat=axis(), lon=axis(20, 7, 7, 1), mask=None,
             skip_nan=0, min_valid=0.0, fill=0.0, y=p):
        return lib.msfno_regrid(x, S_in, slab, S_out, None if lat is None else ctypes.byref(lat),
                                None if lon is None else ctypes.byref(lon), mask, skip_nan,
                                min_valid, fill, y, None)

    for kw in (dict(x=None), dict(y=None), dict(lat=None), dict(lon=None),
               dict(lat=axis(start=None)), dict(lat=axis(count=None)), dict(lat=axis(w=None)),
               dict(lon=axis(start=None)), dict(lon=axis(count=None)), dict(lon=axis(w=None)),
               dict(S_in=0), dict(S_out=0), dict(S_out=-1),
               dict(lat=axis(n_in=0)), dict(lat=axis(n_out=0)), dict(lon=axis(n_in=0)),
               dict(lon=axis(n_out=-2)),
               dict(lat=axis(taps=0)), dict(lat=axis(taps=33)), dict(lon=axis(taps=0)),
               dict(lon=axis(taps=33)), dict(lon=axis(taps=-1)),
               dict(S_out=4),                                   # identity needs S_out <= S_in
               dict(min_valid=-0.5), dict(min_valid=float("nan")), dict(min_valid=float("inf")),
               dict(skip_nan=1, min_valid=-1e-30)):
        assert call(**kw) == N.MSFNO_EINVAL, kw
    for kw in (dict(lon=axis(n_in=8189, n_out=7)), dict(lon=axis(n_in=1 << 20, n_out=7)),
               dict(lon=axis(n_in=8189, n_out=7), slab=p, S_out=9, mask=p)):
        assert call(**kw) == N.MSFNO_EUNSUPPORTED, kw
    with pytest.raises(NotImplementedError, match="8188"):
        N.check(call(lon=axis(n_in=8189, n_out=7)), "msfno_regrid")
    with pytest.raises(ValueError, match="taps"):
        N.check(call(lat=axis(taps=33)), "msfno_regrid")
    with pytest.raises(ValueError, match="slab list"):
        N.check(call(S_out=4), "msfno_regrid")


def test_python_refusals():
    import torch
    from msfno_amd import regrid as G
    from msfno_amd.rollout import Rollout
    R = G.Regridder(G.Grid(13, 26), G.Grid(5, 10))
    x = torch.zeros(1, 2, 13, 26)
    with pytest.raises(ValueError, match="GPU"):
        R(x)                                                         # no CPU path
    with pytest.raises(ValueError, match="B, C, H, W"):
        R(x[0])
    with pytest.raises(ValueError, match="maps"):
        R(torch.zeros(1, 2, 12, 26))
    with pytest.raises(ValueError, match="min_valid"):
        R(x, skip_nan=True, min_valid=-1.0)
    with pytest.raises(ValueError, match="channels"):
        R(x, channels=[2])
    with pytest.raises(NotImplementedError, match="gradient"):
        R(x.clone().requires_grad_(), skip_nan=True)
    with pytest.raises(ValueError, match="destination"):
        G.Regridder(G.Grid(13, 26))
    with pytest.raises(ValueError, match="method"):
        G.Regridder(G.Grid(13, 26), G.Grid(5, 10), "nearest")
    with pytest.raises(NotImplementedError, match="8188"):
        G.Regridder((4, 8192), method=G.block_mean(1, 2))

    class Sharded:
        world = 2

    for call in (lambda r: r.verify(x, [], 1, regrid=R),
                 lambda r: r.verify_ensemble(x, [], 1, regrid=R),
                 lambda r: r.export(x, 1, writer=None, regrid=R)):
        with pytest.raises(NotImplementedError, match="band-sharded"):
            call(Rollout(Sharded(), graph=False))


@pytest.mark.parametrize("src,dst,method", [
    ((13, 26), (5, 10), "conservative"), ((12, 20), (5, 7), "conservative"),
    ((33, 64), (9, 16), "conservative"), ((9, 1443), (3, 241), "conservative"),
    ((130, 16), (65, 8), "conservative"), ((5, 10), (13, 26), "bilinear")])
def test_the_bound_leaves_room_for_an_fp32_sum_without_fma(src, dst, method):
    """The derived bound against the least favourable form of the kernel's order: a
    sequential fp32 sum that rounds every product, on 300 + N(0, 1)."""
    from msfno_amd import regrid as G
    R = G.Regridder(G.Grid(*src), G.Grid(*dst), method)
    x = RU.field((3,) + src, seed=5)
    want, bound = RU.linear(R, x)
    ratio = RU.check(f"{src} -> {dst} {method}", RU.emulate32(R, x), want, bound)
    assert ratio < 0.5
