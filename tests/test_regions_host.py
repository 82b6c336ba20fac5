"""CPU-side checks of the regional verification (msfno_amd/regions.py,
msfno_amd/verification.py, csrc/verify_regions.hip): the C-ABI additions are declared,
exported and bound and refuse bad arguments before any launch, the region builders equal
dense boolean arrays formed here from the definition, and ``finish_regions`` on fp64 host
sums equals the restatement (tests/verify_regions_util.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import verify_regions_util as RU
from conftest import REPO

AXIS_VALUES = (1, 2, 3, 7, 28, 29, 64, 65, 73, 128, 721, 1024, 1025, 2047, 2048, 2049, 5000)


def test_region_symbols_declared_exported_and_bound():
    from msfno_amd import _native as N
    hdr = open(os.path.join(REPO, "include", "msfno.h")).read()
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in ("msfno_verify_regions_workspace_size", "msfno_verify_region_sums"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(N.lib(), s), s
        assert s in bound, s
    assert N.lib().msfno_abi_version() == 6


def test_regions_workspace_size_positive_and_monotone():
    from msfno_amd import _native as N
    f = N.lib().msfno_verify_regions_workspace_size
    base = (73, 721, 1440, 13)
    assert f(*base) > 0 and f(1, 1, 1, 1) > 0
    for axis in range(4):
        prev = 0
        for v in (range(1, 33) if axis == 3 else AXIS_VALUES):
            a = list(base)
            a[axis] = v
            cur = f(*a)
            assert cur > 0 and cur >= prev, (axis, v, cur, prev)
            prev = cur
    # against the other extreme of the region count too
    for R in (1, 32):
        for axis in range(3):
            prev = 0
            for v in AXIS_VALUES:
                a = [73, 721, 1440, R]
                a[axis] = v
                cur = f(*a)
                assert cur > 0 and cur >= prev, (R, axis, v)
                prev = cur
    assert f(0, 721, 1440, 1) == 0 and f(73, -1, 1440, 1) == 0 and f(73, 721, 0, 1) == 0
    assert f(73, 721, 1440, 0) == 0 and f(73, 721, 1440, 33) == 0


def test_region_sums_refuses_bad_arguments_before_any_launch():
    """MSFNO_EINVAL for null pointers, nregions outside 1..32, extents below 1 and only one of
    clim / clim_slab, MSFNO_EWORKSPACE for a short workspace; on host pointers that no kernel
    may touch."""
    from msfno_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    big = 1 << 20

    def call(prd=p, tar=p, w=p, clim=None, slab=None, row=p, col=p, pix=None, R=3, skip=0,
             sums=p, BC=1, nlat=2, nlon=2, ws=p, nbytes=big):
        return lib.msfno_verify_region_sums(prd, tar, w, clim, slab, row, col, pix, R, skip,
                                            sums, BC, nlat, nlon, ws, nbytes, None)

    for name in ("prd", "tar", "w", "row", "col", "sums", "ws"):
        assert call(**{name: None}) == N.MSFNO_EINVAL, name
    for name in ("BC", "nlat", "nlon"):
        assert call(**{name: 0}) == N.MSFNO_EINVAL, name
        assert call(**{name: -3}) == N.MSFNO_EINVAL, name
    for R in (0, -1, 33, 64):
        assert call(R=R) == N.MSFNO_EINVAL, R
    assert b"nregions" in lib.msfno_last_error()
    assert call(clim=p) == N.MSFNO_EINVAL
    assert call(slab=p) == N.MSFNO_EINVAL
    assert b"clim" in lib.msfno_last_error()
    assert call(nbytes=8) == N.MSFNO_EWORKSPACE
    for R in (1, 9, 32):
        short = lib.msfno_verify_regions_workspace_size(1, 2, 2, R) - 1
        assert call(clim=p, slab=p, pix=p, R=R, nbytes=short) == N.MSFNO_EWORKSPACE


# ---- the builders against dense boolean arrays formed from the definition ----------------------

def _grids():
    from msfno_amd.regrid import Grid
    return [(721, 1440), (121, 240), Grid(120, 240, "legendre-gauss")]


def _lat_lon(grid):
    from msfno_amd.regrid import Grid
    g = grid if isinstance(grid, Grid) else Grid(*grid)
    return g, 90.0 - np.degrees(g.theta), 360.0 * np.arange(g.nlon) / g.nlon


def _dense_box(lat, lon, box):
    lat_min, lat_max, lon_min, lon_max = box
    rows = np.ones(lat.shape, bool) if lat_min is None else \
        (lat >= lat_min - 1e-9) & (lat <= lat_max + 1e-9)
    if lon_min is None:
        cols = np.ones(lon.shape, bool)
    else:
        lo, hi = lon_min % 360.0, lon_max % 360.0
        cols = (lon >= lo) & (lon <= hi) if lo <= hi else (lon >= lo) | (lon <= hi)
    return rows[:, None] & cols[None, :]


BOXES = {"all": (None, None, None, None), "europe": (35, 75, -12.5, 42.5),
         "pacific": (-30, 30, 150, -120), "cap": (60, 90, None, None),
         "meridian": (None, None, 350, 10), "line": (0, 0, 90, 90), "none": (91, 95, 0, 10)}


@pytest.mark.parametrize("grid", _grids(), ids=["721x1440", "121x240", "gauss120"])
def test_boxes_bands_mask_rows_against_dense(grid):
    from msfno_amd.regions import Regions
    g, lat, lon = _lat_lon(grid)
    rg = Regions.boxes(grid, BOXES)
    assert rg.names == tuple(BOXES) and len(rg) == len(BOXES) and rg.shape == g.shape
    assert rg.pix_bits is None and rg.row_bits.dtype == np.uint32
    for name, box in BOXES.items():
        assert np.array_equal(rg.mask(name), _dense_box(lat, lon, box)), name
    assert rg.mask("all").all() and not rg.mask("none").any()
    if g.kind == "equiangular":
        assert rg.mask("line").sum() == 1                       # the equator at 90 E
    assert rg.mask("meridian")[:, 0].all() and rg.mask("pacific")[g.nlat // 2, g.nlon // 2]

    bands = {"extra": [(-90, -20), (20, 90)], "tropics": [(-20, 20)], "one": [(45, 46)]}
    rb = Regions.bands(grid, bands)
    for name, pairs in bands.items():
        rows = np.zeros(g.nlat, bool)
        for lo, hi in pairs:
            rows |= (lat >= lo - 1e-9) & (lat <= hi + 1e-9)
        assert np.array_equal(rb.mask(name), np.repeat(rows[:, None], g.nlon, 1)), name

    rng = np.random.default_rng(5)
    m1, m2 = rng.random(g.shape) < 0.3, rng.random(g.shape) < 0.6
    rm = rg.with_mask("land", m1).with_mask("eu-land", m2, within="europe") \
           .with_mask("eu-land-land", m1, within="eu-land")
    assert rm.names == tuple(BOXES) + ("land", "eu-land", "eu-land-land")
    assert rm.pix_bits is not None and rg.pix_bits is None      # the original is unchanged
    for name, box in BOXES.items():
        assert np.array_equal(rm.mask(name), _dense_box(lat, lon, box)), name
    eu = _dense_box(lat, lon, BOXES["europe"])
    assert np.array_equal(rm.mask("land"), m1)
    assert np.array_equal(rm.mask("eu-land"), m2 & eu)
    assert np.array_equal(rm.mask("eu-land-land"), m1 & m2 & eu)
    # the definition on the tables themselves
    for k, name in enumerate(rm.names):
        bits = rm.row_bits[:, None] & rm.col_bits[None, :] & rm.pix_bits
        assert np.array_equal((bits >> np.uint32(k)) & np.uint32(1) == 1, rm.mask(name)), name

    idx = list(range(3, g.nlat, 7))
    sub = rm.rows(idx)
    assert sub.shape == (len(idx), g.nlon) and sub.names == rm.names
    for name in rm.names:
        assert np.array_equal(sub.mask(name), rm.mask(name)[idx]), name
    with pytest.raises(ValueError):
        rm.rows([g.nlat])
    with pytest.raises(ValueError):
        rg.with_mask("bad", m1[:-1])
    with pytest.raises(ValueError):
        rg.with_mask("bad", m1.astype(np.float32))
    with pytest.raises(KeyError):
        rg.with_mask("bad", m1, within="atlantis")


def test_land_sea_from_the_nan_pattern():
    from msfno_amd import regions
    rng = np.random.default_rng(2)
    sst = rng.standard_normal((19, 36)).astype(np.float32)
    land = rng.random((19, 36)) < 0.3
    sst[land] = np.nan
    for field in (sst, torch.from_numpy(sst)):
        rg = regions.land_sea(field)
        assert rg.names == ("sea", "land") and rg.shape == (19, 36)
        assert np.array_equal(rg.mask("land"), land) and np.array_equal(rg.mask("sea"), ~land)
    with pytest.raises(ValueError):
        regions.land_sea(sst[0])


SCORECARD_COUNTS = {
    (721, 1440): {"global": (721, 1440), "tropics": (161, 1440), "extra-tropics": (562, 1440),
                  "northern-hemisphere": (281, 1440), "southern-hemisphere": (281, 1440),
                  "arctic": (121, 1440), "antarctic": (121, 1440), "europe": (161, 221),
                  "north-america": (141, 181), "north-atlantic": (161, 241),
                  "north-pacific": (141, 341), "east-asia": (141, 191), "ausnz": (131, 221)},
    (121, 240): {"global": (121, 240), "tropics": (27, 240), "extra-tropics": (94, 240),
                 "northern-hemisphere": (47, 240), "southern-hemisphere": (47, 240),
                 "arctic": (21, 240), "antarctic": (21, 240), "europe": (27, 37),
                 "north-america": (24, 31), "north-atlantic": (27, 40),
                 "north-pacific": (24, 57), "east-asia": (24, 32), "ausnz": (22, 37)},
}


@pytest.mark.parametrize("shape", sorted(SCORECARD_COUNTS), ids=lambda s: "x".join(map(str, s)))
def test_scorecard_counts(shape):
    from msfno_amd import regions
    rg = regions.scorecard(shape)
    assert rg.names == tuple(SCORECARD_COUNTS[shape]) and len(rg) == 13
    for name, (nrow, ncol) in SCORECARD_COUNTS[shape].items():
        m = rg.mask(name)
        assert (int(m.any(axis=1).sum()), int(m.any(axis=0).sum())) == (nrow, ncol), name
        assert int(m.sum()) == nrow * ncol, name                # a product of rows and columns
    lat = 90.0 - 180.0 * np.arange(shape[0]) / (shape[0] - 1)
    assert np.array_equal(rg.mask("extra-tropics")[:, 0], np.abs(lat) >= 20 - 1e-9)
    # north-pacific wraps through the date line, europe through Greenwich
    lon = 360.0 * np.arange(shape[1]) / shape[1]
    assert np.array_equal(rg.mask("north-pacific").any(axis=0), (lon >= 145) & (lon <= 230))
    assert np.array_equal(rg.mask("europe").any(axis=0), (lon >= 347.5) | (lon <= 42.5))


def test_more_than_32_regions_are_refused():
    from msfno_amd.regions import Regions
    boxes = {f"b{k}": (-90 + k, 90, None, None) for k in range(33)}
    with pytest.raises(ValueError, match="32"):
        Regions.boxes((19, 36), boxes)
    with pytest.raises(ValueError, match="32"):
        Regions.bands((19, 36), {k: [(v[0], v[1])] for k, v in boxes.items()})
    full = Regions.boxes((19, 36), dict(list(boxes.items())[:32]))
    assert len(full) == 32 and full.mask("b31")[0, 0] and full.row_bits.max() >= 1 << 31
    with pytest.raises(ValueError, match="32"):
        full.with_mask("one-more", np.ones((19, 36), bool))
    with pytest.raises(ValueError):
        Regions((), np.zeros(3, np.uint32), np.zeros(4, np.uint32))
    with pytest.raises(ValueError):
        Regions(("a", "a"), np.zeros(3, np.uint32), np.zeros(4, np.uint32))


# ---- finish_regions ----------------------------------------------------------------------------

def _host_problem(B=2, C=5, H=9, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    tar = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    prd = tar + 0.4 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    clim = 0.5 * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    w = torch.rand(H, generator=g, dtype=torch.float64) + 0.1
    slab = [(-1 if c in (1, 3) else c) for _ in range(B) for c in range(C)]
    return prd, tar, clim, w, slab


@pytest.mark.parametrize("batch_mean", [False, True])
def test_finish_regions_equals_restatement(batch_mean):
    from msfno_amd import verification as V
    prd, tar, clim, w, slab = _host_problem()
    _, member = RU.region_problem(9, 16, 8)
    s, _ = RU.sums(prd, tar, w, member, clim, slab)
    assert s.shape == (2, 5, 8, 7)
    has = torch.tensor(slab).reshape(2, 5) >= 0
    got = V.finish_regions(s, batch_mean=batch_mean)
    want = RU.scores(s, has, batch_mean=batch_mean)
    assert got.mse.dtype == torch.float64
    assert got.mse.shape == ((5, 8) if batch_mean else (2, 5, 8))
    for name in RU.NAMES:
        g, v = getattr(got, name), want[name]
        assert g.shape == v.shape, name
        assert torch.equal(torch.isnan(g), torch.isnan(v)), name
        ok = ~torch.isnan(v)
        assert ((g[ok] - v[ok]).abs() <= 1e-12 * v[ok].abs().clamp(min=1e-300)).all(), name
    # region 1 is empty: n = 0 and every score NaN; region 0 is the whole grid
    for name in RU.NAMES:
        assert torch.isnan(getattr(got, name)[..., 1]).all(), name
    assert (s[..., 1, :] == 0).all()
    n = 16 * w.sum()
    assert ((s[..., 0, 0] - n).abs() <= 1e-12 * n).all()
    whole = V.finish(s[..., 0, 1:], w, 16, batch_mean=batch_mean)
    assert ((whole.mse - got.mse[..., 0]).abs() <= 1e-12 * whole.mse).all()
    # slabs without a climatology: NaN skill and ACC, finite everything else
    nan_cols = torch.tensor([False, True, False, True, False])
    live = [r for r in range(8) if r != 1]
    assert torch.equal(torch.isnan(got.skill[..., live]).reshape(-1, 5, 7).all(dim=0).all(-1),
                       nan_cols)
    assert torch.equal(torch.isnan(got.acc[..., live]).reshape(-1, 5, 7).any(dim=0).any(-1),
                       nan_cols)
    for name in ("mse", "rmse", "bias", "mae"):
        assert torch.isfinite(getattr(got, name)[..., live]).all()
    stacked = V.finish_regions(torch.stack((s, 2 * s)), batch_mean=batch_mean)
    assert stacked.mse.shape == (2,) + got.mse.shape
    with pytest.raises(ValueError):
        V.finish_regions(torch.zeros(2, 5, 6))
    with pytest.raises(ValueError):
        V.finish_regions(torch.zeros(5, 8, 7))


def test_restatement_skips_missing_values():
    """The restatement itself: skip_nan sums equal the sums under a membership without the
    missing pixels."""
    prd, tar, clim, w, slab = _host_problem(seed=4)
    _, member = RU.region_problem(9, 16, 8)
    miss = torch.rand(9, 16, generator=torch.Generator().manual_seed(1)) < 0.3
    holes = tar.clone()
    holes[:, :, miss] = float("nan")
    a, _ = RU.sums(prd, holes, w, member, clim, slab, skip_nan=True)
    b, _ = RU.sums(prd, tar, w, member & ~miss, clim, slab)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_region_sums_refuses_host_tensors_and_bad_regions():
    from msfno_amd import verification as V
    from msfno_amd.regions import Regions
    x = torch.zeros(1, 2, 4, 8)
    rg = Regions.boxes((4, 8), {"all": (None, None, None, None)})
    with pytest.raises(ValueError):
        V.region_sums(x, x, torch.ones(4), rg)            # libmsfno has no CPU path
    with pytest.raises(ValueError, match="requires grad"):
        V.region_sums(x.clone().requires_grad_(), x, torch.ones(4), rg)
    with pytest.raises(ValueError):
        V.RegionalVerifier("uniform", "europe", 1, 1, 2, device="cpu")
