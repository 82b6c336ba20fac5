"""Named regions of one (nlat, nlon) grid for regional and masked verification
(``verification.region_sums``, csrc/verify_regions.hip).

A ``Regions`` holds R <= 32 regions as three uint32 bit tables; bit r speaks for region r:

    row_bits (nlat,)   col_bits (nlon,)   pix_bits (nlat, nlon), optional (absent: all ones)

and pixel (h, x) belongs to region r iff bit r of ``row_bits[h] & col_bits[x] &
pix_bits[h, x]`` is set.  Membership is binary: there are no fractional cells.  The form covers
any set of rows (the union of two latitude caps), any set of columns (a box across longitude
0), any 2-D mask and a box intersected with a mask.  Everything here is host-side numpy; the
device copies are made once per device (``tables``).

Latitudes are ``90 - theta * 180 / pi`` of the grid's nodes, north to south; longitudes
``360 i / nlon``.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_REGIONS = 32
_LAT_EPS = 1e-9   # degrees


def _as_grid(grid):
    from .regrid import Grid, _as_grid as as_grid
    return grid if isinstance(grid, Grid) else as_grid(grid)


def _lat_lon(grid):
    lat = 90.0 - grid.theta * (180.0 / np.pi)
    lon = 360.0 * np.arange(grid.nlon) / grid.nlon
    return lat, lon


def _rows_in(lat, lat_min, lat_max):
    if lat_min is None and lat_max is None:
        return np.ones(lat.shape, dtype=bool)
    if lat_min is None or lat_max is None:
        raise ValueError("give both latitudes of a band, or None for both")
    return (lat >= lat_min - _LAT_EPS) & (lat <= lat_max + _LAT_EPS)


def _cols_in(lon, lon_min, lon_max):
    """The closed interval from lon_min eastward to lon_max, both mod 360."""
    if lon_min is None and lon_max is None:
        return np.ones(lon.shape, dtype=bool)
    if lon_min is None or lon_max is None:
        raise ValueError("give both longitudes of a box, or None for both")
    lo = float(lon_min) % 360.0
    span = (float(lon_max) % 360.0 - lo) % 360.0
    east = (lon - lo) % 360.0      # how far east of lon_min the node lies
    return (east <= span + _LAT_EPS) | (east >= 360.0 - _LAT_EPS)


def _bits(members):
    """uint32 bits of a (R, n...) boolean stack: bit r where members[r] holds."""
    out = np.zeros(members.shape[1:], dtype=np.uint32)
    for r, m in enumerate(members):
        out |= np.where(m, np.uint32(1) << np.uint32(r), np.uint32(0)).astype(np.uint32)
    return out


class Regions:
    """R named regions of a (nlat, nlon) grid as bit tables (see the module)."""

    def __init__(self, names, row_bits, col_bits, pix_bits=None):
        names = tuple(str(n) for n in names)
        if not 1 <= len(names) <= MAX_REGIONS:
            raise ValueError(f"a Regions holds 1 to {MAX_REGIONS} regions, got {len(names)}")
        if len(set(names)) != len(names):
            raise ValueError(f"region names must differ, got {names}")
        row_bits = np.ascontiguousarray(row_bits, dtype=np.uint32)
        col_bits = np.ascontiguousarray(col_bits, dtype=np.uint32)
        if row_bits.ndim != 1 or col_bits.ndim != 1 or not row_bits.size or not col_bits.size:
            raise ValueError("row_bits must be (nlat,) and col_bits (nlon,)")
        if pix_bits is not None:
            pix_bits = np.ascontiguousarray(pix_bits, dtype=np.uint32)
            if pix_bits.shape != (row_bits.size, col_bits.size):
                raise ValueError(f"pix_bits must be (nlat, nlon) = "
                                 f"{(row_bits.size, col_bits.size)}, got {pix_bits.shape}")
        self.names = names
        self.row_bits, self.col_bits, self.pix_bits = row_bits, col_bits, pix_bits
        self._dev = {}

    # ---- the builders ------------------------------------------------------------------------

    @classmethod
    def _from_sets(cls, grid, sets):
        """``sets``: name -> (rows (nlat,) bool, cols (nlon,) bool)."""
        if not 1 <= len(sets) <= MAX_REGIONS:
            raise ValueError(f"a Regions holds 1 to {MAX_REGIONS} regions, got {len(sets)}")
        rows = np.stack([np.asarray(r, dtype=bool) for r, _ in sets.values()])
        cols = np.stack([np.asarray(c, dtype=bool) for _, c in sets.values()])
        if rows.shape[1:] != (grid.nlat,) or cols.shape[1:] != (grid.nlon,):
            raise ValueError("row and column sets must match the grid")
        return cls(tuple(sets), _bits(rows), _bits(cols))

    @classmethod
    def boxes(cls, grid, boxes):
        """``boxes``: name -> (lat_min, lat_max, lon_min, lon_max) in degrees.  A node belongs
        iff lat_min <= lat <= lat_max (within 1e-9 degrees) and its longitude lies in the
        closed interval from lon_min eastward to lon_max, both taken mod 360 (lon_min >
        lon_max after the mod wraps through 0).  None for a pair means all."""
        grid = _as_grid(grid)
        lat, lon = _lat_lon(grid)
        sets = {}
        for name, (lat_min, lat_max, lon_min, lon_max) in boxes.items():
            sets[name] = (_rows_in(lat, lat_min, lat_max), _cols_in(lon, lon_min, lon_max))
        return cls._from_sets(grid, sets)

    @classmethod
    def bands(cls, grid, bands):
        """``bands``: name -> [(lat_min, lat_max), ...]: the union of latitude bands, all
        longitudes."""
        grid = _as_grid(grid)
        lat, lon = _lat_lon(grid)
        sets = {}
        for name, pairs in bands.items():
            rows = np.zeros(grid.nlat, dtype=bool)
            for lat_min, lat_max in pairs:
                rows |= _rows_in(lat, lat_min, lat_max)
            sets[name] = (rows, np.ones(grid.nlon, dtype=bool))
        return cls._from_sets(grid, sets)

    def with_mask(self, name, mask2d, within=None):
        """These regions and one more, ``name``: the pixels where the boolean (nlat, nlon)
        ``mask2d`` holds, intersected with the region ``within`` if one is named."""
        R = len(self)
        if R >= MAX_REGIONS:
            raise ValueError(f"a Regions holds at most {MAX_REGIONS} regions")
        if isinstance(mask2d, torch.Tensor):
            mask2d = mask2d.detach().cpu().numpy()
        mask2d = np.asarray(mask2d)
        if mask2d.dtype != np.bool_ or mask2d.shape != self.shape:
            raise ValueError(f"mask2d must be a boolean {self.shape} array, got "
                             f"{mask2d.dtype} {mask2d.shape}")
        bit = np.uint32(1) << np.uint32(R)
        one = np.uint32(1)
        if within is None:
            rows = np.ones(self.shape[0], dtype=bool)
            cols = np.ones(self.shape[1], dtype=bool)
        else:
            k = np.uint32(self.index(within))
            rows, cols = (self.row_bits >> k) & one == 1, (self.col_bits >> k) & one == 1
            if self.pix_bits is not None:
                mask2d = mask2d & ((self.pix_bits >> k) & one == 1)
        pix = self.pix_bits
        if pix is None:
            pix = np.full(self.shape, (1 << R) - 1, dtype=np.uint32)
        z = np.uint32(0)
        return Regions(self.names + (str(name),),
                       self.row_bits | np.where(rows, bit, z).astype(np.uint32),
                       self.col_bits | np.where(cols, bit, z).astype(np.uint32),
                       pix | np.where(mask2d, bit, z).astype(np.uint32))

    def rows(self, index):
        """The same regions restricted to the rows ``index`` (a latitude-band rank's rows):
        pair it with the rank's rows of the fields and ``w[index]``."""
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        if not index.size or index.min() < 0 or index.max() >= self.shape[0]:
            raise ValueError(f"rows must be a non-empty subset of range({self.shape[0]})")
        return Regions(self.names, self.row_bits[index], self.col_bits,
                       None if self.pix_bits is None else self.pix_bits[index])

    # ---- what it holds -----------------------------------------------------------------------

    def __len__(self):
        return len(self.names)

    @property
    def shape(self):
        return (self.row_bits.size, self.col_bits.size)

    def index(self, name):
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"no region {name!r}; the regions are {self.names}") from None

    def mask(self, name):
        """The dense boolean (nlat, nlon) membership of one region."""
        k, one = np.uint32(self.index(name)), np.uint32(1)
        m = ((self.row_bits >> k) & one)[:, None] & ((self.col_bits >> k) & one)[None, :]
        if self.pix_bits is not None:
            m = m & ((self.pix_bits >> k) & one)
        return m == 1

    def tables(self, device):
        """(row_bits, col_bits, pix_bits or None) on ``device``, as int32 tensors holding the
        uint32 bits; made once per device."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(
                None if a is None else torch.from_numpy(a.view(np.int32)).to(device)
                for a in (self.row_bits, self.col_bits, self.pix_bits))
        return self._dev[key]

    def __repr__(self):
        return (f"Regions({self.shape[0]} x {self.shape[1]}, {list(self.names)}"
                f"{', pix_bits' if self.pix_bits is not None else ''})")


def land_sea(nan_field):
    """Two regions, ``sea`` and ``land``, from the NaN pattern of a 2-D (nlat, nlon) field:
    NaN is land, as in an SST field."""
    if isinstance(nan_field, torch.Tensor):
        nan_field = nan_field.detach().cpu().numpy()
    nan_field = np.asarray(nan_field)
    if nan_field.ndim != 2 or not nan_field.size:
        raise ValueError(f"land_sea takes one 2-D field, got shape {nan_field.shape}")
    land = np.isnan(nan_field)
    nlat, nlon = land.shape
    return Regions(("sea", "land"), np.full(nlat, 3, dtype=np.uint32),
                   np.full(nlon, 3, dtype=np.uint32), _bits(np.stack([~land, land])))


# (lat_min, lat_max, lon_min, lon_max); extra-tropics is the union of two caps
_SCORECARD_BOXES = {
    "global": (None, None, None, None),
    "tropics": (-20, 20, None, None),
    "extra-tropics": None,
    "northern-hemisphere": (20, 90, None, None),
    "southern-hemisphere": (-90, -20, None, None),
    "arctic": (60, 90, None, None),
    "antarctic": (-90, -60, None, None),
    "europe": (35, 75, -12.5, 42.5),
    "north-america": (25, 60, -120, -75),
    "north-atlantic": (25, 65, -70, -10),
    "north-pacific": (25, 60, 145, -130),
    "east-asia": (25, 60, 102.5, 150),
    "ausnz": (-45, -12.5, 120, 175),
}


def scorecard(grid):
    """The 13 regions of a forecast scorecard: global, tropics (|lat| <= 20), extra-tropics
    (|lat| >= 20), the hemispheres poleward of 20, the polar caps poleward of 60, and the
    boxes europe, north-america, north-atlantic, north-pacific, east-asia and ausnz."""
    grid = _as_grid(grid)
    lat, lon = _lat_lon(grid)
    sets = {}
    for name, box in _SCORECARD_BOXES.items():
        if box is None:
            sets[name] = (_rows_in(lat, 20, 90) | _rows_in(lat, -90, -20),
                          np.ones(grid.nlon, dtype=bool))
        else:
            sets[name] = (_rows_in(lat, box[0], box[1]), _cols_in(lon, box[2], box[3]))
    return Regions._from_sets(grid, sets)
