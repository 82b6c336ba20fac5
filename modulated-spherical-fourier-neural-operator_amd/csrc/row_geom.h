// Work decomposition of the latitude-weighted row reductions over (BC, nlat, nlon) fields
// (loss.hip, verify.hip): a workgroup is 256 / lpr row groups of lpr lanes (whole waves), a
// group sweeps one row at a time, 4 floats per lane; a unit is (bc, chunk of rows) on a
// capped grid, one partial per unit, combined per (b, c) in fp64 in a fixed order.
#pragma once
#include <algorithm>

#include "common.h"

namespace msfno {

constexpr int kRowThreads = 256;
constexpr int kRowMaxRows = 64;    // rows per unit: bounds a lane's fp32 chain (below)
constexpr int kRowGridCap = 2048;  // 8 workgroups per CU

// lpr: the one of 256, 128, 64 with the fewest idle lane slots over the row (1440: 360
// float4 = 3 sweeps of 128, not 2 of 256 with the second 40 % full).
struct RowGeom {
  int lpr;      // lanes per row group
  int rows;     // rows per unit (a multiple of the group count unless one unit has them all)
  int chunks;   // units per (b, c) slab
};

inline RowGeom row_geom(int BC, int nlat, int nlon) {
  RowGeom g;
  const int nvec = std::max(1, nlon / 4);
  g.lpr = 256;
  for (int l = 128; l >= 64; l >>= 1)
    if (cdiv(nvec, l) * l < cdiv(nvec, g.lpr) * g.lpr) g.lpr = l;
  const int ngrp = kRowThreads / g.lpr;
  // enough units to fill the chip at small BC, at most kRowMaxRows rows each: a lane's
  // sequential fp32 chain is its share of a row (nlon / lpr terms) plus one weighted add
  // per row it visits, <= 128 terms for nlon <= 16384
  int64_t chunks = std::max<int64_t>(cdiv(kRowGridCap, BC), cdiv(nlat, kRowMaxRows));
  chunks = std::min<int64_t>(chunks, nlat);
  g.rows = (int)std::min<int64_t>(round_up(cdiv(nlat, chunks), ngrp), kRowMaxRows);
  g.chunks = (int)cdiv(nlat, g.rows);
  return g;
}

// Upper bound of BC * chunks that is non-decreasing in every argument (BC * chunks itself
// is not: more slabs means fewer chunks each): chunks <= nlat and
// chunks <= cdiv(cap, BC) + cdiv(nlat, maxrows).
inline int64_t row_units_bound(int BC, int nlat) {
  const int64_t a = (int64_t)BC * nlat;
  const int64_t b = kRowGridCap + (int64_t)BC + (int64_t)BC * cdiv(nlat, kRowMaxRows);
  return std::min(a, b);
}

// position of p on the 16-byte grid, in floats
__device__ __forceinline__ int misalign4(const float* p) {
  return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
}

}  // namespace msfno
