"""Sweep of the compiled-codelet row FFTs: the cases and their CPU references, shared by
test_fft_codelet_cases_host.py and test_gpu_fft_codelets.py.

Six grid widths have a compiled codelet (csrc/fft.hip MSFNO_FFT_CODELETS: nlon 1440, 240,
64, 48, 180, 32).  Five of them (nlon % 8 == 0) run under the LDS-DMA row kernels,
fft_r2c_dma_kernel and eight instantiations of fft_c2r_dma_kernel; 180 runs its codelet
under the register-prefetch kernels fft_r2c_rows_kernel / fft_c2r_rows_kernel, as every
width does with MSFNO_FFT_DMA=0.  Which kernel a call takes depends on the shape
(launch_r2c / launch_c2r), mirrored here by c2r_ncy, c2r_kernel and rows_for_trips; the
module-level asserts pin the edges the cases are built around.

Stand-alone cases are fft_size_cases.Case tuples with their references, inputs, error
measures and bar taken from fft_size_cases unchanged ("grid": equiangular quadrature of an
odd nlat; "dense": a seeded table without symmetry, the general Legendre layout).  Block
cases use legendre_cases' symmetric dense tables (the folded layout), its oracle and its
bar; a case with an MLP is compared through the whole block (the MLP turns the plane
outputs of the inverse FFT on), the others through global_conv.

Linear-filter block cases at nlon 1440 keep lmax = 16 (the per-mode weight of a full
721-degree spectrum would be 100 MB and more): their Fourier bins m >= 16 are zero, they are
there for the dispatch and the GELU epilogue; the non-linear ones have lmax = mmax, so every
staged bin carries weight."""
import functools
from collections import namedtuple

import torch

import fft_size_cases as F
import legendre_cases as L

GPU_BAR = F.GPU_BAR
FP32_BAR = GPU_BAR / 2
Case = F.Case
KINDS = F.KINDS
WIDTHS = (1440, 240, 64, 48, 180, 32)      # csrc/fft.hip MSFNO_FFT_CODELETS
LDS_BYTES = 160 * 1024
MI355X_CUS = 256                           # the host tests build the multi-trip cases for it

R2C_WV = 12                                # launch_r2c: fft_r2c_dma_kernel<CL, 12, PL, 2>
C2R_WV = 4                                 # launch_c2r: the stand-alone inverse's 4-wave kernel


def is_dma(nlon, mmax):
    """The shape conditions of launch_r2c (`(2 * CL::H) % 8 == 0 && mmax <= CL::H + 1`),
    to which launch_c2r adds `ncy <= 5` (see c2r_kernel)."""
    return nlon % 8 == 0 and mmax <= nlon // 2 + 1


def c2r_ncy(mmax):
    """KiB of spectrum the inverse stages per row.  Mirrors launch_c2r and
    fft_c2r_planes_supported in csrc/fft.hip: `ncy = (mmax * 8 + 16 + 1023) / 1024`."""
    return (mmax * 8 + 16 + 1023) // 1024


def _c2r_lds(nlon, mmax, skip):
    """(tw, per_reg, per) of launch_c2r: `rb = 2 * CL::H * 4`, `nca = (rb + 1023) / 1024`,
    `per_reg = rb + ncy * 1024`, `per = per_reg + (addsrc ? nca * 1024 : 0)`,
    `tw = (2 * CL::H + 2) * sizeof(float2)`."""
    rb = nlon * 4
    nca = (rb + 1023) // 1024
    per_reg = rb + c2r_ncy(mmax) * 1024
    return (nlon + 2) * 8, per_reg, per_reg + (nca * 1024 if skip else 0)


def c2r_kernel(nlon, mmax, skip, planes, areg=True, wide=True, swz=False, dma=True):
    """The inverse kernel launch_c2r picks, as (name, waves): its if / else-if chain in
    csrc/fft.hip, `dma` MSFNO_FFT_DMA, `areg` MSFNO_C2R_AREG, `wide` MSFNO_C2R_WV != 4,
    `swz` MSFNO_C2R_SWZ=1.  Names: <ADD, WV, PL, AR, SWI> of fft_c2r_dma_kernel."""
    if not (dma and is_dma(nlon, mmax) and c2r_ncy(mmax) <= 5):
        assert not planes, "fft_c2r_planes_supported is off here"
        return "fft_c2r_rows_kernel", 4
    tw, per_reg, per = _c2r_lds(nlon, mmax, skip)
    fits = lambda wv, p: tw + wv * p <= LDS_BYTES
    if planes and skip and areg and fits(16, per_reg):
        return "dma<add,16,planes,areg>", 16
    if planes and skip and wide and fits(10, per):
        return "dma<add,10,planes>", 10
    if planes and skip:
        return "dma<add,4,planes>", 4
    if planes:
        return "dma<4,planes>", 4
    if skip and areg and swz and fits(12, per_reg):
        return "dma<add,12,areg,swz>", 12
    if skip and areg and fits(16, per_reg):
        return "dma<add,16,areg>", 16
    if skip:
        return "dma<add,4>", 4
    return "dma<4>", 4


C2R_DMA_KERNELS = {"dma<add,16,planes,areg>", "dma<add,10,planes>", "dma<add,4,planes>",
                   "dma<4,planes>", "dma<add,12,areg,swz>", "dma<add,16,areg>", "dma<add,4>",
                   "dma<4>"}


def grid_rows(kernel, nlon, mmax, cus):
    """Rows one trip of the whole grid covers, WV * (the cap of the grid), of a stand-alone
    transform.  "r2c": launch_r2c's `grid = min(cdiv(rows, WV), device_cus())` with WV = 12.
    "c2r": launch_c2r's `wg_cu = max(1, (160 * 1024) / (tw + 4 * per))` and, in `go`,
    `grid = min(cdiv(rows, WV), device_cus() * wgs)` with WV = 4, wgs = wg_cu."""
    assert is_dma(nlon, mmax) and c2r_ncy(mmax) <= 5
    if kernel == "r2c":
        return R2C_WV * cus
    assert kernel == "c2r"
    tw, _, per = _c2r_lds(nlon, mmax, False)
    return C2R_WV * cus * max(1, LDS_BYTES // (tw + 4 * per))


def rows_for_trips(kernel, nlon, mmax, cus, trips):
    """The smallest row count at which some wave of the grid-stride loop (`for (row = row0;
    row < rows; row += stride)`, stride = gridDim.x * WV, in fft_r2c_dma_kernel and
    fft_c2r_dma_kernel) makes `trips` trips: the capped grid covers grid_rows per trip."""
    return (trips - 1) * grid_rows(kernel, nlon, mmax, cus) + 1


# the edges the cases below are built around
assert [c2r_ncy(m) for m in (126, 127, 254, 255, 382, 383, 510, 511, 638, 639)] == \
    [1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
assert c2r_kernel(1440, 638, False, False)[0] == "dma<4>"
assert c2r_kernel(1440, 639, False, False)[0] == "fft_c2r_rows_kernel"
# 1440: the 16-wave register-skip kernel fits up to mmax 382 (152,848 B), from 383 (169,232 B)
# neither it nor the 10-wave form does and the 4-wave LDS-DMA-skip kernels run
assert _c2r_lds(1440, 382, True)[0] + 16 * _c2r_lds(1440, 382, True)[1] == 152848
assert _c2r_lds(1440, 383, True)[0] + 16 * _c2r_lds(1440, 383, True)[1] == 169232
assert _c2r_lds(1440, 383, True)[0] + 10 * _c2r_lds(1440, 383, True)[2] > LDS_BYTES
assert c2r_kernel(1440, 382, True, True) == ("dma<add,16,planes,areg>", 16)
assert c2r_kernel(1440, 383, True, True) == ("dma<add,4,planes>", 4)
assert c2r_kernel(1440, 382, True, False) == ("dma<add,16,areg>", 16)
assert c2r_kernel(1440, 383, True, False) == ("dma<add,4>", 4)
assert c2r_kernel(1440, 383, True, True, areg=False)[0] == "dma<add,4,planes>"
assert c2r_kernel(240, 121, True, True, areg=False) == ("dma<add,10,planes>", 10)
assert not is_dma(180, 31) and c2r_kernel(180, 31, False, False)[0] == "fft_c2r_rows_kernel"
assert all(is_dma(n, n // 2 + 1) for n in WIDTHS if n != 180)
assert rows_for_trips("c2r", 32, 5, 256, 3) == 67585     # tw 272 + 4 * 1152: 33 workgroups a CU


# ---- stand-alone transforms ----------------------------------------------------------
NLAT = {1440: 3, 240: 5, 64: 9, 48: 7, 180: 7, 32: 5}     # odd and small
# 15 fields (an odd row count) and 12 (an even one).  fft_size_cases.LEAD's 3 fields are too
# few at nlat 3: on the grid only the equator row reaches the orders m > 0, and of 721 columns
# with 3 samples each some come out under COLUMN_FLOOR by chance
LEAD, LEAD_EVEN = (5, 3), (4, 3)


def _width_cases(nlon):
    """mmax 1 and 2, an even and an odd one near H / 3, H, and H + 1 (the Nyquist bin), with
    LEAD: rows = 15 nlat is odd, rows * mmax is odd for every odd mmax (the codelet
    inverse then stages a last 16-B chunk that is half outside the spectrum) and even for the
    others; H + 1, odd for every width, also with an even row count."""
    H, third = nlon // 2, nlon // 2 // 3
    even, odd = (third, third + 1) if third % 2 == 0 else (third + 1, third)
    cs = [Case(NLAT[nlon], nlon, m, LEAD) for m in (1, 2, even, odd, H, H + 1)]
    return cs + [Case(NLAT[nlon], nlon, H + 1, LEAD_EVEN)]


# nlon 180 stays in the sweep: 2 H % 8 != 0, so it runs the FFT180 codelet under the
# register-prefetch kernels fft_r2c_rows_kernel / fft_c2r_rows_kernel, never the DMA ones
WIDTH_CASES = [c for n in WIDTHS for c in _width_cases(n)]
# 1440: the forward kernel's store count nst = ceil(mmax / 64) + .. steps at 64 -> 65 and
# 128 -> 129; ncy steps at 126 -> 127, 254 -> 255, 382 -> 383, 510 -> 511; at 638 -> 639 the
# inverse leaves the DMA kernel for fft_c2r_rows_kernel (and its register prefetch of the
# spectrum row, mmax <= kStageMax = 512, is already off)
EDGES_1440 = [Case(3, 1440, m, LEAD) for m in (64, 65, 128, 129, 126, 127, 254, 255, 382, 383, 510,
                                         511, 638, 639)]     # 720 and 721 are WIDTH_CASES'
EDGES_240 = [Case(5, 240, m, LEAD) for m in (64, 65)]              # 120 and 121 are WIDTH_CASES'
# row counts below, at and above the waves of a workgroup (12 forward, 4 inverse); a wave
# without a row must not touch anything (one row: ROW1_CASES below)
ROW_CASES = [Case(rows, nlon, mmax, (1,)) for nlon, mmax in ((32, 5), (48, 9))
             for rows in (C2R_WV - 1, C2R_WV + 1, R2C_WV - 1, R2C_WV + 1)]
CASES = WIDTH_CASES + EDGES_1440 + EDGES_240 + ROW_CASES
# one row: one field of one latitude, a one-workgroup launch in which only wave 0 has a row
# and no second copy is issued.  The equiangular rule needs two latitudes, so the module is
# built on a one-node Legendre-Gauss grid and only the "dense" kind (which replaces the
# module's table) runs.  With a single row a column's maximum is one product of a Fourier
# coefficient and a table entry (a few for the low orders): mmax 4 and 7 are the widths at
# which these seeds leave every column above COLUMN_FLOOR in both directions (mmax 5 at nlon
# 32 leaves a forward column at 0.03 of the largest)
ROW1_CASES = [Case(1, 32, 4, (1,)), Case(1, 48, 7, (1,))]
ROW1_KINDS = ("dense",)
for _m in (720, 721):
    assert Case(3, 1440, _m, LEAD) in CASES
for _m in (120, 121):
    assert Case(5, 240, _m, LEAD) in CASES


def case_id(c):
    return f"{c.nlat}x{c.nlon}-m{c.mmax}-b{'x'.join(map(str, c.lead))}"


def rows_of(c):
    r = c.nlat
    for n in c.lead:
        r *= n
    return r


IDS = [case_id(c) for c in CASES]
ROW1_IDS = [case_id(c) for c in ROW1_CASES]
assert len(set(IDS)) == len(IDS)
for _n in WIDTHS:
    _par = {rows_of(c) * c.mmax % 2 for c in WIDTH_CASES if c.nlon == _n}
    assert _par == {0, 1}, _n

# the inverse through the C ABI on a dirty workspace: the ncy edges, mmax 1 and 2, and every
# other case with an odd count of spectrum values
ABI_CASES = [c for c in CASES
             if c in EDGES_1440 or c.mmax <= 2 or rows_of(c) * c.mmax % 2 == 1]
ABI_IDS = [case_id(c) for c in ABI_CASES]

# multi-trip: (kernel, nlon, mmax); the row count follows the device's CUs at run time
TRIP_NLAT = {32: 129, 64: 129, 240: 129, 1440: 9}   # (a dense 383 x 383 x 129 table is 150 MB)
TRIPS = [(k, nlon, mmax, t) for k in ("r2c", "c2r") for nlon, mmax in ((32, 5), (64, 12))
         for t in (2, 3)]
# the forward kernel's store count nst = ceil(mmax / 64) + .. enters its wait_vmcnt from a
# wave's second row on: its steps 64 -> 65 and 128 -> 129 at 1440 (6 copy instructions a
# row) and 240 (one), and the inverse's second trip with ncy = 3 and 4 KiB a row
TRIPS += [("r2c", 1440, m, 2) for m in (64, 65, 128, 129)]
TRIPS += [("r2c", 240, m, 3) for m in (64, 65)]
TRIPS += [("c2r", 1440, m, 2) for m in (255, 383)]
TRIP_IDS = [f"{k}-{n}-m{m}-trips{t}" for k, n, m, t in TRIPS]


def trip_case(kernel, nlon, mmax, trips, cus):
    """The case whose grid-stride loop makes `trips` trips on a device of `cus` CUs: rows are
    raised through `lead` at nlat 129 (9 at nlon 1440, where mmax is large), so the Legendre
    stage and its table stay small."""
    rows = rows_for_trips(kernel, nlon, mmax, cus, trips)
    return Case(TRIP_NLAT[nlon], nlon, mmax, (-(-rows // TRIP_NLAT[nlon]),))


# ---- block cases ---------------------------------------------------------------------
BlockCase = namedtuple("BlockCase",
                       "filter nlat nlon lmax mmax B C skip mlp offset wave_hi wave1 kind",
                       defaults=(False, 0, 0.75, "dense"))
NL, LIN = L.NL, L.LIN
LIN_LMAX_1440 = 16


def _b(filt, nlon, mmax, skip, mlp, B=1, C=12, offset=False):
    lmax = LIN_LMAX_1440 if filt == LIN and nlon == 1440 else mmax
    # the input's extra waves (legendre_cases.block_input): order 1 and, where the spectrum
    # reaches it, order mmax - mmax // 6 (mmax // 6 degrees: bin mmax - 2 with its two would
    # carry a fifth of that weight), so that the host file's mutation condition holds for a
    # bin of the first KiB the inverse FFT stages per row and for one of the last, or, where
    # the last holds the final bin alone (mmax 383, 511), of the one before it
    return BlockCase(filt, NLAT[nlon], nlon, lmax, mmax, B, C, skip, mlp, offset,
                     mmax - mmax // 6 if lmax == mmax else 0)


BATCH2 = _b(NL, 1440, 383, "linear", True, B=2)
BATCH1 = BATCH2._replace(B=1)
OFFSET = _b(NL, 1440, 361, "identity", False, offset=True)
BLOCK_CASES = [
    # 1440: the default dispatch crosses 16-wave -> 4-wave ADMA (NCA = 6) -> row kernel
    _b(NL, 1440, 361, "linear", True), _b(LIN, 1440, 361, "identity", False),
    _b(LIN, 1440, 382, "identity", True), _b(NL, 1440, 382, "linear", False),
    _b(NL, 1440, 382, None, True),
    BATCH1, BATCH2, _b(NL, 1440, 383, "identity", False), _b(LIN, 1440, 383, None, False),
    _b(NL, 1440, 383, None, True, C=20),
    _b(LIN, 1440, 511, "identity", True, C=20), _b(NL, 1440, 511, "identity", False),
    _b(NL, 1440, 638, "linear", True), _b(LIN, 1440, 638, None, True),
    _b(NL, 1440, 638, "identity", False),
    _b(NL, 1440, 639, "linear", True), _b(LIN, 1440, 639, "identity", False),
    _b(NL, 1440, 639, None, False),
    OFFSET,
    # 240 (NCA = 1) and 64
    _b(NL, 240, 121, "linear", True, C=20), _b(LIN, 240, 121, "identity", False, C=20),
    _b(LIN, 240, 121, None, True, B=2), _b(NL, 240, 121, None, False, B=2, C=20),
    _b(LIN, 64, 33, "linear", True), _b(NL, 64, 33, "identity", False, B=2),
    _b(NL, 64, 33, None, True, C=20), _b(LIN, 64, 33, None, False, C=20),
    _b(NL, 64, 33, "identity", True, B=2),
]


def block_id(c):
    return (f"{c.filter}-{c.nlat}x{c.nlon}-l{c.lmax}-m{c.mmax}-B{c.B}-C{c.C}-skip_{c.skip}"
            f"-{'mlp' if c.mlp else 'conv'}{'-offset' if c.offset else ''}")


BLOCK_IDS = [block_id(c) for c in BLOCK_CASES]
assert len(set(BLOCK_IDS)) == len(BLOCK_IDS)


def block_planes(c, dma=True):
    """block_fwd.cpp x1_planes: the inverse FFT writes the MLP's input as planes when the block has
    an (unfused: C != 256) MLP, the pixel count is a multiple of 8 and
    fft_c2r_planes_supported; global_conv (cases without MLP) never asks for planes."""
    return bool(c.mlp and dma and (c.nlat * c.nlon) % 8 == 0 and is_dma(c.nlon, c.mmax)
                and c2r_ncy(c.mmax) <= 5)


def block_c2r_kernel(c, **env):
    dma = env.get("dma", True)
    return c2r_kernel(c.nlon, c.mmax, c.skip is not None, block_planes(c, dma), **env)[0]


# under the default switches the block cases reach six of the eight instantiations and the
# row kernel; the 10-wave form needs MSFNO_C2R_AREG=0, the swizzled one MSFNO_C2R_SWZ=1
_DEFAULT = {block_c2r_kernel(c) for c in BLOCK_CASES}
assert _DEFAULT == (C2R_DMA_KERNELS - {"dma<add,10,planes>", "dma<add,12,areg,swz>"}
                    | {"fft_c2r_rows_kernel"}), _DEFAULT
assert "dma<add,10,planes>" in {block_c2r_kernel(c, areg=False) for c in BLOCK_CASES}
assert "dma<add,12,areg,swz>" in {block_c2r_kernel(c, swz=True) for c in BLOCK_CASES}
assert {"dma<add,4,planes>", "dma<add,4>"} <= {block_c2r_kernel(c) for c in BLOCK_CASES
                                             if c.nlon == 1440 and 383 <= c.mmax <= 638}
assert all(block_planes(c) for c in (BATCH1, BATCH2))


@functools.lru_cache(maxsize=None)
def block_zero_film(c):
    """gamma = beta = 0: FiLM is the identity, as in the oracle's block_forward without it."""
    return torch.zeros(c.B, c.C), torch.zeros(c.B, c.C)
