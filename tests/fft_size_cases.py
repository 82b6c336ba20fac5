"""Longitude-FFT size sweep: the cases and their CPU references, shared by
test_fft_sizes_host.py and test_gpu_fft_sizes.py.

Six grid widths have a compiled FFT codelet (csrc/fft.hip: nlon 1440, 240, 64, 48, 180,
32); every other width runs GenericFFT, radix passes 4, 2, 3, 5, 7, 11, 13 on the
half-length H (nlon / 2 for even nlon, nlon for odd).  CASES lists the widths at which that
fallback takes another path: each prime radix alone and after a twiddled pass, passes of
more than 64 butterflies (a second, ragged trip of the lane loops), the float4 / float2 /
scalar row loads, the Nyquist bin, and the two largest transforms its LDS check admits.

Every case has two references, both fp64 on the CPU:

  "grid"   oracle.sht_ref transforms on an equiangular grid of odd nlat with
           lmax = mmax.  The equator row has sin(theta) = 1, so the Legendre functions
           of every order m stay O(1) there and every FFT bin reaches the output.  (On an
           even-nlat Gauss grid the high-m columns underflow and would hide their bins.)
  "dense"  a seeded randn(mmax, lmax, nlat) table, zero where l < m, put in place of the
           module's table; the expected result follows the transform's definition,
           2 pi rfft(x, norm="forward")[..., :mmax] contracted with the table, and
           irfft(einsum(...), n=nlon, norm="forward").  Every bin of every row carries
           O(1) weight, and the table has no equatorial symmetry, so the general
           (non-folded) Legendre layout runs.

Inverse inputs are random phases on a band of degrees (inverse_input): the imaginary parts
at m = 0 and at the Nyquist column are not zero, irfft ignores them and so must the kernel.

The error is measured per column m (column_errors): for the forward transform column m of
the (..., lmax, mmax) result; for the inverse one the m-th longitude Fourier coefficient
(fp64 rfft, norm="forward") of the (..., nlat, nlon) result, over the leading dimensions
and all latitudes.  An error confined to a few bins cannot hide behind the global maximum
that way.  fp32_* restate both references in fp32 (sht_ref modules .float(), torch's fp32
FFT): what an exact fp32 implementation achieves, the yardstick for the GPU bar."""
import functools
from collections import namedtuple

import torch

from oracle import sht_ref as S

LEAD = (1, 3)
GPU_BAR = 2e-6            # the transform parity bar of test_gpu_parity.py, here per column
DEGREE_BAND = 2           # degrees per order in the inverse transform's input
COLUMN_FLOOR = 0.05       # smallest column maximum / largest column maximum of a reference

# lead: the leading dimensions of the case's fields; the sweep of the compiled codelets
# (fft_codelet_cases.py) varies it, the cases below all use LEAD
Case = namedtuple("Case", "nlat nlon mmax lead", defaults=(LEAD,))


def _full(nlat, nlon):
    return Case(nlat, nlon, nlon // 2 + 1)


# nlat is odd and small; with LEAD = (1, 3) the row count 3 nlat is no multiple of the 4
# waves of a workgroup
CASES = [
    _full(5, 14),        # H = 7: one radix-7 pass
    _full(7, 22),        # H = 11: one radix-11 pass
    _full(9, 28),        # H = 14 = 2.7: nlon % 4 == 0 (float4 loads); mmax = 15, Nyquist bin
    _full(5, 63),        # H = 63 = 3.3.7: odd, full complex path, radix 7 after twiddles
    _full(7, 98),        # H = 49 = 7.7: twiddles between two radix-7 passes
    _full(9, 242),       # H = 121 = 11.11
    _full(5, 338),       # H = 169 = 13.13
    _full(7, 308),       # H = 154 = 2.7.11: first pass 77 butterflies = 64 + a ragged 13
    _full(9, 364),       # H = 182 = 2.7.13: first pass 91 butterflies
    _full(5, 256),       # H = 128 = 4.4.4.2: common user grid
    _full(7, 720),       # H = 360 = 4.2.3.3.5: common user grid
    _full(9, 770),       # H = 385 = 5.7.11: nlon % 4 == 2, float2 load loop with H > 64
    _full(5, 891),       # H = 891 = 3^4.11: odd; LDS 64152 B, just under the limit
    _full(7, 1820),      # H = 910 = 2.5.7.13: LDS 65520 B, the largest the check admits
    Case(7, 308, 52),    # mmax about a third: zero fill (inverse) and truncation (forward)
    Case(5, 63, 11),
]
IDS = [f"{c.nlat}x{c.nlon}-m{c.mmax}" for c in CASES]
KINDS = ("grid", "dense")


def _seed(case, salt):
    return 1000003 * salt + 4099 * case.nlon + 17 * case.nlat + case.mmax


@functools.lru_cache(maxsize=None)
def dense_table(case, inverse):
    """The synthetic (mmax, lmax, nlat) fp64 table, lmax = mmax, zero where l < m."""
    m = case.mmax
    g = torch.Generator().manual_seed(_seed(case, 5 if inverse else 3))
    t = torch.randn(m, m, case.nlat, generator=g, dtype=torch.float64)
    l_lt_m = torch.arange(m)[None, :] < torch.arange(m)[:, None]       # [m, l]
    t[l_lt_m] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def forward_input(case):
    g = torch.Generator().manual_seed(_seed(case, 1))
    return torch.randn(*case.lead, case.nlat, case.nlon, generator=g)


@functools.lru_cache(maxsize=None)
def inverse_table(case, kind):
    """The fp64 (mmax, lmax, nlat) table of the inverse reference."""
    if kind == "grid":
        return _modules(case, S.InverseRealSHT).pct
    return dense_table(case, True)


@functools.lru_cache(maxsize=None)
def inverse_input(case, kind):
    """Random phases of unit modulus (..., lmax, mmax) on the DEGREE_BAND degrees
    m <= l < m + DEGREE_BAND of every order, zero elsewhere, column m divided by the
    table's weight on that band, max_k sqrt(sum_l table[m, l, k]^2), so that every Fourier
    bin of the result has about the same size (on the grid at high m: exactly, only
    P_m^m at the equator is left).

    Why not noise on all l >= m: mmax - m degrees then add up in bin m, so bin 0 comes out
    some sqrt(mmax) times larger than the last one (and, on the grid, larger again at the
    poles, where P_l^0 = sqrt((2l + 1) / 4 pi)) and the rounding of the large bins swamps
    the small ones; and the fp32 sum over up to 911 degrees alone costs 1.7e-6 per column
    on the restatement, which is the Legendre stage's rounding, not the FFT's.  Measured
    on the restatement, worst per-column error over CASES: Gaussian noise on 8 degrees
    7.7e-7, unit modulus on 8 degrees 5.9e-7, unit modulus on 2 degrees 4.6e-7; only the
    last leaves the fp32 restatement under a quarter of the bar.  The Legendre stage's own
    parity on full noise is test_gpu_parity.py's and the boundary test's business."""
    g = torch.Generator().manual_seed(_seed(case, 2))
    a = torch.view_as_complex(torch.randn(*case.lead, case.mmax, case.mmax, 2, generator=g))
    a = a / a.abs()
    d = torch.arange(case.mmax)[:, None] - torch.arange(case.mmax)[None, :]   # l - m
    band = (d >= 0) & (d < DEGREE_BAND)                                       # [l, m]
    t = inverse_table(case, kind) * band.t()[:, :, None]
    weight = t.square().sum(1).sqrt().max(-1).values                          # [m]
    return a * (band / weight).float()


def _forward(x, table, mmax):
    X = 2.0 * torch.pi * torch.fft.rfft(x, norm="forward")[..., :mmax]
    return torch.einsum("...km,mlk->...lm", X, table.to(X.dtype))


def _inverse(a, table, nlon):
    Y = torch.einsum("...lm,mlk->...km", a, table.to(a.dtype))
    return torch.fft.irfft(Y, n=nlon, norm="forward")


def _modules(case, cls):
    return cls(case.nlat, case.nlon, lmax=case.mmax, mmax=case.mmax, grid="equiangular")


@functools.lru_cache(maxsize=None)
def forward_reference(case, kind):
    """fp64 (..., lmax, mmax) complex128; computed once, shared, never modified."""
    x = forward_input(case).double()
    if kind == "grid":
        return _modules(case, S.RealSHT)(x)
    return _forward(x, dense_table(case, False), case.mmax)


@functools.lru_cache(maxsize=None)
def inverse_reference(case, kind):
    """fp64 (..., nlat, nlon)."""
    a = inverse_input(case, kind).to(torch.complex128)
    if kind == "grid":
        return _modules(case, S.InverseRealSHT)(a)
    return _inverse(a, dense_table(case, True), case.nlon)


def fp32_forward(case, kind):
    """The forward reference restated in fp32."""
    x = forward_input(case)
    if kind == "grid":
        return _modules(case, S.RealSHT).float()(x)
    return _forward(x, dense_table(case, False).float(), case.mmax)


def fp32_inverse(case, kind):
    a = inverse_input(case, kind)
    if kind == "grid":
        return _modules(case, S.InverseRealSHT).float()(a)
    return _inverse(a, dense_table(case, True).float(), case.nlon)


def columns(t, case, inverse):
    """`t` as fp64 columns (..., rows, mmax): the forward result as it is, the inverse one
    as its longitude Fourier coefficients m < mmax."""
    if inverse:
        return torch.fft.rfft(t.double(), norm="forward")[..., :case.mmax]
    return t.to(torch.complex128)


def column_maxima(t, case, inverse):
    c = columns(t, case, inverse).abs()
    return c.reshape(-1, c.shape[-1]).max(0).values


def column_errors(got, want, case, inverse):
    """(mmax,) tensor: max |got - want| over column m / max |want| over column m."""
    d = (columns(got, case, inverse) - columns(want, case, inverse)).abs()
    return d.reshape(-1, d.shape[-1]).max(0).values / column_maxima(want, case, inverse)


def rel(a, b):
    """The global measure of test_gpu_parity.py."""
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
