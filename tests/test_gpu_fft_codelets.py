"""The compiled-codelet row FFTs (csrc/fft.hip: fft_r2c_dma_kernel, the eight
fft_c2r_dma_kernel instantiations, and the FFT1440 / FFT180 codelets under the
register-prefetch row kernels) over mmax, row count and kernel variant.
fft_codelet_cases.py has the cases, the mirrored launch arithmetic and the references;
test_fft_codelet_cases_host.py the conditions that give the bars their meaning.

Bars, both the project's: fft_size_cases.GPU_BAR (2e-6) per column m for the transforms,
legendre_cases.block_bar for the blocks.

Measured on an MI355X (256 CUs), worst per-column error in units of 1e-7, with the fp32
restatement's error on the same inputs in parentheses; 15 fields of nlat 3 (1440), 5 (240,
32), 7 (180, 48) and 9 (64) latitudes.  The worst, 5.9e-7 (inverse, grid, 1440, mmax 720), is
3.4 times under the bar of 2e-6; no step of ncy, of the forward store count or of the inverse
kernel (mmax 638 -> 639 at 1440) shows in the figures.

  nlon mmax |  forward grid     forward dense  |  inverse grid     inverse dense
  1440    1 |   1.1 (0.8)       0.8 (1.2)     |   3.3 (0.6)       0.7 (0.7)
  1440    2 |   1.9 (1.8)       1.6 (1.7)     |   1.7 (0.5)       1.6 (0.6)
  1440   64 |   3.3 (2.4)       3.7 (2.7)     |   3.0 (1.6)       2.2 (1.4)
  1440   65 |   3.4 (2.5)       3.7 (2.9)     |   3.4 (1.6)       3.1 (1.5)
  1440  126 |   3.5 (2.8)       4.7 (2.6)     |   3.8 (1.9)       3.2 (1.7)
  1440  127 |   3.9 (2.7)       3.8 (2.7)     |   3.8 (2.1)       3.1 (1.8)
  1440  128 |   4.5 (3.0)       4.4 (2.9)     |   4.1 (1.9)       2.7 (1.8)
  1440  129 |   3.8 (2.7)       3.6 (2.3)     |   3.6 (1.9)       3.5 (1.9)
  1440  240 |   4.0 (2.9)       4.1 (2.7)     |   3.6 (2.6)       3.6 (2.2)
  1440  241 |   4.7 (2.9)       3.6 (3.1)     |   4.0 (3.2)       3.4 (2.0)
  1440  254 |   4.2 (3.3)       3.6 (2.6)     |   4.3 (2.3)       3.6 (2.0)
  1440  255 |   4.2 (2.9)       3.7 (2.8)     |   4.5 (2.5)       3.8 (2.1)
  1440  382 |   5.1 (2.8)       3.8 (2.9)     |   4.7 (3.4)       3.9 (2.2)
  1440  383 |   4.1 (3.6)       3.8 (3.1)     |   5.2 (3.4)       4.3 (2.6)
  1440  510 |   4.2 (3.4)       4.3 (2.8)     |   5.6 (3.5)       4.1 (3.1)
  1440  511 |   4.2 (2.9)       4.1 (2.9)     |   5.5 (3.6)       3.6 (2.8)
  1440  638 |   4.6 (3.0)       4.6 (3.2)     |   5.4 (4.0)       4.3 (3.3)
  1440  639 |   4.0 (3.6)       4.6 (3.2)     |   5.4 (3.7)       4.7 (3.0)
  1440  720 |   5.4 (3.6)       5.5 (2.9)     |   5.9 (4.4)       5.0 (2.9)
  1440  721 |   5.2 (3.2)       4.1 (3.1)     |   5.7 (4.7)       4.5 (3.2)
   240    1 |   1.5 (1.0)       1.6 (1.6)     |   2.3 (0.8)       1.8 (0.3)
   240    2 |   2.0 (1.3)       1.1 (2.0)     |   1.2 (0.9)       1.6 (0.8)
   240   40 |   4.9 (3.0)       2.7 (2.5)     |   3.3 (1.7)       3.4 (1.6)
   240   41 |   4.1 (2.9)       2.3 (2.8)     |   3.1 (1.7)       2.7 (1.5)
   240   64 |   3.0 (2.5)       2.8 (2.6)     |   4.1 (2.3)       3.4 (1.8)
   240   65 |   4.2 (2.9)       3.4 (2.8)     |   3.5 (2.5)       2.9 (1.7)
   240  120 |   3.2 (2.8)       2.9 (2.7)     |   4.1 (3.3)       3.3 (2.4)
   240  121 |   3.0 (3.1)       2.9 (2.6)     |   4.1 (3.0)       3.2 (2.4)
   180    1 |   1.8 (1.2)       2.4 (1.3)     |   3.0 (0.7)       1.4 (0.4)
   180    2 |   2.9 (1.4)       1.8 (1.3)     |   1.9 (0.9)       1.7 (0.8)
   180   30 |   2.9 (2.4)       2.8 (2.6)     |   3.3 (1.9)       3.2 (1.6)
   180   31 |   3.5 (2.7)       2.7 (2.3)     |   3.2 (1.9)       3.0 (1.5)
   180   90 |   3.6 (2.4)       2.9 (2.8)     |   3.8 (3.2)       3.5 (2.4)
   180   91 |   3.4 (2.1)       2.8 (2.5)     |   4.3 (3.6)       3.1 (2.2)
    64    1 |   0.7 (2.1)       0.8 (1.0)     |   3.1 (0.7)       0.6 (0.6)
    64    2 |   1.4 (2.0)       1.9 (1.5)     |   1.4 (0.6)       1.5 (0.9)
    64   10 |   2.4 (1.6)       2.5 (1.5)     |   3.3 (1.4)       2.7 (1.3)
    64   11 |   1.8 (1.5)       2.0 (1.6)     |   2.2 (1.6)       2.3 (1.1)
    64   32 |   2.4 (2.0)       2.8 (1.6)     |   3.5 (1.9)       2.9 (1.6)
    64   33 |   3.2 (1.4)       2.2 (1.8)     |   3.1 (2.1)       2.9 (2.0)
    48    1 |   1.5 (1.2)       1.6 (0.8)     |   2.4 (0.6)       0.9 (0.5)
    48    2 |   1.3 (1.7)       1.4 (1.7)     |   2.6 (0.8)       1.8 (1.0)
    48    8 |   2.2 (1.5)       1.8 (1.5)     |   2.1 (1.3)       2.3 (1.4)
    48    9 |   1.8 (1.6)       1.8 (2.3)     |   2.2 (1.7)       3.2 (1.4)
    48   24 |   2.4 (1.8)       2.0 (2.0)     |   3.5 (2.2)       2.6 (2.0)
    48   25 |   2.6 (2.4)       2.6 (2.3)     |   3.1 (2.2)       2.6 (1.8)
    32    1 |   1.2 (1.0)       1.1 (1.1)     |   1.9 (0.7)       1.7 (0.4)
    32    2 |   2.5 (1.5)       1.4 (1.1)     |   1.7 (0.6)       1.3 (0.6)
    32    5 |   2.3 (1.2)       2.0 (2.1)     |   2.4 (1.4)       1.5 (0.9)
    32    6 |   1.6 (1.3)       1.7 (1.5)     |   2.6 (1.2)       2.4 (1.1)
    32   16 |   2.1 (1.4)       2.5 (1.2)     |   3.8 (1.7)       2.6 (1.5)
    32   17 |   3.6 (1.3)       2.2 (1.4)     |   3.6 (2.1)       2.7 (2.1)

  H + 1 with 12 fields (an even row count), all six widths        2.3 .. 5.7 (1.3 .. 4.1)
  3, 5, 11 and 13 rows at nlon 32 (mmax 5) and 48 (mmax 9)        1.1 .. 4.8 (0.5 .. 2.9)
  one row (one latitude, dense only) at nlon 32 and 48            1.4 .. 4.5 (0.6 .. 5.5)
  second and third trips, 3078 .. 67596 rows (dense only)         1.9 .. 4.4 (1.3 .. 5.7)

Block cases, max-abs error against the fp64 oracle in units of e32 (the fp32 oracle's own
distance; bar 8): 0.30 .. 1.45 over the 27 cases without offset.  The offset case (|mean| 30
.. 100 standard deviations ahead of norm1) comes to 7.86: 3.83e-5 absolute against a bar of
3.90e-5 (3.46e-5 or 3.83e-5 under the variants).  It is the tightest case of the file, and by design
rather than by the FFT: norm1 is applied as one affine x * scale + shift per channel, and
with |mean| = 100 sigma both terms are some 50 times the result, so each of their roundings
costs 2^-24 * 50, where the oracle subtracts the mean first.  A batch of two is bit-identical
to two batches of one, and every multi-trip case to its second run.

Kernels reached (rocprofv3 --kernel-trace of this file; the variants' child processes traced
one by one, the tracer did not follow them): fft_r2c_dma_kernel<CL, 12, false, 2> and, under
MSFNO_SKIP_PLANES=1, <CL, 12, true, 2>; fft_c2r_dma_kernel<CL, ADD, WV, 1, PL, AR, SWI> as
<false, 4, false>, <false, 4, true>, <true, 4, false>, <true, 4, true>, <true, 16, false,
AR> and <true, 16, true, AR> in this process, <true, 10, true> under MSFNO_C2R_AREG=0 and
<true, 12, false, AR, SWI> under MSFNO_C2R_SWZ=1, each of the eight with CL = FFT1440, FFT240
and FFT64; fft_r2c_rows_kernel / fft_c2r_rows_kernel with FFT180 (always) and FFT1440 (the
inverse from mmax 639, both under MSFNO_FFT_DMA=0).  None is unreachable.

No bug was found: every case passed on the first run.

What the sweep catches, tried on scratch builds of fft.hip (each against this whole file as
it stood before the one-row cases were added, 364 tests):
* the clamp of issue_y as it was before the Legendre sweep's fix (the last chunk wholly inside
  Yn): 58 tests fail, the 29 cases with an odd count of spectrum values that run a DMA
  inverse, on the dense table in the parity test and in the C ABI one (on the grid the last
  row is a pole, where the reference has the same value two bins earlier or none at all);
* the inverse kernels told ncy - 1 (one KiB of spectrum a row too few staged): 164 fail (100
  inverse parity, 36 C ABI, 4 multi-trip, 18 block cases and 6 of the 7 variants);
* nst of fft_r2c_dma_kernel with mmax / 64 instead of ceil(mmax / 64): none fails, and none
  can.  The count is what the wave issued after the copy it waits for; too small a count only
  makes s_waitcnt vmcnt wait for more than it needs.  The harmful direction is a count that
  is too large: with mmax / 64 + 1 (one too many at mmax 64 and 128) the multi-trip cases at
  1440 and 240, mmax 64 / 65 / 128 / 129, also passed, twice bit-equal: that count lets at
  most the last 1-KiB piece of a row's copy stay in flight, and it had landed every time.
  The sweep does not catch an nst that is one too large.
"""
import json
import os
import subprocess
import sys
from functools import partial

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":             # a variant's child process: no conftest sets the path
    for _p in (HERE, os.path.dirname(HERE),
               os.path.join(os.path.dirname(HERE), "modulated-spherical-fourier-neural-operator_amd")):
        sys.path.insert(0, _p)

import fft_codelet_cases as K  # noqa: E402
import fft_size_cases as F  # noqa: E402
import legendre_cases as L  # noqa: E402
from test_gpu_legendre_shapes import _global_conv_abi, _sht  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- stand-alone transforms ----------------------------------------------------------
def _module(cls, case, kind):
    """The native transform of `case`; for the dense reference with the synthetic table in
    place of its own."""
    from msfno_amd import harmonics as H
    # (one latitude: the equiangular rule needs two; the dense table replaces the grid's)
    assert case.nlat > 1 or kind == "dense"
    mod = getattr(H, cls)(case.nlat, case.nlon, lmax=case.mmax, mmax=case.mmax,
                          grid="equiangular" if case.nlat > 1 else "legendre-gauss").float()
    if kind == "dense":
        if cls == "RealSHT":
            mod.weights = F.dense_table(case, False).float()
        else:
            mod.pct = F.dense_table(case, True).float()
    return mod.to(DEV)


def _kernels(case):
    if not K.is_dma(case.nlon, case.mmax):
        return "r2c rows / c2r rows"
    return f"r2c dma / c2r {K.c2r_kernel(case.nlon, case.mmax, False, False)[0]} ncy {K.c2r_ncy(case.mmax)}"


def _check_forward(case, kind, got):
    want = F.forward_reference(case, kind)
    assert got.shape == want.shape and got.dtype == torch.complex64
    assert torch.isfinite(torch.view_as_real(got)).all()
    col = F.column_errors(got, want, case, False)
    tot = F.rel(got.to(torch.complex128), want)
    ref = F.column_errors(F.fp32_forward(case, kind), want, case, False).max().item()
    print(f"forward {kind} {K.case_id(case)} ({_kernels(case)}): per-column "
          f"{col.max().item():.2e} at m = {col.argmax().item()} overall {tot:.2e} "
          f"(fp32 restatement per-column {ref:.2e})")
    assert col.max().item() < K.GPU_BAR and tot < K.GPU_BAR, (col, tot)
    # structural zeros l < m are exact
    l_lt_m = torch.arange(case.mmax)[:, None] < torch.arange(case.mmax)[None, :]
    assert (got[..., l_lt_m] == 0).all()


def _check_inverse(case, kind, got):
    want = F.inverse_reference(case, kind)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    col = F.column_errors(got, want, case, True)
    tot = F.rel(got.double(), want)
    ref = F.column_errors(F.fp32_inverse(case, kind), want, case, True).max().item()
    print(f"inverse {kind} {K.case_id(case)} ({_kernels(case)}): per-column "
          f"{col.max().item():.2e} at m = {col.argmax().item()} overall {tot:.2e} "
          f"(fp32 restatement per-column {ref:.2e})")
    assert col.max().item() < K.GPU_BAR and tot < K.GPU_BAR, (col, tot)


def _inverse_input(case, kind):
    a = F.inverse_input(case, kind)
    nyq = case.nlon // 2 if case.mmax > case.nlon // 2 else 0
    # the imaginary parts irfft ignores are not zero
    assert a[..., 0, 0].imag.abs().min() > 0 and a[..., nyq, nyq].imag.abs().min() > 0
    return a.to(DEV)


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_forward_matches_reference(case, kind):
    got = _module("RealSHT", case, kind)(F.forward_input(case).to(DEV)).cpu()
    _check_forward(case, kind, got)


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_inverse_matches_reference(case, kind):
    got = _module("InverseRealSHT", case, kind)(_inverse_input(case, kind)).cpu()
    _check_inverse(case, kind, got)


@pytest.mark.parametrize("kind", K.ROW1_KINDS)
@pytest.mark.parametrize("case", K.ROW1_CASES, ids=K.ROW1_IDS)
def test_one_row(case, kind):
    """One field of one latitude: one workgroup in which only wave 0 has a row, and no second
    copy in flight.  Forward, and the inverse through the C ABI on a 0xFF workspace,
    bit-identical to the result on a zeroed one."""
    assert K.rows_of(case) == 1
    got = _module("RealSHT", case, kind)(F.forward_input(case).to(DEV)).cpu()
    _check_forward(case, kind, got)
    mod, a = _module("InverseRealSHT", case, kind), _inverse_input(case, kind)
    _check_inverse(case, kind, mod(a).cpu())
    dirty, clean = _sht(mod, a, 0xFF), _sht(mod, a, 0x00)
    _check_inverse(case, kind, dirty.cpu())
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))


@pytest.mark.parametrize("case", K.ABI_CASES, ids=K.ABI_IDS)
def test_inverse_ignores_what_the_workspace_held(case):
    """msfno_sht_inverse on a workspace of 0xFF bytes (NaN as floats) with a guard behind it
    and a NaN-filled output: within the bar, and bit-identical to the result on a zeroed
    workspace.  A chunk staged from beyond the row, or a bin k >= mmax that reaches the FFT,
    shows up here."""
    mod, a = _module("InverseRealSHT", case, "dense"), _inverse_input(case, "dense")
    dirty, clean = _sht(mod, a, 0xFF), _sht(mod, a, 0x00)
    _check_inverse(case, "dense", dirty.cpu())
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))


@pytest.mark.parametrize("kernel,nlon,mmax,trips", K.TRIPS, ids=K.TRIP_IDS)
def test_grid_stride_loop_goes_round(kernel, nlon, mmax, trips):
    """Row counts at which some wave of fft_r2c_dma_kernel (12 waves, one workgroup a CU) or
    of the stand-alone inverse's 4-wave fft_c2r_dma_kernel makes a second and a third trip:
    the `(i >= 1 ? nst : 0)` accounting of wait_vmcnt and the refill of a consumed slot.  Run
    twice: a miscounted vmcnt is a race, which a single run may pass."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = K.trip_case(kernel, nlon, mmax, trips, cus)
    rows, full = K.rows_of(case), K.grid_rows(kernel, nlon, mmax, cus)
    assert rows > (trips - 1) * full, (rows, full, cus)
    print(f"{kernel} nlon {nlon} mmax {mmax}: {cus} CUs, {full} rows a trip, {rows} rows")
    if kernel == "r2c":
        mod, x = _module("RealSHT", case, "dense"), F.forward_input(case).to(DEV)
        got, again = mod(x), mod(x)
        assert torch.equal(torch.view_as_real(got).view(torch.int32),
                           torch.view_as_real(again).view(torch.int32))
        _check_forward(case, "dense", got.cpu())
    else:
        mod, a = _module("InverseRealSHT", case, "dense"), _inverse_input(case, "dense")
        got, again = mod(a), mod(a)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        _check_inverse(case, "dense", got.cpu())


# ---- blocks ----------------------------------------------------------------------------
def _block(c, params=None):
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno import FourierNeuralOperatorBlock_Filmed
    sht = RealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    isht = InverseRealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    sht.weights = L.table(c, False).float()
    isht.pct = L.table(c, True).float()
    norm = partial(torch.nn.InstanceNorm2d, num_features=c.C, eps=1e-6, affine=True,
                   track_running_stats=False)
    blk = FourierNeuralOperatorBlock_Filmed(sht, isht, c.C, filter_type=c.filter, mlp_ratio=2.0,
                                            norm_layer=(norm, norm), inner_skip=c.skip,
                                            outer_skip=None,
                                            mlp_mode="distributed" if c.mlp else "none",
                                            spectral_layers=3)
    missing, unexpected = blk.load_state_dict(params or L.block_params(c), strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith((".weights", ".pct")) for k in missing), missing
    assert hasattr(blk, "inner_skip") == (c.skip is not None) and hasattr(blk, "mlp") == c.mlp
    return blk.eval().to(DEV)


def _run_block(blk, c, x):
    """The whole block (FiLM with gamma = beta = 0: the identity) where the case has an MLP,
    global_conv(x, x) where it has none."""
    with torch.no_grad():
        if c.mlp:
            gamma, beta = (t.to(DEV) for t in K.block_zero_film(c))
            return blk(x, gamma[:x.shape[0]], beta[:x.shape[0]], 1.0)
        return blk.global_conv(x, x)


def _block_error(c, oracle=None):
    """(max-abs error against the fp64 oracle, the case's bar); `oracle`: the case's
    (parameters, reference, bar) where another process has computed them."""
    params, want, bar = oracle or (L.block_params(c), L.block_reference(c), L.block_bar(c))
    got = _run_block(_block(c, params), c, L.block_input(c).to(DEV)).cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return (got.double() - want).abs().max().item(), bar


@pytest.mark.parametrize("case", K.BLOCK_CASES, ids=K.BLOCK_IDS)
def test_block_matches_oracle(case):
    err, bar = _block_error(case)
    e32 = L.block_e32(case)
    print(f"block {K.block_id(case)} ({K.block_c2r_kernel(case)}): max-abs {err:.2e} = "
          f"{err / e32:.2f} e32, bar {bar:.2e}")
    assert err <= bar, (err, bar, err / e32)


def test_block_workspace_holds_anything():
    """msfno_block_global_conv at 1440 / mmax 383 with the identity skip (the 4-wave kernel
    with the skip row staged by LDS-DMA in NCA = 6 pieces) on a workspace of 0xFF bytes: bit-
    identical to the result on a zeroed one, the guard behind it untouched."""
    case = next(c for c in K.BLOCK_CASES
                if K.block_c2r_kernel(c) == "dma<add,4>" and c.mmax == 383)
    blk, x = _block(case), L.block_input(case).to(DEV)
    dirty, clean = _global_conv_abi(blk, x, 0xFF), _global_conv_abi(blk, x, 0x00)
    assert torch.isfinite(dirty).all()
    err = (dirty.cpu().double() - L.block_reference(case)).abs().max().item()
    assert err <= L.block_bar(case), (err, L.block_bar(case))
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))


def test_batch_of_two_equals_two_batches_of_one():
    """The 1440 / mmax 383 block (plane output, 4-wave LDS-DMA-skip inverse): a batch of two
    is bit-identical to two calls with one field each."""
    c = K.BATCH2
    blk, x = _block(c), L.block_input(c).to(DEV)
    both = _run_block(blk, c, x)
    for b in range(c.B):
        one = _run_block(blk, c, x[b:b + 1].contiguous())
        assert torch.equal(one[0].view(torch.int32), both[b].view(torch.int32)), b


# ---- the switches that pick another row kernel, read once per process ---------------------
VARIANTS = [
    {"MSFNO_C2R_AREG": "0"},
    {"MSFNO_C2R_AREG": "0", "MSFNO_C2R_WV": "4"},
    {"MSFNO_C2R_SWZ": "1"},
    {"MSFNO_FFT_DMA": "0"},
    {"MSFNO_X1_PLANES": "0", "MSFNO_H_PLANES": "0"},
    {"MSFNO_SKIP_PLANES": "0"},
    # the forward kernel's plane output (fft_r2c_dma_kernel<.., true, 2>) is off by default
    {"MSFNO_SKIP_PLANES": "1"},
]


def _variant_errors(oracles):
    return {K.block_id(c): _block_error(c, oracles[K.block_id(c)]) for c in K.BLOCK_CASES}


@pytest.fixture(scope="module")
def oracle_file(tmp_path_factory):
    """Every block case's parameters (the filter balanced against the skip), fp64 reference
    and bar in one file: the seven children load it instead of running the fp64 and fp32
    oracles of all cases again (they are cached in this process)."""
    path = tmp_path_factory.mktemp("codelets") / "oracles.pt"
    torch.save({K.block_id(c): (L.block_params(c), L.block_reference(c), L.block_bar(c))
                for c in K.BLOCK_CASES}, path)
    return str(path)


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_variant_matches_oracle(env, oracle_file):
    """Every block case under one variant, in a fresh child process that prints one JSON line
    of (error, bar) per case; same bars."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), oracle_file],
                       env=dict(os.environ, **env), cwd=HERE, capture_output=True, text=True,
                       timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    errs = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(errs) == sorted(K.BLOCK_IDS)
    for k, (err, bar) in errs.items():
        print(f"{env} {k}: max-abs {err:.2e} bar {bar:.2e}")
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


if __name__ == "__main__":
    print(json.dumps(_variant_errors(torch.load(sys.argv[1]))))
