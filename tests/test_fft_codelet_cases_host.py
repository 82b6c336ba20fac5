"""The conditions that give the GPU bars of test_gpu_fft_codelets.py their meaning, checked
on the CPU for every case of fft_codelet_cases.py (none is skipped or left out of a measure):

* stand-alone cases, the multi-trip ones included (built for a 256-CU device): an exact fp32
  implementation (the reference restated in fp32) stays at or below FP32_BAR = GPU_BAR / 2
  per column, and every column's maximum is at least COLUMN_FLOOR of the largest, so no bin
  hides behind another;
* block cases: every dense table meets check_symmetry_kernel's rule exactly (the folded
  Legendre layout runs), the fp32 oracle differs from the fp64 one (e32 > 0), and scaling one
  Fourier bin (order m = 1, all degrees) of one batch element's forward coefficients by 1.001
  inside the fp64 oracle moves its output by at least 4 times the case's bar, so the bar can
  fail (test_legendre_cases_host.py's condition, on a bin instead of an (m, parity) block);
  where the spectrum is full (lmax = mmax) the same holds for bin mmax - mmax // 6, which
  lies in the last KiB of spectrum the inverse FFT stages per row (in the one before it at
  mmax 383 and 511, where the last KiB holds the final bin alone);
* the mirrored launch arithmetic gives the row counts the multi-trip cases need."""
import pytest
import torch

import fft_codelet_cases as K
import fft_size_cases as F
import legendre_cases as L

TRIP_CASES = [K.trip_case(k, n, m, t, K.MI355X_CUS) for k, n, m, t in K.TRIPS]
ALL = K.CASES + TRIP_CASES
ALL_IDS = K.IDS + K.TRIP_IDS
# (case, kind): both kinds of every case, the dense kind of the one-row cases
PAIRS = [(c, k) for c in ALL for k in K.KINDS] + [(c, k) for c in K.ROW1_CASES for k in K.ROW1_KINDS]
PAIR_IDS = [f"{i}-{k}" for i in ALL_IDS for k in K.KINDS] + [f"{i}-{k}" for i in K.ROW1_IDS
                                                             for k in K.ROW1_KINDS]


@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_forward_reference(case, kind):
    want = F.forward_reference(case, kind)
    assert want.shape == (*case.lead, case.mmax, case.mmax)
    l_lt_m = torch.arange(case.mmax)[:, None] < torch.arange(case.mmax)[None, :]
    assert (want[..., l_lt_m] == 0).all()
    col = F.column_errors(F.fp32_forward(case, kind), want, case, False)
    cmax = F.column_maxima(want, case, False)
    assert col.shape == cmax.shape == (case.mmax,)
    print(f"forward {kind} {K.case_id(case)}: fp32 restatement per-column "
          f"{col.max().item():.2e}, smallest column {(cmax.min() / cmax.max()).item():.2f}")
    assert col.max().item() <= K.FP32_BAR, col
    assert cmax.min() >= F.COLUMN_FLOOR * cmax.max(), cmax


@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_inverse_reference(case, kind):
    want = F.inverse_reference(case, kind)
    assert want.shape == (*case.lead, case.nlat, case.nlon)
    col = F.column_errors(F.fp32_inverse(case, kind), want, case, True)
    cmax = F.column_maxima(want, case, True)
    assert col.shape == cmax.shape == (case.mmax,)
    print(f"inverse {kind} {K.case_id(case)}: fp32 restatement per-column "
          f"{col.max().item():.2e}, smallest column {(cmax.min() / cmax.max()).item():.2f}")
    assert col.max().item() <= K.FP32_BAR, col
    assert cmax.min() >= F.COLUMN_FLOOR * cmax.max(), cmax


@pytest.mark.parametrize("kernel,nlon,mmax,trips", K.TRIPS, ids=K.TRIP_IDS)
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_trip_case_goes_round(kernel, nlon, mmax, trips, cus):
    c = K.trip_case(kernel, nlon, mmax, trips, cus)
    full = K.grid_rows(kernel, nlon, mmax, cus)
    rows = K.rows_of(c)
    assert (trips - 1) * full < rows <= (trips - 1) * full + c.nlat
    assert rows * c.nlon * 4 < 32 << 20          # the field stays under 32 MB (10 at nlon 32)


@pytest.mark.parametrize("case", K.BLOCK_CASES, ids=K.BLOCK_IDS)
def test_block_bar_can_fail(case):
    for inverse in (False, True):
        t = L.table(case, inverse)
        assert t.shape == (case.mmax, case.lmax, case.nlat)
        assert L.is_symmetric(t) and L.is_symmetric(t.float())
    want = L.block_reference(case)
    assert want.shape == (case.B, case.C, case.nlat, case.nlon) and torch.isfinite(want).all()
    e32, bar = L.block_e32(case), L.block_bar(case)
    shift = L.block_mutation_shift(case, L.MUTATED_BIN)
    print(f"block {K.block_id(case)} ({K.block_c2r_kernel(case)}): |want|max "
          f"{want.abs().max().item():.3f} e32 {e32:.2e} bar {bar:.2e} a {L.MUTATION} bin "
          f"moves it by {shift:.2e} = {shift / e32:.0f} e32")
    assert e32 > 0
    assert shift >= L.MUTATION_MARGIN * bar, (shift, bar)
    if case.lmax == case.mmax:            # (the linear filter at 1440 has no degree up there)
        kib, last = (8 * case.wave_hi + 8) // 1024, K.c2r_ncy(case.mmax) - 1
        assert kib >= last - 1 and (kib == last or 128 * last >= case.mmax - 1), (kib, last)
        hi = L.block_mutation_shift(case, (case.wave_hi, None))
        print(f"  bin {case.wave_hi}, in KiB {kib} of 0 .. {last} staged: {hi:.2e} = "
              f"{hi / e32:.0f} e32")
        assert hi >= L.MUTATION_MARGIN * bar, (hi, bar)


def test_offset_case_is_ill_conditioned():
    """The offset case's input channels, and with the identity skip its pre-norm1 state, have
    |mean| of 30 .. 100 standard deviations."""
    x = L.block_input(K.OFFSET)
    r = x.mean((-2, -1)).abs() / x.std((-2, -1))
    assert r.min() > 25 and r.max() < 110, r
