"""The conditions that give the GPU bar of test_gpu_fft_sizes.py its meaning, checked on
the CPU for every case of fft_size_cases.py and both references:

* an exact fp32 implementation (the references restated in fp32: sht_ref modules
  .float(), torch's fp32 FFT) stays below a quarter of the GPU bar, per column and overall,
  so the bar leaves a kernel room for its own rounding and nothing more;
* every m column of the fp64 result has a maximum of at least COLUMN_FLOOR times the
  largest column maximum, so every FFT bin is visible in the result.  This is a condition
  on the inputs and holds for the reference alone."""
import pytest

import fft_size_cases as F

FP32_BAR = F.GPU_BAR / 4


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_forward_reference(case, kind):
    want = F.forward_reference(case, kind)
    cm = F.column_maxima(want, case, False)
    assert want.shape == (*F.LEAD, case.mmax, case.mmax)
    assert cm.min().item() >= F.COLUMN_FLOOR * cm.max().item(), (cm.min().item(), cm.max().item())
    got = F.fp32_forward(case, kind)
    col = F.column_errors(got, want, case, False).max().item()
    tot = F.rel(got.to(want.dtype), want)
    print(f"forward {kind} {case}: fp32 per-column {col:.2e} overall {tot:.2e} "
          f"column maxima {cm.min().item():.3f}..{cm.max().item():.3f}")
    assert col < FP32_BAR and tot < FP32_BAR, (col, tot)


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_inverse_reference(case, kind):
    want = F.inverse_reference(case, kind)
    cm = F.column_maxima(want, case, True)
    assert want.shape == (*F.LEAD, case.nlat, case.nlon)
    assert cm.min().item() >= F.COLUMN_FLOOR * cm.max().item(), (cm.min().item(), cm.max().item())
    got = F.fp32_inverse(case, kind)
    col = F.column_errors(got, want, case, True).max().item()
    tot = F.rel(got.double(), want)
    print(f"inverse {kind} {case}: fp32 per-column {col:.2e} overall {tot:.2e} "
          f"column maxima {cm.min().item():.3f}..{cm.max().item():.3f}")
    assert col < FP32_BAR and tot < FP32_BAR, (col, tot)
