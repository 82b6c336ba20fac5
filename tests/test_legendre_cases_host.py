"""The conditions that give the GPU bars of test_gpu_legendre_shapes.py their meaning,
checked on the CPU for every case of legendre_cases.py:

* every dense table meets check_symmetry_kernel's rule exactly, in fp64 and after .float(),
  so the plan folds it and the register-resident kernels run;
* an exact fp32 implementation (the reference restated in fp32: fp32 table, fp32 einsum and
  FFT) stays at or below FP32_BAR = GPU_BAR / 2 per (m, parity) block of the forward result
  and per Fourier column of the inverse one, so the GPU bar leaves a kernel a factor 2 over
  it and no more;
* for every block case, scaling one (m, parity) block of one batch element's forward
  coefficients by 1.001 inside the fp64 oracle moves its output by at least 4 times that
  case's bar, so the bar can fail."""
import pytest
import torch

import legendre_cases as L


@pytest.mark.parametrize("case", [c for c in L.CASES + L.BLOCK_CASES if c.kind == "dense"],
                         ids=lambda c: L.block_id(c) if hasattr(c, "B") else L.case_id(c))
def test_dense_table_is_exactly_symmetric(case):
    for inverse in (False, True):
        t = L.table(case, inverse)
        assert t.shape == (case.mmax, case.lmax, case.nlat) and t.dtype == torch.float64
        assert L.is_symmetric(t) and L.is_symmetric(t.float())
        l_lt_m = torch.arange(case.lmax)[None, :] < torch.arange(case.mmax)[:, None]
        assert (t[l_lt_m] == 0).all() and (t[~l_lt_m].abs().amax(-1) > 0).all()


def test_a_perturbed_table_is_not_symmetric():
    t = L.symmetric_table(3, 5, 9, 1).clone()
    t[1, 2, 7] *= 1.5
    assert not L.is_symmetric(t)


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_forward_reference(case):
    want = L.forward_reference(case)
    assert want.shape == (*case.lead, case.lmax, case.mmax)
    blocks = L.forward_blocks(case)
    assert len(blocks) == sum(min(2, case.lmax - m) for m in range(min(case.mmax, case.lmax)))
    err = L.forward_block_errors(L.fp32_forward(case), want, case)
    assert sorted(err) == blocks
    worst = max(err.values())
    print(f"forward {L.case_id(case)}: fp32 restatement worst block {worst:.2e}")
    assert worst <= L.FP32_BAR, err


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_inverse_reference(case):
    want = L.inverse_reference(case)
    assert want.shape == (*case.lead, case.nlat, L.NLON)
    col = L.inverse_column_errors(L.fp32_inverse(case), want, case)
    assert col.shape == (min(case.mmax, case.lmax),)
    print(f"inverse {L.case_id(case)}: fp32 restatement worst column {col.max().item():.2e}")
    assert col.max().item() <= L.FP32_BAR, col


@pytest.mark.parametrize("case", L.BLOCK_CASES, ids=L.BLOCK_IDS)
def test_block_bar_can_fail(case):
    want = L.block_reference(case)
    assert torch.isfinite(want).all()
    e32, bar, shift = L.block_e32(case), L.block_bar(case), L.block_mutation_shift(case)
    print(f"block {L.block_id(case)}: |want|max {want.abs().max().item():.3f} e32 {e32:.2e} "
          f"bar {bar:.2e} a {L.MUTATION} block moves it by {shift:.2e} = {shift / e32:.0f} e32")
    assert e32 > 0
    assert shift >= L.MUTATION_MARGIN * bar, (shift, bar)
