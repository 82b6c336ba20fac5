"""The conditions that give the GPU bars of test_gpu_spectral_mlp.py their meaning, checked
on the CPU for the cases of spectral_mlp_cases.py:

* the layout mirror reproduces SpecLayout::build at the pairs worked out by hand;
* the table crosses every threshold its comments claim (depths, both chains, both engines
  of the 3M chain, k-tile remainders, ragged and exact row tiles, column-tile counts, the
  508 / 512 tile products, an order without degrees);
* every case's fp64 output has 0.1 <= |y|max <= 100, so the bar's floor 1e-6 max(1, |y|max)
  is a relative bound of 1e-5 at the worst;
* the layer-by-layer restatement of the oracle equals the oracle bit for bit, and with one
  fault injected (spectral_mlp_cases.faults) it misses the GPU bar even with its deviation
  divided by MUTATION_MARGIN: the bar would catch each of these faults."""
import pytest
import torch

import spectral_mlp_cases as M
from test_gpu_ring_refill import _bar


@pytest.mark.parametrize("lmax,mmax,Tp", [(3, 4, 40), (8, 9, 120), (12, 13, 184), (12, 6, 96),
                                          (5, 9, 72), (24, 25, 496)])
def test_layout_mirror(lmax, mmax, Tp):
    L = M.spec_layout(lmax, mmax)
    assert L.Tp == Tp and L.ldT == M.round_up(max(Tp, 8), 8)
    assert L.T == sum(max(lmax - m, 0) for m in range(mmax))
    modes = [lm for lm in M.column_modes(lmax, mmax) if lm is not None]
    assert len(modes) == L.T == len(set(modes))
    assert set(modes) == {(l, m) for m in range(mmax) for l in range(m, lmax)}


def test_table_crosses_what_it_claims():
    cs = M.CASES
    assert {1, 2, 4, 8} <= {c.layers for c in cs}
    # both engines of the 3M chain, and a case within one bit on either side of the range test
    assert {M.engine_of(c.C, M.hidden(c), c.layers) for c in cs} == {"x3h", "x6c", "x6p"}
    bits = [M.x3h_range_bits(c.C, M.hidden(c), c.layers) for c in cs
            if M.chain_of(c.C, M.hidden(c)) == "3m"]
    assert any(M.X3H_RANGE_BITS - 1 < b <= M.X3H_RANGE_BITS for b in bits)
    assert any(M.X3H_RANGE_BITS < b <= M.X3H_RANGE_BITS + 1 for b in bits)
    assert M.x3h_range_bits(256, 512, 3) == 16.0     # the flagship block stays on x3h
    assert {M.chain_of(c.C, M.hidden(c)) for c in cs} == {"3m", "4m"}
    assert any(M.hidden(c) == c.C for c in cs)
    dims = [d for c in cs for d in M.layer_dims(c)]
    assert {ci % M.X6C_BK for ci, _ in dims} >= {0, 4, 8, 12}
    assert any(ci < M.X6C_BK for ci, _ in dims) and any(M.k_tiles(ci) >= 4 for ci, _ in dims)
    for bm in (M.X6C_BM, M.X3C_BM64):
        assert any(co % bm == 0 for _, co in dims)
        assert any(co > bm and co % bm for _, co in dims)
    assert (136, 68) in dims and (68, 136) in dims
    assert {M.col_tiles(M.layout(c).Tp) for c in cs} >= {1, 2, 4}
    assert any(M.layout(c).Tp < 64 for c in cs)
    assert any(M.layout(c).Tp % M.X6C_BN == 0 for c in cs) == (M.TP128 is not None)
    assert any(c.mmax > c.lmax + 1 for c in cs) and any(c.mmax < c.lmax for c in cs)
    assert {c.B for c in cs} >= {1, 2, 3}
    lo, hi = M.BOUNDARY
    assert set(M.tile_products(lo)) == {508} and set(M.tile_products(hi)) == {512}
    assert all(M.bm64(co, M.layout(lo).Tp, lo.B) for _, co in M.layer_dims(lo))
    assert not any(M.bm64(co, M.layout(hi).Tp, hi.B) for _, co in M.layer_dims(hi))
    assert all(p < M.BM64_TILES for c in cs if c not in M.BOUNDARY for p in M.tile_products(c))
    for sub in (M.WORKSPACE_CASES, M.ENGINE_CASES):
        assert all(c in cs for c in sub)


def test_a_batch_is_a_prefix_of_a_larger_one():
    lo, hi = M.BOUNDARY
    assert torch.equal(M.input_of(hi)[:lo.B], M.input_of(lo))
    assert all(torch.equal(a, b) for a, b in zip(M.weights(lo)[0], M.weights(hi)[0]))
    assert torch.equal(M.want64(hi)[:lo.B], M.want64(lo))


@pytest.mark.parametrize("case", M.CASES, ids=M.IDS)
def test_output_is_of_order_one(case):
    want = M.want64(case)
    assert want.shape == (case.B, case.C, case.nlat, case.nlon) and torch.isfinite(want).all()
    ymax = want.abs().max().item()
    e32 = (M.want32(case) - want).abs().max().item()
    print(f"{M.case_id(case)}: |y|max {ymax:.3f}  e32 {e32:.3e}")
    assert 0.1 <= ymax <= 100.0
    assert e32 > 0


@pytest.mark.parametrize("case", M.CASES, ids=M.IDS)
def test_bar_catches_every_fault(case):
    want, w32 = M.want64(case), M.want32(case)
    assert torch.equal(M.chain(case), want)
    fs = M.faults(case)
    assert fs
    for f in fs:
        got = M.chain(case, f)
        shrunk = want + (got - want) / M.MUTATION_MARGIN
        with pytest.raises(AssertionError):
            _bar(shrunk, want, w32, f"{M.case_id(case)} {f.kind}@{f.layer} / {M.MUTATION_MARGIN}")


def test_every_fault_kind_is_shown_somewhere():
    kinds = {f.kind for c in M.CASES for f in M.faults(c)}
    assert kinds == {"ktail", "rowtail", "skip", "relu_imag", "stale", "coltail"}
    # a stale read of layer 0's input needs Hs = C (the factor-1 case)
    assert any(f == M.Fault("stale", 0) for c in M.HIDDEN for f in M.faults(c))
