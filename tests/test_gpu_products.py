"""Ensemble products and threshold counts on the GPU (csrc/ens_products.hip through the C-ABI,
msfno_amd/ensemble.py, EnsembleVerifier and Rollout.ensemble_products) against the fp64
restatement (tests/products_util.py).  Outputs and workspaces are pre-filled with NaN.

Shapes and member counts are those of tests/test_gpu_ensemble.py: M in {2, 3, 5, 8, 9, 16, 17,
32} (both sides of every register bucket) at slabs (S, H, W) where the kernels take another
path (a single element, rows shorter than a float4, slabs off the 16-byte grid, nlon % 4 != 0,
a row wider than one sweep), and the real 721 x 1440 rows at M = 4.  Inputs are 300 + N(0, 1)
members against a 300.5 + N(0, 1) truth; thresholds per slab from {296.0, 300.0, 300.7, 302.0}
(always, common, middling, rare); no member and no truth value sits on a threshold of its
slab (moved to the next fp32 value, asserted), a separate case pins strict > on deliberate
ties on both sides.  Levels {0, 0.1, 0.25, 0.5, 0.9, 1}.

Bounds (derived from the kernel's chains, u = 2^-24; the worst ratio per case is printed):
  min, max and every level whose frac is 0 (q = 0, 1, the median of odd M): torch.equal to the
    sorted fp32 members.  q = 1 at M in {3, 5, 9, 17} is the case that the +inf padding of the
    bucket breaks without the clamp hi <= M - 1.
  other levels: |got - want| <= 2 u max(|x_lo|, |x_hi|): one rounded difference and the
    rounded frac (relative u each on a term frac (x_hi - x_lo) that is far below the value),
    and one fma rounded at the magnitude of the value.
  mean: |got - want| <= u |want| + (M + 2) u (1/M) sum |x_i - x_0|: the final add at the
    field's magnitude; M - 1 rounded differences, M - 2 adds and the product with the rounded
    1 / M on the differences.  A raw-sum mean (M adds at 300 M) fails it.
  std: relative error <= (M + 10) u: per term a rounded difference, the subtraction of dm
    (itself within (M + 1) u), the fma chain of M terms (non-negative: relative M u on the
    sum, halved by the root), the product with the rounded 1 / (M - 1) and the root; exactly 0
    on equal members.
  prob: round(got M) is the integer count, and |got - k / M| <= 2 u (the rounded 1 / M and
    the product).
  counts: exactly 0 where the restatement is 0, 1e-5 relative elsewhere (integer counts per
    row and wave, the weighted adds a chain of <= 64 + 4 terms), as the rank histogram; the
    sum over k of counts[..., 0, :] is nlon sum(w) to the same bound.

Measured worst ratios to these bounds on the shapes above: quantiles 0.43, mean 0.86 (0.98 on
the fixture network's fields), std 0.20; counts 1.6e-7 relative.

What the tests catch (edits of csrc/ens_products.hip and of the host's level positions on
scratch builds, none of which can index out of bounds; the failing tests of this file in
brackets):
  - the mean as a raw sum times 1 / M: 11 tests [test_products_kernel at every M,
    test_std_is_zero_on_equal_members_and_the_mean_is_the_member,
    test_strict_greater_on_deliberate_ties, the fixture-network driver];
  - >= in place of > on the members (prob and counts): 1 test
    [test_strict_greater_on_deliberate_ties; the other inputs have no tie, by construction];
  - >= in place of > on the truth: 1 test [the same];
  - hi = lo + 1 unclamped: 12 tests [test_products_kernel at M = 2, 3, 5, 9, 17 (the level 1
    then reads the +inf padding: NaN), and every test that takes all levels at such an M:
    ties, optional outputs at 3 and 17, strides at 3 and 9, the band's maps at 17, the 17
    levels]; at M = 8, 16, 32 the bucket has no padding and hi = M selects nothing;
  - the third comparator of the network removed: 9 tests [test_products_kernel at every M
    but 5, the 17 levels, the fixture-network driver];
  - o taken from the member count (more than half above) instead of the truth: 15 tests
    [test_threshold_counts_kernel at every M, ties, the latitude split, the 11 thresholds,
    test_scores_from_gpu_counts, the graph and the driver tests].
"""
import functools

import pytest
import torch

import ensemble_util as EU
import products_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

MS = [2, 3, 5, 8, 9, 16, 17, 32]
SHAPES = [(1, 1, 1), (1, 2, 8), (2, 7, 9), (6, 5, 12), (3, 121, 250), (1, 3, 4100)]
BIG = (4, (2, 721, 1440))
NAMES = ("mean", "std", "min", "max", "quant", "prob")
ALL = frozenset(NAMES)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _products(ens, stride, M, shape, levels=PU.LEVELS, thr=None, want=ALL, bufs=None):
    """msfno_ens_products on device pointers (any 16-byte phase, any member stride) into
    NaN-filled outputs (or the views ``bufs``); a dict of the outputs, None if not wanted."""
    import ctypes
    from msfno_amd import _native as N
    S, H, W = shape
    nq, nt = len(levels), 0 if thr is None else thr.shape[1]
    lead = dict(quant=(nq,), prob=(nt,))
    out = {k: None for k in NAMES}
    for k in want:
        out[k] = bufs[k] if bufs else _nan(*lead.get(k, ()), S, H, W)
    q = (ctypes.c_double * max(1, nq))(*levels)
    o = N.EnsProductsOut(**{k: N.ptr(v) for k, v in out.items()})
    N.check(N.lib().msfno_ens_products(ens.data_ptr(), stride, q, nq, N.ptr(thr), nt,
                                       ctypes.byref(o), M, S, H, W, N.stream_of(ens.device)),
            "msfno_ens_products")
    return out


def _counts(ens, stride, tar, w, thr, M, shape, ws_fill=float("nan")):
    """msfno_ens_threshold_sums on device pointers; NaN-filled counts, a workspace full of
    ``ws_fill``."""
    from msfno_amd import _native as N
    S, H, W = shape
    nt = thr.shape[1]
    lib = N.lib()
    nbytes = lib.msfno_ens_threshold_workspace_size(S, M, nt, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), ws_fill, dtype=torch.float32, device=DEV)
    counts = _nan(S, nt, 2, M + 1)
    N.check(lib.msfno_ens_threshold_sums(ens.data_ptr(), stride, tar.data_ptr(), w.data_ptr(),
                                         thr.data_ptr(), nt, counts.data_ptr(), M, S, H, W,
                                         ws.data_ptr(), nbytes, N.stream_of(ens.device)),
            "msfno_ens_threshold_sums")
    return counts


@functools.lru_cache(maxsize=None)
def _gpu(M, shape):
    """The kernels' products (all of them, on the device) and counts (fp64, host) of
    PU.problem(M, shape)."""
    ens, tar, w, thr = PU.problem(M, shape)[:4]
    S, H, W = shape
    e, t = ens.to(DEV), thr.to(DEV)
    return (_products(e, S * H * W, M, shape, thr=t),
            _counts(e, S * H * W, tar.to(DEV), w.to(DEV), t, M, shape).cpu().double())


def _check_products(tag, got, ens, thr, srt, levels=PU.LEVELS):
    """Every wanted output of ``got`` against the members ens (M, S, H, W) fp32 (host), the
    thresholds (S, nt) and the sorted members."""
    M = ens.shape[0]
    e64, s64 = ens.double(), srt.double()
    worst = {}
    for k, v in got.items():
        if v is not None:
            assert torch.isfinite(v).all(), (tag, k)
    if got["min"] is not None:
        assert torch.equal(got["min"].cpu(), srt[0]), tag
        assert torch.equal(got["max"].cpu(), srt[M - 1]), tag
    if got["quant"] is not None:
        for l, q in enumerate(levels):
            want, xlo, xhi, frac = PU.quantile(s64, q)
            g = got["quant"][l].cpu()
            if frac == 0:
                assert torch.equal(g, srt[PU.position(q, M)[0]]), (tag, q)
            else:
                bound = 2 * U * torch.maximum(xlo.abs(), xhi.abs())
                err = (g.double() - want).abs()
                worst["quant"] = max(worst.get("quant", 0.0), (err / bound).max().item())
                assert (err <= bound).all(), (tag, q, worst)
    if got["mean"] is not None:
        want = e64.mean(dim=0)
        bound = U * want.abs() + (M + 2) * U * (e64 - e64[:1]).abs().mean(dim=0)
        err = (got["mean"].cpu().double() - want).abs()
        worst["mean"] = (err / bound).max().item()
        assert (err <= bound).all(), (tag, worst)
    if got["std"] is not None:
        want = e64.std(dim=0, unbiased=True)
        err = (got["std"].cpu().double() - want).abs()
        worst["std"] = (err / ((M + 10) * U * want)).max().item()
        assert (err <= (M + 10) * U * want).all(), (tag, worst)
        assert (want > 0).all()
    if got["prob"] is not None:
        k = PU.exceed(ens, thr)
        p = got["prob"].cpu().double()
        assert torch.equal((p * M).round().long(), k), tag
        assert ((p - k.double() / M).abs() <= 2 * U).all(), tag
    print(f"{tag}: worst error / bound " +
          ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


def _check_counts(tag, got, want, w=None, nlon=None):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    assert (got[want == 0] == 0).all(), tag
    err = (got - want).abs()
    print(f"{tag}: counts max relative err "
          f"{(err / want.clamp(min=1e-300))[want > 0].max().item():.3e}")
    assert (err <= 1e-5 * want).all(), tag
    if w is not None:
        n = nlon * w.double().sum()
        total = got[..., 0, :].sum(dim=-1)
        assert ((total - n).abs() <= 1e-5 * n).all(), tag


def _cases(M):
    return [(M, s) for s in SHAPES] + ([BIG] if M == 2 else [])


@pytest.mark.parametrize("M", MS)
def test_products_kernel(M):
    """(The 721 x 1440 case at M = 4 rides with M = 2.)"""
    for m, shape in _cases(M):
        ens, _, _, thr, srt, _ = PU.problem(m, shape)
        _check_products(f"M={m} {shape}", _gpu(m, shape)[0], ens, thr, srt)


@pytest.mark.parametrize("M", MS)
def test_threshold_counts_kernel(M):
    for m, shape in _cases(M):
        _, _, w, _, _, want = PU.problem(m, shape)
        _check_counts(f"M={m} {shape}", _gpu(m, shape)[1], want, w, shape[2])


def test_std_is_zero_on_equal_members_and_the_mean_is_the_member():
    M, shape = 9, (2, 7, 9)
    ens = EU.inputs(M, shape, seed=1)[0]
    ens[:, 0] = ens[0, 0]                              # slab 0: all members equal
    got = _products(ens.to(DEV), ens[0].numel(), M, shape, want={"mean", "std"})
    assert (got["std"][0] == 0).all() and (got["std"][1] > 0).all()
    assert torch.equal(got["mean"][0].cpu(), ens[0, 0])


def test_strict_greater_on_deliberate_ties():
    """Members and truth values placed on the threshold itself do not exceed it: x_0 = thr on
    row 1, x_1 = x_2 = thr on row 2, y = thr on rows 2 and 3."""
    M, shape = 5, (2, 4, 37)
    ens, tar, w, thr = PU.inputs(M, shape, seed=1)
    for s in range(2):
        ens[0, s, 1] = thr[s, 1]
        ens[1, s, 2] = thr[s, 1]
        ens[2, s, 2] = thr[s, 1]
        tar[s, 2:4] = thr[s, 1]
    want = PU.counts(ens.double(), tar.double(), w.double(), thr)
    t = thr.t()[:, :, None, None]
    loose_k = (ens[None] >= t[:, None]).sum(dim=1)
    assert (loose_k != PU.exceed(ens, thr)).any()      # >= in place of > would show
    e, td = ens.to(DEV), thr.to(DEV)
    got = _counts(e, ens[0].numel(), tar.to(DEV), w.to(DEV), td, M, shape)
    _check_counts("ties", got, want, w, shape[2])
    # the truth side: with >= the tied rows would count as events
    loose_o = PU.counts(ens.double(), tar.double() + 1e-3, w.double(), thr)
    assert (want[..., 1, :] - loose_o[..., 1, :]).abs().max() > 0.1
    _check_products("ties", _products(e, ens[0].numel(), M, shape, thr=td), ens, thr,
                    ens.sort(dim=0).values)


SUBSETS = [{"mean"}, {"min", "max"}, {"quant"}, {"prob"}, {"std"}, set(ALL)]


@pytest.mark.parametrize("M", [3, 8, 17, 32])
def test_optional_outputs_and_two_calls_are_bit_identical(M):
    """Every subset of the outputs gives the bits of the full call for what it writes; the
    counts of two calls are the same bits (whatever the workspace held)."""
    shape = (3, 121, 250)
    ens, tar, w, thr = (t.to(DEV) for t in PU.problem(M, shape)[:4])
    n = ens[0].numel()
    full = _gpu(M, shape)[0]
    for want in SUBSETS:
        got = _products(ens, n, M, shape, thr=thr, want=want)
        for k in NAMES:
            if k in want:
                assert torch.equal(got[k], full[k]), (want, k)
            else:
                assert got[k] is None
    # the unwanted outputs are not touched: hand the call NaN-filled buffers for two only
    bufs = {k: _nan(*full[k].shape) for k in NAMES}
    _products(ens, n, M, shape, thr=thr, want={"mean", "quant"}, bufs=bufs)
    for k in NAMES:
        if k in ("mean", "quant"):
            assert torch.equal(bufs[k], full[k])
        else:
            assert torch.isnan(bufs[k]).all(), k
    a = _counts(ens, n, tar, w, thr, M, shape)
    b = _counts(ens, n, tar, w, thr, M, shape, ws_fill=1e30)
    assert torch.equal(a, b) and torch.equal(a.cpu().double(), _gpu(M, shape)[1])
    # fewer thresholds: the same bits for those
    c = _counts(ens, n, tar, w, thr[:, :1].contiguous(), M, shape)
    assert torch.equal(c, a[:, :1])


@pytest.mark.parametrize("M", [3, 8, 9, 32])
def test_member_stride_and_phase(M):
    """Members as views into a larger buffer at strides of every residue mod 4, the truth and
    every output on each of the four 16-byte phases: the scalar path, the vector path with a
    head and a tail, the same bits as the packed call; nothing written around the outputs."""
    from msfno_amd import ensemble as E
    for shape in ((2, 7, 9), (1, 3, 4100)):
        ens, tar, w, thr, srt, cwant = PU.problem(M, shape)
        S, H, W = shape
        n = S * H * W
        full, cfull = _gpu(M, shape)
        td, wd = thr.to(DEV), w.to(DEV)
        for pad, off in ((1, 0), (2, 1), (3, 3), (4, 0), (4, 2), (8, 1), (8, 3), (4, 3)):
            buf = _nan(M * (n + pad) + 3)
            view = torch.as_strided(buf, (M, S, H, W), (n + pad, H * W, W, 1), 3)
            view.copy_(ens)
            tbuf = _nan(n + 4)
            t = tbuf[off:off + n].view(S, H, W)
            t.copy_(tar)
            tag = f"M={M} {shape} stride n+{pad} phase {off}"
            got = _counts(view, n + pad, t, wd, td, M, shape)
            assert torch.equal(got.cpu().double(), cfull), tag
            # the members' base is on phase 3: (8, 3) is the vector path with a head and a
            # tail; the outputs all on phase off, or (the last case) each on one of its own
            raw = {k: _nan(full[k].numel() + 8) for k in NAMES}
            ph = {k: (i % 4 if (pad, off) == (4, 3) else off) for i, k in enumerate(NAMES)}
            bufs = {k: raw[k][ph[k]:ph[k] + full[k].numel()].view(full[k].shape) for k in NAMES}
            _products(view, n + pad, M, shape, thr=td, bufs=bufs)
            for k in NAMES:
                assert torch.equal(bufs[k], full[k]), (tag, k)
                assert torch.isnan(raw[k][:ph[k]]).all(), (tag, k)
                assert torch.isnan(raw[k][ph[k] + full[k].numel():]).all(), (tag, k)
            # the Python entries keep the view (no copy) and give the same bits
            v5 = torch.as_strided(buf, (M, 1, S, H, W), (n + pad, n, H * W, W, 1), 3)
            assert E._members(v5).data_ptr() == v5.data_ptr()
            pc = E.threshold_sums(v5, t.view(1, S, H, W), wd, td)
            assert torch.equal(pc.view(S, -1, 2, M + 1).cpu().double(), cfull), tag
        pp = E.products(v5, quantiles=PU.LEVELS, thresholds=td, minmax=True)
        for k, v in zip(NAMES, pp):
            assert torch.equal(v.reshape(full[k].shape), full[k]), (shape, k)


@pytest.mark.parametrize("M", [4, 17])
def test_a_latitude_split_of_the_counts_adds_up(M):
    from msfno_amd import ensemble as E
    shape = (3, 121, 250)
    ens, tar, w, thr, _, want = PU.problem(M, shape)
    S, H, W = shape
    e, t, wd = ens.to(DEV).view(M, 1, S, H, W), tar.to(DEV).view(1, S, H, W), w.to(DEV)
    td = thr.to(DEV)
    whole = E.threshold_sums(e, t, wd, td)
    assert whole.shape == (1, S, 4, 2, M + 1)
    total = torch.zeros(1, S, 4, 2, M + 1, dtype=torch.float64)
    for a, b in ((0, 50), (50, 51), (51, 121)):
        total += E.threshold_sums(e[..., a:b, :], t[..., a:b, :], wd[a:b], td).cpu().double()
    assert ((total[0] - want).abs() <= 2e-5 * want).all()
    assert (total[0][want == 0] == 0).all()
    assert torch.equal(whole[0].cpu().double(), _gpu(M, shape)[1])
    # the maps are row-local: a band's products are the rows of the whole
    full = _gpu(M, shape)[0]
    band = E.products(e[..., 50:121, :], quantiles=PU.LEVELS, thresholds=td, minmax=True)
    for k, v in zip(NAMES, band):
        assert torch.equal(v.reshape(-1, S, 71, W), full[k].reshape(-1, S, H, W)[:, :, 50:]), k


def test_more_than_eight_levels_and_thresholds_through_python():
    from msfno_amd import ensemble as E
    M, shape = 9, (2, 7, 9)
    ens, tar, w, _ = PU.inputs(M, shape)
    S, H, W = shape
    wd = w.to(DEV)
    levels = [i / 16 for i in range(17)]               # every member and every midpoint
    thr = (299.0 + 0.2 * torch.arange(11)[None] + 0.05 * torch.arange(S)[:, None]).float()
    ens, tar = PU.untie(ens, thr), PU.untie(tar, thr)
    e, t = ens.to(DEV).view(M, 1, S, H, W), tar.to(DEV).view(1, S, H, W)
    td = thr.to(DEV)
    got = E.products(e, quantiles=levels, thresholds=td, mean=False, std=False)
    assert got.mean is None and got.std is None and got.min is None and got.max is None
    assert got.quantiles.shape == (17, 1, S, H, W) and got.prob.shape == (11, 1, S, H, W)
    for a in range(0, 17, 8):
        part = E.products(e, quantiles=levels[a:a + 8], mean=False, std=False)
        assert part.prob is None and torch.equal(part.quantiles, got.quantiles[a:a + 8])
    for a in range(0, 11, 8):
        part = E.products(e, thresholds=td[:, a:a + 8], mean=False, std=False)
        assert part.quantiles is None and torch.equal(part.prob, got.prob[a:a + 8])
    srt = ens.sort(dim=0).values
    assert torch.equal(got.quantiles[::2, 0].cpu(), srt)           # level i / (M - 1): member i
    _check_products("17 levels, 11 thresholds",
                    dict(mean=None, std=None, min=None, max=None, quant=got.quantiles[:, 0],
                         prob=got.prob[:, 0]), ens, thr, srt, levels)
    counts = E.threshold_sums(e, t, wd, td)
    assert counts.shape == (1, S, 11, 2, M + 1)
    for a in range(0, 11, 8):
        part = E.threshold_sums(e, t, wd, td[:, a:a + 8])
        assert torch.equal(part, counts[:, :, a:a + 8])
    _check_counts("11 thresholds", counts[0], PU.counts(ens.double(), tar.double(), w.double(),
                                                        thr), w, W)
    # (C, nt) thresholds are those of every batch element
    both = E.threshold_sums(e.view(M, S, 1, H, W), t.view(S, 1, H, W), wd, td[:1, :3])
    same = E.threshold_sums(e.view(M, S, 1, H, W), t.view(S, 1, H, W), wd,
                            td[:1, :3].expand(S, 3).reshape(S, 1, 3))
    assert torch.equal(both, same)


def test_scores_from_gpu_counts():
    from msfno_amd import ensemble as E
    M, shape = 8, (3, 121, 250)
    ens, tar, w, thr, _, want = PU.problem(M, shape)
    got = _gpu(M, shape)[1]
    ref = E.finish_thresholds(want, w.double(), shape[2], M)
    sc = E.finish_thresholds(got, w.double(), shape[2], M)
    brier, fair, base = PU.pixel_scores(ens.double(), tar.double(), w.double(), thr)
    assert torch.allclose(ref.brier, brier, rtol=0, atol=1e-12)
    dsc = E.finish_thresholds(got.float().to(DEV), w.to(DEV), shape[2], M)
    for name in ("base_rate", "brier", "fair_brier", "uncertainty", "reliability", "resolution"):
        a, r = getattr(sc, name), getattr(ref, name)
        # the counts are within 1e-5 relative and sum to n; a score is a sum over the bins
        # whose derivatives in N_k / n and O_k / n are below 3 and 2 (reliability: (p - f)^2 +
        # 2 f (p - f) and -2 (p - f)), so it moves by at most 5e-5
        assert ((a - r).abs() <= 5e-5).all(), name
        assert ((getattr(dsc, name).cpu().double() - r).abs() <= 1e-4).all(), name
    some = (ref.base_rate > 0.01) & (ref.base_rate < 0.99)
    assert some.sum() >= 9 and ((sc.roc_area - ref.roc_area).abs()[some] <= 1e-4).all()
    # the members are drawn independently of the truth: no skill
    assert ((ref.roc_area[some] - 0.5).abs() <= 0.05).all()


def _capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(0)
    return graph


def test_verifier_with_thresholds_captures_in_a_graph():
    """No allocation, synchronisation or memset on the C side: update with thresholds records
    into a graph and replays on new values like eager."""
    from msfno_amd import ensemble as E
    M, B, C, H, W = 5, 2, 3, 5, 12
    ens, tar, w, thr = PU.inputs(M, (B * C, H, W), seed=3)
    se, st = ens.view(M, B, C, H, W).to(DEV), tar.view(B, C, H, W).to(DEV)
    wd = w.to(DEV)
    ver = E.EnsembleVerifier(wd, H, W, 2, M, B, C, device=DEV, thresholds=thr.view(B, C, 4))
    assert ver.tcounts.shape == (2, B, C, 4, 2, M + 1) and torch.isnan(ver.tcounts).all()
    graph = _capture(lambda slot: ver.update(slot, se, st))
    ens2, tar2, _, _ = PU.inputs(M, (B * C, H, W), seed=5)
    se.copy_(ens2.view(M, B, C, H, W))
    st.copy_(tar2.view(B, C, H, W))
    for t in (ver.sums, ver.hist, ver.tcounts):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isnan(ver.tcounts[1]).all()
    ver.update(1, se, st)
    assert torch.equal(ver.tcounts[0], ver.tcounts[1])
    assert torch.equal(ver.sums[0], ver.sums[1]) and torch.equal(ver.hist[0], ver.hist[1])
    want = PU.counts(ens2.double(), tar2.double(), w.double(), thr)
    _check_counts("graph replay", ver.tcounts[0].view(B * C, 4, 2, M + 1), want, w, W)
    sc = ver.threshold_scores()
    assert sc.brier.shape == (2, B, C, 4) and sc.hit_rate.shape == (2, B, C, 4, M + 2)
    assert torch.isfinite(sc.brier).all()
    # update does not synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ver.update(0, se, st)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_a_default_verifier_is_unchanged():
    """Without thresholds: no tcounts, no second workspace, and the sums and rank counts of
    msfno_ens_sums bit for bit."""
    from test_gpu_ensemble import _sums
    from msfno_amd import ensemble as E
    M, B, C, H, W = 5, 2, 3, 5, 12
    ens, tar, w = EU.inputs(M, (B * C, H, W), seed=3)
    e, t, wd = ens.to(DEV), tar.to(DEV), w.to(DEV)
    ver = E.EnsembleVerifier(wd, H, W, 1, M, B, C, device=DEV)
    assert not hasattr(ver, "tcounts") and not hasattr(ver, "_tws")
    assert not hasattr(ver, "thresholds")
    ver.update(0, e.view(M, B, C, H, W), t.view(B, C, H, W))
    sums, hist = _sums(e, B * C * H * W, t, wd, M, (B * C, H, W))
    assert torch.equal(ver.sums[0].view(B * C, 5), sums)
    assert torch.equal(ver.hist[0].view(B * C, M + 1), hist)
    with pytest.raises(ValueError, match="without thresholds"):
        ver.threshold_scores()


def test_rollout_products_and_thresholded_verification_on_the_fixture_network():
    """M = 4 members, 3 steps, every = 2: the products of steps 0 and 2, and the threshold
    counts of a thresholded verify_ensemble, against the restatement on the very outputs of
    run() that the driver saw (recorded), so the kernels' own bounds hold: the indexing, the
    pairing and the denormalisation."""
    from test_gpu_ensemble import _rollout
    from msfno_amd import ensemble as E
    r, x0, stds = _rollout(True)
    M, C, H, W = x0.shape
    first = next(iter(r.run(x0, 1)))[1]
    thr = torch.stack([first[:, c].median() + torch.tensor([-0.1, 0.2], device=DEV) * stds[0, c, 0, 0]
                       for c in range(C)]).float()                     # (C, 2), field units
    # the outputs that the driver itself sees (a second run need not give the same bits)
    rec, run = [], r.run

    def recording(*args, **kwargs):
        for i, y in run(*args, **kwargs):
            rec.append(y.clone())
            yield i, y

    r.run = recording
    levels = (0.0, 0.3, 0.5, 1.0)
    seen = []
    for i, p in r.ensemble_products(x0, 3, every=2, quantiles=levels, thresholds=thr,
                                    minmax=True):
        seen.append(i)
        assert p.mean.shape == (1, C, H, W) and p.quantiles.shape == (4, 1, C, H, W)
        assert p.prob.shape == (2, 1, C, H, W)
        ens = rec[i].cpu()
        got = dict(mean=p.mean[0], std=p.std[0], min=p.min[0], max=p.max[0],
                   quant=p.quantiles[:, 0], prob=p.prob[:, 0])
        _check_products(f"rollout step {i}", got, ens, thr.cpu(), ens.sort(dim=0).values, levels)
    assert seen == [0, 2] and len(rec) == 3
    scored = [0, 2]
    truths = [(rec[i][0].flip(1).roll(W // 2, 2) + 0.25 * (k + 1) * stds[0]).contiguous()
              for k, i in enumerate(scored)]
    del rec[:]
    ver = E.EnsembleVerifier("cosine", H, W, 2, M, 1, C, device=DEV, thresholds=thr)
    r.verify_ensemble(x0, iter(truths), 3, every=2, verifier=ver)
    w32 = ver.w.cpu()
    for k, i in enumerate(scored):
        want = PU.counts(rec[i].cpu().double(), truths[k].cpu().double(), w32.double(),
                         thr.cpu())
        _check_counts(f"verify_ensemble step {i}", ver.tcounts[k, 0], want, w32, W)
    sc = ver.threshold_scores()
    assert sc.brier.shape == (2, 1, C, 2) and torch.isfinite(sc.brier).all()

    class Sharded:
        world = 2

    from msfno_amd.rollout import Rollout
    with pytest.raises(NotImplementedError, match="row-local"):
        Rollout(Sharded(), graph=False).ensemble_products(x0, 1)
    with pytest.raises(ValueError, match="steps"):
        r.ensemble_products(x0, 0)
