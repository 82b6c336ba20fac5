"""Ensemble verification and the CRPS gradient on the GPU (csrc/ensemble.hip through the
C-ABI, msfno_amd/ensemble.py and Rollout.verify_ensemble) against the fp64 restatement
(tests/ensemble_util.py).  Outputs and workspaces are pre-filled with NaN.

Kernel sums: M in {2, 3, 5, 8, 9, 16, 17, 32} (both sides of every register bucket 4 / 8 /
16 / 32, odd sizes, both ends) at slabs (S, H, W) where the kernel takes another path: a
single element, rows shorter than a float4, slabs off the 16-byte grid (7 x 9), many rows
per unit, nlon % 4 != 0 (250), a row wider than one sweep of a workgroup (4100), and the
real 721 x 1440 rows at M = 4.  Inputs are 300 + N(0, 1) members against a 300.5 + N(0, 1)
truth: a raw mean or raw squares would lose five digits.
  Every sum within tol(M) = (131 + 2 (M + 2) + M (M - 1) / 2) 2^-24 of its magnitude sum
  (EU.tol: 8.3e-6 at M = 2, 4.1e-5 at M = 32), derived, not measured.  The kernel's chains:
  per pixel, dbar is a chain of M - 1 adds and a product with the rounded 1 / M (M + 1
  roundings, 2 (M + 1) + 1 once squared); the pair sums are one sequential chain of
  M (M - 1) / 2 non-negative terms per pixel; a lane then adds one term per pixel of its
  share of a row (nlon / lpr <= 64 for nlon <= 16384) and one weighted term per row it
  visits (<= 64), which is the 128-term chain of csrc/row_reduce.h, and the wave / block
  tree and the fp64 combine are the "+ 3".  The worst ratio per case is printed.
Histogram: every bin within 1e-5 relative, exactly 0 where the restatement is 0 (counts are
integers per row and wave; the weighted adds are a chain of <= 64 + 4 terms); the inputs
have no x_i == y tie (asserted), a separate case pins strict < on deliberate ties.
Backward: |got - want| <= 1e-6 w[h] |g[s]| against fp64 autograd of the restatement (the
bracket is a difference of two short exact-integer forms: the rounded 1 / M and kappa, a
product, a difference and the product with w g are 5 roundings of at most 2^-24 each on a
bracket below 1).
Driver: Rollout.verify_ensemble on the small fixture network against fp64 scoring of run()'s
outputs at 1e-3 of the magnitude sums: the indexing, the pairing and the denormalisation.

What the tests catch (edits of csrc/ensemble.hip on scratch builds, none of which can index
out of bounds; the failing tests of this file in brackets):
  - the pair loop starting at j = i + 2 (the neighbouring pair left out of gini and sq): 23
    tests [test_ens_sums_kernel at every M, test_member_stride_and_phase,
    test_a_latitude_split_adds_up, test_scores_from_gpu_sums, test_crps_loss_through_autograd,
    the graph, driver and refusal tests, which all check sums];
  - kappa in place of 1 / M on sign(x_i - y) in the gradient: 17 tests
    [test_crps_backward_kernel at every M and kappa but M = 2 fair, where kappa = 1 / M,
    and test_crps_loss_through_autograd];
  - the rank counted with <= : 1 test [test_rank_histogram_counts_strictly_smaller_members;
    the other inputs have no tie, by construction];
  - dbar formed from the raw mean, (1/M) sum x_i - y, against the difference-first rule
    (an error of about 300 x 2^-24 per pixel, partly averaged out by the sum): 7 tests
    [test_ens_sums_kernel at M = 3, 8, 9, 16, 17, test_member_stride_and_phase[3],
    test_refusals_on_the_gpu]; at M = 2, 5 and 32 it stays inside the bound.
  (The pair loop starting at j = i adds exact zeros and changes nothing.)
"""
import functools
import os

import pytest
import torch

import ensemble_util as EU

pytestmark = pytest.mark.gpu
DEV = "cuda"

MS = [2, 3, 5, 8, 9, 16, 17, 32]
SHAPES = [(1, 1, 1), (1, 2, 8), (2, 7, 9), (6, 5, 12), (3, 121, 250), (1, 3, 4100)]
BIG = (4, (2, 721, 1440))
BWD_SHAPES = [(2, 7, 9), (1, 3, 4100)]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _sums(ens, stride, tar, w, M, shape, with_hist=True, ws=None):
    """msfno_ens_sums on device pointers (any 16-byte phase, any member stride); NaN-filled
    outputs and workspace."""
    from msfno_amd import _native as N
    S, H, W = shape
    lib = N.lib()
    nbytes = lib.msfno_ens_workspace_size(S, M, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    if ws is None:
        ws = _nan(nbytes // 4)
    sums = _nan(S, 5)
    hist = _nan(S, M + 1) if with_hist else None
    N.check(lib.msfno_ens_sums(ens.data_ptr(), stride, tar.data_ptr(), w.data_ptr(),
                               sums.data_ptr(), N.ptr(hist), M, S, H, W, ws.data_ptr(), nbytes,
                               N.stream_of(ens.device)), "msfno_ens_sums")
    return sums, hist


def _backward(ens, stride, tar, w, g, kappa, dens, dstride, M, shape):
    from msfno_amd import _native as N
    S, H, W = shape
    N.check(N.lib().msfno_ens_crps_backward(ens.data_ptr(), stride, tar.data_ptr(), w.data_ptr(),
                                            g.data_ptr(), kappa, dens.data_ptr(), dstride, M, S,
                                            H, W, N.stream_of(ens.device)),
            "msfno_ens_crps_backward")


@functools.lru_cache(maxsize=None)
def _gpu(M, shape):
    """The kernel's (sums, hist) of EU.problem(M, shape), as fp64 host tensors."""
    ens, tar, w = EU.problem(M, shape)[:3]
    S, H, W = shape
    sums, hist = _sums(ens.to(DEV), S * H * W, tar.to(DEV), w.to(DEV), M, shape)
    return sums.cpu().double(), hist.cpu().double()


def _check_sums(tag, got, want, mag, tol):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    err = (got - want).abs()
    worst = (err / mag.clamp(min=1e-300)).max().item()
    print(f"{tag}: sums max err / magnitude sum {worst:.3e} (tol {tol:.3e})")
    assert (err <= tol * mag).all(), (tag, worst, tol)
    return worst


def _check_hist(tag, got, want):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    assert (got[want == 0] == 0).all(), tag
    err = (got - want).abs()
    print(f"{tag}: hist max relative err "
          f"{(err / want.clamp(min=1e-300))[want > 0].max().item():.3e}")
    assert (err <= 1e-5 * want).all(), tag


def _cases(M):
    return [(M, s) for s in SHAPES] + ([BIG] if M == 2 else [])


@pytest.mark.parametrize("M", MS)
def test_ens_sums_kernel(M):
    """(The 721 x 1440 case at M = 4 rides with M = 2.)"""
    for m, shape in _cases(M):
        _, _, _, want, mag, _ = EU.problem(m, shape)
        got, _ = _gpu(m, shape)
        _check_sums(f"M={m} {shape}", got, want, mag, EU.tol(m))


@pytest.mark.parametrize("M", MS)
def test_rank_histogram(M):
    for m, shape in _cases(M):
        ens, tar, w, _, _, want = EU.problem(m, shape)
        assert not (ens == tar).any()          # no tie: the fp32 and fp64 ranks are the same
        _, got = _gpu(m, shape)
        _check_hist(f"M={m} {shape}", got, want)
        n = shape[2] * w.double().sum()
        assert torch.allclose(got.sum(dim=-1), n.expand(shape[0]), rtol=1e-5, atol=0)


def test_rank_histogram_counts_strictly_smaller_members():
    """x_0 = y on row 1, x_1 = x_2 = y on row 2: a tie is not 'smaller'."""
    M, shape = 5, (2, 4, 37)
    ens, tar, w = EU.inputs(M, shape, seed=1)
    ens[0, :, 1] = tar[:, 1]
    ens[1, :, 2] = tar[:, 2]
    ens[2, :, 2] = tar[:, 2]
    want = EU.hist(ens.double(), tar.double(), w.double())
    loose = torch.stack([(w.double()[:, None] * ((ens <= tar).sum(dim=0) == r)).sum(dim=(-1, -2))
                         for r in range(M + 1)], dim=-1)
    assert (want - loose).abs().max() > 0.1    # <= in place of < would show
    sums, got = _sums(ens.to(DEV), ens[0].numel(), tar.to(DEV), w.to(DEV), M, shape)
    _check_hist("ties", got, want)
    s64, mag = EU.sums(ens.double(), tar.double(), w.double())
    _check_sums("ties", sums, s64, mag, EU.tol(M))


@pytest.mark.parametrize("M", [3, 8, 17])
def test_two_calls_are_bit_identical_and_hist_is_optional(M):
    shape = (3, 121, 250)
    ens, tar, w = (t.to(DEV) for t in EU.problem(M, shape)[:3])
    n = ens[0].numel()
    a, ha = _sums(ens, n, tar, w, M, shape)
    b, hb = _sums(ens, n, tar, w, M, shape)
    c, hc = _sums(ens, n, tar, w, M, shape, with_hist=False)
    assert torch.equal(a, b) and torch.equal(ha, hb)
    assert hc is None and torch.equal(a, c)
    assert torch.equal(a.cpu().double(), _gpu(M, shape)[0])


@pytest.mark.parametrize("M", [3, 8, 9, 32])
def test_member_stride_and_phase(M):
    """Members as views into a larger buffer at strides of every residue mod 4 (only a
    multiple of 4 floats lets the members share a 16-byte phase), and the truth off the
    16-byte grid: the scalar path, the vector path with a head and a tail, same sums."""
    from msfno_amd import ensemble as E
    for shape in ((2, 7, 9), (1, 3, 4100)):
        ens, tar, w, want, mag, hwant = EU.problem(M, shape)
        S, H, W = shape
        n = S * H * W
        for pad, toff in ((1, 0), (2, 1), (3, 3), (4, 0), (4, 2), (8, 1)):
            buf = _nan(M * (n + pad) + 3)
            view = torch.as_strided(buf, (M, S, H, W), (n + pad, H * W, W, 1), 3)
            view.copy_(ens)
            tbuf = _nan(n + 4)
            t = tbuf[toff:toff + n].view(S, H, W)
            t.copy_(tar)
            got, hist = _sums(view, n + pad, t, w.to(DEV), M, shape)
            tag = f"M={M} {shape} stride n+{pad} tar+{toff}"
            _check_sums(tag, got, want, mag, EU.tol(M))
            _check_hist(tag, hist, hwant)
            # the Python entry keeps the view (no copy) and gives the same bits
            v5 = torch.as_strided(buf, (M, 1, S, H, W), (n + pad, n, H * W, W, 1), 3)
            assert E._members(v5).data_ptr() == v5.data_ptr()
            ps, ph = E.ensemble_sums(v5, t.view(1, S, H, W), w.to(DEV))
            assert torch.equal(ps.view(S, 5), got) and torch.equal(ph.view(S, M + 1), hist)


@pytest.mark.parametrize("M", [4, 17])
def test_a_latitude_split_adds_up(M):
    from msfno_amd import ensemble as E
    shape = (3, 121, 250)
    ens, tar, w, want, mag, hwant = EU.problem(M, shape)
    S, H, W = shape
    e, t, wd = ens.to(DEV).view(M, 1, S, H, W), tar.to(DEV).view(1, S, H, W), w.to(DEV)
    whole, hwhole = E.ensemble_sums(e, t, wd)
    total = torch.zeros(1, S, 5, dtype=torch.float64)
    htotal = torch.zeros(1, S, M + 1, dtype=torch.float64)
    for a, b in ((0, 50), (50, 51), (51, 121)):
        s, h = E.ensemble_sums(e[..., a:b, :], t[..., a:b, :], wd[a:b])
        total += s.cpu().double()
        htotal += h.cpu().double()
    assert ((total - whole.cpu().double()).abs() <= 2 * EU.tol(M) * mag).all()
    _check_sums(f"split M={M}", total[0], want, mag, 2 * EU.tol(M))
    assert ((htotal[0] - hwant).abs() <= 2e-5 * hwant).all()
    assert torch.equal(whole.cpu().double().view(S, 5), _gpu(M, shape)[0])


def _want_grad(M, shape, fair, g):
    ens, tar, w = EU.problem(M, shape)[:3]
    x = ens.double().requires_grad_()
    (g.double() * EU.crps_sums(x, tar.double(), w.double(), EU.kappa(M, fair))).sum().backward()
    return x.grad


def _check_grad(tag, got, want, w, g):
    """|got - want| <= 1e-6 w[h] |g[s]|; got, want (M, S, H, W)."""
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    bound = 1e-6 * w.double()[None, None, :, None] * g.double().abs()[None, :, None, None]
    err = (got - want).abs()
    print(f"{tag}: grad max err / (w |g|) {(err / bound).max().item() * 1e-6:.3e}")
    assert (err <= bound).all(), tag
    assert want.abs().max() > 0


@pytest.mark.parametrize("fair", [True, False], ids=["fair", "plain"])
@pytest.mark.parametrize("M", MS)
def test_crps_backward_kernel(M, fair):
    for shape in BWD_SHAPES:
        ens, tar, w = EU.problem(M, shape)[:3]
        S, H, W = shape
        n = S * H * W
        g = torch.linspace(-1.5, 2.0, S) if S > 1 else torch.tensor([0.75])
        want = _want_grad(M, shape, fair, g)
        e, t, wd, gd = ens.to(DEV), tar.to(DEV), w.to(DEV), g.to(DEV)
        dens = _nan(M, S, H, W)
        _backward(e, n, t, wd, gd, EU.kappa(M, fair), dens, n, M, shape)
        _check_grad(f"M={M} {shape} fair={fair}", dens, want, w, g)
        if M in (3, 8, 32):
            # members and gradients as views at strides off the 16-byte grid
            for pe, pd in ((1, 4), (4, 2), (4, 4)):
                ebuf, dbuf = _nan(M * (n + pe) + 1), _nan(M * (n + pd) + 2)
                ev = torch.as_strided(ebuf, (M, S, H, W), (n + pe, H * W, W, 1), 1)
                dv = torch.as_strided(dbuf, (M, S, H, W), (n + pd, H * W, W, 1), 2)
                ev.copy_(e)
                _backward(ev, n + pe, t, wd, gd, EU.kappa(M, fair), dv, n + pd, M, shape)
                _check_grad(f"M={M} {shape} strides n+{pe}, n+{pd}", dv, want, w, g)
                # nothing written between the members
                gaps = torch.as_strided(dbuf, (M, pd), (n + pd, 1), 2 + n)
                assert torch.isnan(gaps).all() and torch.isnan(dbuf[:2]).all()


@pytest.mark.parametrize("fair", [True, False], ids=["fair", "plain"])
def test_crps_loss_through_autograd(fair):
    from msfno_amd import ensemble as E
    from msfno_amd.losses import sphere_weights
    M, B, C, H, W = 5, 2, 3, 7, 9
    ens, tar, _ = EU.inputs(M, (B * C, H, W), seed=2)
    w64 = torch.from_numpy(sphere_weights("cosine", H))
    w32 = w64.float()
    x = ens.view(M, B, C, H, W).to(DEV).requires_grad_()
    loss = E.CRPSLoss("cosine", fair=fair)(x, tar.view(B, C, H, W).to(DEV))
    loss.backward()
    k = EU.kappa(M, fair)
    n = W * w32.double().sum()
    x64 = ens.double().requires_grad_()
    want = EU.crps_sums(x64, tar.double(), w32.double(), k).mean() / n
    want.backward()
    s64, mag = EU.sums(ens.double(), tar.double(), w32.double())
    scale = ((mag[:, EU.ABS] + k * mag[:, EU.GINI]).mean() / n).item()
    print(f"CRPSLoss {loss.item():.8e} want {want.item():.8e} scale {scale:.3e}")
    # the sums' bound, and 8 more roundings for the fp32 finish (the two sums' casts, the
    # product with kappa, the difference, the mean over 6 slabs, the division)
    assert abs(loss.item() - want.item()) <= (EU.tol(M) + 8 * 2.0 ** -24) * scale
    g = torch.full((B * C,), 1.0 / (B * C * n.item()))
    _check_grad(f"CRPSLoss fair={fair}", x.grad.view(M, B * C, H, W), x64.grad, w32, g)
    assert x.grad.shape == x.shape
    with pytest.raises(NotImplementedError):
        E.CRPSLoss()(x, tar.view(B, C, H, W).to(DEV).requires_grad_())


@pytest.mark.parametrize("M", [2, 8, 32])
def test_scores_from_gpu_sums(M):
    from msfno_amd import ensemble as E
    shape = (3, 121, 250)
    ens, tar, w, want, mag, hwant = EU.problem(M, shape)
    S, H, W = shape
    got, hist = _gpu(M, shape)
    tol = EU.tol(M)
    n = (W * w.double().sum()).item()
    ref = EU.scores(want, hwant, w.double(), W, M)
    sc = E.finish(got, hist, w.double(), W, M)
    # |sqrt(a + d) - sqrt(a)| <= |d| / sqrt(a)
    assert ((sc.rmse - ref["rmse"]).abs() <= tol * mag[:, EU.SE] / n / ref["rmse"]).all()
    assert ((sc.mse - ref["mse"]).abs() <= tol * mag[:, EU.SE] / n).all()
    assert ((sc.bias - ref["bias"]).abs() <= tol * mag[:, EU.ERR] / n).all()
    assert ((sc.mae - ref["mae"]).abs() <= tol * ref["mae"]).all()
    assert ((sc.spread - ref["spread"]).abs() <= tol * ref["spread"]).all()
    for name, k in (("crps", EU.kappa(M, False)), ("fair_crps", EU.kappa(M, True))):
        bound = tol * (mag[:, EU.ABS] + k * mag[:, EU.GINI]) / n
        assert ((getattr(sc, name) - ref[name]).abs() <= bound).all(), name
        assert (ref[name] > 0).all()
    # rmse and spread within tol each, relative; the ratio within their sum (and slack)
    rel = tol * mag[:, EU.SE] / n / ref["rmse"] ** 2 + tol
    assert ((sc.spread_skill - ref["spread_skill"]).abs()
            <= 1.01 * rel * ref["spread_skill"]).all()
    assert ((sc.rank_hist - ref["rank_hist"]).abs() <= 1e-5 * ref["rank_hist"]).all()
    # the device form: fp32 sums finished on the device
    dsc = E.finish(got.float().to(DEV), hist.float().to(DEV), w.to(DEV), W, M)
    for name in EU.NAMES:
        v = getattr(dsc, name).cpu().double()
        assert ((v - ref[name]).abs() <= 1e-4 * ref[name].abs()).all(), name


def test_verifier_and_loss_capture_in_a_graph():
    """No allocation, synchronisation or memset on the C side: EnsembleVerifier.update and
    CRPSLoss forward + backward record into a graph and replay on new values like eager."""
    from msfno_amd import ensemble as E
    M, B, C, H, W = 5, 2, 3, 5, 12
    ens, tar, w = EU.inputs(M, (B * C, H, W), seed=3)
    se = ens.view(M, B, C, H, W).to(DEV).requires_grad_()
    st = tar.view(B, C, H, W).to(DEV)
    wd = w.to(DEV)
    ver = E.EnsembleVerifier(wd, H, W, 2, M, B, C, device=DEV)
    loss_fn = E.CRPSLoss(wd, fair=True)

    def step(slot):
        ver.update(slot, se.detach(), st)
        v = loss_fn(se, st)
        (g,) = torch.autograd.grad(v, se)
        return v, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v_out, g_out = step(0)
    ens2, tar2, _ = EU.inputs(M, (B * C, H, W), seed=5)
    with torch.no_grad():  # new values in the captured buffers
        se.copy_(ens2.view(M, B, C, H, W))
        st.copy_(tar2.view(B, C, H, W))
    ver.sums.fill_(float("nan"))
    ver.hist.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    v_eager, g_eager = step(1)
    assert torch.equal(ver.sums[0], ver.sums[1]) and torch.equal(ver.hist[0], ver.hist[1])
    assert torch.equal(v_out, v_eager) and torch.equal(g_out, g_eager)
    e64, t64 = se.detach().cpu().double().view(M, B * C, H, W), st.cpu().double().view(-1, H, W)
    want, mag = EU.sums(e64, t64, w.double())
    _check_sums("graph replay", ver.sums[0].view(B * C, 5), want, mag, EU.tol(M))
    _check_hist("graph replay", ver.hist[0].view(B * C, M + 1), EU.hist(e64, t64, w.double()))
    sc = ver.scores()
    assert sc.fair_crps.shape == (2, B, C) and sc.rank_hist.shape == (2, B, C, M + 1)
    assert all(torch.isfinite(v).all() for v in sc)


def test_verifier_update_does_not_synchronise():
    from msfno_amd import ensemble as E
    M, B, C, H, W = 3, 1, 2, 5, 12
    ens, tar, w = EU.inputs(M, (B * C, H, W), seed=4)
    e, t = ens.view(M, B, C, H, W).to(DEV), tar.view(B, C, H, W).to(DEV)
    ver = E.EnsembleVerifier("cosine", H, W, 2, M, B, C, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ver.update(0, e, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ver.update(1, e, t.cpu())                 # a host truth is copied over
    assert torch.equal(ver.sums[0], ver.sums[1]) and torch.equal(ver.hist[0], ver.hist[1])
    assert torch.isfinite(ver.sums).all()
    with pytest.raises(IndexError):
        ver.update(2, e, t)
    with pytest.raises(ValueError):
        ver.update(0, e[:2], t)


# ---- the driver: Rollout.verify_ensemble on the small fixture network -------------------

def _rollout(graph):
    from msfno_amd.rollout import Rollout
    from test_gpu_net import _build
    from test_oracle_net import NET_FIXTURES, load_net
    path = [p for p in NET_FIXTURES if os.path.basename(p) == "net_nl.npz"][0]
    meta, params, x, _, _ = load_net(path)
    net = _build(meta, params)
    g = torch.Generator().manual_seed(1)
    means = torch.randn(1, meta["in_chans"], 1, 1, generator=g).to(DEV)
    stds = (torch.rand(1, meta["in_chans"], 1, 1, generator=g) + 0.5).to(DEV)
    M = 4
    members = x[:1] + 0.05 * torch.randn(M, *x.shape[1:], generator=g)   # perturbed x0
    return Rollout(net, means, stds, graph=graph), members.to(DEV) * stds + means, stds


def test_rollout_verify_ensemble_on_the_fixture_network():
    """M = 4 members from a perturbed x0, 3 steps, every = 2: steps 0 and 2 are scored.  The
    truth of a step is the antipode (latitude flip, half-turn roll) of member 0's own output
    of that step plus (k + 1) / 4 standard deviations: a mispaired step, a member taken for
    a batch element or a missing denormalisation changes the sums by O(1).  A rank bin is
    held to 1e-3 of the slab's total weight (the bins of a slab sum to it)."""
    from msfno_amd import ensemble as E
    from msfno_amd.losses import sphere_weights
    sums = {}
    for graph in (True, False):
        r, x0, stds = _rollout(graph)
        M, C, H, W = x0.shape
        outs = [o.clone() for _, o in r.run(x0, 3)]
        scored = [0, 2]
        truths = [(outs[i][0].flip(1).roll(W // 2, 2) + 0.25 * (k + 1) * stds[0]).contiguous()
                  for k, i in enumerate(scored)]
        ver = E.EnsembleVerifier("cosine", H, W, 2, M, 1, C, device=DEV)
        got = r.verify_ensemble(x0, iter(truths), 3, every=2, verifier=ver)
        assert all(v.shape == (2, 1, C) for v in got[:-1])
        assert got.rank_hist.shape == (2, 1, C, M + 1)
        assert all(torch.isfinite(v).all() for v in got)
        w64 = torch.from_numpy(sphere_weights("cosine", H))
        total = W * w64.sum()
        mags = torch.zeros(2, 1, C, 5, dtype=torch.float64)
        for k, i in enumerate(scored):
            e64, t64 = outs[i].cpu().double(), truths[k].cpu().double()
            want, mag = EU.sums(e64, t64, w64)
            mags[k, 0] = mag
            _check_sums(f"graph={graph} step {i}", ver.sums[k, 0], want, mag, 1e-3)
            hwant = EU.hist(e64, t64, w64)
            assert ((ver.hist[k, 0].cpu().double() - hwant).abs() <= 1e-3 * total).all()
        sums[graph] = (ver.sums.cpu().double(), mags)
        # the default: uniform weights, a (1, C, H, W) truth, a host truth
        plain = r.verify_ensemble(x0, [truths[0][None], truths[1].cpu()], 3, every=2)
        mse = ((outs[0].double().mean(dim=0) - truths[0].double()) ** 2).mean(dim=(1, 2)).cpu()
        assert ((plain.mse[0, 0].cpu().double() - mse).abs() <= 1e-3 * mse).all()
        with pytest.raises(ValueError, match="ran out"):
            r.verify_ensemble(x0, truths[:1], 3, every=2)
    # graph and eager agree (the truths differ by the two runs' own outputs: same bound)
    assert ((sums[True][0] - sums[False][0]).abs() <= 2e-3 * sums[True][1]).all()


def test_refusals_on_the_gpu():
    """Each refusal is raised on the host with no launch; a small call works afterwards."""
    from msfno_amd import _native as N
    from msfno_amd import ensemble as E
    from msfno_amd.rollout import Rollout
    M, shape = 3, (2, 7, 9)
    ens, tar, w, want, mag, _ = EU.problem(M, shape)
    S, H, W = shape
    n = S * H * W
    e, t, wd = ens.to(DEV), tar.to(DEV), w.to(DEV)
    lib = N.lib()
    nbytes = lib.msfno_ens_workspace_size(S, M, H, W)
    ws, out = _nan(nbytes // 4), _nan(S, 5)

    def call(M=M, stride=n, nbytes=nbytes):
        return lib.msfno_ens_sums(e.data_ptr(), stride, t.data_ptr(), wd.data_ptr(),
                                  out.data_ptr(), None, M, S, H, W, ws.data_ptr(), nbytes,
                                  N.stream_of(e.device))

    assert call(M=1) == N.MSFNO_EINVAL
    assert call(M=33) == N.MSFNO_EUNSUPPORTED
    assert call(nbytes=nbytes - 1) == N.MSFNO_EWORKSPACE
    assert call(stride=n - 1) == N.MSFNO_EINVAL
    g = torch.ones(S, device=DEV)
    dens = _nan(M, S, H, W)
    for kw in (dict(M=1), dict(M=33), dict(stride=n - 1), dict(dstride=n - 1)):
        a = dict(M=M, stride=n, dstride=n)
        a.update(kw)
        rc = lib.msfno_ens_crps_backward(e.data_ptr(), a["stride"], t.data_ptr(), wd.data_ptr(),
                                         g.data_ptr(), 0.1, dens.data_ptr(), a["dstride"],
                                         a["M"], S, H, W, N.stream_of(e.device))
        assert rc == (N.MSFNO_EUNSUPPORTED if a["M"] == 33 else N.MSFNO_EINVAL), kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all() and torch.isnan(dens).all()
    e5, t4 = e.view(M, 1, S, H, W), t.view(1, S, H, W)
    with pytest.raises(ValueError):
        E.ensemble_sums(e5.cpu(), t4.cpu(), w)                        # no CPU path
    with pytest.raises(ValueError):
        E.ensemble_sums(e5, t4.cpu(), wd)
    with pytest.raises(ValueError):
        E.ensemble_sums(e5[:1], t4, wd)
    with pytest.raises(NotImplementedError):
        E.ensemble_sums(e5[:1].expand(33, 1, S, H, W), t4, wd)
    with pytest.raises(ValueError):
        E.ensemble_sums(e5, t4, torch.ones(H + 1, device=DEV))        # one weight per row
    with pytest.raises(ValueError, match="requires grad"):
        E.ensemble_sums(e5.clone().requires_grad_(), t4, wd)

    class Sharded:
        world = 2

    with pytest.raises(NotImplementedError, match="ensemble_sums"):
        Rollout(Sharded(), graph=False).verify_ensemble(e5[:, 0], [t4], 1)
    # an expanded member (stride 0) is copied, not refused; and a small call still works
    same, _ = E.ensemble_sums(e5[:1].expand(2, 1, S, H, W), t4, wd)
    assert (same[..., EU.GINI] == 0).all() and (same[..., EU.SQ] == 0).all()
    assert call() == N.MSFNO_OK
    _check_sums("after the refusals", out, want, mag, EU.tol(M))
