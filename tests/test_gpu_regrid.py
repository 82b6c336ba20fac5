"""Device tests of the regridder (msfno_amd/regrid.py, csrc/regrid.hip) against the fp64
restatement and the derived bound of tests/regrid_util.py: every output is counted.

    linear       |y - y64| <= (K + 4) 2^-24 (|Wlat| |x| |Wlon|^T),   K = taps_lat + taps_lon
    normalised   |y - y64| <= 2 (K + 4) 2^-24 mag / den

Fields are 300 + N(0, 1).  Masks are chosen so that den is not within 1e-3 of min_valid,
except under the dyadic block-mean weights, where den is exact and the tie den == min_valid
counts as valid."""
import functools

import numpy as np
import pytest
import torch

import regrid_util as RU

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _R(src, dst, method="conservative", kind="equiangular"):
    from msfno_amd import regrid as G
    if method == "block":
        return G.Regridder(src, method=G.block_mean(*dst))
    return G.Regridder(G.Grid(*src), G.Grid(*dst, kind=kind), method)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(R, x, **kw):
    """R on (S, H, W) numpy slabs as a (1, S, H, W) batch; (S', H', W') numpy."""
    y = R(_dev(x)[None], **kw)
    torch.cuda.synchronize()
    return y[0].cpu().numpy()


@pytest.mark.parametrize("src,dst,S", [
    ((13, 26), (5, 10), 3),      # row length = 2 mod 4, non-integer ratio, wrapped bands
    ((12, 20), (5, 7), 3),
    ((33, 64), (9, 16), 3),      # the 16-byte body
    ((9, 1443), (3, 241), 2),    # an odd row longer than a sweep: the phase moves by row
    ((130, 16), (65, 8), 3),     # more output rows than one unit holds
])
def test_conservative_is_within_the_bound(src, dst, S):
    R = _R(src, dst)
    x = RU.field((S,) + src, seed=11)
    want, bound = RU.linear(R, x)
    RU.check(f"{src} -> {dst}", _run(R, x), want, bound)


@pytest.mark.parametrize("name", ["bilinear", "adjoint", "block 32", "gauss"])
def test_other_operators_are_within_the_bound(name):
    R = {"bilinear": lambda: _R((5, 10), (13, 26), "bilinear"),
         "adjoint": lambda: _R((13, 26), (5, 10)).T,
         "block 32": lambda: _R((64, 96), (32, 32), "block"),       # the tap limit
         "gauss": lambda: _R((33, 64), (8, 16), kind="legendre-gauss")}[name]()
    if name == "block 32":
        assert R.out_shape == (2, 3) and (R.lat.taps, R.lon.taps) == (32, 32)
    x = RU.field((3,) + R.in_shape, seed=12)
    want, bound = RU.linear(R, x)
    RU.check(name, _run(R, x), want, bound)


def test_identity_is_a_bitwise_copy():
    R = _R((7, 9), (7, 9))
    assert (R.lat.taps, R.lon.taps) == (1, 1)
    x = RU.field((3, 7, 9), seed=13, kind="normal")
    x[0, 0, 0], x[1, 3, 4] = -0.0, np.float32(1e-42)       # a signed zero and a subnormal
    assert np.array_equal(_run(R, x).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("src,dst", [((13, 26), (5, 10)), ((33, 64), (9, 16))])
def test_addressing_guards_and_slab_lists(src, dst, off):
    """x and y start `off` floats past an aligned base; y is NaN-filled inside guard words;
    the slab list repeats, permutes and is longer than the input."""
    from workspace_guard import GUARD
    R = _R(src, dst)
    S, chans = 3, [2, 0, 2, 1, 1]
    x = RU.field((S,) + src, seed=14 + off)
    nx, ny = x.size, len(chans) * dst[0] * dst[1]
    xb = torch.zeros(nx + 8, device=DEV)
    xv = xb[off:off + nx].view(1, S, *src)
    xv.copy_(_dev(x)[None])
    G4 = GUARD // 4
    yb = torch.full((G4 + off + ny + G4,), float("nan"), device=DEV)
    yb[:G4 + off] = 12345.0
    yb[G4 + off + ny:] = 12345.0
    yv = yb[G4 + off:G4 + off + ny].view(1, len(chans), *dst)
    assert xv.data_ptr() % 16 == 4 * off and yv.data_ptr() % 16 == 4 * off
    assert xv.is_contiguous() and yv.is_contiguous()
    got = R(xv, channels=chans, out=yv)
    torch.cuda.synchronize()
    assert got.data_ptr() == yv.data_ptr()
    assert (yb[:G4 + off] == 12345.0).all() and (yb[G4 + off + ny:] == 12345.0).all()
    want, bound = RU.linear(R, x[chans])
    got = got[0].cpu().numpy()
    RU.check(f"{src} offset {off}", got, want, bound)        # no NaN left: every word written
    whole = _run(R, x)
    assert np.array_equal(got, whole[chans])                 # a slab does not see its position


def test_a_nan_reaches_exactly_the_outputs_whose_taps_cover_it():
    R = _R((13, 26), (5, 10))
    la, lo = R.lat, R.lon
    j = 2
    r_end = int(la.start[j] + la.count[j] - 1)               # the end of a latitude band
    i_wrap = int(np.flatnonzero(lo.start + lo.count > lo.n_in)[0])
    c_wrap = int((lo.start[i_wrap] + lo.count[i_wrap] - 1) % lo.n_in)   # reached through the wrap
    c_end = int((lo.start[3] + lo.count[3] - 1) % lo.n_in)
    for r, c in ((r_end, c_end), (0, c_wrap), (12, 25), (6, 13)):
        x = RU.field((2, 13, 26), seed=15)
        x[1, r, c] = np.nan
        got = _run(R, x)
        reach = RU.nan_reach(R, r, c)
        assert reach.any() and not reach.all()
        assert not np.isnan(got[0]).any()
        assert np.array_equal(np.isnan(got[1]), reach), (r, c)
    assert RU.nan_reach(R, 0, c_wrap)[0, i_wrap]


def _mask(shape, seed):
    """Weights in {0, 0.25 .. 1} with a patch of zeros that covers whole cells."""
    g = np.random.default_rng(seed)
    m = g.integers(0, 5, shape).astype(np.float32) / 4
    m[: shape[0] // 2, : shape[1] // 3] = 0
    return m


@pytest.mark.parametrize("mode", ["skip_nan", "mask", "both"])
@pytest.mark.parametrize("src,dst", [((13, 26), (5, 10)), ((33, 64), (9, 16))])
def test_normalised_mode_is_within_the_bound(src, dst, mode):
    R = _R(src, dst)
    x = RU.field((3,) + src, seed=16)
    g = np.random.default_rng(17)
    kw = {}
    if mode != "mask":
        x[g.random(x.shape) < 0.3] = np.nan
        x[:, src[0] // 2:, src[1] // 2:] = np.nan            # whole cells without a value
        kw["skip_nan"] = True
    if mode != "skip_nan":
        kw["mask"] = _mask(src, 18)
    min_valid, fill = 0.2375, -7.0                           # clear of every den of the six cases
    want, bound, den, valid = RU.normalised(R, x, min_valid=min_valid, fill=fill, **kw)
    assert (np.abs(den - min_valid) > 1e-3).all()            # no output sits on the threshold
    assert valid.any() and (~valid).any() and (den == 0).any() and ((den > 0) & ~valid).any()
    if "mask" in kw:
        kw["mask"] = _dev(kw["mask"])
    got = _run(R, x, min_valid=min_valid, fill=fill, **kw)
    assert (got[~valid] == fill).all()
    RU.check(f"{src} {mode}", got, want, bound)
    # fill defaults to NaN
    got = _run(R, x, min_valid=min_valid, **kw)
    assert np.isnan(got[~valid]).all() and not np.isnan(got[valid]).any()


def test_the_min_valid_tie_counts_as_valid_under_dyadic_weights():
    R = _R((8, 12), (4, 4), "block")
    x = RU.field((2, 8, 12), seed=19)
    x[0, 0:2, 0:4] = np.nan                                  # 8 of 16 valid: den == 0.5
    x[0, 4:8, 4:8] = np.nan                                  # none valid
    x[1, 0:4, 8:12][np.arange(4) >= 1] = np.nan              # 4 of 16: below
    want, bound, den, valid = RU.normalised(R, x, skip_nan=True, min_valid=0.5)
    assert den[0, 0, 0] == 0.5 and valid[0, 0, 0] and not valid[0, 1, 1] and not valid[1, 0, 2]
    got = _run(R, x, skip_nan=True, min_valid=0.5)
    RU.check("tie", got, want, bound)
    assert not np.isnan(got[0, 0, 0])


def test_sst_input_is_a_nanmean_and_the_affine():
    from msfno_amd import regrid as G
    B, T, H, W = 2, 3, 24, 48
    x = (RU.field((B, T, H, W), seed=20) - 12.0).astype(np.float32)
    x[:, :, 4:12, 8:20] = np.nan                             # whole cells
    x[:, :, 13:18, 30:33] = np.nan                           # parts of cells
    x[:, :, 0, :] = np.nan                                   # a row of every cell of the top band
    g = np.random.default_rng(21)
    means = (288 + g.standard_normal((1, T, 1, 1))).astype(np.float32)
    stds = (1 + g.random((1, T, 1, 1))).astype(np.float32)
    with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        coarse = np.nanmean(x.astype(np.float64).reshape(B, T, 6, 4, 12, 4), axis=(3, 5))
    want = (coarse - means) / stds
    assert np.isnan(want).any() and not np.isnan(want).all()
    got = G.sst_input(_dev(x), 4, _dev(means), _dev(stds)).cpu().numpy()
    assert got.shape == (B, T, 6, 12)
    assert np.array_equal(np.isnan(got), np.isnan(want))     # the reference's nan_mask
    # the mean within the normalised bound (K = 8, den <= 1), then two fp32 operations
    R = G.Regridder((H, W), method=G.block_mean(4, 4))
    y64, bound, _, _ = RU.normalised(R, x, skip_nan=True)
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    tol = (bound[ok] + 2 * RU.EPS * (np.abs(y64[ok]) + np.abs(means + 0 * y64)[ok])) / \
        (stds + 0 * y64)[ok] + 2 * RU.EPS * np.abs(want[ok])
    print(f"sst_input: worst error / bound {(err / tol).max():.3f}")
    assert (err <= tol).all()
    raw = G.sst_input(_dev(x)).cpu().numpy()
    RU.check("sst_input raw", raw, np.where(ok, y64, np.nan), bound)


def test_calls_agree_bitwise_and_a_slab_does_not_see_its_batch():
    R = _R((33, 64), (9, 16))
    x = RU.field((5, 33, 64), seed=22)
    x[2, 5, 7] = np.nan
    for kw in ({}, {"skip_nan": True, "min_valid": 0.2}):
        a = _run(R, x, **kw)
        b = _run(R, x, **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for s in range(5):
            alone = _run(R, x[s:s + 1], **kw)
            assert np.array_equal(alone[0].view(np.uint32), a[s].view(np.uint32)), s
    xd = _dev(x).view(5, 1, 33, 64)                          # as a batch of single channels
    assert np.array_equal(R(xd)[:, 0].cpu().numpy().view(np.uint32), _run(R, x).view(np.uint32))


def test_a_call_captures_in_a_graph_and_does_not_synchronise():
    R = _R((13, 26), (5, 10))
    x1, x2 = RU.field((1, 3, 13, 26), seed=23), RU.field((1, 3, 13, 26), seed=24)
    xd = _dev(x1)
    out = torch.empty(1, 2, 5, 10, device=DEV)
    R(xd, channels=[2, 0], out=out)                          # tables and slab list uploaded here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        R(xd, channels=[2, 0], out=out)
    xd.copy_(_dev(x2))
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().numpy().copy()
    eager = R(xd, channels=[2, 0]).cpu().numpy()
    assert np.array_equal(replayed.view(np.uint32), eager.view(np.uint32))
    torch.cuda.set_sync_debug_mode("error")
    try:
        R(xd, channels=[2, 0], out=out)
        R(xd, skip_nan=True, out=torch.empty(1, 3, 5, 10, device=DEV))
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_the_gradient_is_the_adjoint():
    R = _R((13, 26), (5, 10))
    x = RU.field((2, 3, 13, 26), seed=25)
    g = RU.field((2, 3, 5, 10), seed=26)
    xd = _dev(x).requires_grad_()
    (R(xd) * _dev(g)).sum().backward()
    want, bound = RU.linear(R.T, g)
    RU.check("x.grad", xd.grad.cpu().numpy(), want, bound)
    # a channel list scatters the gradient
    xd = _dev(x).requires_grad_()
    (R(xd, channels=[2, 2]) * _dev(g[:, :2])).sum().backward()
    w2, b2 = RU.linear(R.T, g[:, 0] + g[:, 1])
    grad = xd.grad.cpu().numpy()
    assert not grad[:, :2].any()
    RU.check("x.grad of a repeated channel", grad[:, 2], w2, 2 * b2 + 2 * RU.EPS * np.abs(w2))
    with pytest.raises(NotImplementedError, match="gradient"):
        R(_dev(x).requires_grad_(), skip_nan=True)
    with torch.no_grad():
        assert not R(_dev(x).requires_grad_()).requires_grad


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_rollout_drivers_regrid_what_run_yields(graph):
    """verify(regrid=R) is scoring R(y) by hand and export(regrid=R) delivers pack(R(y)), for
    the very outputs of run() that the driver saw (recorded: a second run need not give the
    same bits)."""
    from test_gpu_ensemble import _rollout
    from msfno_amd import export as X
    from msfno_amd import regrid as G
    from msfno_amd import verification as V
    r, x0, stds = _rollout(graph)
    B, C, H, W = x0.shape
    Ho, Wo = max(H // 3, 2), max(W // 3, 2)
    R = G.Regridder(G.Grid(H, W), G.Grid(Ho, Wo))
    rec, run = [], r.run

    def recording(*args, **kwargs):
        for i, y in run(*args, **kwargs):
            rec.append(y.clone())
            yield i, y

    r.run = recording
    g = torch.Generator().manual_seed(3)
    truths = [torch.randn(B, C, Ho, Wo, generator=g).to(DEV) for _ in range(2)]
    sc = r.verify(x0, truths, 3, every=2, weights="cosine", regrid=R)
    assert len(rec) == 3 and tuple(sc.rmse.shape) == (2, B, C)
    ver = V.Verifier("cosine", Ho, Wo, 2, B, C, device=DEV)
    for k, i in enumerate((0, 2)):
        ver.update(k, R(rec[i]), truths[k])
    want = ver.scores()
    for name in ("rmse", "bias"):
        a, b = getattr(sc, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    del rec[:]
    sel = X.Selection(channels=[C - 1, 0])
    wr = X.ForecastWriter((B, C, Ho, Wo), selection=sel, depth=2, device=DEV)
    assert r.export(x0, 3, wr, every=2, regrid=R) == 2
    wr.flush()
    assert wr.sink.steps == [0, 2] and len(rec) == 3
    for step, item in zip(wr.sink.steps, wr.sink.items):
        p = X.pack(R(rec[step]), sel).copy()
        assert item.shape == (B, 2, Ho, Wo)
        for a, b in ((item.q, p.q), (item.ref, p.ref), (item.exp2, p.exp2)):
            assert np.array_equal(np.asarray(a), np.asarray(b)), step
    del rec[:]
    # the members of an ensemble go through the regridder too
    es = r.verify_ensemble(x0, [t[:1] for t in truths], 3, every=2, regrid=R)
    from msfno_amd import ensemble as E
    ev = E.EnsembleVerifier("uniform", Ho, Wo, 2, B, 1, C, device=DEV)
    for k, i in enumerate((0, 2)):
        ev.update(k, R(rec[i]).view(B, 1, C, Ho, Wo), truths[k][:1])
    a, b = es.crps.cpu().numpy(), ev.scores().crps.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
