"""The spherical random fields on the GPU: ``msfno_noise_spectral`` against the fp64
reference stream (tests/noise_ref.py), its independence of how fields are split over calls,
the AR(1) update, the device draw counter, the ``GaussianRandomFieldS2`` / ``SphericalAR1``
modules, ``ensemble.perturb`` and the ``Rollout`` noise hook.  Outputs are pre-filled with
NaN, so an element the kernel leaves out fails every comparison."""
import numpy as np
import pytest
import torch

import noise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# seed 7, draw 5: the one-coefficient case (1, 1, 1) then has a float32 reference error of
# 2.2 and 1.4 ulp (K = 1, K = 3), a typical one; over 12 seeds it ranges from 0.05 to 5.6
# ulp, and a bound taken from a single lucky rounding would say nothing
SEED, DRAW = 7, 5

SHAPES = [
    (1, 1, 1),        # smallest
    (3, 5, 7),        # odd mmax wider than lmax; the 16-byte phase alternates by row
    (2, 9, 4),        # mmax < lmax, even
    (1, 33, 33),      # square
    (70, 16, 17),     # many short fields
    (64, 64, 65),     # 135,168 Philox blocks
    (64, 128, 129),   # 532,480 Philox blocks: more than the 2,048 x 256 lanes of one pass of
                      # the launch, so the grid-stride runs
]


def table(K, lmax):
    """(K, lmax) fp32 in [0.5, 1.5), every row and degree different."""
    return (0.5 + (np.arange(K * lmax).reshape(K, lmax) * 0.37 % 1.0)).astype(np.float32)


def nan_coeffs(n, lmax, mmax, offset=0):
    """(n, lmax, mmax) complex64 of NaN; ``offset`` complex numbers into a larger buffer (an
    odd offset leaves the 16-byte grid)."""
    buf = torch.full((n * lmax * mmax + offset,), complex(float("nan"), float("nan")),
                     dtype=torch.complex64, device=DEV)
    return buf[offset:].view(n, lmax, mmax)


def fill(n, lmax, mmax, se, seed=SEED, draw=DRAW, field0=0, a=0.0, b=1.0, prev=None, out=None,
         draw_dev=None, offset=0):
    from msfno_amd import _native as N
    se = torch.as_tensor(se, device=DEV).reshape(-1, lmax).contiguous()
    if out is None:
        out = nan_coeffs(n, lmax, mmax, offset)
    N.check(N.lib().msfno_noise_spectral(out.data_ptr(), N.ptr(prev), se.data_ptr(), se.shape[0],
                                         n, field0, lmax, mmax, a, b, seed, draw,
                                         N.ptr(draw_dev), N.stream_of(out.device)),
            "msfno_noise_spectral")
    return out


def check_values(got, want64, want32, what):
    """max |got - fp64| <= 4 max |float32 numpy - fp64| (the inputs u are exact in both
    precisions, so this compares function evaluation only: the 4 covers a <= 2 ulp device
    log / sincos against numpy's <= 1 ulp and one more rounding of the angle)."""
    got = got.cpu().numpy().astype(np.complex128)
    assert np.isfinite(got.view(np.float64)).all(), f"{what}: an element was not written"
    err = np.abs(got - want64).max()
    err32 = np.abs(want32.astype(np.complex128) - want64).max()
    print(f"{what}: max abs error {err:.3e}, float32 numpy {err32:.3e}")
    assert err <= 4 * err32, (what, err, err32)
    return got


def check_zeros(got, lmax, mmax):
    l, m = np.arange(lmax)[:, None], np.arange(mmax)[None, :]
    assert (got[:, m > l] == 0).all()
    assert (got[..., 0].imag == 0).all()


@pytest.mark.parametrize("K,field0", [(1, 0), (3, 2)])
@pytest.mark.parametrize("n,lmax,mmax", SHAPES)
def test_values_match_the_reference_stream(n, lmax, mmax, K, field0):
    """Measured on an MI355X, max abs error against fp64, kernel / float32 numpy (the kernel
    forms the angle as sincospi(2 u), which spares it the rounding of 2 pi u that numpy has):

        (n, lmax, mmax)   K = 1, field0 = 0     K = 3, field0 = 2
        (1, 1, 1)         1.3e-8 / 1.3e-7       6.8e-8 / 1.7e-7
        (3, 5, 7)         1.6e-7 / 5.8e-7       1.3e-7 / 5.1e-7
        (2, 9, 4)         2.1e-7 / 4.7e-7       2.1e-7 / 7.3e-7
        (1, 33, 33)       4.0e-7 / 9.8e-7       4.7e-7 / 7.9e-7
        (70, 16, 17)      5.7e-7 / 1.3e-6       6.6e-7 / 1.2e-6
        (64, 64, 65)      6.1e-7 / 1.7e-6       5.8e-7 / 1.4e-6
        (64, 128, 129)    7.5e-7 / 1.7e-6       7.5e-7 / 1.5e-6
    """
    se = table(K, lmax)
    want64 = R.spectral(SEED, DRAW, n, field0, lmax, mmax, se)
    want32 = R.spectral(SEED, DRAW, n, field0, lmax, mmax, se, dtype=np.float32)
    got = check_values(fill(n, lmax, mmax, se, field0=field0), want64, want32,
                       f"{(n, lmax, mmax)} K={K}")
    check_zeros(got, lmax, mmax)


@pytest.mark.parametrize("n,lmax,mmax", [(3, 5, 7), (2, 9, 4), (70, 16, 17)])
def test_values_do_not_depend_on_the_16_byte_phase(n, lmax, mmax):
    """An output one complex number off the 16-byte grid holds the same bits."""
    se = table(3, lmax)
    assert torch.equal(fill(n, lmax, mmax, se, field0=2, offset=1),
                       fill(n, lmax, mmax, se, field0=2))


def test_split_calls_seed_and_draw():
    """n = 5 in one call equals [0:2] and [2:5] with field0 = 0 and 2, bitwise; another
    seed, another draw (in either counter word) give other numbers."""
    lmax, mmax = 16, 17
    se = table(3, lmax)
    whole = fill(5, lmax, mmax, se)
    assert torch.equal(whole[:2], fill(2, lmax, mmax, se, field0=0))
    assert torch.equal(whole[2:], fill(3, lmax, mmax, se, field0=2))
    inside = whole != 0
    for other in (fill(5, lmax, mmax, se, seed=SEED + 1), fill(5, lmax, mmax, se, draw=DRAW + 1),
                  fill(5, lmax, mmax, se, seed=SEED + (1 << 32)),
                  fill(5, lmax, mmax, se, draw=DRAW + (1 << 32))):
        assert (other[inside] != whole[inside]).float().mean().item() > 0.99
    assert not torch.equal(whole[0], whole[3])   # fields 0 and 3 share row 0 of the table


@pytest.mark.parametrize("n,lmax,mmax", [(3, 5, 7), (2, 9, 4), (1, 33, 33)])
@pytest.mark.parametrize("offset", [0, 1])
def test_ar1_update(n, lmax, mmax, offset):
    """a prev + b sqrt_eig xi against the reference with prev separate and in place; the
    triangle m > l is zero although prev is not.  Measured on an MI355X (max abs error
    against fp64, kernel / float32 numpy; the same on and off the 16-byte grid):
    (3, 5, 7) 1.5e-7 / 3.6e-7, (2, 9, 4) 1.2e-7 / 2.7e-7, (1, 33, 33) 2.1e-7 / 4.7e-7."""
    a, b = 0.8, 0.6
    se = table(3, lmax)
    g = torch.Generator().manual_seed(n * lmax)
    prev = torch.randn(n, lmax, mmax, dtype=torch.complex64, generator=g) + (1 + 1j)
    pd = nan_coeffs(n, lmax, mmax, offset)
    pd.copy_(prev)
    want64 = R.spectral(SEED, DRAW, n, 1, lmax, mmax, se, a, b, prev.numpy())
    want32 = R.spectral(SEED, DRAW, n, 1, lmax, mmax, se, a, b, prev.numpy(), dtype=np.float32)
    sep = fill(n, lmax, mmax, se, field0=1, a=a, b=b, prev=pd)
    got = check_values(sep, want64, want32, f"AR(1) {(n, lmax, mmax)} offset {offset}")
    l, m = np.arange(lmax)[:, None], np.arange(mmax)[None, :]
    assert (got[:, m > l] == 0).all()
    assert torch.equal(pd.cpu(), prev)            # a separate prev is only read
    fill(n, lmax, mmax, se, field0=1, a=a, b=b, prev=pd, out=pd)
    assert torch.equal(pd, sep)                   # in place: the same bits
    # without prev, a is ignored
    assert torch.equal(fill(n, lmax, mmax, se, a=123.0), fill(n, lmax, mmax, se))


@pytest.mark.parametrize("d", [41, (1 << 32) - 1])
def test_device_draw_counter(d):
    """Two step-style calls through draw_dev equal host-draw calls at d and d + 1, bitwise,
    and the counter then reads d + 2 (the second d crosses into the high counter word)."""
    from msfno_amd import _native as N
    n, lmax, mmax = 3, 9, 9
    se = table(1, lmax)
    ctr = torch.from_numpy(np.array([d], dtype=np.uint64)).to(DEV)
    got = []
    for _ in range(2):
        got.append(fill(n, lmax, mmax, se, draw=999, draw_dev=ctr))
        N.check(N.lib().msfno_noise_advance(ctr.data_ptr(), 1, N.stream_of(ctr.device)),
                "msfno_noise_advance")
    assert torch.equal(got[0], fill(n, lmax, mmax, se, draw=d))
    assert torch.equal(got[1], fill(n, lmax, mmax, se, draw=d + 1))
    assert not torch.equal(got[0], got[1])
    assert ctr.cpu().numpy()[0] == d + 2


def _field(grid, nlat, nlon, K, seed=11):
    from msfno_amd.harmonics import GaussianRandomFieldS2, matern_sqrt_eig, unit_variance
    lmax = min(nlat, nlon // 2)
    se = unit_variance(matern_sqrt_eig(lmax))
    if K is not None:
        se = torch.stack([se * (k + 1) for k in range(K)])
    return GaussianRandomFieldS2(nlat, nlon, grid=grid, sqrt_eig=se, seed=seed).to(DEV)


@pytest.mark.parametrize("K", [None, 1, 3])
@pytest.mark.parametrize("grid,nlat,nlon", [("equiangular", 17, 32), ("legendre-gauss", 24, 48)])
def test_module_shapes_deterministic_form_and_state_dict(grid, nlat, nlon, K):
    from msfno_amd.harmonics import InverseRealSHT
    g = _field(grid, nlat, nlon, K)
    L = g.lmax
    lead = (2,) if K is None else (2, K)
    assert (g.lmax, g.mmax) == (min(nlat, nlon // 2),) * 2
    # forward(N, xi) = InverseRealSHT(xi * sqrt_eig), bitwise
    gen = torch.Generator().manual_seed(3)
    xi = torch.randn(*lead, L, L, dtype=torch.complex64, generator=gen).to(DEV)
    isht = InverseRealSHT(nlat, nlon, lmax=L, mmax=L, grid=grid).float().to(DEV)
    want = isht(xi * g.sqrt_eig.unsqueeze(-1))
    assert g.next_draw == 0
    got = g(2, xi=xi)
    assert got.shape == lead + (nlat, nlon) and got.dtype == torch.float32
    assert torch.equal(got, want) and g.next_draw == 0
    # sample_coeffs: the kernel's stream at (seed, draw), one draw per call
    c0 = g.sample_coeffs(2)
    assert c0.shape == lead + (L, L) and c0.dtype == torch.complex64
    assert torch.equal(c0.reshape(-1, L, L), fill(2 * g.nrows, L, L, g.sqrt_eig, seed=11, draw=0))
    assert g.rng_state.tolist() == [11, 1]
    # a state_dict round trip into a fresh module continues the stream
    fresh = _field(grid, nlat, nlon, K, seed=0)
    fresh.load_state_dict(g.state_dict())
    f1 = fresh(2)
    assert f1.shape == lead + (nlat, nlon)
    c1 = g.sample_coeffs(2)
    assert torch.equal(f1, g.isht(c1)) and not torch.equal(c1, c0)
    assert torch.equal(c1.reshape(-1, L, L), fill(2 * g.nrows, L, L, g.sqrt_eig, seed=11, draw=1))
    assert fresh.rng_state.tolist() == g.rng_state.tolist() == [11, 2]


def test_power_per_degree_statistics():
    """256 fields at lmax 16, a fixed seed: the mean power of every degree l >= 1 lies within
    1 +- 5 sqrt(2 / (256 (2l + 1))) of (2l + 1) S_l (the reference stream stays within 4 of
    those deviations: test_noise_host)."""
    from msfno_amd.harmonics import GaussianRandomFieldS2, matern_sqrt_eig, power_spectrum
    L = R.STAT_LMAX
    se = matern_sqrt_eig(L)
    g = GaussianRandomFieldS2(L, sqrt_eig=se, seed=R.STAT_SEED).to(DEV)
    c = g.sample_coeffs(R.STAT_FIELDS)
    l = torch.arange(1, L, dtype=torch.float64)
    S = (se.float().double() ** 2)[1:]
    ratio = power_spectrum(c).double().mean(0).cpu()[1:] / ((2 * l + 1) * S)
    dev = (ratio - 1) / torch.from_numpy(R.degree_power_sigma(R.STAT_FIELDS, L))
    print("deviations per degree:", [round(v, 2) for v in dev.tolist()])
    assert dev.abs().max().item() <= 5.0
    # the fields themselves: variance field_variance(sqrt_eig) at every latitude.  A row has
    # at least 256 independent Gaussian samples (at a pole the 32 longitudes are one point),
    # so its variance estimate has a relative deviation of at most sqrt(2 / 256); 5 of them
    from msfno_amd.harmonics import field_variance
    var = g.isht(c).double().pow(2).mean(dim=(0, 2)).cpu()
    rel = var / field_variance(se.float()) - 1
    print("variance per latitude, relative:", [round(v, 3) for v in rel.tolist()])
    assert (rel.abs() <= 5 * (2 / 256) ** 0.5).all()


@pytest.mark.parametrize("K", [3, None])
def test_perturb(K):
    from msfno_amd import ensemble as E
    from msfno_amd import _fields as F
    C, H, W, M = 3, 17, 32, 6
    g = _field("equiangular", H, W, K)
    gen = torch.Generator().manual_seed(2)
    x0 = (300 + torch.randn(C, H, W, generator=gen)).to(DEV)
    amp = torch.tensor([1.0, 0.0, 0.5])
    ens = E.perturb(x0, M, g, amplitude=amp)
    assert ens.shape == (M, C, H, W) and ens.dtype == torch.float32 and g.next_draw == 1
    mean = ens.double().mean(0)
    assert (mean - x0.double()).abs().max().item() <= 2.0 ** -23 * x0.abs().max().item()
    assert all(torch.equal(ens[i, 1], x0[1]) for i in range(M))
    d = ens - x0
    assert not torch.equal(d[0], d[2]) and not torch.equal(d[0, 0], d[0, 2])
    assert (d[0, 0] + d[1, 0]).abs().max().item() <= 2.0 ** -22 * 310
    assert d[:, 0].std().item() > 0.1 and d[:, 2].std().item() > 0.1
    assert torch.equal(E.perturb(x0[None], M, g, amplitude=0.0), x0.expand(M, C, H, W))
    free = E.perturb(x0, 3, g, amplitude=0.25, centred=False)
    assert free.shape == (3, C, H, W) and not torch.equal(free[0], free[1])
    w = F.lat_weights("cosine", H, x0.device)
    sums, hist = E.ensemble_sums(ens.view(M, 1, C, H, W), x0[None], w)
    assert sums.shape == (1, C, E.NSUMS) and hist.shape == (1, C, M + 1)
    assert torch.isfinite(sums).all()
    assert sums[0, 1].abs().max().item() == 0      # the unperturbed channel has no spread


def test_ar1_process_steps_and_graph_replay():
    """reset() is draw 0 of the process's key, step() the in-place update at the device
    counter; a captured step yields new noise on every replay, the same as eager steps."""
    from msfno_amd.harmonics import SphericalAR1
    g = _field("equiangular", 17, 32, 3)
    L, phi = g.lmax, 0.75
    p = SphericalAR1(g, (2, 3), dt=6.0, tau_t=6.0 / -np.log(phi))
    assert abs(p.phi - phi) < 1e-15
    a, b = phi, float(np.sqrt(1 - phi * phi))
    want = fill(6, L, L, g.sqrt_eig, seed=p.seed, draw=0)
    assert torch.equal(p.coeffs.view(6, L, L), want)
    fields = []
    for k in (1, 2, 3):
        prev = want.clone()
        want = fill(6, L, L, g.sqrt_eig, seed=p.seed, draw=k, a=a, b=b, prev=prev)
        f = p.step()
        assert f.shape == (2, 3, 17, 32)
        assert torch.equal(p.coeffs.view(6, L, L), want) and torch.equal(f, g.isht(p.coeffs))
        fields.append(f)
    assert p.counter.cpu().numpy()[0] == 4
    q = SphericalAR1(g, (2, 3), phi=phi)
    q.step()                                       # warm-up: the transform's plan
    q.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = q.step()
    for k in range(3):
        graph.replay()
        assert torch.equal(out, fields[k])
    assert q.counter.cpu().numpy()[0] == 4
    # one spectrum serves every channel, with different noise per channel
    one = SphericalAR1(_field("equiangular", 17, 32, None), (1, 4), phi=0.5)
    f = one.step()
    assert f.shape == (1, 4, 17, 32) and not torch.equal(f[0, 0], f[0, 1])
    with pytest.raises(ValueError):
        SphericalAR1(g, (2, 4), phi=0.5)


def _net():
    from test_rollout import _small_net
    net, params, x, meta = _small_net()
    net.load_state_dict(params, strict=False)
    net = net.eval().to(DEV)
    gen = torch.Generator().manual_seed(1)
    means = torch.randn(1, meta["in_chans"], 1, 1, generator=gen).to(DEV)
    stds = (torch.rand(1, meta["in_chans"], 1, 1, generator=gen) + 0.5).to(DEV)
    return net, means, stds, x.to(DEV) * stds + means, meta


def _noise(meta, B):
    from msfno_amd.harmonics import (GaussianRandomFieldS2, SphericalAR1, matern_sqrt_eig,
                                     unit_variance)
    g = GaussianRandomFieldS2(meta["nlat"], meta["nlon"], seed=5,
                              sqrt_eig=0.05 * unit_variance(matern_sqrt_eig(32))).to(DEV)
    return SphericalAR1(g, (B, meta["in_chans"]), phi=0.9)


def test_rollout_with_noise_graph_and_eager_agree():
    """The 33 x 64, C = 16 network: graph and eager rollouts with the same seed agree step by
    step to the bound of the graph-vs-eager rollout test, and differ from the rollout without
    noise."""
    from msfno_amd.rollout import Rollout
    net, means, stds, x0, meta = _net()
    B = x0.shape[0]
    eager = [o.clone() for _, o in Rollout(net, means, stds, graph=False,
                                           noise=_noise(meta, B)).run(x0, 3)]
    graph = [o.clone() for _, o in Rollout(net, means, stds, graph=True,
                                           noise=_noise(meta, B)).run(x0, 3)]
    plain = [o.clone() for _, o in Rollout(net, means, stds, graph=False).run(x0, 3)]
    for e, g, p in zip(eager, graph, plain):
        assert (g - e).abs().max().item() < 1e-5 * max(1.0, e.abs().max().item())
        assert (e - p).abs().max().item() > 1e-3
    with pytest.raises(ValueError):
        next(Rollout(net, means, stds, noise=_noise(meta, B + 1)).run(x0, 1))


@pytest.mark.parametrize("graph", [False, True])
def test_rollout_noise_differs_from_step_to_step(graph):
    """With a model that returns zeros the outputs are the noise fields: those of an equal
    process stepped by hand, bitwise, and different at every step."""
    from msfno_amd.rollout import Rollout
    meta = {"nlat": 33, "nlon": 64, "in_chans": 5}
    r = Rollout(torch.zeros_like, graph=graph, noise=_noise(meta, 2))
    outs = [o.clone() for _, o in r.run(torch.ones(2, 5, 33, 64, device=DEV), 3)]
    by_hand = _noise(meta, 2)
    for o in outs:
        assert torch.equal(o, by_hand.step())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    # red in time: neighbouring steps correlate at about phi = 0.9
    c = torch.corrcoef(torch.stack([outs[0].flatten(), outs[1].flatten()]))[0, 1].item()
    assert 0.8 < c < 0.97


def test_rollout_without_noise_is_unchanged():
    from msfno_amd.rollout import Rollout
    net, means, stds, x0, meta = _net()
    outs = [o.clone() for _, o in Rollout(net, means, stds, graph=False, noise=None).run(x0, 2)]
    with torch.no_grad():
        s = (x0 - means) / stds
        for o in outs:
            s = net(s)
            assert torch.equal(o, s * stds + means)
