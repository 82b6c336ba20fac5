"""Forecast verification on the GPU (csrc/verify.hip through msfno_amd/verification.py
and Rollout.verify) against the fp64 restatement (tests/verify_util.py).

Kernel level: msfno_verify_sums at the shapes where the kernel takes another path (single
element, rows shorter than a float4, slabs off the 16-byte grid, nlon % 4 != 0, a row
wider than one sweep of a workgroup, many small slabs, the real 721 x 1440 rows), each
without a climatology, with one for every slab and with a mixed map (some -1, a
batch-broadcast, a permuted stack); outputs and workspace pre-filled with NaN.
  se, ae, pa2, ta2: 1e-5 relative -- the bound tests/test_gpu_loss.py derives, (3 + 128)
        2^-24 for a 128-term sequential fp32 chain of non-negative terms; the kernel's
        chain is that of the loss sums (a lane's share of a row plus one weighted add per
        row it visits, csrc/row_reduce.h), so the bound is unchanged;
  err, cross: 1e-5 of their magnitude sums  sum w |p-t|,  sum w |(p-c)(t-c)|  (the same
        chain on signed terms), the magnitude sums from the restatement.
Scores from GPU sums: |acc - want| <= 3e-5 (by Cauchy-Schwarz the magnitude sum of cross
is at most sqrt(pa2 ta2): 1e-5 from the numerator, 1e-5 from the denominator, slack);
skill within 2e-5 se / ta2; bias within 1e-5 mae.
Driver level: Rollout.verify on the small fixture network against fp64 scoring of run()'s
outputs, 1e-3 of the (magnitude) sums: the step indexing, the pairing and the
denormalisation, not the forward's parity."""
import os

import pytest
import torch

import verify_util as VU

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNEL_SHAPES = [(1, 1, 1, 1), (1, 1, 2, 8), (1, 2, 7, 9), (2, 3, 5, 12), (3, 7, 121, 250),
                 (1, 1, 3, 4100), (1, 73, 45, 90), (1, 2, 721, 1440)]
NONNEG = [0, 2, 3, 4]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _sums(prd, tar, w, clim=None, slab=None, ws=None):
    """msfno_verify_sums on device tensors (any 16-byte phase); NaN-filled output and
    workspace unless a workspace is handed in."""
    from msfno_amd import _native as N
    B, C, H, W = prd.shape
    lib = N.lib()
    nbytes = lib.msfno_verify_workspace_size(B * C, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    if ws is None:
        ws = _nan(nbytes // 4)
    sums = _nan(B, C, 6)
    N.check(lib.msfno_verify_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), N.ptr(clim),
                                  N.ptr(slab), sums.data_ptr(), B * C, H, W, ws.data_ptr(),
                                  nbytes, N.stream_of(prd.device)), "msfno_verify_sums")
    return sums, ws


def _check_sums(tag, got, want, tol=1e-5):
    """Every entry within tol of its magnitude sum (the sum itself for the non-negative
    ones, so that is tol relative); an exact zero where the magnitude sum is zero."""
    want, mag = want
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    assert torch.equal(want[..., NONNEG], mag[..., NONNEG])
    err = (got - want).abs()
    worst = (err / mag.clamp(min=1e-300)).max().item()
    print(f"{tag}: sums max err / magnitude sum {worst:.3e}")
    assert (err <= tol * mag).all(), (tag, worst)


def _device_map(slab):
    return None if slab is None else torch.tensor(slab, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_verify_sums_kernel(shape):
    B, C, H, W = shape
    prd, tar, clim, w, want = VU.problem(shape)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    base = None
    for name, rows, slab in VU.slab_maps(B, C):
        stack = None if rows is None else cd[rows].contiguous()
        sd = _device_map(slab)
        got, ws = _sums(p, t, wd, stack, sd)
        _check_sums(f"{shape} {name}", got, want[name])
        # every workspace word read was written by the call: a second call on the
        # workspace as the first one left it (and a NaN-filled output) is bitwise identical
        again, _ = _sums(p, t, wd, stack, sd, ws=ws)
        assert torch.equal(got, again), name
        if name == "none":
            base = got
            assert (got[..., 3:] == 0).all()
        if name == "mixed":
            miss = (torch.tensor(slab).reshape(B, C) < 0).to(DEV)
            assert miss.any()
            assert (got[miss][:, 3:] == 0).all()
            assert torch.equal(got[miss][:, :3], base[miss][:, :3])
            assert (got[~miss][:, 3:5] > 0).all()


def _shifted(t, k):
    """A contiguous device copy of t that starts k floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k
    return v


@pytest.mark.parametrize("kp,kt,kc", [(1, 1, 1), (3, 3, 3), (0, 2, 0), (2, 2, 1)])
def test_verify_sums_on_views_off_the_16_byte_grid(kp, kt, kc):
    """prd, tar and clim each at their own phase of the 16-byte grid: where all pointers in
    play share a phase the vector path runs with a scalar head and tail, else the scalar
    path ((2, 2, 1): vector without a climatology, scalar with one)."""
    shape = (3, 7, 121, 250)
    prd, tar, clim, w, want = VU.problem(shape)
    p, t, c = _shifted(prd, kp), _shifted(tar, kt), _shifted(clim, kc)
    wd = w.to(DEV)
    got, _ = _sums(p, t, wd)
    _check_sums(f"phase {kp},{kt} none", got, want["none"])
    got, _ = _sums(p, t, wd, c, _device_map(list(range(21))))
    _check_sums(f"phase {kp},{kt},{kc} full", got, want["full"])


@pytest.mark.parametrize("shape", [(3, 7, 121, 250), (1, 2, 721, 1440)],
                         ids=lambda s: "x".join(map(str, s)))
def test_scores_from_gpu_sums(shape):
    from msfno_amd import verification as V
    B, C, H, W = shape
    prd, tar, clim, w, want = VU.problem(shape)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    for name, rows, slab in VU.slab_maps(B, C)[1:]:
        s = V.field_sums(p, t, wd, cd[rows].contiguous(), slab)
        assert s.shape == (B, C, 6) and s.dtype == torch.float32 and s.is_cuda
        _check_sums(f"{shape} {name}", s, want[name])
        has = torch.tensor(slab).reshape(B, C) >= 0
        for batch_mean in (False, True):
            got = V.finish(s, wd, W, batch_mean=batch_mean)
            ref = VU.scores(want[name][0], w.double(), W, has, batch_mean=batch_mean)
            ws = want[name][0].sum(dim=0) if batch_mean else want[name][0]
            g = {k: getattr(got, k).cpu().double() for k in VU.NAMES}
            ok = ~torch.isnan(ref["acc"])
            assert torch.equal(torch.isnan(g["acc"]), ~ok)
            assert torch.equal(torch.isnan(g["skill"]), ~ok)
            assert ok.any()
            e_acc = (g["acc"] - ref["acc"]).abs()[ok].max().item()
            e_skill = ((g["skill"] - ref["skill"]).abs() / (ws[..., 0] / ws[..., 4]))[ok]
            e_bias = (g["bias"] - ref["bias"]).abs() / ref["mae"]
            print(f"{shape} {name} batch_mean={batch_mean}: acc err {e_acc:.3e}, skill err / "
                  f"(se/ta2) {e_skill.max().item():.3e}, bias err / mae "
                  f"{e_bias.max().item():.3e}")
            assert e_acc <= 3e-5
            assert (e_skill <= 2e-5).all()
            assert (e_bias <= 1e-5).all()
            # n = nlon sum(w) is rounded to fp32 and divided by: two more roundings
            for k in ("mse", "mae"):
                assert ((g[k] - ref[k]).abs() <= 1.1e-5 * ref[k]).all(), k
            assert ((g["rmse"] - ref["rmse"]).abs() <= 1e-5 * ref["rmse"]).all()


def test_field_sums_climatology_forms():
    """(B, C, H, W) and (C, H, W) climatologies build (and cache) their slab map; an
    explicit map over a (K, H, W) stack may live on the host or the device."""
    from msfno_amd import verification as V
    shape = (2, 3, 5, 12)
    B, C, H, W = shape
    prd, tar, clim, w, want = VU.problem(shape)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    maps = dict((n, (r, s)) for n, r, s in VU.slab_maps(B, C))
    full = V.field_sums(p, t, wd, cd.view(B, C, H, W))
    _check_sums("clim (B,C,H,W)", full, want["full"])
    raw, _ = _sums(p, t, wd, cd, _device_map(maps["full"][1]))
    assert torch.equal(full, raw)
    bcast = V.field_sums(p, t, wd, cd[:C])
    _check_sums("clim (C,H,W)", bcast, VU.sums(prd.double(), tar.double(), w.double(),
                                               clim[:C].double(), list(range(C)) * B))
    assert V._default_slabs(3, B, C, p.device) is V._default_slabs(3, B, C, p.device)
    rows, slab = maps["mixed"]
    stack = cd[rows].contiguous()
    host = V.field_sums(p, t, wd, stack, slab)
    _check_sums("explicit map", host, want["mixed"])
    assert torch.equal(host, V.field_sums(p, t, wd, stack, _device_map(slab).view(B, C)))
    _check_sums("no clim", V.field_sums(p, t, wd), want["none"])
    with pytest.raises(ValueError):
        V.field_sums(p, t, wd, stack, [C] + slab[1:])      # slab index out of range
    with pytest.raises(ValueError):
        V.field_sums(p, t, wd, stack, slab[:-1])           # one index per (b, c)
    with pytest.raises(ValueError):
        V.field_sums(p, t, wd, cd[:C - 1])                 # neither (C,H,W) nor (B,C,H,W)
    with pytest.raises(ValueError):
        V.field_sums(p, t, wd, None, slab)                 # a map without a climatology


@pytest.mark.parametrize("world", [2, 3])
def test_band_local_sums_add_up_to_the_whole_field(world):
    """A latitude-band rank passes its own rows, w[rows] and clim[..., rows, :]; the ranks'
    (B, C, 6) sums add up to the whole field's.  No communicator involved."""
    from msfno_amd import verification as V
    from msfno_amd.sfno.latband import band_partition, local_rows
    shape = (1, 3, 91, 180)
    prd, tar, clim, w, want = VU.problem(shape)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    row_start, _ = band_partition(world, shape[2], 45, 46)
    total = torch.zeros(1, 3, 6, dtype=torch.float64)
    seen = []
    for rank in range(world):
        rows = local_rows(world, rank, shape[2], row_start)
        seen += rows
        idx = torch.tensor(rows, device=DEV)
        total += V.field_sums(p[:, :, idx], t[:, :, idx], wd[idx], cd[:, idx]).cpu().double()
    assert sorted(seen) == list(range(shape[2]))
    _check_sums(f"world {world} bands", total, want["full"])
    _check_sums(f"world {world} whole", V.field_sums(p, t, wd, cd), want["full"])
    sc = V.finish(total, w.double(), shape[3])
    ref = VU.scores(want["full"][0], w.double(), shape[3], torch.ones(1, 3, dtype=torch.bool))
    assert ((sc.acc - ref["acc"]).abs() <= 3e-5).all()


def _verifier_problem():
    shape = (2, 3, 5, 12)
    prd, tar, clim, w, want = VU.problem(shape)
    return shape, prd.to(DEV), tar.to(DEV), clim.to(DEV).view(shape), w, want


def test_verifier_update_captures_in_a_graph():
    """No allocation, sync or memset on the C side: update records into a graph on the
    current stream and replays on new values in the captured buffers like eager."""
    from msfno_amd import verification as V
    (B, C, H, W), sp, st, sc, w, _ = _verifier_problem()
    sp, st, sc = sp.clone(), st.clone(), sc.clone()
    ver = V.Verifier(w, H, W, 2, B, C, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ver.update(0, sp, st, sc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ver.update(0, sp, st, sc)
    sp.copy_(1.7 * sp + 0.25)
    st.copy_(0.5 * st - 0.125)
    sc.copy_(0.75 * sc + 0.5)
    ver.sums.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    ver.update(1, sp, st, sc)
    assert torch.equal(ver.sums[0], ver.sums[1])
    _check_sums("graph replay", ver.sums[0],
                VU.sums(sp.cpu().double(), st.cpu().double(), w.double(),
                        sc.cpu().double().view(B * C, H, W), list(range(B * C))))


def test_verifier_update_does_not_synchronise():
    from msfno_amd import verification as V
    (B, C, H, W), p, t, c, w, want = _verifier_problem()
    ver = V.Verifier(w, H, W, 3, B, C, device=DEV)
    slab = _device_map(VU.slab_maps(B, C)[2][2])
    stack = c[0].flip(0).contiguous()      # sample 0's slabs in reversed channel order
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ver.update(0, p, t)
        ver.update(1, p, t, c)
        ver.update(2, p, t, stack, slab)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k, name in enumerate(("none", "full", "mixed")):
        _check_sums(f"slot {k}", ver.sums[k], want[name])
    got = ver.scores(batch_mean=True)
    assert got.mse.shape == (3, C) and torch.isnan(got.acc[0]).all()
    # host truths are copied over
    ver.update(0, p, t.cpu(), c.cpu())
    assert torch.equal(ver.sums[0], ver.sums[1])


def test_refusals_on_the_gpu():
    from msfno_amd import verification as V
    x = torch.zeros(1, 2, 4, 8, device=DEV)
    w = torch.ones(4, device=DEV)
    with pytest.raises(ValueError):
        V.field_sums(x.cpu(), x.cpu(), w.cpu())                    # no CPU path
    with pytest.raises(ValueError):
        V.field_sums(x, x.cpu(), w)
    with pytest.raises(ValueError):
        V.field_sums(x, x, torch.ones(5, device=DEV))              # one weight per row
    with pytest.raises(ValueError, match="requires grad"):
        V.field_sums(x.clone().requires_grad_(), x, w)
    with pytest.raises(ValueError, match="requires grad"):
        V.field_sums(x, x.clone().requires_grad_(), w)
    with pytest.raises(ValueError, match="requires grad"):
        V.field_sums(x, x, w, x[0].clone().requires_grad_())
    with pytest.raises(ValueError):
        V.Verifier("uniform", 4, 8, 1, 1, 2, device=DEV).update(0, x[:, :1], x[:, :1])
    with pytest.raises(IndexError):
        V.Verifier("cosine", 4, 8, 1, 1, 2, device=DEV).update(1, x, x)
    with pytest.raises(ValueError):
        V.Verifier(torch.ones(5), 4, 8, 1, 1, 2, device=DEV)


# ---- the driver: Rollout.verify on the small fixture network --------------------------

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
    return Rollout(net, means, stds, graph=graph), x.to(DEV) * stds + means, stds


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_rollout_verify_on_the_fixture_network(graph):
    """5 steps, every = 2: steps 0, 2, 4 are scored.  The truth of a step is the antipode
    (latitude flip, half-turn roll) of that step's own output plus (k + 1) standard
    deviations: a mispaired step or a missing denormalisation changes se by O(1)."""
    from msfno_amd import verification as V
    from msfno_amd.losses import sphere_weights
    r, x0, stds = _rollout(graph)
    B, C, H, W = x0.shape
    outs = [o.clone() for _, o in r.run(x0, 5)]
    scored = [0, 2, 4]
    truths = [(outs[i].flip(2).roll(W // 2, 3) + (k + 1) * stds).contiguous()
              for k, i in enumerate(scored)]
    clim = (0.5 * (outs[1][0] + outs[3][0].flip(1))).contiguous()          # (C, H, W)
    ver = V.Verifier("cosine", H, W, 3, B, C, device=DEV)
    got = r.verify(x0, ((t, clim) for t in truths), 5, every=2, verifier=ver)
    assert all(v.shape == (3, B, C) for v in got)
    w64 = torch.from_numpy(sphere_weights("cosine", H))
    for k, i in enumerate(scored):
        want = VU.sums(outs[i].cpu().double(), truths[k].cpu().double(), w64,
                       clim.cpu().double(), list(range(C)) * B)
        _check_sums(f"step {i}", ver.sums[k], want, tol=1e-3)
    assert torch.isfinite(got.acc).all() and torch.isfinite(got.skill).all()
    # the default: uniform weights (the reference's MSELoss), truths alone, a host truth
    plain = r.verify(x0, [truths[0], truths[1].cpu(), truths[2]], 5, every=2)
    assert plain.mse.shape == (3, B, C) and torch.isnan(plain.acc).all()
    for k, i in enumerate(scored):
        mse = ((outs[i].double() - truths[k].double()) ** 2).mean(dim=(2, 3)).cpu()
        assert ((plain.mse[k].cpu().double() - mse).abs() <= 1e-3 * mse).all()
    with pytest.raises(ValueError, match="ran out"):
        r.verify(x0, truths[:2], 5, every=2)


def test_rollout_verify_refuses_a_sharded_model():
    from msfno_amd.rollout import Rollout

    class Sharded:
        world = 2

    x = torch.zeros(1, 2, 4, 8, device=DEV)
    with pytest.raises(NotImplementedError, match="field_sums"):
        Rollout(Sharded(), graph=False).verify(x, [x], 1)
