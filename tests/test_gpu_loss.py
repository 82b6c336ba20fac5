"""The sphere-weighted losses on the GPU (csrc/loss.hip through msfno_amd/losses.py).

Kernel level: msfno_loss_sums / msfno_loss_backward under arbitrary positive weights
against the fp64 restatement (tests/loss_util.py), outputs and workspace pre-filled with
NaN, at the shapes where the kernels take another path (single element, rows shorter than
a float4, slabs and views off the 16-byte grid, nlon % 4 != 0, a row wider than one sweep
of a workgroup, many small slabs, the real 721 x 1440 rows).
  sums: 1e-5 relative per entry -- the worst-case bound (3 + 128) 2^-24 of a 128-term
        sequential fp32 chain of non-negative terms (a lane's share of a row plus one
        weighted add per row it visits, csrc/row_reduce.h), 10x inside the 1e-4 parity line;
  dprd: 4 x 2^-24 |want| + 1e-30 per element: three fp32 roundings (coefficient,
        difference, product) on exact inputs.
Class level: the three modules against the reference's own fp64 results
(tests/golden/loss/): loss 1e-5 relative, gradient 1e-5 x max|grad| per (b, c) slab (the
channel scales span seven decades; a global bound would hide a broken small channel).
The fixtures have H >= 5: at H = 2 every L2Sphere weight is rounding noise of cos(pi/2).
"""
import functools
import os

import pytest
import torch

import loss_util as LU

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

KERNEL_SHAPES = [(1, 1, 1, 1), (1, 1, 2, 8), (1, 2, 7, 9), (2, 3, 5, 12), (3, 7, 121, 250),
                 (1, 3, 91, 180), (1, 1, 3, 4100), (1, 73, 45, 90), (1, 2, 721, 1440)]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """Inputs (fp32, channel scales 1e-3 .. 1e4), weights, incoming gradient and the fp64
    answers of one shape; computed once, shared, never modified."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 + B + 10 * C + 100 * H + W)
    scale = torch.logspace(-3, 4, C)[None, :, None, None] if C > 1 else torch.ones(1, 1, 1, 1)
    tar = ((torch.randn(shape, generator=g) + 0.5) * scale).float()
    prd = (tar + 0.3 * scale * torch.randn(shape, generator=g)).float()
    w = (torch.rand(H, generator=g) + 0.1).float()
    gnum = torch.randn(B, C, generator=g).float()
    want = LU.sums(prd.double(), tar.double(), w.double())
    dwant = (2.0 * gnum.double()[:, :, None, None] * w.double()[None, None, :, None]
             * (prd.double() - tar.double()))
    return prd, tar, w, gnum, want, dwant


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _sums(prd, tar, w, ws=None):
    """msfno_loss_sums on device tensors (any 16-byte phase); NaN-filled output and
    workspace unless a workspace is handed in."""
    from msfno_amd import _native as N
    B, C, H, W = prd.shape
    lib = N.lib()
    nbytes = lib.msfno_loss_workspace_size(B * C, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    if ws is None:
        ws = _nan(nbytes // 4)
    sums = _nan(B, C, 2)
    N.check(lib.msfno_loss_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), sums.data_ptr(),
                                B * C, H, W, ws.data_ptr(), nbytes, N.stream_of(prd.device)),
            "msfno_loss_sums")
    return sums, ws


def _backward(prd, tar, w, gnum, out=None):
    from msfno_amd import _native as N
    B, C, H, W = prd.shape
    if out is None:
        out = _nan(B, C, H, W)
    N.check(N.lib().msfno_loss_backward(prd.data_ptr(), tar.data_ptr(), w.data_ptr(),
                                        gnum.data_ptr(), out.data_ptr(), B * C, H, W,
                                        N.stream_of(prd.device)), "msfno_loss_backward")
    return out


def _check_sums(tag, got, want):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"{tag}: sums max rel err {rel:.3e}")
    assert rel <= 1e-5, (tag, rel)


def _check_dprd(tag, got, want):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    excess = ((got - want).abs() - (4 * U * want.abs() + 1e-30)).max().item()
    ulps = ((got - want).abs() / (U * want.abs() + 1e-300)).max().item()
    print(f"{tag}: dprd max err {ulps:.2f} x 2^-24 |want|")
    assert excess <= 0, (tag, ulps)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_sums_kernel(shape):
    prd, tar, w, _, want, _ = _problem(shape)
    p, t, wd = prd.to(DEV), tar.to(DEV), w.to(DEV)
    got, ws = _sums(p, t, wd)
    _check_sums(str(shape), got, want)
    # every workspace word read was written by the call: a second call on the workspace
    # as the first one left it (and a NaN-filled output) is bitwise identical
    again, _ = _sums(p, t, wd, ws=ws)
    assert torch.equal(got, again)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_backward_kernel(shape):
    prd, tar, w, gnum, _, dwant = _problem(shape)
    got = _backward(prd.to(DEV), tar.to(DEV), w.to(DEV), gnum.to(DEV))
    _check_dprd(str(shape), got, dwant)


def _shifted(t, k):
    """A contiguous device copy of t that starts k floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k
    return v


@pytest.mark.parametrize("kp,kt,ko", [(1, 1, 1), (3, 3, 0), (0, 2, 0), (2, 0, 3)])
def test_loss_kernels_on_views_off_the_16_byte_grid(kp, kt, ko):
    """prd, tar and dprd each at their own phase of the 16-byte grid: equal phases take the
    vector path with a scalar head and tail, unequal ones the scalar path."""
    shape = (3, 7, 121, 250)
    prd, tar, w, gnum, want, dwant = _problem(shape)
    p, t = _shifted(prd, kp), _shifted(tar, kt)
    got, _ = _sums(p, t, w.to(DEV))
    _check_sums(f"phase {kp},{kt}", got, want)
    out = _shifted(torch.full(shape, float("nan")), ko)
    _backward(p, t, w.to(DEV), gnum.to(DEV), out=out)
    _check_dprd(f"phase {kp},{kt},{ko}", out, dwant)


def _fixture_cases():
    out = []
    for path in LU.fixture_files():
        _, _, cases = LU.load_fixture(path)
        for i, c in enumerate(cases):
            out.append(pytest.param(path, i, id=f"{os.path.basename(path)[:-4]}-{c['reduction']}"))
    return out


@pytest.mark.parametrize("path,i", _fixture_cases())
def test_loss_classes_match_reference_fixtures(path, i):
    from msfno_amd import losses as L
    prd, tar, cases = LU.load_fixture(path)
    c = cases[i]
    assert prd.shape[2] >= 3
    if c["cls"] == "CosineMSELoss":
        mod = L.CosineMSELoss(reduction=c["reduction"])
    else:
        mod = getattr(L, c["cls"])(relative=c["relative"], squared=c["squared"],
                                   reduction=c["reduction"])
    p = prd.float().to(DEV).requires_grad_()
    v = mod(p, tar.float().to(DEV))
    v.backward()
    rel = abs(v.item() - c["loss"].item()) / abs(c["loss"].item())
    err = (p.grad.cpu().double() - c["grad"]).abs().amax(dim=(-1, -2))
    ref = c["grad"].abs().amax(dim=(-1, -2))
    print(f"loss rel err {rel:.3e}, grad max err / slab max {(err / ref).max().item():.3e}")
    assert v.dim() == 0 and rel <= 1e-5, rel
    assert (err <= 1e-5 * ref).all(), (err / ref)


def test_mse_helpers_match_torch_mse():
    from msfno_amd import losses as L
    prd, tar, _ = LU.load_fixture(LU.fixture_files()[-1])
    want = torch.nn.MSELoss()(prd, tar)
    want_c = torch.nn.MSELoss(reduction="none")(prd, tar).mean(dim=(0, 2, 3))
    p, t = prd.float().to(DEV), tar.float().to(DEV)
    got, got_c = L.mse(p, t), L.per_variable_mse(p, t)
    assert got.dim() == 0 and got_c.shape == (prd.shape[1],)
    assert abs(got.item() - want.item()) <= 1e-5 * want.item()
    assert ((got_c.cpu().double() - want_c).abs() <= 1e-5 * want_c).all()


@pytest.mark.parametrize("world", [2, 3])
def test_band_local_sums_add_up_to_the_whole_field(world):
    """A latitude-band rank passes its own rows (msfno_band_local_rows) and w[rows]; the
    ranks' (B, C, 2) sums add up to the whole field's.  No communicator involved."""
    from msfno_amd import losses as L
    from msfno_amd.sfno.latband import band_partition, local_rows
    shape = (1, 3, 91, 180)
    prd, tar, w, _, want, _ = _problem(shape)
    p, t, wd = prd.to(DEV), tar.to(DEV), w.to(DEV)
    row_start, _ = band_partition(world, shape[2], 45, 46)
    total = torch.zeros(1, 3, 2, dtype=torch.float64)
    seen = []
    for rank in range(world):
        rows = local_rows(world, rank, shape[2], row_start)
        seen += rows
        idx = torch.tensor(rows, device=DEV)
        total += L.weighted_sums(p[:, :, idx], t[:, :, idx], wd[idx]).cpu().double()
    assert sorted(seen) == list(range(shape[2]))
    whole = L.weighted_sums(p, t, wd).cpu().double()
    assert ((total - whole).abs() <= 1e-5 * whole.abs()).all()
    assert ((total - want).abs() <= 1e-5 * want.abs()).all()


def test_refusals_on_the_gpu():
    from msfno_amd import losses as L
    x = torch.zeros(1, 2, 4, 8, device=DEV)
    with pytest.raises(NotImplementedError):
        L.L2Sphere(reduction="none")
    with pytest.raises(ValueError):
        L.weighted_sums(x.cpu(), x.cpu(), torch.ones(4))
    with pytest.raises(ValueError):
        L.weighted_sums(x, x, torch.ones(5, device=DEV))  # one weight per latitude row
    with pytest.raises(NotImplementedError):
        L.weighted_sums(x, x.clone().requires_grad_(), torch.ones(4, device=DEV))


def test_weighted_sums_forward_and_backward_capture_in_a_graph():
    """No allocation, sync or memset on the C side: forward + backward record into one
    graph on the current stream and replay on new input values like eager."""
    from msfno_amd import losses as L
    shape = (2, 3, 5, 12)
    prd, tar, w, gnum, _, _ = _problem(shape)
    wd = w.to(DEV)
    gout = torch.stack((gnum, torch.zeros_like(gnum)), dim=-1).to(DEV)
    sp = prd.to(DEV).requires_grad_()
    st = tar.to(DEV)

    def step():
        s = L.weighted_sums(sp, st, wd)
        (g,) = torch.autograd.grad(s, sp, grad_outputs=gout)
        return s, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out, g_out = step()
    with torch.no_grad():  # new values in the captured buffers
        sp.copy_(1.7 * sp + 0.25)
        st.copy_(0.5 * st - 0.125)
    graph.replay()
    torch.cuda.synchronize()
    s_eager, g_eager = step()
    assert torch.equal(s_out, s_eager) and torch.equal(g_out, g_eager)
    want = LU.sums(sp.detach().cpu().double(), st.cpu().double(), w.double())
    assert ((s_out.cpu().double() - want).abs() <= 1e-5 * want.abs()).all()


def test_one_training_step_end_to_end():
    """L2Sphere_noSine(relative, squared, "mean")(net(x), tar).backward() on the small
    plain network (tests/golden/net/net_nl.npz), every parameter requiring grad, against
    fp64 autograd through oracle.sfno_ref.net_forward plus the restatement.  Tolerance and
    conventions are those of test_gpu_film_backward.py (_compare_params): 1e-4 x
    max|grad| per parameter, the oracle under the GPU's ComplexReLU masks, a bias whose
    exact gradient vanishes held to its weight's gradient scale.

    The target is the output field's antipode (flipped in latitude, rotated half way in
    longitude): the statistics of the output in every channel, but an independent
    structure at a distance of about sqrt(2) standard deviations, as in the first steps of
    training.  dL/dy is proportional to y - tar, so the fp32 forward's own error in y
    (6e-5 of a channel's standard deviation here, inside the 1e-4 forward parity) enters
    the gradient divided by |y - tar|: a target within a fraction of a standard deviation
    of the output would measure that amplification, not the backward."""
    import oracle.sfno_ref as R
    from msfno_amd import losses as L
    from test_gpu_film_backward import _compare_params, _masked_oracle, _tap_blocks
    from test_gpu_net import _build
    from test_oracle_net import NET_FIXTURES, load_net, net_cfg
    path = [p for p in NET_FIXTURES if os.path.basename(p) == "net_nl.npz"][0]
    meta, params, x, y, _ = load_net(path)
    net = _build(meta, params)
    assert all(p.requires_grad for p in net.parameters())
    taps = {}
    _tap_blocks(net, taps)
    tar = y.flip(2).roll(y.shape[3] // 2, 3).contiguous()
    loss_fn = L.L2Sphere_noSine(relative=True, squared=True, reduction="mean")
    v = loss_fn(net(x.to(DEV)), tar.to(DEV))
    v.backward()
    cfg = net_cfg(meta)
    pd = {k: (t.double().requires_grad_() if t.is_floating_point() else t)
          for k, t in params.items()}
    tr64 = R.make_net_transforms(cfg, torch.float64)
    orig = R.complex_relu_real
    R.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)
    try:
        yd = R.net_forward(pd, x.double(), cfg, tr64)
        vd = LU.loss("L2Sphere_noSine", yd, tar.double(), "mean", relative=True, squared=True)
        vd.backward()
    finally:
        R.complex_relu_real = orig
    print(f"loss GPU {v.item():.8e} oracle {vd.item():.8e}")
    assert abs(v.item() - vd.item()) <= 1e-4 * abs(vd.item())
    n = _compare_params("train step", list(net.named_parameters()),
                        lambda k: pd[k].grad if pd[k].grad is not None
                        else torch.zeros_like(pd[k]))
    assert n >= 20
