"""The power spectrum and the spectral losses on the GPU (csrc/spectrum.hip through
msfno_amd/harmonics/spectrum.py and msfno_amd/losses.py).

Kernel level: msfno_spectrum_power / msfno_spectrum_power_backward against fp64, outputs
pre-filled with NaN, at the shapes where the kernels take another path (one element, rows
shorter than one 16-byte load, every group width, a row wider than one sweep, many short
rows, odd mmax -- the 16-byte phase alternates from row to row --, slices and views that
shift the phase of the whole tensor).
  power:    1e-5 x want + 1e-30 per entry -- the worst-case bound (3 + 128) 2^-24 of a
            128-term sequential fp32 chain of non-negative terms (csrc/spectrum.hip states
            its own chain, 74 terms);
  backward: 2 x 2^-24 |want| + 1e-30 per component: the coefficient 2 e_m g is exact, the
            product is one rounding (2^-24 relative), 2 is the cap.
Loss level: the three functions against the reference's own fp64 results
(tests/golden/spectral_loss/): loss 1e-5 relative, gradient 1e-5 x max|grad| per (b, c)
slab, the class-level bounds of test_gpu_loss.py (the same recipe in CPU fp32 measures
2.3e-7 and 3.7e-7)."""
import functools

import pytest
import torch

import spectral_util as SU

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

KERNEL_SHAPES = [(1, 1, 1), (1, 1, 2), (2, 3, 5), (3, 7, 9), (2, 32, 33), (1, 2, 1025),
                 (73, 45, 46), (2, 360, 361)]


def _want_power(c):
    a = c.real.double() ** 2 + c.imag.double() ** 2
    return a[..., 0] + 2 * a[..., 1:].sum(dim=-1)


def _want_backward(c, g):
    e = torch.full((c.shape[-1],), 4.0, dtype=torch.float64)
    e[0] = 2.0
    return c.to(torch.complex128) * (g.double()[..., None] * e)


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """Coefficients (complex64, per-n scales spread over 1e-3 .. 1e4), the incoming
    gradient and the fp64 answers of one shape; computed once, shared, never modified."""
    N, lmax, mmax = shape
    gen = torch.Generator().manual_seed(2000 + N + 10 * lmax + 100 * mmax)
    scale = torch.logspace(-3, 4, N)[:, None, None, None] if N > 1 else torch.ones(1, 1, 1, 1)
    c = torch.view_as_complex((torch.randn(N, lmax, mmax, 2, generator=gen) * scale).float())
    g = torch.randn(N, lmax, generator=gen).float()
    return c, g, _want_power(c), _want_backward(c, g)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _power(c):
    """msfno_spectrum_power on a contiguous device tensor at any 16-byte phase."""
    from msfno_amd import _native as N
    n, lmax, mmax = c.shape
    assert c.is_contiguous() and c.dtype == torch.complex64
    out = _nan(n, lmax)
    N.check(N.lib().msfno_spectrum_power(c.data_ptr(), out.data_ptr(), n, lmax, mmax,
                                         N.stream_of(c.device)), "msfno_spectrum_power")
    return out


def _backward(c, g, out=None):
    from msfno_amd import _native as N
    n, lmax, mmax = c.shape
    assert c.is_contiguous() and g.is_contiguous()
    if out is None:
        out = _nan(n, lmax, mmax, dtype=torch.complex64)
    assert out.is_contiguous() and out.shape == c.shape
    N.check(N.lib().msfno_spectrum_power_backward(c.data_ptr(), g.data_ptr(), out.data_ptr(), n,
                                                  lmax, mmax, N.stream_of(c.device)),
            "msfno_spectrum_power_backward")
    return out


def _check_power(tag, got, want):
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    rel = ((got - want).abs() / (want + 1e-300)).max().item()
    print(f"{tag}: power max rel err {rel:.3e}")
    assert ((got - want).abs() <= 1e-5 * want + 1e-30).all(), (tag, rel)


def _check_backward(tag, got, want):
    got = torch.view_as_real(got.cpu().to(torch.complex128))
    want = torch.view_as_real(want)
    assert torch.isfinite(got).all(), tag
    ulps = ((got - want).abs() / (U * want.abs() + 1e-300)).max().item()
    print(f"{tag}: backward max err {ulps:.2f} x 2^-24 |want|")
    assert ((got - want).abs() <= 2 * U * want.abs() + 1e-30).all(), (tag, ulps)


def _shifted(t, k):
    """A contiguous device copy of the complex tensor t that starts k floats past a
    16-byte boundary (k even: a complex tensor sits on the 8-byte grid)."""
    buf = torch.empty(2 * t.numel() + 4, dtype=torch.float32, device=DEV)
    v = torch.view_as_complex(buf[k:k + 2 * t.numel()].view(*t.shape, 2))
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k
    return v


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectrum_power_kernel(shape):
    c, _, want, _ = _problem(shape)
    cd = c.to(DEV)
    got = _power(cd)
    _check_power(str(shape), got, want)
    assert torch.equal(got, _power(cd))  # one writer, fixed order: bitwise reproducible


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectrum_power_backward_kernel(shape):
    c, g, _, dwant = _problem(shape)
    cd, gd = c.to(DEV), g.to(DEV)
    got = _backward(cd, gd)
    _check_backward(str(shape), got, dwant)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(_backward(cd, gd)))


@pytest.mark.parametrize("shape", [(2, 32, 33), (3, 7, 9)], ids=lambda s: "x".join(map(str, s)))
def test_spectrum_kernels_on_a_slice_that_shifts_the_16_byte_phase(shape):
    """c[1:] of an (N + 1, lmax, mmax) tensor: where lmax * mmax is odd (7 x 9) the slice
    starts 8 bytes past a 16-byte boundary and every row's phase flips; where it is even
    (32 x 33) the slice keeps the phase at a storage offset."""
    N, lmax, mmax = shape
    c, g, want, dwant = _problem((N + 1, lmax, mmax))
    cd = c.to(DEV)[1:]
    assert cd.is_contiguous() and cd.data_ptr() % 16 == 8 * ((lmax * mmax) % 2)
    _check_power(f"slice {shape}", _power(cd), want[1:])
    _check_backward(f"slice {shape}", _backward(cd, g.to(DEV)[1:].contiguous()), dwant[1:])


@pytest.mark.parametrize("kc,ko", [(2, 2), (2, 0), (0, 2)])
def test_spectrum_kernels_on_views_off_the_16_byte_grid(kc, ko):
    """Input and gradient output each at their own phase of the 16-byte grid: equal phases
    take the 16-byte path, unequal ones move single complex numbers."""
    shape = (2, 32, 33)
    c, g, want, dwant = _problem(shape)
    cd = _shifted(c, kc)
    _check_power(f"phase {kc}", _power(cd), want)
    out = _shifted(torch.full(shape, float("nan"), dtype=torch.complex64), ko)
    _backward(cd, g.to(DEV), out=out)
    _check_backward(f"phase {kc},{ko}", out, dwant)


def test_degree_zero_is_the_single_coefficient_exactly():
    """A tensor that is zero for m > l: power[..., 0] is |c_00|^2 with weight 1 and nothing
    else.  c_00 has integer parts below 64 times a power of two, so re^2 + im^2 is exact
    in fp32 however it is evaluated."""
    N, lmax, mmax = 5, 9, 11
    gen = torch.Generator().manual_seed(5)
    c = torch.view_as_complex(torch.randn(N, lmax, mmax, 2, generator=gen))
    l = torch.arange(lmax)[:, None]
    m = torch.arange(mmax)[None, :]
    c = torch.where(m <= l, c, torch.zeros_like(c))
    c00 = torch.randint(-63, 64, (N, 2), generator=gen).float() * 2.0 ** -7
    c[:, 0, 0] = torch.view_as_complex(c00)
    got = _power(c.to(DEV).contiguous()).cpu()
    assert torch.equal(got[:, 0], c00[:, 0] ** 2 + c00[:, 1] ** 2)


def test_power_spectrum_function_and_refusals():
    from msfno_amd.harmonics import power_spectrum
    c, g, want, dwant = _problem((3, 7, 9))
    cd = c.to(DEV).view(1, 3, 7, 9).requires_grad_()
    p = power_spectrum(cd)
    assert p.shape == (1, 3, 7) and p.dtype == torch.float32 and p.requires_grad
    p.backward(g.to(DEV).view(1, 3, 7))
    _check_power("function", p.detach()[0], want)
    _check_backward("function", cd.grad[0], dwant)
    # a complex128, non-contiguous leaf gets a gradient of its own dtype and shape
    c2 = c.to(torch.complex128).transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)
    c2.requires_grad_()
    power_spectrum(c2).backward(g.to(DEV))
    assert c2.grad.dtype == torch.complex128 and c2.grad.shape == c2.shape
    _check_backward("complex128", c2.grad.to(torch.complex64), dwant)
    with pytest.raises(ValueError):
        power_spectrum(c)                                    # CPU
    with pytest.raises(ValueError):
        power_spectrum(torch.zeros(0, 3, 4, dtype=torch.complex64, device=DEV))
    with pytest.raises(ValueError):
        power_spectrum(torch.zeros(4, dtype=torch.complex64, device=DEV))


def test_power_spectrum_forward_and_backward_capture_in_a_graph():
    """No allocation, sync or memset on the C side: forward + backward record into one
    graph and replay on new input values bitwise like eager."""
    from msfno_amd.harmonics import power_spectrum
    c, g, _, _ = _problem((2, 32, 33))
    sc = c.to(DEV).requires_grad_()
    gd = g.to(DEV)

    def step():
        p = power_spectrum(sc)
        (d,) = torch.autograd.grad(p, sc, grad_outputs=gd)
        return p, d

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p_out, d_out = step()
    with torch.no_grad():  # new values in the captured buffer
        sc.copy_(1.7 * sc + 0.25)
    graph.replay()
    torch.cuda.synchronize()
    p_eager, d_eager = step()
    assert torch.equal(p_out, p_eager)
    assert torch.equal(torch.view_as_real(d_out), torch.view_as_real(d_eager))
    _check_power("graph", p_out, _want_power(sc.detach().cpu()))


def _solver(f):
    from msfno_amd.harmonics import RealSHT
    from types import SimpleNamespace
    return SimpleNamespace(sht=RealSHT(f["nlat"], f["nlon"], lmax=f["lmax"], mmax=f["mmax"],
                                       grid=f["grid"]).float().to(DEV))


def _loss_fn(name):
    from msfno_amd import losses as L
    return {"l2": L.spectral_l2loss_sphere, "spectral": L.spectral_loss_sphere,
            "h1": L.h1loss_sphere}[name]


def _check_grad(tag, got, want):
    err = (got.cpu().double() - want).abs().amax(dim=(-1, -2))
    ref = want.abs().amax(dim=(-1, -2))
    print(f"{tag}: grad max err / slab max {(err / ref).max().item():.3e}")
    assert (err <= 1e-5 * ref).all(), (tag, err / ref)


@pytest.mark.parametrize("path", SU.fixture_files(), ids=SU.fixture_id)
def test_losses_match_reference_fixtures(path):
    f = SU.load_fixture(path)
    p = f["prd"].float().to(DEV).requires_grad_()
    v = _loss_fn(f["fn"])(_solver(f), p, f["tar"].float().to(DEV), relative=f["relative"],
                          squared=f["squared"])
    v.backward()
    rel = abs(v.item() - f["loss"].item()) / abs(f["loss"].item())
    print(f"loss rel err {rel:.3e}")
    assert v.dim() == 0 and rel <= 1e-5, rel
    _check_grad(SU.fixture_id(path), p.grad, f["grad"])


def test_target_gradient_matches_fp64_autograd():
    """Relative l2 at 24 x 48 with a target that requires grad: both gradients against fp64
    autograd of the restatement."""
    path = [q for q in SU.fixture_files() if SU.fixture_id(q) == "l2_rel_sq_2x3x24x48_l24m25lg"]
    f = SU.load_fixture(path[0])
    pd, td = f["prd"].clone().requires_grad_(), f["tar"].clone().requires_grad_()
    vd = SU.loss("l2", SU.oracle_sht(f), pd, td, relative=True, squared=True)
    vd.backward()
    assert (pd.grad - f["grad"]).abs().max() <= 1e-12 * f["grad"].abs().max()
    p = f["prd"].float().to(DEV).requires_grad_()
    t = f["tar"].float().to(DEV).requires_grad_()
    v = _loss_fn("l2")(_solver(f), p, t, relative=True, squared=True)
    v.backward()
    assert abs(v.item() - vd.item()) <= 1e-5 * abs(vd.item())
    _check_grad("d/dprd", p.grad, pd.grad)
    _check_grad("d/dtar", t.grad, td.grad)


def test_the_transform_itself_in_place_of_a_solver():
    path = [q for q in SU.fixture_files() if SU.fixture_id(q) == "h1_abs_sqrt_2x3x5x12_l5m7eq"]
    f = SU.load_fixture(path[0])
    p = f["prd"].float().to(DEV).requires_grad_()
    v = _loss_fn("h1")(_solver(f).sht, p, f["tar"].float().to(DEV), squared=False)
    v.backward()
    assert abs(v.item() - f["loss"].item()) <= 1e-5 * abs(f["loss"].item())
    _check_grad("transform as solver", p.grad, f["grad"])


def test_real_size_power_spectrum_is_finite():
    """721 x 1440 at lmax 360, mmax 361 (odd: the 16-byte phase alternates over 1440
    rows), forward and backward: finite everywhere, offsets past a slab included."""
    from msfno_amd.harmonics import RealSHT, power_spectrum
    sht = RealSHT(721, 1440, lmax=360, mmax=361).float().to(DEV)
    x = torch.randn(1, 4, 721, 1440, device=DEV).requires_grad_()
    p = power_spectrum(sht(x))
    assert p.shape == (1, 4, 360) and torch.isfinite(p).all() and (p > 0).all()
    p.sum().backward()
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    assert x.grad.abs().amax(dim=(-1, -2)).min() > 0
