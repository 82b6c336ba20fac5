"""RealSHT / InverseRealSHT as autograd ops (msfno_amd/harmonics/sht.py): the backward is
one native transform on an adjoint plan.

Reference: fp64 autograd through oracle.sht_ref, written on real tensors only
(L = sum(Re g Re y + Im g Im y), complex leaves as view_as_complex of a real leaf), so
torch's convention for complex gradients, dL/dRe + i dL/dIm, is what is tested rather
than assumed.  Bound: max error <= 2e-6 x max|want|, the transform parity bound of
test_gpu_parity.py -- the backward is the same kernels with a table rounded once more.
Measured maxima are printed (DESIGN.md section 9c records them)."""
import functools

import pytest
import torch

from oracle import sht_ref as S
from test_gpu_parity import SHT_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAD = (2, 3)
IDS = ["-".join(map(str, c)) for c in SHT_CASES]


def _err(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


@functools.lru_cache(maxsize=None)
def _forward_problem(case, scale=1.0):
    """x, the complex cotangent g and dL/dx in fp64 of the forward transform; computed
    once, shared, never modified."""
    grid, nlat, nlon, lmax, mmax = case
    gen = torch.Generator().manual_seed(17 * nlat + nlon)
    x = torch.randn(*LEAD, nlat, nlon, generator=gen)
    g = torch.view_as_complex(torch.randn(*LEAD, lmax, mmax, 2, generator=gen))
    ref = S.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)
    ref.weights = ref.weights * scale
    xd = x.double().requires_grad_()
    y = torch.view_as_real(ref(xd))
    (y * torch.view_as_real(g).double()).sum().backward()
    return x, g, xd.grad


@functools.lru_cache(maxsize=None)
def _inverse_problem(case):
    grid, nlat, nlon, lmax, mmax = case
    gen = torch.Generator().manual_seed(29 * nlat + nlon)
    a = torch.randn(*LEAD, lmax, mmax, 2, generator=gen)
    g = torch.randn(*LEAD, nlat, nlon, generator=gen)
    ref = S.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)
    ad = a.double().requires_grad_()
    (ref(torch.view_as_complex(ad)) * g.double()).sum().backward()
    return torch.view_as_complex(a), g, torch.view_as_complex(ad.grad)


def _mine(cls, case):
    from msfno_amd import harmonics as H
    grid, nlat, nlon, lmax, mmax = case
    return getattr(H, cls)(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)


@pytest.mark.parametrize("case", SHT_CASES, ids=IDS)
def test_forward_transform_backward_matches_fp64_autograd(case):
    x, g, want = _forward_problem(case)
    mod = _mine("RealSHT", case)
    xg = x.to(DEV).requires_grad_()
    y = mod(xg)
    assert y.requires_grad and y.grad_fn is not None
    # forward values are those of the plain path, bit for bit
    assert torch.equal(y.detach(), mod(x.to(DEV)))
    y.backward(g.to(DEV))
    got = xg.grad
    assert got.dtype == torch.float32 and got.shape == x.shape
    e = _err(got.cpu().double(), want)
    print(f"RealSHT backward {case}: max err / max|want| = {e:.3e}")
    assert e <= 2e-6, e


@pytest.mark.parametrize("case", SHT_CASES, ids=IDS)
def test_inverse_transform_backward_matches_fp64_autograd(case):
    a, g, want = _inverse_problem(case)
    mod = _mine("InverseRealSHT", case)
    ag = a.to(DEV).requires_grad_()
    y = mod(ag)
    assert y.requires_grad and y.grad_fn is not None
    assert torch.equal(y.detach(), mod(a.to(DEV)))
    y.backward(g.to(DEV))
    got = ag.grad
    assert got.dtype == torch.complex64 and got.shape == a.shape
    e = _err(got.cpu().to(torch.complex128), want)
    print(f"InverseRealSHT backward {case}: max err / max|want| = {e:.3e}")
    assert e <= 2e-6, e


def test_no_adjoint_plan_without_a_backward():
    """Calls under no_grad or on inputs that do not require grad take the plain path and
    build no adjoint plan; the first backward builds one per device and keeps it."""
    case = SHT_CASES[0]
    x, g, _ = _forward_problem(case)
    mod = _mine("RealSHT", case)
    xg = x.to(DEV).requires_grad_()
    with torch.no_grad():
        y = mod(xg)
    assert not y.requires_grad
    assert not mod(x.to(DEV)).requires_grad
    assert mod._adj_plans == {}
    y = mod(xg)
    assert mod._adj_plans == {}  # lazily: not before the backward
    y.backward(g.to(DEV))
    assert len(mod._adj_plans) == 1
    plan = next(iter(mod._adj_plans.values()))
    xg.grad = None
    mod(xg).backward(g.to(DEV))
    assert next(iter(mod._adj_plans.values())) is plan and len(mod._adj_plans) == 1


def test_backward_follows_a_rescaled_table():
    """The reference's recipe (sfnonet.py:551-555) re-assigns weights = 1e5 * weights; a
    backward after one on the old table uses the new one."""
    case = SHT_CASES[2]
    x, g, want = _forward_problem(case)
    _, _, want5 = _forward_problem(case, 1e5)
    mod = _mine("RealSHT", case)
    xg = x.to(DEV).requires_grad_()
    mod(xg).backward(g.to(DEV))
    assert _err(xg.grad.cpu().double(), want) <= 2e-6
    mod.weights = 1e5 * mod.weights
    xg.grad = None
    mod(xg).backward(g.to(DEV))
    e = _err(xg.grad.cpu().double(), want5)
    print(f"after the x1e5 rescale: {e:.3e}")
    assert e <= 2e-6, e


def test_gradient_has_the_dtype_and_layout_of_the_input():
    """The cast to fp32 / complex64 and .contiguous() stay inside autograd's view: an
    fp64 (complex128), transposed leaf gets a gradient of its own dtype and strides."""
    case = SHT_CASES[1]
    x, g, want = _forward_problem(case)
    mod = _mine("RealSHT", case)
    xg = x.double().transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2).requires_grad_()
    assert not xg.is_contiguous() and xg.is_leaf
    mod(xg).backward(g.to(DEV))
    assert xg.grad.dtype == torch.float64 and xg.grad.shape == xg.shape
    assert xg.grad.stride() == xg.stride()
    assert _err(xg.grad.cpu(), want) <= 2e-6

    a, g, want = _inverse_problem(case)
    inv = _mine("InverseRealSHT", case)
    ag = (a.to(torch.complex128).transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)
          .requires_grad_())
    assert not ag.is_contiguous() and ag.is_leaf
    inv(ag).backward(g.to(DEV))
    assert ag.grad.dtype == torch.complex128 and ag.grad.shape == ag.shape
    assert ag.grad.stride() == ag.stride()
    assert _err(ag.grad.cpu(), want) <= 2e-6


def test_adopted_foreign_transforms_are_differentiable_too():
    from msfno_amd.harmonics import adopt
    case = SHT_CASES[2]
    grid, nlat, nlon, lmax, mmax = case
    x, g, want = _forward_problem(case)
    fwd = adopt(S.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV), False)
    xg = x.to(DEV).requires_grad_()
    fwd(xg).backward(g.to(DEV))
    assert _err(xg.grad.cpu().double(), want) <= 2e-6
    a, g, want = _inverse_problem(case)
    inv = adopt(S.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV),
                True)
    ag = a.to(DEV).requires_grad_()
    inv(ag).backward(g.to(DEV))
    assert _err(ag.grad.cpu().to(torch.complex128), want) <= 2e-6


def test_cotangent_that_carries_the_lazy_conjugate_bit():
    """L = Re sum(conj(y) z): autograd hands the backward conj(z).conj(), a tensor whose
    conjugate is only a bit that .contiguous() keeps.  L = sum(Re y Re z + Im y Im z), so
    the gradient is that of _forward_problem with z as the cotangent; an unresolved bit
    would flip the sign of the imaginary parts' share."""
    case = SHT_CASES[2]
    x, z, want = _forward_problem(case)
    mod = _mine("RealSHT", case)
    xg = x.to(DEV).requires_grad_()
    (mod(xg).conj() * z.to(DEV)).real.sum().backward()
    e = _err(xg.grad.cpu().double(), want)
    print(f"through y.conj(): {e:.3e}")
    assert e <= 2e-6, e
    # a cross-spectrum: d/da Re sum(sht(a) conj(sht(b))) = adjoint(sht(b)), against fp64
    grid, nlat, nlon, lmax, mmax = case
    ref = S.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)
    b = x.flip(-1).contiguous()
    ad = x.double().requires_grad_()
    (ref(ad) * ref(b.double()).conj()).real.sum().backward()
    ag, bg = x.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    (mod(ag) * mod(bg).conj()).real.sum().backward()
    assert _err(ag.grad.cpu().double(), ad.grad) <= 2e-6
    bd = b.double().requires_grad_()
    (ref(x.double()) * ref(bd).conj()).real.sum().backward()
    assert _err(bg.grad.cpu().double(), bd.grad) <= 2e-6


def test_inputs_and_cotangents_with_lazy_conj_or_neg_bits_are_resolved():
    """c.conj() into the inverse transform, a negated-view field into the forward one and
    a negated-view real cotangent: each gives what its materialised copy gives, bit for
    bit."""
    case = SHT_CASES[2]
    a, g, _ = _inverse_problem(case)
    inv = _mine("InverseRealSHT", case)
    ac = a.to(DEV).conj()
    assert ac.is_conj()
    assert torch.equal(inv(ac), inv(ac.resolve_conj()))
    assert not torch.equal(inv(ac), inv(a.to(DEV)))
    gd = g.to(DEV)
    gneg = torch._neg_view(-gd)  # == gd behind a neg bit, contiguous
    assert gneg.is_neg() and gneg.contiguous().is_neg() and torch.equal(gneg.resolve_neg(), gd)
    assert torch.equal(torch.view_as_real(inv._native_adjoint(gneg)),
                       torch.view_as_real(inv._native_adjoint(gd)))
    fwd = _mine("RealSHT", case)
    x, _, _ = _forward_problem(case)
    xd = x.to(DEV)
    xneg = torch._neg_view(-xd)
    assert xneg.is_neg() and xneg.contiguous().is_neg()
    assert torch.equal(torch.view_as_real(fwd(xneg)), torch.view_as_real(fwd(xd)))
