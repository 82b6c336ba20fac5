"""RealVectorSHT / InverseRealVectorSHT and the wind diagnostics on the GPU, against the
dense fp64 reference of vector_util (independent tables, einsums of the definitions).

Bound of the transforms and their backwards: max error <= 4e-6 x max|want|: each output is
the sum of two scalar transforms, each held to 2e-6 in test_gpu_parity.py.  Measured maxima
are printed (DESIGN.md section 9e records them)."""
import functools
import math

import numpy as np
import pytest
import torch

import vector_util as VU
from oracle import sht_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAD = (2, 3)
CASES = [
    ("equiangular", 13, 26, 7, 9),       # generic FFT, poles, zero m-blocks
    ("equiangular", 33, 64, 32, 33),     # codelet, Nyquist column, lmax + 1 = nlat
    ("legendre-gauss", 24, 48, 24, 25),  # lmax + 1 > nlat
    ("legendre-gauss", 20, 45, 20, 21),  # odd nlon
    ("legendre-gauss", 120, 240, 60, 61),
    ("legendre-gauss", 16, 32, 385, 17),  # the two plans on either side of the 384-degree edge
]
IDS = ["-".join(map(str, c)) for c in CASES]
KNOWN = ("legendre-gauss", 24, 48, 12, 12)  # no Nyquist column
BOUND = 4e-6


def _err(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


def _mods(case):
    from msfno_amd import harmonics as H
    grid, nlat, nlon, lmax, mmax = case
    return (H.RealVectorSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV),
            H.InverseRealVectorSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV))


@functools.lru_cache(maxsize=None)
def _forward_problem(case, grad=False):
    """v, the cotangent g, the fp64 coefficients (complex) and, with grad, dL/dv of
    L = sum(Re g Re y + Im g Im y); computed once, shared, never modified."""
    grid, nlat, nlon, lmax, mmax = case
    gen = torch.Generator().manual_seed(31 * nlat + nlon)
    v = torch.randn(*LEAD, 2, nlat, nlon, generator=gen)
    g = torch.randn(*LEAD, 2, lmax, mmax, 2, generator=gen)
    dw, qw = VU.torch_tables(grid, nlat, lmax, mmax, False)
    vd = v.double().requires_grad_(grad)
    y = VU.dense_analysis(vd, dw, qw)
    if grad:
        (y * g.double()).sum().backward()
    return v, torch.view_as_complex(g), torch.view_as_complex(y.detach()), vd.grad


@functools.lru_cache(maxsize=None)
def _inverse_problem(case, grad=False):
    grid, nlat, nlon, lmax, mmax = case
    gen = torch.Generator().manual_seed(37 * nlat + nlon)
    a = torch.randn(*LEAD, 2, lmax, mmax, 2, generator=gen)
    g = torch.randn(*LEAD, 2, nlat, nlon, generator=gen)
    d, q = VU.torch_tables(grid, nlat, lmax, mmax, True)
    ad = a.double().requires_grad_(grad)
    y = VU.dense_synthesis(ad, d, q, nlon)
    if grad:
        (y * g.double()).sum().backward()
    return (torch.view_as_complex(a), g, y.detach(),
            torch.view_as_complex(ad.grad) if grad else None)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_matches_dense_fp64(case):
    v, _, want, _ = _forward_problem(case)
    fwd, _ = _mods(case)
    got = fwd(v.to(DEV))
    assert got.dtype == torch.complex64 and got.shape == want.shape
    grid, nlat, nlon, lmax, mmax = case
    l, m = torch.arange(lmax)[:, None], torch.arange(mmax)[None, :]
    zero = ((l < m) | (l == 0)).expand(lmax, mmax)
    assert (torch.view_as_real(got.cpu())[..., zero, :] == 0).all()  # exact zeros
    e = _err(got.cpu().to(torch.complex128), want)
    print(f"RealVectorSHT {case}: max err / max|want| = {e:.3e}")
    assert e <= BOUND, e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inverse_matches_dense_fp64(case):
    a, _, want, _ = _inverse_problem(case)
    _, inv = _mods(case)
    got = inv(a.to(DEV))
    assert got.dtype == torch.float32 and got.shape == want.shape
    e = _err(got.cpu().double(), want)
    print(f"InverseRealVectorSHT {case}: max err / max|want| = {e:.3e}")
    assert e <= BOUND, e


@pytest.mark.parametrize("case", CASES[:4], ids=IDS[:4])
def test_forward_backward_matches_fp64_autograd(case):
    v, g, _, want = _forward_problem(case, True)
    fwd, _ = _mods(case)
    vg = v.to(DEV).requires_grad_()
    with torch.no_grad():
        fwd(vg)
    assert fwd._adj_plans == {}  # never under no_grad
    y = fwd(vg)
    assert y.requires_grad and fwd._adj_plans == {}  # nor before the backward
    assert torch.equal(torch.view_as_real(y.detach()), torch.view_as_real(fwd(v.to(DEV))))
    y.backward(g.to(DEV))
    assert len(fwd._adj_plans) == 1
    assert vg.grad.dtype == torch.float32 and vg.grad.shape == v.shape
    e = _err(vg.grad.cpu().double(), want)
    print(f"RealVectorSHT backward {case}: max err / max|want| = {e:.3e}")
    assert e <= BOUND, e


@pytest.mark.parametrize("case", CASES[:4], ids=IDS[:4])
def test_inverse_backward_matches_fp64_autograd(case):
    a, g, _, want = _inverse_problem(case, True)
    _, inv = _mods(case)
    ag = a.to(DEV).requires_grad_()
    y = inv(ag)
    assert y.requires_grad and inv._adj_plans == {}
    assert torch.equal(y.detach(), inv(a.to(DEV)))
    y.backward(g.to(DEV))
    assert ag.grad.dtype == torch.complex64 and ag.grad.shape == a.shape
    e = _err(ag.grad.cpu().to(torch.complex128), want)
    print(f"InverseRealVectorSHT backward {case}: max err / max|want| = {e:.3e}")
    assert e <= BOUND, e


# ---- known answers on the 24 x 48 Gauss grid, lmax = mmax = 12 -------------------------
def _theta():
    return torch.from_numpy(S.colatitudes(KNOWN[1], KNOWN[0])[0])


def _only(st, comp, l, m, value, tol=1e-5):
    """st (2, lmax, mmax) complex holds `value` at [comp, l, m] and nothing else."""
    st = st.cpu().to(torch.complex128).clone()
    assert abs(st[comp, l, m].item() - value) < tol, st[comp, l, m].item()
    st[comp, l, m] = 0
    assert st.abs().max().item() < tol, st.abs().max().item()


def test_solid_body_rotation():
    """(v_theta, v_phi) = (0, sin theta): v_phi = D_1^0 t_10 with D_1^0 = -sqrt(3 / 4 pi)
    sin theta, so t_10 = -sqrt(4 pi / 3) and nothing else; its vorticity is 2 cos theta.
    The same field as the model's (u, v) = (sin theta, 0): the signs of uv_to_vector."""
    from msfno_amd import harmonics as H
    grid, nlat, nlon, lmax, mmax = KNOWN
    th = _theta()
    u = torch.sin(th)[:, None].expand(nlat, nlon).float().contiguous()
    x = H.uv_to_vector(u, torch.zeros_like(u))
    assert torch.equal(x[1], u) and (x[0] == 0).all()
    un, vn = H.vector_to_uv(x)
    assert torch.equal(un, u) and (vn == 0).all()
    fwd, _ = _mods(KNOWN)
    _only(fwd(x.to(DEV)), 1, 1, 0, -math.sqrt(4 * math.pi / 3))
    isht = H.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)
    zeta, delta = H.vorticity_divergence(u.to(DEV), torch.zeros_like(u).to(DEV), fwd, isht)
    want = (2 * torch.cos(th))[:, None].expand(nlat, nlon)
    assert (zeta.cpu().double() - want).abs().max().item() < 1e-5
    assert delta.abs().max().item() < 1e-5


def test_gradient_of_y21_is_purely_spheroidal():
    """s_21 = 1 alone is the field grad(2 Re Y_2^1) = (2 D_2^1 cos phi, -2 Q_2^1 sin phi);
    P_2^1 in closed form, -sqrt(15 / 8 pi) sin theta cos theta, pins the helper's tables."""
    grid, nlat, nlon, lmax, mmax = KNOWN
    th = S.colatitudes(nlat, grid)[0]
    d, q, _ = VU.dq_tables(grid, nlat, lmax, mmax)
    p21 = S.ylm_closed_form(2, 1, th)
    assert np.abs(q[1, 2] - p21 / np.sin(th)).max() < 1e-12
    assert np.abs(d[1, 2] + math.sqrt(15 / (8 * math.pi)) * np.cos(2 * th)).max() < 1e-12
    phi = 2 * math.pi * np.arange(nlon) / nlon
    v = np.stack((2 * d[1, 2][:, None] * np.cos(phi)[None, :],
                  -2 * q[1, 2][:, None] * np.sin(phi)[None, :]))
    fwd, inv = _mods(KNOWN)
    _only(fwd(torch.from_numpy(v).float().to(DEV)), 0, 2, 1, 1.0)
    st = torch.zeros(2, lmax, mmax, dtype=torch.complex64)
    st[0, 2, 1] = 1.0
    assert (inv(st.to(DEV)).cpu().double() - torch.from_numpy(v)).abs().max().item() < 1e-5


def _band_limited(lmax, mmax, seed):
    gen = torch.Generator().manual_seed(seed)
    st = torch.view_as_complex(torch.randn(2, lmax, mmax, 2, generator=gen))
    l, m = torch.arange(lmax)[:, None], torch.arange(mmax)[None, :]
    st = st * ((l >= m) & (l >= 1))
    st[..., 0] = st[..., 0].real + 0j  # a real field
    return st


def test_round_trip():
    grid, nlat, nlon, lmax, mmax = KNOWN
    fwd, inv = _mods(KNOWN)
    st = _band_limited(lmax, mmax, 5)
    got = fwd(inv(st.to(DEV))).cpu()
    e = _err(got, st)
    print(f"vector round trip {KNOWN}: {e:.3e}")
    assert e <= 2e-4, e


def test_parseval_kinetic_energy():
    """sum_l KE_l = the global mean of |v|^2 / 2, by Gauss quadrature in fp64 on the host
    from the same fp32 field: exact for lmax = 11 on 24 rows (|v|^2 has degree <= 20)."""
    from msfno_amd import harmonics as H
    from msfno_amd.verification import kinetic_energy_spectrum
    grid, nlat, nlon = KNOWN[:3]
    lmax, mmax = 11, 12
    d, q = VU.torch_tables(grid, nlat, lmax, mmax, True)
    st = _band_limited(lmax, mmax, 6)
    v = VU.dense_synthesis(torch.view_as_real(st).double(), d, q, nlon).float()
    w = torch.from_numpy(S.colatitudes(nlat, grid)[1])
    mean = (0.5 * (v.double() ** 2).sum(0).mean(-1) * w).sum().item() / 2  # sum w = 2
    vsht = H.RealVectorSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)
    u, vn = H.vector_to_uv(v.to(DEV))
    ke = kinetic_energy_spectrum(u, vn, vsht)
    assert ke.shape == (lmax,) and ke.dtype == torch.float32
    got = ke.double().sum().item()
    print(f"Parseval: sum KE_l = {got:.8e}, quadrature mean = {mean:.8e}, "
          f"rel {abs(got - mean) / mean:.3e}")
    assert abs(got - mean) <= 1e-5 * mean


def test_kinetic_energy_spectrum_and_vorticity_against_dense():
    """Tolerances from the transform bound delta = 4e-6 max|st| per coefficient:
    |d power_l| <= 2 delta sum_m e_m |c_lm| <= 2 delta sqrt(2 mmax power_l) (Cauchy-Schwarz)
    plus the (3 + 128) 2^-24 summation bound of power_spectrum; and for the grids
    |d zeta(k)| <= delta sum_lm e_m l(l+1) |P_l^m(theta_k)| plus the scalar synthesis'
    2e-6 max|zeta|."""
    from msfno_amd import harmonics as H
    from msfno_amd.verification import kinetic_energy_spectrum
    grid, nlat, nlon, lmax, mmax = KNOWN
    gen = torch.Generator().manual_seed(8)
    u, v = torch.randn(2, *LEAD, nlat, nlon, generator=gen)
    dw, qw = VU.torch_tables(grid, nlat, lmax, mmax, False)
    st = torch.view_as_complex(VU.dense_analysis(torch.stack((-v, u), -3).double(), dw, qw))
    delta = BOUND * st.abs().max().item()
    l = torch.arange(lmax, dtype=torch.float64)
    ll1 = l * (l + 1)
    e_m = torch.full((mmax,), 2.0, dtype=torch.float64)
    e_m[0] = 1.0
    power = (st.abs() ** 2 * e_m).sum(-1)  # (..., 2, lmax)
    want = ll1 / (8 * math.pi) * power.sum(-2)
    tol = (ll1 / (8 * math.pi) * (2 * delta * torch.sqrt(2 * mmax * power)).sum(-2)
           + 131 * 2.0 ** -24 * want)
    fwd, _ = _mods(KNOWN)
    ke = kinetic_energy_spectrum(u.to(DEV), v.to(DEV), fwd).cpu().double()
    assert ke.shape == want.shape
    print(f"KE spectrum: max err / tol = {((ke - want).abs() / tol.clamp_min(1e-300))[..., 1:].max():.3e}")
    assert ((ke - want).abs() <= tol).all()

    ref = S.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)
    isht = H.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)
    zeta, div = H.vorticity_divergence(u.to(DEV), v.to(DEV), fwd, isht)
    amp = delta * torch.einsum("mlk,l,m->k", ref.pct.abs(), ll1, e_m)[:, None]
    for got, comp, name in ((zeta, 1, "vorticity"), (div, 0, "divergence")):
        w = ref(-ll1[:, None] * st[..., comp, :, :])
        bound = amp + 2e-6 * w.abs().max()
        err = (got.cpu().double() - w).abs()
        print(f"{name}: max err / max|want| = {err.max() / w.abs().max():.3e}, "
              f"max err / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all()


def test_wind_from_vorticity_divergence_inverts():
    """A band-limited wind survives wind -> (zeta, delta) -> wind; four fp32 transforms in a
    row, the round-trip bound 2e-4 of the transforms."""
    from msfno_amd import harmonics as H
    grid, nlat, nlon, lmax, mmax = KNOWN
    fwd, inv = _mods(KNOWN)
    sht = H.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)
    isht = H.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float().to(DEV)
    u, v = H.vector_to_uv(inv(_band_limited(lmax, mmax, 9).to(DEV)))
    zeta, delta = H.vorticity_divergence(u, v, fwd, isht)
    u2, v2 = H.wind_from_vorticity_divergence(zeta, delta, sht, inv)
    scale = max(u.abs().max().item(), v.abs().max().item())
    e = max((u2 - u).abs().max().item(), (v2 - v).abs().max().item()) / scale
    print(f"wind -> (zeta, delta) -> wind: {e:.3e}")
    assert e <= 2e-4, e


def test_short_workspace_is_refused_before_any_launch():
    from msfno_amd import _native as N
    v, _, _, _ = _forward_problem(CASES[0])
    fwd, _ = _mods(CASES[0])
    x = v.to(DEV)
    pair = fwd._plan(x.device)
    bc = int(np.prod(LEAD))
    need = N.lib().msfno_vsht_workspace_size(pair.d.handle, pair.q.handle, bc)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((*LEAD, 2, fwd.lmax, fwd.mmax, 2), 7.0, device=DEV)
    rc = N.lib().msfno_vsht_forward(pair.d.handle, pair.q.handle, x.data_ptr(), out.data_ptr(),
                                    bc, ws.data_ptr(), need - 1, N.stream_of(x.device))
    assert rc == N.MSFNO_EWORKSPACE
    with pytest.raises(ValueError):
        N.check(rc, "msfno_vsht_forward")
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # refusals of the pair itself: swapped plans, an inverse call on forward plans, bc < 1
    args = (x.data_ptr(), out.data_ptr(), bc, ws.data_ptr(), need, N.stream_of(x.device))
    assert N.lib().msfno_vsht_forward(pair.q.handle, pair.d.handle, *args) == N.MSFNO_EINVAL
    assert N.lib().msfno_vsht_inverse(pair.d.handle, pair.q.handle, *args) == N.MSFNO_EINVAL
    assert N.lib().msfno_vsht_forward(pair.d.handle, pair.q.handle, x.data_ptr(), out.data_ptr(),
                                      0, ws.data_ptr(), need, None) == N.MSFNO_EINVAL
    assert N.lib().msfno_vsht_forward(pair.d.handle, pair.q.handle, None, out.data_ptr(),
                                      bc, ws.data_ptr(), need, None) == N.MSFNO_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_transforms_record_into_a_graph():
    """One forward and one inverse transform captured on a single stream and replayed on
    new values in the captured buffers equal the eager results bit for bit."""
    case = CASES[1]
    v, _, _, _ = _forward_problem(case)
    fwd, inv = _mods(case)
    x = v.to(DEV).clone()

    def step():
        st = fwd(x)
        return st, inv(st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st_out, v_out = step()
    x.copy_(1.7 * x + 0.25)
    graph.replay()
    torch.cuda.synchronize()
    st_eager, v_eager = step()
    assert torch.equal(torch.view_as_real(st_out), torch.view_as_real(st_eager))
    assert torch.equal(v_out, v_eager)


def test_pickle_drops_the_plans():
    import pickle
    case = CASES[0]
    v, _, _, _ = _forward_problem(case)
    fwd, _ = _mods(case)
    want = fwd(v.to(DEV))
    assert len(fwd._plans) == 1
    again = pickle.loads(pickle.dumps(fwd))
    assert again._plans == {} and again._adj_plans == {}
    assert torch.equal(torch.view_as_real(again(v.to(DEV))), torch.view_as_real(want))
