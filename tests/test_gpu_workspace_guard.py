"""Every entry point whose workspace is laid out by one carve_* function (csrc/mlp.cpp
carve_mlp, carve_mlp_bwd; csrc/api.cpp carve_conv1x1; csrc/block_bwd.cpp carve_film_bwd),
called through the C ABI with exactly the bytes its *_workspace_size function returns.

Each case allocates those bytes and a 4 KiB guard of 0x5A behind them (workspace_guard),
pre-fills every output with NaN and runs the call twice, on a workspace of 0xFF bytes
(NaN as floats) and on one of 0x00.  Both runs return MSFNO_OK and leave the guard
untouched; their outputs are finite and equal bit for bit (nothing reads workspace it did
not write) and match an fp64 reference at the bar of the entry point's own accuracy test.
One byte less returns MSFNO_EWORKSPACE with every output still NaN.

Shapes are the smallest that reach each carve's conditional buffers: Cin2 > 0 (the second
split-weight buffer), a hidden width the fused MLP kernel refuses (40) and one it takes
(256), P = 33 (no multiple of 8: the hidden planes' row stride differs from P; of 4: the
one-tile skip kernel), 256 -> 256 channels (launch_skip_h, which takes every P >= 1) and
24 -> 9 (gemm_x3)."""
import pytest
import torch

from backward_util import _compare, _film_oracle_grads
from block_util import make_block
from golden_util import GOLDEN, load
from test_gpu_backward_shapes import MLP_GRADS, _mlp_compare, _mlp_module, _mlp_reference, _mlp_tensors
from test_gpu_corun import _conv_error
from test_gpu_mlp_gen import _reference as _mlp_forward_reference
from workspace_guard import guard_intact, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _all_nan(outs):
    for k, o in outs.items():
        assert torch.isnan(o).all(), f"{k} written by a refused call"


def _run_guarded(nbytes, outs, call):
    """call(ws_ptr, ws_bytes) -> rc on a 0xFF and on a 0x00 workspace of exactly nbytes, then
    with one byte less (module docstring).  Returns the outputs (clones) of the first run."""
    from msfno_amd import _native as N
    assert nbytes > 0
    runs = []
    for fill in (0xFF, 0x00):
        ws = guarded(nbytes, fill, DEV)
        for o in outs.values():
            o.fill_(NAN)
        rc = call(ws.data_ptr(), nbytes)
        torch.cuda.synchronize()
        assert rc == N.MSFNO_OK, (rc, N.lib().msfno_last_error())
        guard_intact(ws, nbytes)
        for k, o in outs.items():
            assert torch.isfinite(o).all(), f"{k} not finite on a workspace of {fill:#x} bytes"
        runs.append({k: o.clone() for k, o in outs.items()})
    for k in outs:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k} depends on the workspace's old bytes"
    for o in outs.values():
        o.fill_(NAN)
    assert call(ws.data_ptr(), nbytes - 1) == N.MSFNO_EWORKSPACE
    torch.cuda.synchronize()
    _all_nan(outs)
    guard_intact(ws, nbytes)
    return runs[0]


# ---- msfno_mlp_forward ----------------------------------------------------------------
# (Cin, Cin2, Hid, Cout, fused, bar): 5e-7 is test_gpu_gemm_x6.py's bar for the two-GEMM
# x6 path, 2e-6 test_gpu_mlp_gen.py's for the fused x3h kernel, both on |y - y64| / scale
MLP_FWD = [(24, 5, 40, 9, False, 5e-7), (24, 0, 40, 9, False, 5e-7),
           (73, 0, 256, 256, True, 2e-6)]


@pytest.mark.parametrize("Cin,Cin2,Hid,Cout,fused,bar", MLP_FWD,
                         ids=["two_gemm_cin2", "two_gemm", "fused_width"])
def test_mlp_forward_workspace(Cin, Cin2, Hid, Cout, fused, bar):
    from msfno_amd import _native as N
    B, P = 2, 33
    t = _mlp_tensors(Cin, Cin2, Hid, Cout, B, P, seed=7)
    m = _mlp_module(t)
    d, keep = m.native_desc(Cin2)
    L = N.lib()
    assert bool(L.msfno_mlp_fused_supported(d)) == fused
    x = t["x"].to(DEV).contiguous()
    x2 = t["x2"].to(DEV).contiguous() if Cin2 else None
    outs = {"y": _nan(B, Cout, 1, P)}

    def call(ws, ws_bytes):
        return L.msfno_mlp_forward(d, x.data_ptr(), N.ptr(x2), None, 0, outs["y"].data_ptr(), B, P,
                                   ws, ws_bytes, N.stream_of(torch.device(DEV)))

    got = _run_guarded(L.msfno_mlp_workspace_size(d, B, P), outs, call)["y"]
    y64, scale = _mlp_forward_reference(m.cpu(), t["x"], t["x2"], None)
    err = ((got.double().cpu()[:, :, 0, :] - y64).abs() / scale).max().item()
    print(f"mlp forward {Cin}+{Cin2} -> {Hid} -> {Cout}: max |err| / scale = {err:.3e}")
    assert err < bar
    del keep


# ---- msfno_mlp_backward_params / msfno_mlp_backward_input ----------------------------
def _mlp_backward(Cin, Cin2, wanted):
    """One backward at Hid 40, Cout 9, B 2, P 33 writing the gradients `wanted`:
    (lib, desc, call, outs, nbytes of the matching size function, tensors, keep-alive)."""
    from msfno_amd import _native as N
    Hid, Cout, B, P = 40, 9, 2, 33
    t = _mlp_tensors(Cin, Cin2, Hid, Cout, B, P, seed=9)
    m = _mlp_module(t)
    d, keep = m.native_desc(Cin2)
    L = N.lib()
    x, dy = t["x"].to(DEV).contiguous(), t["dy"].to(DEV).contiguous()
    x2 = t["x2"].to(DEV).contiguous() if Cin2 else None
    shapes = {"dx": (B, Cin, 1, P), "dx2": (B, Cin2, 1, P), "dfc1_w": (Hid, Cin + Cin2, 1, 1),
              "dfc1_b": (Hid,), "dfc2_w": (Cout, Hid, 1, 1), "dfc2_b": (Cout,)}
    outs = {k: _nan(*shapes[k]) for k in wanted}
    s = N.stream_of(torch.device(DEV))
    if wanted == ("dx",):
        nbytes = L.msfno_mlp_backward_input_workspace_size(d, B, P)

        def call(ws, ws_bytes):
            return L.msfno_mlp_backward_input(d, x.data_ptr(), N.ptr(x2), dy.data_ptr(),
                                              outs["dx"].data_ptr(), B, P, ws, ws_bytes, s)
    else:
        nbytes = L.msfno_mlp_backward_params_workspace_size(d, B, P)

        def call(ws, ws_bytes):
            return L.msfno_mlp_backward_params(
                d, x.data_ptr(), N.ptr(x2), dy.data_ptr(),
                *[N.ptr(outs.get(k)) for k in MLP_GRADS], B, P, ws, ws_bytes, s)
    return L, d, call, outs, nbytes, t, (m, keep, x, x2, dy)


def test_mlp_backward_params_workspace_all_six_gradients():
    L, d, call, outs, nbytes, t, keep = _mlp_backward(24, 5, MLP_GRADS)
    got = _run_guarded(nbytes, outs, call)
    _mlp_compare("guarded", got, _mlp_reference(t))
    del keep


def test_mlp_backward_input_workspace():
    L, d, call, outs, nbytes, t, keep = _mlp_backward(24, 5, ("dx",))
    assert nbytes < L.msfno_mlp_backward_params_workspace_size(d, 2, 33)
    got = _run_guarded(nbytes, outs, call)
    _compare("guarded dx", got["dx"], _mlp_reference(t)["dx"])
    del keep


def test_mlp_backward_refuses_dx2_wider_than_dx_before_writing_anything():
    """dx2 shares dx's transpose buffer and split-weight workspace, so Cin2 <= Cin: Cin 5,
    Cin2 24 with dx2 requested returns MSFNO_EINVAL with all six outputs still NaN."""
    from msfno_amd import _native as N
    L, d, call, outs, nbytes, t, keep = _mlp_backward(5, 24, MLP_GRADS)
    ws = guarded(nbytes, 0xFF, DEV)
    assert call(ws.data_ptr(), nbytes) == N.MSFNO_EINVAL
    torch.cuda.synchronize()
    _all_nan(outs)
    guard_intact(ws, nbytes)
    del keep


# ---- msfno_conv1x1 --------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout", [(24, 9), (256, 256)], ids=["gemm_x3", "skip_h"])
def test_conv1x1_workspace(Cin, Cout):
    from msfno_amd import _native as N
    B, P = 2, 33
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, Cin, P, generator=g, device=DEV)
    w = torch.randn(Cout, Cin, generator=g, device=DEV) / Cin ** 0.5
    b = torch.randn(Cout, generator=g, device=DEV)
    outs = {"y": _nan(B, Cout, P)}
    L = N.lib()

    def call(ws, ws_bytes):
        return L.msfno_conv1x1(w.data_ptr(), b.data_ptr(), x.data_ptr(), outs["y"].data_ptr(), B,
                               Cin, Cout, P, ws, ws_bytes, N.stream_of(x.device))

    got = _run_guarded(L.msfno_conv1x1_workspace_size(B, Cin, Cout), outs, call)["y"]
    err = _conv_error(got, w, b, x)
    print(f"conv1x1 B={B} {Cin}->{Cout} P={P}: max |err| / sum|w x| = {err:.3e}")
    assert err < 2e-6  # test_gpu_corun.py test_conv1x1_matches_fp64


# ---- msfno_block_film_backward --------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_nl_film_middle", "c1_nl_film_last"],
                         ids=["with_mlp", "without_mlp"])
def test_block_film_backward_workspace(name):
    """The smallest filmed fixture of test_gpu_film_backward.py, with the channel MLP (middle
    wiring) and without it (last wiring), at that test's bar of 1e-4 x max|grad|."""
    from msfno_amd import _native as N
    meta, params, arrays, _ = load(f"{GOLDEN}/{name}.npz")
    blk, _, _ = make_block(meta, params)
    blk = blk.to(DEV).requires_grad_(False)
    x0, gamma0, beta0, scale = arrays["x"], arrays["gamma"], arrays["beta"], float(meta["scale"])
    B, C = x0.shape[:2]
    dout0 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(11))
    x, dout = x0.to(DEV).contiguous(), dout0.to(DEV).contiguous()
    gamma = gamma0.float().reshape(B, C).to(DEV).contiguous()
    beta = beta0.float().reshape(B, C).to(DEV).contiguous()
    fwd, inv = blk._transforms()
    pf, pi = fwd._plan(x.device), inv._plan(x.device)
    d, keep = blk.native_desc()
    assert bool(d.has_mlp) == (name.endswith("middle"))
    L = N.lib()
    outs = {"dgamma": _nan(B, C), "dbeta": _nan(B, C)}

    def call(ws, ws_bytes):
        return L.msfno_block_film_backward(
            d, pf.handle, pi.handle, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), scale,
            dout.data_ptr(), outs["dgamma"].data_ptr(), outs["dbeta"].data_ptr(), B, ws, ws_bytes,
            N.stream_of(x.device))

    nbytes = L.msfno_block_film_backward_workspace_size(d, pf.handle, pi.handle, B)
    got = _run_guarded(nbytes, outs, call)
    wg, wb = _film_oracle_grads(meta, params, x0, gamma0, beta0, scale, dout0)
    _compare("guarded dgamma", got["dgamma"].reshape(wg.shape), wg)
    _compare("guarded dbeta", got["dbeta"].reshape(wb.shape), wb)
    del keep
