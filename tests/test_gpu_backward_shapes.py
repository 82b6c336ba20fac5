"""The training backward (msfno_mlp_backward_params, msfno_block_backward_params; the
kernels of csrc/param_bwd.hip and csrc/film_bwd.hip) at the smallest shapes that reach what
the fixtures of test_gpu_film_backward.py (C <= 16, hidden <= 32, P <= 2112) never do.

The thresholds the cases are placed against -- move the cases with them:
  * wgrad_nt_kernel: WG_T = 64 (output tile, rows and columns), WG_K = 32 (k per LDS
    stage), WG_KC = 4096 (k per workgroup: ksplit = cdiv(K, 4096) fp32 partials per batch
    element, summed in fp64 by wgrad_reduce_kernel); the strided write-outs ldc / cs.
  * grid caps: gelu_grad_mul 8192 blocks x 256 threads (2 097 152 elements), relu_real_mask
    the same (left unstrided here), fill 4096, tril_map 1024 x rows, conj_swap01 65536.
  * x6_tile (csrc/gemm_x6.hip): the 256 x 256 tile once M > 128 and
    cdiv(M, 256) cdiv(N, 256) batch >= 512, else 128 x 128.
  * transpose_mat_kernel: 32 x 32 tiles.

Every gradient is held to max-abs < 1e-4 x max|grad| per tensor against fp64 autograd: a
plain torch MLP for the standalone MLP, the oracle block under the GPU's ReLU masks for
the block (the protocol of test_block_param_grads_match_oracle_autograd)."""
import functools

import pytest
import torch

from backward_util import _compare, _compare_params, _masked_oracle, _oracle_transforms, _tap_blocks
from block_util import make_block
from golden_util import param_recipe, recipe_normal, wiring_cfg
from oracle import sfno_ref
from workspace_guard import guard_intact, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MLP_GRADS = ("dx", "dx2", "dfc1_w", "dfc1_b", "dfc2_w", "dfc2_b")


# ---- 1. standalone MLP ---------------------------------------------------------------

def _mlp_tensors(Cin, Cin2, Hid, Cout, B, P, seed):
    """Seeded fp32 weights (unit-gain), inputs and output gradient of one case."""
    g = torch.Generator().manual_seed(seed)
    Ct = Cin + Cin2
    t = {"W1": torch.randn(Hid, Ct, generator=g) / Ct ** 0.5,
         "b1": 0.1 * torch.randn(Hid, generator=g),
         "W2": torch.randn(Cout, Hid, generator=g) / Hid ** 0.5,
         "b2": 0.1 * torch.randn(Cout, generator=g),
         "x": torch.randn(B, Cin, 1, P, generator=g),
         "x2": torch.randn(B, Cin2, 1, P, generator=g) if Cin2 else None,
         "dy": torch.randn(B, Cout, 1, P, generator=g)}
    return t


def _mlp_reference(t, dev="cpu"):
    """fp64 autograd through fc2(GELU(fc1(cat(x, x2)))) with exact GELU, loss (y * dy).sum();
    the gradients as CPU fp64 tensors keyed as MLP_GRADS (dx2 None without x2)."""
    leaves = {k: t[k].to(dev).double().requires_grad_() for k in ("x", "W1", "b1", "W2", "b2")}
    x2 = t["x2"].to(dev).double().requires_grad_() if t["x2"] is not None else None
    xc = leaves["x"] if x2 is None else torch.cat([leaves["x"], x2], 1)
    xc = xc[:, :, 0, :]
    pre = leaves["W1"] @ xc + leaves["b1"][None, :, None]
    y = leaves["W2"] @ torch.nn.functional.gelu(pre) + leaves["b2"][None, :, None]
    (y * t["dy"].to(dev).double()[:, :, 0, :]).sum().backward()
    want = {"dx": leaves["x"].grad, "dx2": x2.grad if x2 is not None else None,
            "dfc1_w": leaves["W1"].grad[:, :, None, None], "dfc1_b": leaves["b1"].grad,
            "dfc2_w": leaves["W2"].grad[:, :, None, None], "dfc2_b": leaves["b2"].grad}
    return {k: (v.cpu() if v is not None else None) for k, v in want.items()}


def _mlp_module(t):
    from msfno_amd.sfno import MLP
    Hid, Ct = t["W1"].shape
    m = MLP(in_features=Ct, hidden_features=Hid, out_features=t["W2"].shape[0]).eval()
    with torch.no_grad():
        m.fwd[0].weight.copy_(t["W1"][:, :, None, None])
        m.fwd[0].bias.copy_(t["b1"])
        m.fwd[2].weight.copy_(t["W2"][:, :, None, None])
        m.fwd[2].bias.copy_(t["b2"])
    return m.to(DEV)


def _mlp_native(t):
    """The native forward and backward through autograd (MLP.forward / _MLPFn); x and dy
    must come back unchanged.  Gradients keyed as MLP_GRADS."""
    from msfno_amd.sfno.layers import _MLPFn
    m = _mlp_module(t)
    x = t["x"].to(DEV).requires_grad_()
    dy = t["dy"].to(DEV)
    x2 = None
    if t["x2"] is not None:
        x2 = t["x2"].to(DEV).requires_grad_()  # dx2 requested
        y = _MLPFn.apply(x, x2, None, m, *m.parameters())
    else:
        y = m(x)
    y.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(x.detach().cpu(), t["x"]), "the backward changed x"
    assert torch.equal(dy.cpu(), t["dy"]), "the backward changed dy"
    return {"dx": x.grad, "dx2": x2.grad if x2 is not None else None,
            "dfc1_w": m.fwd[0].weight.grad, "dfc1_b": m.fwd[0].bias.grad,
            "dfc2_w": m.fwd[2].weight.grad, "dfc2_b": m.fwd[2].bias.grad}


def _mlp_compare(tag, got, want):
    for k in MLP_GRADS:
        if want[k] is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        _compare(f"{tag} {k}", got[k], want[k])


def _bitwise(a, b):
    for k in MLP_GRADS:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{k} differs between two runs of the same call"


# (Cin, Cin2, Hid, Cout, B, P, seed)
RAGGED = (70, 0, 130, 65, 2, 4131, 41)


@functools.lru_cache(maxsize=1)
def _ragged():
    """Tensors and fp64 reference of the ragged-tiles case, computed once for the autograd
    test and the C-ABI workspace test."""
    t = _mlp_tensors(*RAGGED)
    return t, _mlp_reference(t)


def test_mlp_backward_ragged_second_tiles_two_k_chunks():
    """Cin 70, Hid 130, Cout 65, B 2, P 4131.  dW1 (130 x 70) spans 3 x 2 tiles of 64 with
    ragged edges 2 and 6, dW2 (65 x 130) 2 x 3 tiles with ragged edges 1 and 2: second-tile
    offsets m0 / n0 and the m < M, n < N guards act.  K = 4131 pixels gives ksplit = 2; the
    second chunk holds 35 pixels: one full 32-stage and a sub-stage tail of 3, and
    blockIdx.z / ksplit, % ksplit are both non-trivial (B = 2).  The partials are reduced in
    a fixed order without atomics, so two runs agree bit for bit."""
    t, want = _ragged()
    got = _mlp_native(t)
    _mlp_compare("ragged", got, want)
    _bitwise(got, _mlp_native(t))


def test_mlp_backward_params_abi_workspace_holds_anything_and_is_not_overrun():
    """One direct msfno_mlp_backward_params call at the ragged-tiles shape: the workspace is
    exactly msfno_mlp_backward_params_workspace_size bytes of 0xFF (NaN as floats) followed
    by a 4 KiB guard, every output is pre-filled with NaN.  The call returns OK, every
    output is finite and matches the fp64 reference, the guard is untouched; one byte less
    returns MSFNO_EWORKSPACE and launches nothing (outputs still NaN)."""
    from msfno_amd import _native as N
    t, want = _ragged()
    Cin, _, Hid, Cout, B, P, _ = RAGGED
    m = _mlp_module(t)
    d, keep = m.native_desc(0)
    L = N.lib()
    nbytes = L.msfno_mlp_backward_params_workspace_size(d, B, P)
    assert nbytes > 0
    buf = guarded(nbytes, 0xFF, DEV)
    x, dy = t["x"].to(DEV).contiguous(), t["dy"].to(DEV).contiguous()
    outs = {"dx": (B, Cin, 1, P), "dfc1_w": (Hid, Cin, 1, 1), "dfc1_b": (Hid,),
            "dfc2_w": (Cout, Hid, 1, 1), "dfc2_b": (Cout,)}
    outs = {k: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
            for k, s in outs.items()}

    def call(ws_bytes):
        rc = L.msfno_mlp_backward_params(
            d, x.data_ptr(), None, dy.data_ptr(), outs["dx"].data_ptr(), None,
            outs["dfc1_w"].data_ptr(), outs["dfc1_b"].data_ptr(), outs["dfc2_w"].data_ptr(),
            outs["dfc2_b"].data_ptr(), B, P, buf.data_ptr(), ws_bytes,
            N.stream_of(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc

    assert call(nbytes) == N.MSFNO_OK, L.msfno_last_error()
    guard_intact(buf, nbytes)
    got = dict(outs, dx2=None)
    _mlp_compare("abi", got, want)
    assert torch.equal(x.cpu(), t["x"]) and torch.equal(dy.cpu(), t["dy"])
    # one byte short: refused before anything is launched
    for o in outs.values():
        o.fill_(float("nan"))
    assert call(nbytes - 1) == N.MSFNO_EWORKSPACE
    for k, o in outs.items():
        assert torch.isnan(o).all(), f"{k} written by a refused call"
    guard_intact(buf, nbytes)
    del keep


CHUNK_EDGES = [(1, "one_pixel"), (31, "under_a_stage"), (32, "exact_stage"),
               (33, "stage_plus_one"), (4095, "under_a_chunk"), (4096, "exact_chunk"),
               (4097, "chunk_of_one_pixel"), (8192, "two_exact_chunks"),
               (8193, "third_chunk_of_one_pixel")]


@pytest.mark.parametrize("P", [p for p, _ in CHUNK_EDGES],
                         ids=[f"P{p}_{name}" for p, name in CHUNK_EDGES])
def test_mlp_backward_k_chunk_and_stage_edges(P):
    """Cin 8, Hid 16, Cout 8, B 1 over P pixels on either side of a 32-pixel stage (WG_K)
    and of a 4096-pixel chunk (WG_KC): ke = min(K, kb + WG_KC), the k < ke staging guards
    and the number of partials wgrad_reduce sums."""
    t = _mlp_tensors(8, 0, 16, 8, 1, P, 100 + P)
    _mlp_compare(f"P={P}", _mlp_native(t), _mlp_reference(t))


def test_mlp_backward_decoder_shape_cin2_column_blocks():
    """The decoder, cat(x, residual) 256 + 73 -> 256 -> 73, B 2, P 4131 (ksplit = 2), dx2
    requested: dW1 is written as two column blocks [:, :256] and [:, 256:] with ldc = 329,
    each by its own wgrad_nt call (a wrong ldc or offset clobbers the neighbour), and W1's
    two column blocks are transposed from a matrix with lda = 329 over 8 x 8 and 3 x 8
    32 x 32 tiles.  Two runs agree bit for bit."""
    t = _mlp_tensors(256, 73, 256, 73, 2, 4131, 43)
    want = _mlp_reference(t)
    got = _mlp_native(t)
    _mlp_compare("decoder", got, want)
    for tag, cols in (("[:, :256]", slice(0, 256)), ("[:, 256:]", slice(256, 329))):
        _compare(f"decoder dfc1_w{tag}", got["dfc1_w"][:, cols].contiguous(),
                 want["dfc1_w"][:, cols].contiguous())
    _bitwise(got, _mlp_native(t))


def test_mlp_backward_encoder_shape():
    """The encoder's widths, 73 -> 256 -> 256, B 1, P 4131: dW1 256 x 73 (4 x 2 tiles, ragged
    by 9), dW2 256 x 256 (4 x 4 full tiles), ksplit = 2."""
    t = _mlp_tensors(73, 0, 256, 256, 1, 4131, 44)
    _mlp_compare("encoder", _mlp_native(t), _mlp_reference(t))


def test_mlp_backward_block_mlp_width_gelu_grad_mul_grid_stride():
    """The block MLP's widths, 256 -> 512 -> 256, B 1, P 4131: B Hid P = 2 115 072 elements
    exceed gelu_grad_mul's 8192 x 256 grid, so its grid-stride loop is entered; the forward
    runs on the fused MLP kernels, the backward on gemm_dense (M = 512 and 256, K = 256 and
    512, 128 x 128 tile)."""
    assert 512 * 4131 > 8192 * 256
    t = _mlp_tensors(256, 0, 512, 256, 1, 4131, 45)
    _mlp_compare("block-mlp", _mlp_native(t), _mlp_reference(t))


def test_mlp_backward_256x256_gemm_tile():
    """256 -> 512 -> 256, B 4, P 16400: cdiv(512, 256) cdiv(16400, 256) 4 = 520 >= 512, so
    x6_tile gives the backward's M = 512 GEMMs (pre, dh) the 256 x 256 tile; P = 16400 is no
    multiple of 256 (ragged last column tile) and runs the weight gradients in five chunks,
    the last of 16 pixels.  (The fp64 reference, 33.6 M hidden activations, takes about two
    seconds on the CPU; _mlp_reference(t, DEV) builds it on the device instead.)"""
    assert -(-512 // 256) * -(-16400 // 256) * 4 >= 512
    t = _mlp_tensors(256, 0, 512, 256, 4, 16400, 46)
    _mlp_compare("tile256", _mlp_native(t), _mlp_reference(t))


# ---- 3. block backward at widths and grids without a fixture -----------------------------

MID = dict(nlat=91, nlon=180, lmax=45, mmax=46, grid="equiangular")
BLOCK_CASES = {
    # 91 x 180 (P = 16380: four K chunks, the last of 4092 pixels = 127 stages + 28), C = 72
    # (two tiles, ragged by 8), MLP hidden 144 (three tiles, ragged by 16); spectral weight
    # gradients over 2 * 45 * 46 = 4140 real columns (ksplit = 2, tail 44) in WGRAD_PLAIN and
    # WGRAD_CSWAP with the cs = 2 interleaved write; B * 144 * 16380 = 4.7 M elements stride
    # gelu_grad_mul's grid
    "wide_nl_C72_two_ragged_tiles_ksplit4_cswap_across_chunk": dict(
        MID, C=72, B=2, filter="non-linear"),
    "wide_lin_C72_two_ragged_tiles_ksplit4": dict(MID, C=72, B=2, filter="linear"),
    # the width training runs: C = 256, MLP hidden 512, on a 32 x 64 grid
    "c256_nl_C256_hidden512": dict(nlat=32, nlon=64, lmax=32, mmax=33, grid="equiangular",
                                   C=256, B=1, filter="non-linear"),
}
WIDE_NL = "wide_nl_C72_two_ragged_tiles_ksplit4_cswap_across_chunk"

# the spectral MLP off its usual build (three layers, hidden 2 C; the forward's sweep is
# test_gpu_spectral_mlp.py): carve_* of csrc/block_bwd.cpp size r.h[l] by the layer count and
# the per-layer loops take ci and co from the hidden width.  13 x 26, lmax 12, C 24, B 2
SMALL = dict(nlat=13, nlon=26, lmax=12, mmax=13, grid="equiangular", C=24, B=2,
             filter="non-linear")
BLOCK_CASES.update({
    # one layer: the output layer's gradient reads layer 0's activation, r.h has one entry
    "spec_L1_C24_hidden48": dict(SMALL, spectral_layers=1, mlp_ratio=2.0),
    # four layers of hidden 36 (no multiple of 16 or 32): three square hidden layers
    "spec_L4_C24_hidden36": dict(SMALL, spectral_layers=4, mlp_ratio=1.5),
    # hidden 12 < C: the forward's real-ified 4M chain; block MLP hidden 12 as well
    "spec_L2_C24_hidden12": dict(SMALL, spectral_layers=2, mlp_ratio=0.5),
})


def _recipe_params(blk, meta):
    """Every parameter of the block from the committed recipe (golden_util.param_recipe /
    recipe_normal, seeds as make_golden.py --large), plus the block's own index buffers."""
    params = {}
    for i, (n, p) in enumerate(sorted(blk.named_parameters())):
        sigma, offset = param_recipe(n, tuple(p.shape), meta["filter"])
        params[n] = recipe_normal(100 + i, p.shape, sigma, offset)
    for k, v in blk.state_dict().items():
        if k not in params and not k.endswith((".weights", ".pct")):
            params[k] = v.clone()
    return params


def _guarded_workspace(blk, x, B):
    """(ws, nbytes): msfno_block_backward_params_workspace_size bytes of 0xFF, then a guard."""
    from msfno_amd import _native as N
    fwd, inv = blk._transforms()
    pf, pi = fwd._plan(x.device), inv._plan(x.device)
    fa, ga = blk._adjoint_plans(x.device)
    d, keep = blk.native_desc()
    nbytes = N.lib().msfno_block_backward_params_workspace_size(d, pf.handle, pi.handle,
                                                                fa.handle, ga.handle, B)
    del keep
    assert nbytes > 0
    return guarded(nbytes, 0xFF, x.device), nbytes


def _block_case(name, guard_ws=False):
    import oracle.sfno_ref as R
    meta = dict(BLOCK_CASES[name], filmed=1, wiring="middle", scale=0.8)
    B, C = meta["B"], meta["C"]
    blk, _, _ = make_block(meta)
    params = _recipe_params(blk, meta)
    missing, unexpected = blk.load_state_dict(params, strict=False)
    assert not unexpected and all(k.endswith((".weights", ".pct")) for k in missing)
    blk = blk.to(DEV)
    x0 = recipe_normal(9000 + C + meta["nlat"], (B, C, meta["nlat"], meta["nlon"]))
    g = torch.Generator().manual_seed(31)
    gamma0 = 0.1 * torch.randn(B, C, generator=g)
    beta0 = 0.1 * torch.randn(B, C, generator=g)
    x = x0.clone().to(DEV).requires_grad_()
    gamma = gamma0.clone().to(DEV).requires_grad_()
    beta = beta0.clone().to(DEV).requires_grad_()
    ws = nbytes = None
    if guard_ws:
        ws, nbytes = _guarded_workspace(blk, x, B)
        plain = blk.native_backward
        calls = []

        def with_ws(*a, **kw):
            calls.append(1)
            return plain(*a, ws=ws, **kw)
        blk.native_backward = with_ws
    taps = {}
    _tap_blocks(type("OneBlock", (), {"blocks": [blk]}), taps)
    y = blk(x, gamma, beta, meta["scale"])
    dout = torch.randn(y.shape, generator=g)
    (y * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    if guard_ws:
        assert len(calls) == 1
        guard_intact(ws, nbytes)
    inner, outer, has_mlp = wiring_cfg(meta)
    cfg = sfno_ref.BlockCfg(filter_type=meta["filter"], inner_skip=inner, outer_skip=outer,
                            has_mlp=has_mlp, spectral_layers=meta.get("spectral_layers", 3))
    if "spectral_layers" in meta:
        # the block was built at the depth and widths the oracle's own recipe gives them
        shapes = sfno_ref.make_block_params(C, meta["lmax"], meta["mmax"], cfg,
                                            hidden_factor=meta["mlp_ratio"])
        assert {k: tuple(v.shape) for k, v in shapes.items()} == \
            {k: tuple(params[k].shape) for k in shapes}
        assert len(blk.filter_layer.filter.w) == cfg.spectral_layers
        assert blk.filter_layer.filter.hidden_size == int(meta["mlp_ratio"] * C)
    pd = {k: (v.double().requires_grad_() if v.is_floating_point() else v)
          for k, v in params.items()}
    sht, isht = _oracle_transforms(meta)
    xd = x0.double().requires_grad_()
    gd, bd = gamma0.double().requires_grad_(), beta0.double().requires_grad_()
    orig = R.complex_relu_real
    R.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)
    try:
        yd = sfno_ref.block_forward(pd, xd, sht, isht, cfg, gd, bd, meta["scale"])
        (yd * dout.double()).sum().backward()
    finally:
        R.complex_relu_real = orig
    tag = name.split("_C")[0]
    for k, got, want in (("x", x.grad, xd.grad), ("gamma", gamma.grad, gd.grad),
                         ("beta", beta.grad, bd.grad)):
        assert torch.isfinite(got).all(), k
        _compare(f"{tag} d{k}", got, want)
    named = list(blk.named_parameters())
    for k, p in named:
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    n = _compare_params(tag, named, lambda k: pd[k].grad if pd[k].grad is not None
                        else torch.zeros_like(pd[k]))
    if meta["filter"] == "linear":
        assert n >= 11
    elif "spectral_layers" in meta:
        # norm0, norm1, inner skip, fc1, fc2: weight and bias each; layers + 1 spectral
        # weights (ComplexReLU(real) keeps its bias as a buffer)
        assert n == 10 + cfg.spectral_layers + 1, n
    else:
        assert n >= 14


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_param_grads_beyond_one_tile_and_chunk(name):
    """dx, dgamma, dbeta and every parameter gradient of a filmed middle block whose
    parameters come from the committed recipe, against fp64 autograd through the oracle under
    the GPU's ReLU masks (BLOCK_CASES says which thresholds each case crosses)."""
    _block_case(name)


def test_block_backward_params_workspace_holds_anything_and_is_not_overrun():
    """The wide non-linear block once more with native_backward(ws=...): a workspace of
    exactly msfno_block_backward_params_workspace_size bytes of 0xFF (NaN as floats) and a
    4 KiB guard behind it.  Every gradient is finite and matches the oracle, the guard is
    untouched.  (The outputs are allocated inside native_backward; one left unwritten would
    miss the oracle.)"""
    _block_case(WIDE_NL, guard_ws=True)
