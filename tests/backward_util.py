"""Helpers shared by the backward tests (test_gpu_film_backward.py on the fixtures,
test_gpu_backward_shapes.py on shapes without one): the fp64 oracle's transforms, the
1e-4 x max|grad| comparison, and the oracle evaluated under the ComplexReLU(real) masks
the GPU backward applied."""
import torch

from oracle import sfno_ref
from oracle import sht_ref as S


def _oracle_transforms(meta):
    sht, isht = sfno_ref.make_transforms(meta["nlat"], meta["nlon"], meta["lmax"], meta["mmax"],
                                         meta["grid"], dtype=torch.float64)
    if "out_nlat" in meta:
        isht = S.InverseRealSHT(meta["out_nlat"], meta["out_nlon"], lmax=meta["lmax"],
                                mmax=meta["mmax"], grid=meta["out_grid"]).to(torch.float64)
        isht.pct = isht.pct / 1e5
    return sht, isht


def _compare(tag, got, want, rel=1e-4, scale=0.0):
    """max-abs < rel x max(max|want|, scale): `scale` is the matching weight's gradient
    scale for a bias whose exact gradient vanishes (a per-channel constant that the next
    InstanceNorm removes: the fp32 sum of a zero-mean gradient is noise at that scale)."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = rel * max(want.abs().max().item(), scale, 1e-6)
    print(f"{tag}: max-abs {err:.3e} (max|grad| {want.abs().max().item():.3e}, tol {tol:.2e})")
    assert err < tol, (tag, err, tol)


def _film_oracle_grads(meta, params, x, gamma0, beta0, scale, dout):
    """(dL/dgamma, dL/dbeta) of L = (block(x) * dout).sum() by torch autograd through the
    fp64 oracle block of the fixture (meta, params)."""
    from golden_util import wiring_cfg
    inner, outer, has_mlp = wiring_cfg(meta)
    cfg = sfno_ref.BlockCfg(filter_type=meta["filter"], inner_skip=inner, outer_skip=outer,
                            has_mlp=has_mlp)
    pd = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    sht, isht = _oracle_transforms(meta)
    gd = gamma0.double().requires_grad_()
    bd = beta0.double().requires_grad_()
    yd = sfno_ref.block_forward(pd, x.double(), sht, isht, cfg, gd, bd, scale)
    (yd * dout.double()).sum().backward()
    return gd.grad, bd.grad


def _compare_params(tag, named, want_of):
    """Every (name, parameter) of `named` against want_of(name); a bias is held to its
    weight's gradient scale as well (_compare)."""
    wants = {k: want_of(k) for k, _ in named}
    n = 0
    for k, p in named:
        assert p.grad is not None, k
        scale, rel = 0.0, 1e-4
        if k.endswith("bias") and k[:-4] + "weight" in wants:
            scale = wants[k[:-4] + "weight"].abs().max().item()
            if wants[k].abs().max().item() < 1e-6 * scale:
                # exactly zero (a constant the next InstanceNorm removes): the fp32 sum of
                # a zero-mean gradient over the grid, against the weight's scale
                rel = 1e-3
        _compare(f"{tag} d{k}", p.grad, wants[k], rel=rel, scale=scale)
        n += 1
    return n


def _masked_oracle(taps, spectral_layers):
    """A complex_relu_real for the oracle that applies the ComplexReLU(real) masks the GPU
    backward used in the blocks it tapped (call order: block, then layer) and the oracle's
    own elsewhere -- at a pre-activation within rounding of the kink the two sides may
    legitimately differ (activations.py:42-46)."""
    import oracle.sfno_ref as R
    orig = R.complex_relu_real
    calls = [0]

    def relu(z):
        blk, layer = divmod(calls[0], spectral_layers)
        calls[0] += 1
        if blk not in taps:
            return orig(z)
        m = (taps[blk][layer].real > 0).to(z.real.dtype)
        return torch.complex(z.real * m, z.imag)
    return relu


def _tap_blocks(net, taps):
    """Record every block backward's recomputed hidden activations into taps[block]."""
    for i, blk in enumerate(net.blocks):
        def tapped(*a, _i=i, _orig=blk.native_backward, **kwa):
            return _orig(*a, hidden_tap=lambda hs: taps.__setitem__(_i, [h.cpu() for h in hs]),
                         **kwa)
        blk.native_backward = tapped
