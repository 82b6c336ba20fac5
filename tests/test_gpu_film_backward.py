"""FiLM backward: gradients of a loss with respect to the
FiLM modulation (gamma, beta), every SFNO weight frozen, as MSFNO fine-tunes its
FiLM generator (sfnonet.py:787-860: the filmed blocks and the decoder run with
autograd, the blocks before them under no_grad).

The native backward (msfno_block_film_backward / msfno_mlp_backward_input,
through the torch.autograd.Functions of msfno_amd) is checked against torch
autograd through the oracle restatement in fp64 on the CPU, on the reference's
golden block parameters (both filters, middle wiring with the channel MLP and
last wiring without it) and on a small FourierNeuralOperatorNet_Filmed
(film_layers = 1, 2, all, repeat_film), and dL/dx through every block wiring
(msfno_block_backward).  Tolerance: max-abs < 1e-4 x max|grad|."""
import os

import pytest
import torch

from backward_util import (_compare, _compare_params, _film_oracle_grads,  # noqa: F401
                           _masked_oracle, _oracle_transforms, _tap_blocks)
from block_util import make_block
from golden_util import golden_files, load, wiring_cfg
from oracle import sfno_ref
from test_oracle_net import NET_FIXTURES, load_net, net_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"

FILM_CASES = [p for p in golden_files()
              if "_film_" in os.path.basename(p) and "_first" not in os.path.basename(p)]


@pytest.mark.parametrize("path", FILM_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_block_film_grads_match_oracle_autograd(path):
    meta, params, arrays, _ = load(path)
    blk, _, _ = make_block(meta, params)
    blk = blk.to(DEV).requires_grad_(False)  # SFNO frozen (model.py:1016-1023)
    x, scale = arrays["x"], float(meta["scale"])
    g = torch.Generator().manual_seed(11)
    gamma0, beta0 = arrays["gamma"], arrays["beta"]
    # GPU: native forward + native FiLM backward through autograd
    gamma = gamma0.clone().to(DEV).requires_grad_()
    beta = beta0.clone().to(DEV).requires_grad_()
    y = blk(x.to(DEV), gamma, beta, scale)
    dout = torch.randn(y.shape, generator=g)
    (y * dout.to(DEV)).sum().backward()
    # oracle: torch autograd in fp64
    wg, wb = _film_oracle_grads(meta, params, x, gamma0, beta0, scale, dout)
    for got, want in ((gamma.grad, wg), (beta.grad, wb)):
        got = got.cpu().double()
        assert got.shape == want.shape
        tol = 1e-4 * max(want.abs().max().item(), 1e-6)
        assert (got - want).abs().max().item() < tol, ((got - want).abs().max().item(), tol)


@pytest.mark.parametrize("path", NET_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_filmed_net_film_grads_match_oracle_autograd(path):
    """film_layers = 1 (the reference default): the gradient reaches (gamma, beta)
    of the last block through the frozen decoder over cat(x, residual)."""
    from test_gpu_net import _build
    meta, params, x, _, _ = load_net(path)
    net = _build(meta, params, filmed=True, film_layers=1).requires_grad_(False)
    B, C = x.shape[0], meta["C"]
    g = torch.Generator().manual_seed(5)
    film0 = 0.1 * torch.randn(B, 2, 1, C, generator=g)
    film = film0.clone().to(DEV).requires_grad_()
    y = net(x.to(DEV), film, 0.8)
    w = torch.randn(y.shape, generator=g)
    (y * w.to(DEV)).sum().backward()
    pd = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    fd = film0.double().requires_grad_()
    cfg = net_cfg(meta)
    yd = sfno_ref.net_forward(pd, x.double(), cfg, sfno_ref.make_net_transforms(cfg, torch.float64),
                              film=(fd[:, 0], fd[:, 1]), scale=0.8)
    (yd * w.double()).sum().backward()
    got, want = film.grad.cpu().double(), fd.grad
    assert (got - want).abs().max().item() < 1e-4 * want.abs().max().item()


ALL_BLOCK_CASES = golden_files()


@pytest.mark.parametrize("path", ALL_BLOCK_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_block_input_grad_matches_oracle_autograd(path):
    """dL/dx (and dL/dgamma, dL/dbeta) through the block (msfno_block_backward): every
    golden wiring -- middle (linear inner skip, MLP, identity outer skip), first (block 0,
    resampling down), last (no MLP, resampling up), both filters, filmed and plain --
    against fp64 autograd through the oracle.  Tolerance: max-abs < 1e-4 x max|grad|."""
    meta, params, arrays, _ = load(path)
    blk, _, _ = make_block(meta, params)
    blk = blk.to(DEV).requires_grad_(False)  # SFNO frozen (model.py:1016-1023)
    scale = float(meta["scale"])
    filmed = bool(meta["filmed"])
    g = torch.Generator().manual_seed(13)
    x0 = arrays["x"]
    x = x0.clone().to(DEV).requires_grad_()
    gamma = arrays["gamma"].clone().to(DEV).requires_grad_()
    beta = arrays["beta"].clone().to(DEV).requires_grad_()
    y = blk(x, gamma, beta, scale) if filmed else blk(x)
    dout = torch.randn(y.shape, generator=g)
    (y * dout.to(DEV)).sum().backward()
    inner, outer, has_mlp = wiring_cfg(meta)
    cfg = sfno_ref.BlockCfg(filter_type=meta["filter"], inner_skip=inner, outer_skip=outer,
                            has_mlp=has_mlp)
    pd = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    sht, isht = _oracle_transforms(meta)
    xd = x0.double().requires_grad_()
    gd = arrays["gamma"].double().requires_grad_()
    bd = arrays["beta"].double().requires_grad_()
    yd = sfno_ref.block_forward(pd, xd, sht, isht, cfg, gd if filmed else None,
                                bd if filmed else None, scale)
    (yd * dout.double()).sum().backward()
    pairs = [("x", x.grad, xd.grad)]
    if filmed:
        pairs += [("gamma", gamma.grad, gd.grad), ("beta", beta.grad, bd.grad)]
    for name, got, want in pairs:
        got = got.cpu().double()
        assert got.shape == want.shape
        err = (got - want).abs().max().item()
        tol = 1e-4 * max(want.abs().max().item(), 1e-6)
        print(f"{os.path.basename(path)} d{name}: max-abs {err:.3e} (max|grad| "
              f"{want.abs().max().item():.3e})")
        assert err < tol, (name, err, tol)


def _film_away_from_kinks(pd, x, cfg, tr64, B, k, C, margin=2e-5):
    """(generator, FiLM modulation) of the first seed for which no spectral-MLP
    pre-activation of the fp64 oracle forward lies within `margin` (relative to its
    layer's largest) of ComplexReLU's kink at zero: there the derivative jumps, and an
    fp32 forward (whose inputs carry the previous blocks' rounding) may pick the other
    side -- a legitimate difference, not a backward error.  Only the blocks whose dL/dx
    the gradient crosses count; structural zeros (l < m) are exact and excluded."""
    import oracle.sfno_ref as R
    orig = R.complex_relu_real
    for seed in range(7, 64):
        g = torch.Generator().manual_seed(seed)
        film0 = 0.1 * torch.randn(B, 2, k, C, generator=g)
        worst = [1.0]
        calls = [0]

        def rec(z):
            # only the blocks whose dL/dx the gradient crosses (after the first filmed one)
            if calls[0] // cfg.spectral_layers > cfg.num_layers - k:
                a = torch.view_as_real(z)[..., 0].abs()
                nz = a[a > 0]
                if nz.numel():
                    worst[0] = min(worst[0], (nz.min() / a.max()).item())
            calls[0] += 1
            return orig(z)
        R.complex_relu_real = rec
        try:
            with torch.no_grad():
                f = film0.double()
                sfno_ref.net_forward(pd, x.double(), cfg, tr64, film=(f[:, 0], f[:, 1]), scale=0.8)
        finally:
            R.complex_relu_real = orig
        if worst[0] > margin:
            return g, film0
    raise AssertionError("no kink-free FiLM seed found")


@pytest.mark.parametrize("film_layers", [2, 4, "repeat"])
@pytest.mark.parametrize("path", NET_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_filmed_net_multi_layer_film_grads(path, film_layers):
    """--film-layers k (main.py:1083-1087) and --repeat-film (main.py:1133-1136): the
    gradient reaches the modulation of every filmed block through the dL/dx of the
    filmed blocks after it (sfnonet.py:838-844), the last one through the decoder.
    4-block fixture: k = 4 and repeat_film film every block, including block 0
    (resampling down, no skips) and block 3 (resampling up, no MLP)."""
    from types import SimpleNamespace

    from msfno_amd.sfno import FourierNeuralOperatorNet_Filmed
    meta, params, x, _, _ = load_net(path)
    n = meta["num_layers"]
    repeat = film_layers == "repeat"
    k = n if repeat else film_layers
    kw = dict(filter_type=meta["filter"], img_size=(meta["nlat"], meta["nlon"]),
              scale_factor=meta["scale_factor"], in_chans=meta["in_chans"],
              out_chans=meta["out_chans"], embed_dim_sfno=meta["C"], num_layers=n,
              spectral_layers=3)
    net = FourierNeuralOperatorNet_Filmed("cpu", SimpleNamespace(repeat_film=repeat),
                                          film_layers=k, advanced_logging=False,
                                          model_depth=None, **kw)
    missing, unexpected = net.load_state_dict(params, strict=False)
    assert not unexpected and all(m.endswith((".weights", ".pct")) for m in missing)
    net = net.eval().to(DEV).requires_grad_(False)  # model.py:1016-1023
    B, C = x.shape[0], meta["C"]
    cfg = net_cfg(meta)
    pd = {kk: (v.double() if v.is_floating_point() else v) for kk, v in params.items()}
    tr64 = sfno_ref.make_net_transforms(cfg, torch.float64)
    g, film0 = _film_away_from_kinks(pd, x, cfg, tr64, B, k, C)
    film = film0.clone().to(DEV).requires_grad_()
    y = net(x.to(DEV), film, 0.8)
    w = torch.randn(y.shape, generator=g)
    (y * w.to(DEV)).sum().backward()
    fd = film0.double().requires_grad_()
    yd = sfno_ref.net_forward(pd, x.double(), cfg, tr64, film=(fd[:, 0], fd[:, 1]), scale=0.8)
    (yd * w.double()).sum().backward()
    got, want = film.grad.cpu().double(), fd.grad
    err = (got - want).abs().max().item()
    print(f"{os.path.basename(path)} film_layers={film_layers}: max-abs {err:.3e} "
          f"(max|grad| {want.abs().max().item():.3e}); per block and batch "
          f"{[[round((got - want)[b, :, i].abs().max().item(), 5) for i in range(k)] for b in range(B)]}")
    assert err < 1e-4 * want.abs().max().item()
    # every filmed block's modulation gets a gradient
    assert (want.abs().amax(dim=(0, 1, 3)) > 0).all()


# mid_* (91 x 180, C = 16): 16380 pixels, so the pixel reductions of wgrad_nt run in four
# K chunks (ksplit = 4) at narrow width; the wide shapes are in test_gpu_backward_shapes.py
PARAM_CASES = [p for p in golden_files()
               if os.path.basename(p).startswith(("c1_", "c1b2_", "lg_", "down_", "up_", "mid_"))]


@pytest.mark.parametrize("path", PARAM_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_block_param_grads_match_oracle_autograd(path):
    """--retrain-film trains the last film_layers blocks (MSFNO/Models/sfno/model.py:922-923,
    1016-1019): the gradient of every block parameter (norm affines, spectral weights of
    either filter, inner skip, MLP) from msfno_block_backward_params, with dL/dx, against
    fp64 autograd through the oracle.  Tolerance: max-abs < 1e-4 x max|grad| per tensor."""
    import oracle.sfno_ref as R
    meta, params, arrays, _ = load(path)
    blk, _, _ = make_block(meta, params)
    blk = blk.to(DEV)
    taps = {}
    _tap_blocks(type("OneBlock", (), {"blocks": [blk]}), taps)
    scale = float(meta["scale"])
    filmed = bool(meta["filmed"])
    g = torch.Generator().manual_seed(17)
    x0 = arrays["x"]
    x = x0.clone().to(DEV).requires_grad_()
    film = (arrays["gamma"].to(DEV), arrays["beta"].to(DEV), scale) if filmed else ()
    y = blk(x, *film)
    dout = torch.randn(y.shape, generator=g)
    (y * dout.to(DEV)).sum().backward()
    inner, outer, has_mlp = wiring_cfg(meta)
    cfg = sfno_ref.BlockCfg(filter_type=meta["filter"], inner_skip=inner, outer_skip=outer,
                            has_mlp=has_mlp)
    pd = {k: (v.double().requires_grad_() if v.is_floating_point() else v)
          for k, v in params.items()}
    sht, isht = _oracle_transforms(meta)
    xd = x0.double().requires_grad_()
    orig = R.complex_relu_real
    R.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)
    try:
        yd = sfno_ref.block_forward(pd, xd, sht, isht, cfg,
                                    arrays["gamma"].double() if filmed else None,
                                    arrays["beta"].double() if filmed else None, scale)
        (yd * dout.double()).sum().backward()
    finally:
        R.complex_relu_real = orig
    name = os.path.basename(path)[:-4]
    _compare(f"{name} dx", x.grad, xd.grad)
    n = _compare_params(name, list(blk.named_parameters()),
                        lambda k: pd[k].grad if pd[k].grad is not None else torch.zeros_like(pd[k]))
    assert n >= 5


@pytest.mark.parametrize("path", NET_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_retrain_film_param_grads_match_oracle_autograd(path):
    """--retrain-film on a FourierNeuralOperatorNet_Filmed (film_layers = 2): the decoder,
    the last two blocks and the FiLM modulation get gradients (MSFNO/Models/sfno/model.py:
    922-923, 1016-1019; the encoder and earlier blocks stay frozen, sfnonet.py:816-844),
    against fp64 autograd through the oracle network."""
    from types import SimpleNamespace

    from msfno_amd.sfno import FourierNeuralOperatorNet_Filmed
    meta, params, x, _, _ = load_net(path)
    n, k = meta["num_layers"], 2
    kw = dict(filter_type=meta["filter"], img_size=(meta["nlat"], meta["nlon"]),
              scale_factor=meta["scale_factor"], in_chans=meta["in_chans"],
              out_chans=meta["out_chans"], embed_dim_sfno=meta["C"], num_layers=n,
              spectral_layers=3)
    net = FourierNeuralOperatorNet_Filmed("cpu", SimpleNamespace(repeat_film=False),
                                          film_layers=k, advanced_logging=False,
                                          model_depth=None, **kw)
    net.load_state_dict(params, strict=False)
    net = net.eval().to(DEV)
    grad_layers = ["decoder"] + [f"blocks.{n - 1 - i}." for i in range(k)]
    for name, p in net.named_parameters():  # model.py:1014-1019
        p.requires_grad_(any(name.startswith(gl) for gl in grad_layers))
    B, C = x.shape[0], meta["C"]
    g = torch.Generator().manual_seed(23)
    film0 = 0.1 * torch.randn(B, 2, k, C, generator=g)
    taps = {}
    _tap_blocks(net, taps)
    film = film0.clone().to(DEV).requires_grad_()
    y = net(x.to(DEV), film, 0.8)
    w = torch.randn(y.shape, generator=g)
    (y * w.to(DEV)).sum().backward()
    cfg = net_cfg(meta)
    pd = {kk: (v.double() if v.is_floating_point() else v) for kk, v in params.items()}
    for kk in pd:
        if any(kk.startswith(gl) for gl in grad_layers) and pd[kk].is_floating_point():
            pd[kk].requires_grad_()
    tr64 = sfno_ref.make_net_transforms(cfg, torch.float64)
    fd = film0.double().requires_grad_()
    import oracle.sfno_ref as R
    orig = R.complex_relu_real
    R.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)  # the GPU's ReLU masks
    try:
        yd = sfno_ref.net_forward(pd, x.double(), cfg, tr64, film=(fd[:, 0], fd[:, 1]),
                                  scale=0.8)
        (yd * w.double()).sum().backward()
    finally:
        R.complex_relu_real = orig
    tag = os.path.basename(path)[:-4]
    _compare(f"{tag} dfilm", film.grad, fd.grad)
    named = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
    for k, p in net.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
    trained = _compare_params(tag, named, lambda k: pd[k].grad if pd[k].grad is not None
                              else torch.zeros_like(pd[k]))
    assert trained >= 8


@pytest.mark.parametrize("path", NET_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_plain_net_all_param_grads_match_oracle_autograd(path):
    """A plain FourierNeuralOperatorNet in training (sfnonet.py:665-686, no no_grad
    regions): every parameter -- encoder, pos_embed, all blocks, decoder -- and dL/dx
    against fp64 autograd through the oracle network under the GPU's ReLU masks."""
    import oracle.sfno_ref as R
    from test_gpu_net import _build
    meta, params, x, _, _ = load_net(path)
    net = _build(meta, params)
    taps = {}
    _tap_blocks(net, taps)
    g = torch.Generator().manual_seed(29)
    xg = x.clone().to(DEV).requires_grad_()
    y = net(xg)
    w = torch.randn(y.shape, generator=g)
    (y * w.to(DEV)).sum().backward()
    cfg = net_cfg(meta)
    pd = {kk: (v.double().requires_grad_() if v.is_floating_point() else v)
          for kk, v in params.items()}
    tr64 = sfno_ref.make_net_transforms(cfg, torch.float64)
    xd = x.double().requires_grad_()
    orig = R.complex_relu_real
    R.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)
    try:
        yd = sfno_ref.net_forward(pd, xd, cfg, tr64)
        (yd * w.double()).sum().backward()
    finally:
        R.complex_relu_real = orig
    tag = os.path.basename(path)[:-4]
    _compare(f"{tag} dx", xg.grad, xd.grad)
    n = _compare_params(tag, list(net.named_parameters()),
                        lambda k: pd[k].grad if pd[k].grad is not None else torch.zeros_like(pd[k]))
    assert n >= 20


def test_block_weight_grad_without_input_grad():
    """A block whose input needs no gradient but whose fc1 weight does (the first trained
    block under --retrain-film) still builds an autograd node and fills .grad."""
    path = [p for p in FILM_CASES if "_nl_" in os.path.basename(p) and "_middle" in p][0]
    meta, params, arrays, _ = load(path)
    blk, _, _ = make_block(meta, params)
    blk = blk.to(DEV).requires_grad_(False)
    w1 = blk.mlp.fwd[0].weight.requires_grad_(True)
    y = blk(arrays["x"].to(DEV), arrays["gamma"].to(DEV), arrays["beta"].to(DEV), 1.0)
    assert y.requires_grad
    y.sum().backward()
    assert w1.grad is not None and torch.isfinite(w1.grad).all() and w1.grad.abs().max() > 0


@pytest.mark.parametrize("film_layers", [4, "repeat"])
def test_film_grads_at_a_kink_seed_match_oracle_under_gpu_masks(film_layers):
    """The seed the kink-free search skips (7: round 5 measured 4.7e-4 relative on net_nl
    with film_layers 4 / repeat).  The oracle's fp64 autograd is evaluated with the
    ComplexReLU(real) masks the GPU backward actually applied (each block's recomputed
    hidden activations, msfno_block_backward_hidden_offsets); with them the gradients
    agree to 1e-4 x max|grad|, so the difference under the oracle's own masks comes only
    from pre-activations on the other side of the kink (activations.py:42-46)."""
    from types import SimpleNamespace

    import oracle.sfno_ref as R
    from msfno_amd.sfno import FourierNeuralOperatorNet_Filmed
    path = [p for p in NET_FIXTURES if os.path.basename(p) == "net_nl.npz"][0]
    meta, params, x, _, _ = load_net(path)
    n = meta["num_layers"]
    repeat = film_layers == "repeat"
    k = n if repeat else film_layers
    kw = dict(filter_type=meta["filter"], img_size=(meta["nlat"], meta["nlon"]),
              scale_factor=meta["scale_factor"], in_chans=meta["in_chans"],
              out_chans=meta["out_chans"], embed_dim_sfno=meta["C"], num_layers=n,
              spectral_layers=3)
    net = FourierNeuralOperatorNet_Filmed("cpu", SimpleNamespace(repeat_film=repeat),
                                          film_layers=k, advanced_logging=False,
                                          model_depth=None, **kw)
    net.load_state_dict(params, strict=False)
    net = net.eval().to(DEV).requires_grad_(False)
    B, C = x.shape[0], meta["C"]
    g = torch.Generator().manual_seed(7)
    film0 = 0.1 * torch.randn(B, 2, k, C, generator=g)
    # GPU, tapping every block backward's hidden activations
    taps = {}
    for i, blk in enumerate(net.blocks):
        def tapped(*a, _i=i, _orig=blk.native_backward, **kwa):
            return _orig(*a, hidden_tap=lambda hs: taps.__setitem__(_i, [h.cpu() for h in hs]),
                         **kwa)
        blk.native_backward = tapped
    film = film0.clone().to(DEV).requires_grad_()
    y = net(x.to(DEV), film, 0.8)
    w = torch.randn(y.shape, generator=g)
    (y * w.to(DEV)).sum().backward()
    got = film.grad.cpu().double()
    assert taps, "no block backward ran"
    # oracle fp64 autograd: own masks, then the GPU's masks where it has them
    cfg = net_cfg(meta)
    pd = {kk: (v.double() if v.is_floating_point() else v) for kk, v in params.items()}
    tr64 = sfno_ref.make_net_transforms(cfg, torch.float64)
    L = cfg.spectral_layers
    orig = R.complex_relu_real
    flips = [0]

    def oracle_grad(use_gpu_masks):
        calls = [0]

        def relu(z):
            blk, layer = divmod(calls[0], L)
            calls[0] += 1
            if not use_gpu_masks or blk not in taps:
                return orig(z)
            m = (taps[blk][layer].real > 0).to(torch.float64)
            flips[0] += int(((z.real > 0).to(torch.float64) != m).sum())
            return torch.complex(z.real * m, z.imag)
        R.complex_relu_real = relu
        try:
            fd = film0.double().requires_grad_()
            yd = sfno_ref.net_forward(pd, x.double(), cfg, tr64, film=(fd[:, 0], fd[:, 1]),
                                      scale=0.8)
            (yd * w.double()).sum().backward()
        finally:
            R.complex_relu_real = orig
        return fd.grad

    own = oracle_grad(False)
    masked = oracle_grad(True)
    bar = 1e-4 * own.abs().max().item()
    e_own = (got - own).abs().max().item()
    e_mask = (got - masked).abs().max().item()
    print(f"net_nl film_layers={film_layers} seed 7: |GPU - oracle(own masks)| {e_own:.3e}, "
          f"|GPU - oracle(GPU masks)| {e_mask:.3e}, bar {bar:.3e}, "
          f"{flips[0]} mask elements differ (blocks tapped {sorted(taps)})")
    assert e_mask < bar
