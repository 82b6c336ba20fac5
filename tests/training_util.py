"""Helpers of test_gpu_training_loop.py: the two networks a training loop drives (a plain
FourierNeuralOperatorNet with every parameter trainable; a FourierNeuralOperatorNet_Filmed
with the native graph generator as film_gen under the --retrain-film freeze pattern), their
inputs, the weight-update mechanisms, and the fp64 oracle gradients under the GPU's
ComplexReLU masks."""
import functools

import torch

import filmgen_ref as R
from test_oracle_net import load_net, net_cfg

DEV = "cuda"
FILM_LAYERS = 2
GEN_DEPTH, GEN_HIDDEN, GEN_GRID = 1, 64, (12, 24)
MECHANISMS = ["sgd", "adam", "adam_fused", "load_state_dict", "data_copy", "data_assign"]


@functools.lru_cache(maxsize=None)
def fixture(path):
    return load_net(path)


def gen_stack(B):
    """The filmgen tests' shared graph, sst and fp64 / fp32 references at (12, 24)."""
    from test_gpu_filmgen import _stack
    return _stack((GEN_DEPTH, GEN_HIDDEN, 1, B, FILM_LAYERS, GEN_GRID))


def build(kind, path, state=None):
    """kind "plain": the fixture network, every parameter trainable.  kind "filmed": the
    filmed network (film_layers = 2) with Film_wrapper as film_gen; the generator, the
    decoder and the two filmed blocks train, the rest is frozen (model.py:1014-1019).
    ``state``: a state_dict to load (cloned) in place of the fixture's values."""
    from test_gpu_net import _build
    meta, params, x, _, _ = fixture(path)
    if kind == "plain":
        net = _build(meta, params)
    else:
        from test_gpu_filmgen import _wrapper
        net = _build(meta, params, filmed=True, film_layers=FILM_LAYERS)
        C = meta["C"]
        fw = _wrapper(gen_stack(x.shape[0]), GEN_DEPTH, GEN_HIDDEN, FILM_LAYERS, features=C)
        gp = R.make_params(GEN_DEPTH, 1, GEN_HIDDEN, 2 * FILM_LAYERS * C, 21)
        gp["head_film.weight"] *= 0.1   # FiLM of the size the network tests use
        gp["head_film.bias"] *= 0.1
        fw.film_gen.load_state_dict(gp)
        net.film_gen = fw
        n = meta["num_layers"]
        train = ["decoder", "film_gen"] + [f"blocks.{n - 1 - i}." for i in range(FILM_LAYERS)]
        for name, p in net.named_parameters():
            p.requires_grad_(any(name.startswith(t) for t in train))
    if state is not None:
        net.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return net


def inputs(kind, path):
    """The positional arguments of the network's forward, on the device."""
    x = fixture(path)[2].to(DEV)
    if kind == "plain":
        return (x,)
    return (x, gen_stack(x.shape[0]).sst.to(DEV), 0.8)


def target(path, seed=41):
    y = fixture(path)[3]
    return torch.randn(y.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def trainable(net):
    return [(k, p) for k, p in net.named_parameters() if p.requires_grad]


def grads_of(net):
    return {k: p.grad.clone() for k, p in trainable(net)}


def loss_backward(net, args, tar):
    """One training forward and backward of the L2Sphere loss; the detached output."""
    from msfno_amd.losses import L2Sphere
    y = net(*args)
    L2Sphere()(y, tar).backward()
    return y.detach()


def observe(net, args, tar):
    """(the no_grad output, the grad-mode output, every gradient of one backward)."""
    with torch.no_grad():
        y0 = net(*args).clone()
    net.zero_grad(set_to_none=True)
    y = loss_backward(net, args, tar)
    return y0, y, grads_of(net)


def perturbed(p, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(p.shape, generator=g).to(p.device)
    b = torch.randn(p.shape, generator=g).to(p.device)
    return (p.detach() * (1 + 0.05 * a) + 0.005 * b).to(p.dtype)


def apply_update(mech, net, args, tar, only_trainable=True):
    """Change the weights of ``net`` (already warmed: its .grad fields hold one backward)
    by one of MECHANISMS.  The optimizers take two steps on the trainable parameters;
    load_state_dict replaces every parameter; the two ``.data`` mechanisms write the
    trainable ones (what an optimizer that syncs through ``param.data`` touches), or every
    parameter with ``only_trainable=False``."""
    import pytest
    named = trainable(net) if only_trainable else list(net.named_parameters())
    ps = [p for _, p in named]
    if mech in ("sgd", "adam", "adam_fused"):
        if mech == "sgd":
            gmax = max(p.grad.abs().max().item() for p in ps)
            opt = torch.optim.SGD(ps, lr=0.02 / gmax, momentum=0.9)  # first step: 0.02 at most
        elif mech == "adam":
            opt = torch.optim.Adam(ps, lr=5e-3)
        else:
            try:
                opt = torch.optim.Adam(ps, lr=5e-3, fused=True)
            except RuntimeError as e:
                pytest.skip(f"this torch build rejects Adam(fused=True): {e}")
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss_backward(net, args, tar)
            opt.step()
    elif mech == "load_state_dict":
        names = {k for k, _ in net.named_parameters()}
        sd = net.state_dict()
        net.load_state_dict({k: perturbed(v, 100 + i) if k in names else v.clone()
                             for i, (k, v) in enumerate(sd.items())}, strict=True)
    elif mech == "data_copy":
        for i, p in enumerate(ps):
            p.data.copy_(perturbed(p, 100 + i))
    elif mech == "data_assign":
        for i, p in enumerate(ps):
            p.data = perturbed(p, 100 + i)
    elif mech == "mul_no_grad":
        with torch.no_grad():
            for i, p in enumerate(ps):
                p.mul_(1.0 + 0.25 * (-1) ** i)
    else:
        raise ValueError(mech)


def invalidate(net):
    net.apply(lambda m: m.invalidate_weight_cache() if hasattr(m, "invalidate_weight_cache")
              else None)


def assert_same(tag, a, b):
    """(y0, y, grads) of two networks, bitwise."""
    assert torch.equal(a[0], b[0]), f"{tag}: no_grad output"
    assert torch.equal(a[1], b[1]), f"{tag}: grad-mode output"
    assert sorted(a[2]) == sorted(b[2])
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, f"{tag}: gradients differ: {bad}"


def follow(kind, path, mech):
    """Section 1 for one of the two networks."""
    return follow_module(lambda state=None: build(kind, path, state), inputs(kind, path),
                         target(path), mech, f"{kind} {mech}")


def follow_module(make, args, tar, mech, tag):
    """Section 1 for one module and mechanism: warm every cache, update, and hold the
    updated module to a fresh one (``make(state)``) built from a clone of its state_dict,
    bitwise; the output must have moved by more than 1e-3 max|y|.  Returns the updated
    module's (y0, y, grads)."""
    net = make()
    before = observe(net, args, tar)          # one no_grad forward, one forward + backward
    apply_update(mech, net, args, tar)
    fresh = make({k: v.clone() for k, v in net.state_dict().items()})
    got = observe(net, args, tar)
    want = observe(fresh, args, tar)
    moved = (got[0] - before[0]).abs().max().item()
    assert moved > 1e-3 * before[0].abs().max().item(), ("the update changed nothing", moved)
    assert torch.isfinite(got[0]).all() and all(torch.isfinite(g).all() for g in got[2].values())
    assert_same(tag, got, want)
    return got


def oracle_param_grads(path, taps, loss64):
    """{name: dL/dp} in fp64 of L = loss64(net(x)) through the oracle network under the
    ComplexReLU masks in ``taps`` (the GPU backward's, _tap_blocks)."""
    import oracle.sfno_ref as S
    from backward_util import _masked_oracle
    meta, params, x, _, _ = fixture(path)
    cfg = net_cfg(meta)
    pd = {k: (v.double().requires_grad_() if v.is_floating_point() else v)
          for k, v in params.items()}
    tr64 = S.make_net_transforms(cfg, torch.float64)
    orig = S.complex_relu_real
    S.complex_relu_real = _masked_oracle(taps, cfg.spectral_layers)
    try:
        loss64(S.net_forward(pd, x.double(), cfg, tr64)).backward()
    finally:
        S.complex_relu_real = orig
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v))
            for k, v in pd.items() if v.is_floating_point()}


def rel_err(got, want64):
    """max|got - want| / max|want| (filmgen_ref.rel_err: no absolute floor)."""
    return R.rel_err(got.detach(), want64)
