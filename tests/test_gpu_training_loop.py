"""The native modules driven the way a training loop drives them (the reference's
train_epoch, MSFNO/Models/train.py:146-197): weight updates between calls, two applications
of the network in one autograd graph, gradient accumulation, loss scaling and autocast,
and a weight changed between forward and backward.

Sections 1 to 3 compare bitwise (no kernel has atomics; the same kernels on the same bytes
give the same bits), against a fresh network built from the updated state_dict or against
the composition done by hand from single applications, which the fp64 oracle already holds
(test_gpu_film_backward.py).  Section 4 compares with the fp64 oracle under the GPU's ReLU
masks, relative to max|g64| per tensor with no absolute floor: a power-of-two factor on the
cotangent changes only exponents (in fp32, in the bf16 splits and in the x3h per-row range
scales), so err(s) <= 2 err(1) is asked, err(1) being the same network's unscaled error in
the same run.

Measured on an MI355X (the per-tensor figures are printed by the tests): every ratio
err(s) / err(1) is 1.000 for both scales and every tensor, because g(s) / s has the bits of
g(1) -- the backward is exactly homogeneous under a power of two at these sizes.
    net_lin  pos_embed 7.760e-07, blocks.1 filter w 7.252e-07, decoder fc2 w 2.002e-06
             (err(1) = err(2^16) = err(2^-24)); worst ratio 1.000 / 1.000
    net_nl   pos_embed 7.763e-06, blocks.1 filter w.1 7.479e-06, decoder fc2 w 9.568e-06;
             worst ratio 1.000 / 1.000
    filmgen  conv1.weight 2.068e-07, head_film.weight 7.725e-08, dsst 1.672e-07;
             worst ratio 1.000 / 1.000
    biases whose exact gradient is zero (a constant the next InstanceNorm removes) show
    err(1) of 5e-3 to 1e+8 against max|g64| of 1e-13 or less: rounding noise over nothing,
    and the same noise at every scale.
    AMP iteration (net_nl, lr 0.05): err(AMP) = err(plain) for every tensor, 2.1e-06
    (blocks.3 norm1 bias) to 3.4e-04 (pos_embed, whose step is 4.4e-05) where the step is
    not zero; GradScaler's scale stays 2^16.

What the tests found on the commit before them (run against that commit's Python files):
the weight images went stale after ``p.data.copy_`` (as predicted) and, not predicted,
after ``Adam(fused=True)``'s step, which in torch 2.10 for ROCm leaves ``_version`` alone
on the GPU; ``p.data = t`` was caught by the key's data_ptr.  Only the non-linear fixture
network and the fused-width modules hold images at all (the linear one at C = 16 has an
empty cache), hence test_fused_width_modules_follow_their_weights.  _BlockFn,
_FilmedBlockFn and _MLPFn accepted a backward after an in-place weight change.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    _repo = os.path.dirname(HERE)
    for _d in (HERE, _repo, os.path.join(_repo, "modulated-spherical-fourier-neural-operator_amd")):
        sys.path.insert(0, _d)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

import training_util as T  # noqa: E402
from backward_util import _tap_blocks  # noqa: E402
from block_util import make_block  # noqa: E402
from golden_util import golden_files, load  # noqa: E402
from test_oracle_net import NET_FIXTURES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = T.DEV
# the two fixtures have one shape (33 x 64, C = 16, 4 blocks), one per filter type; the
# non-linear one holds fewer parameters and serves where one network is enough
SMALLEST = min(NET_FIXTURES, key=os.path.getsize)
_ids = dict(ids=lambda p: os.path.basename(p)[:-4])
SCALES = (2.0 ** 16, 2.0 ** -24)


# ---- 1. outputs and gradients follow the weights, however they were updated ------------

@pytest.mark.parametrize("mech", T.MECHANISMS)
@pytest.mark.parametrize("path", NET_FIXTURES, **_ids)
@pytest.mark.parametrize("kind", ["plain", "filmed"])
def test_updated_network_equals_a_fresh_one(kind, path, mech):
    T.follow(kind, path, mech)


@pytest.mark.parametrize("kind", ["plain", "filmed"])
def test_frozen_network_changed_through_data_needs_invalidate(kind):
    """A network in eval with every parameter frozen keeps its weight images across calls
    (the graph-capture case).  After ``p.data.copy_`` on every parameter, which no key
    sees, ``invalidate_weight_cache()`` through ``net.apply`` makes the next call rebuild:
    the output equals a fresh network's bitwise, under no_grad and in grad mode (x
    requiring grad, so that the autograd Functions run)."""
    path = SMALLEST
    net = T.build(kind, path).requires_grad_(False)
    args = T.inputs(kind, path)

    def run(n):
        with torch.no_grad():
            y0 = n(*args).clone()
        x = args[0].clone().requires_grad_()
        y = n(x, *args[1:])
        y.square().sum().backward()
        return y0, y.detach(), x.grad

    before = run(net)
    run(net)  # a second call, on valid images
    for i, p in enumerate(net.parameters()):
        p.data.copy_(T.perturbed(p, 300 + i))
    T.invalidate(net)
    got = run(net)
    want = run(T.build(kind, path, state=net.state_dict()).requires_grad_(False))
    assert (got[0] - before[0]).abs().max().item() > 1e-3 * before[0].abs().max().item()
    for name, a, b in zip(("no_grad output", "grad-mode output", "dx"), got, want):
        assert torch.equal(a, b), name


def test_sgd_case_without_the_weight_cache(tmp_path):
    """MSFNO_WCACHE=0 (the images rebuilt inside every call; read once per process, so a
    child process): the SGD case passes there too and gives the bits it gives here."""
    out = str(tmp_path / "nocache.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out],
                       env=dict(os.environ, MSFNO_WCACHE="0"), cwd=HERE, capture_output=True,
                       text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    other = np.load(out)
    y0, y, grads = T.follow("plain", SMALLEST, "sgd")
    assert torch.equal(y0.cpu(), torch.from_numpy(other["y0"]))
    assert torch.equal(y.cpu(), torch.from_numpy(other["y"]))
    for k, g in grads.items():
        assert torch.equal(g.cpu(), torch.from_numpy(other["g__" + k])), k


if __name__ == "__main__":
    _y0, _y, _g = T.follow("plain", SMALLEST, "sgd")
    np.savez(sys.argv[1], y0=_y0.cpu().numpy(), y=_y.cpu().numpy(),
             **{"g__" + k: v.cpu().numpy() for k, v in _g.items()})


def _fused_mlp(state=None):
    from msfno_amd import _native as N
    from msfno_amd.sfno import MLP
    torch.manual_seed(11)
    m = MLP(73, 64, 256).eval().to(DEV)
    assert N.lib().msfno_mlp_fused_supported(m.native_desc()[0])
    if state is not None:
        m.load_state_dict(state)
    return m


def _fused_block(state=None):
    from test_gpu_mlp_fused import CASES, _block, _case
    cfg, p = _case(*CASES[0])[:2]
    blk = _block(cfg, p, *CASES[0][1:4])
    if state is not None:
        blk.load_state_dict(state)
    return blk


@pytest.mark.parametrize("mech", ["sgd", "adam_fused", "data_copy", "mul_no_grad"])
@pytest.mark.parametrize("which", ["mlp", "block"])
def test_fused_width_modules_follow_their_weights(which, mech):
    """The fixture networks (C = 16, 5 channels) are narrower than the fused kernels, so
    of the prepared images they hold only the non-linear filter's.  Here the two others:
    a stand-alone MLP at a fused width (73 -> 64 -> 256, the encoder's kind of cache) and
    a C = 256 filmed block on 33 x 64 (the fused block-MLP image and the spectral
    images), through the same warm / update / compare-with-fresh check."""
    g = torch.Generator().manual_seed(5)
    if which == "mlp":
        make = _fused_mlp
        args = (torch.randn(2, 73, 6, 10, generator=g).to(DEV),)
        tar = torch.randn(2, 256, 6, 10, generator=g).to(DEV)
    else:
        from test_gpu_mlp_fused import CASES, _case
        make = _fused_block
        _, _, x, gamma, beta = _case(*CASES[0])
        args = (x.to(DEV), gamma.to(DEV), beta.to(DEV), 0.7)
        tar = torch.randn(x.shape, generator=g).to(DEV)
    probe = make()
    assert probe._wcache_bytes(probe.native_desc()[0]) > 0
    T.follow_module(make, args, tar, mech, f"{which} {mech}")


def _lin_block():
    path = [p for p in golden_files() if os.path.basename(p) == "c1_lin_film_middle.npz"][0]
    meta, params, arrays, _ = load(path)
    return meta, params, arrays


def _sharded_block(blk, shards, x, gamma, beta, scale):
    from msfno_amd.sfno import LatBandBlock, LocalGroup
    gens = [s.stages(s.take(x), gamma, beta, scale) for s in shards]
    return LatBandBlock.assemble(shards, LocalGroup.run(gens))


@pytest.mark.parametrize("mech", ["data_copy", "mul_no_grad", "data_copy_frozen_invalidate"])
def test_latband_block_follows_its_weights(mech):
    """The latitude-band sharded block (world 2, LocalGroup) on a linear-filter fixture:
    each rank keeps its modes' slice of the filter weight besides the block's images.
    data_copy: the block trains and the calls run in grad mode, as a training step's
    would; mul_no_grad: an in-place update under no_grad (a new _version);
    data_copy_frozen_invalidate: a frozen block under no_grad, changed through .data, then
    invalidate_weight_cache().  Against fresh shards of a fresh block, bitwise."""
    from msfno_amd.sfno import LatBandBlock
    meta, params, arrays = _lin_block()
    blk = make_block(meta, params)[0].to(DEV)
    frozen = mech == "data_copy_frozen_invalidate"
    if frozen:
        blk.requires_grad_(False)
    x, g, b = (arrays[k].to(DEV) for k in ("x", "gamma", "beta"))
    scale = float(meta["scale"])
    shards = [LatBandBlock(blk, r, 2) for r in range(2)]
    with torch.set_grad_enabled(mech == "data_copy"):
        before = _sharded_block(blk, shards, x, g, b, scale).clone()
        assert torch.equal(_sharded_block(blk, shards, x, g, b, scale), before)
        w = blk.filter_layer.filter.w
        if mech == "mul_no_grad":
            with torch.no_grad():
                w.mul_(1.5)
                blk.mlp.fwd[0].weight.mul_(1.25)
        else:
            for i, p in enumerate(blk.parameters()):
                p.data.copy_(T.perturbed(p, 500 + i))
            if frozen:
                blk.invalidate_weight_cache()
        got = _sharded_block(blk, shards, x, g, b, scale)
        fresh = make_block(meta, None)[0].to(DEV).requires_grad_(not frozen)
        fresh.load_state_dict({k: v.clone() for k, v in blk.state_dict().items()})
        want = _sharded_block(fresh, [LatBandBlock(fresh, r, 2) for r in range(2)], x, g, b,
                              scale)
    assert (got - before).abs().max().item() > 1e-3 * before.abs().max().item()
    assert torch.equal(got, want)


def _sharded_net(shards, x):
    from msfno_amd.sfno import LatBandBlock, LocalGroup
    outs = LocalGroup.run([s.stages(s.take(x)) for s in shards])
    return LatBandBlock.assemble([s.shards[-1] for s in shards], outs)


@pytest.mark.parametrize("frozen", [False, True], ids=["training", "frozen_invalidate"])
def test_latband_net_follows_pos_embed_and_weights(frozen):
    """LatBandNet (world 2) keeps a row slice of pos_embed per rank: after ``.data.copy_``
    on every parameter (in grad mode while training; frozen, after an invalidate) the
    sharded output equals that of fresh shards of a fresh network, bitwise."""
    from msfno_amd.sfno import LatBandNet
    path = [p for p in NET_FIXTURES if "lin" in os.path.basename(p)][0]
    net = T.build("plain", path).requires_grad_(not frozen)
    x = T.inputs("plain", path)[0]
    shards = [LatBandNet(net, r, 2) for r in range(2)]
    with torch.set_grad_enabled(not frozen):
        before = _sharded_net(shards, x).clone()
        assert torch.equal(_sharded_net(shards, x), before)
        old_pe = net.pos_embed.detach().clone()
        for i, p in enumerate(net.parameters()):
            p.data.copy_(T.perturbed(p, 700 + i))
        if frozen:
            T.invalidate(net)
        got = _sharded_net(shards, x)
        fresh = T.build("plain", path, state=net.state_dict()).requires_grad_(not frozen)
        want = _sharded_net([LatBandNet(fresh, r, 2) for r in range(2)], x)
        assert torch.equal(got, want)
        # pos_embed alone put back: only its row slices change
        net.pos_embed.data.copy_(old_pe)
        if frozen:
            T.invalidate(net)
        back = _sharded_net(shards, x)
        fresh = T.build("plain", path, state=net.state_dict()).requires_grad_(not frozen)
        want_back = _sharded_net([LatBandNet(fresh, r, 2) for r in range(2)], x)
    assert (got - before).abs().max().item() > 1e-3 * before.abs().max().item()
    assert torch.equal(back, want_back) and not torch.equal(back, got)


# ---- 2. two applications of the network in one graph -----------------------------------

@pytest.mark.parametrize("path", NET_FIXTURES, **_ids)
@pytest.mark.parametrize("kind", ["plain", "filmed"])
def test_two_applications_in_one_graph(kind, path):
    """multi_step_training = 1 with discount 0.9: y1 = net(x), y2 = net(y1),
    L = l(y1, t1) / 2 + 0.9 l(y2, t2) / 2, one backward; against the composition by hand
    of two single applications.  Every sum compared has two fp32 terms (p.grad = g1 + g2;
    the cotangent of the first application = dl1/dy1 + dy1, dy1 being what the second
    application returns for its input: in the graph the loss term, created before the
    second application, is added to it last), so the order of addition cannot matter."""
    from msfno_amd.losses import L2Sphere
    net = T.build(kind, path)
    args = T.inputs(kind, path)
    x, rest = args[0], args[1:]
    t1, t2 = T.target(path, 43), T.target(path, 47)
    loss = L2Sphere()
    net.zero_grad(set_to_none=True)
    y1 = net(x, *rest)
    total = loss(y1, t1) / 2
    y2 = net(y1, *rest)
    total = total + 0.9 * loss(y2, t2) / 2
    total.backward()
    unrolled = T.grads_of(net)
    # by hand: the second application on a detached y1 ...
    net.zero_grad(set_to_none=True)
    y1d = y1.detach().clone().requires_grad_()
    y2h = net(y1d, *rest)
    assert torch.equal(y2h.detach(), y2.detach())
    (0.9 * loss(y2h, t2) / 2).backward()
    g2, dy1 = T.grads_of(net), y1d.grad.clone()
    # ... the first loss term's own cotangent ...
    y1l = y1.detach().clone().requires_grad_()
    (loss(y1l, t1) / 2).backward()
    # ... and the first application under the sum of the two
    net.zero_grad(set_to_none=True)
    net(x, *rest).backward(y1l.grad + dy1)
    g1 = T.grads_of(net)
    assert sorted(unrolled) == sorted(g1) == sorted(g2)
    bad = [k for k in unrolled if not torch.equal(unrolled[k], g1[k] + g2[k])]
    assert not bad, bad
    # both applications contribute: for most tensors neither part alone is the whole
    two = [k for k in unrolled if not torch.equal(unrolled[k], g1[k])
           and not torch.equal(unrolled[k], g2[k])]
    assert 2 * len(two) >= len(unrolled), (len(two), len(unrolled))
    if kind == "filmed":
        assert any("film_gen" in k for k in unrolled)


# ---- 3. accumulation -------------------------------------------------------------------

@pytest.mark.parametrize("path", NET_FIXTURES, **_ids)
@pytest.mark.parametrize("kind", ["plain", "filmed"])
def test_gradient_accumulation(kind, path):
    """Two micro-batches, backward on each without zero_grad: p.grad = ga + gb bitwise,
    ga and gb from separate runs; after zero_grad(set_to_none=True) one backward gives ga
    again; frozen parameters keep grad None throughout."""
    net = T.build(kind, path)
    args, tar = T.inputs(kind, path), T.target(path)

    def micro(i):  # one field of the fixture's batch of two
        return tuple(a[i:i + 1] if torch.is_tensor(a) else a for a in args), tar[i:i + 1]

    (aa, ta), (ab, tb) = micro(0), micro(1)
    assert not torch.equal(aa[0], ab[0])
    net.zero_grad(set_to_none=True)
    T.loss_backward(net, aa, ta)
    ga = T.grads_of(net)
    net.zero_grad(set_to_none=True)
    T.loss_backward(net, ab, tb)
    gb = T.grads_of(net)
    net.zero_grad(set_to_none=True)
    T.loss_backward(net, aa, ta)
    T.loss_backward(net, ab, tb)
    acc = T.grads_of(net)
    bad = [k for k in acc if not torch.equal(acc[k], ga[k] + gb[k])]
    assert not bad, bad
    two = [k for k in acc if not torch.equal(acc[k], ga[k]) and not torch.equal(acc[k], gb[k])]
    assert 2 * len(two) >= len(acc), (len(two), len(acc))   # both micro-batches count
    net.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in net.parameters())
    T.loss_backward(net, aa, ta)
    again = T.grads_of(net)
    bad = [k for k in again if not torch.equal(again[k], ga[k])]
    assert not bad, bad
    for k, p in net.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), k


# ---- 4. cotangent magnitude, GradScaler and autocast -----------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind,path", [("plain", p) for p in NET_FIXTURES] + [("filmed", SMALLEST)],
                         ids=lambda v: os.path.basename(v)[:-4] if v.endswith(".npz") else v)
def test_autocast_leaves_output_and_loss_alone(kind, path, dtype):
    """Inside torch.autocast the network output and the L2Sphere loss are fp32 and bitwise
    what they are outside it (the reference wraps its transforms in
    autocast(enabled=False); the native calls take and return fp32 whatever the mode)."""
    from msfno_amd.losses import L2Sphere
    net = T.build(kind, path)
    args, tar = T.inputs(kind, path), T.target(path)
    y = net(*args)
    l = L2Sphere()(y, tar)
    with torch.autocast("cuda", dtype=dtype):
        ya = net(*args)
        la = L2Sphere()(ya, tar)
    assert ya.dtype == torch.float32 and la.dtype == torch.float32
    assert ya.requires_grad and la.requires_grad
    assert torch.equal(ya, y) and torch.equal(la, l)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        yn = net(*args)
    with torch.no_grad():
        assert yn.dtype == torch.float32 and torch.equal(yn, net(*args))


def _report(tag, errs):
    """errs: {name: (err(1), {s: err(s)})}.  Prints every figure, then asserts."""
    worst = {s: (0.0, None) for s in SCALES}
    for k, (e1, es) in errs.items():
        line = f"{tag} {k}: err(1) {e1:.3e}"
        for s in SCALES:
            ratio = es[s] / e1 if e1 > 0 else (1.0 if es[s] == 0 else float("inf"))
            line += f"  err(2^{int(np.log2(s))}) {es[s]:.3e} (x{ratio:.3f})"
            if ratio > worst[s][0]:
                worst[s] = (ratio, k)
        print(line)
    print(f"{tag} worst ratios: " + ", ".join(
        f"2^{int(np.log2(s))}: {worst[s][0]:.3f} ({worst[s][1]})" for s in SCALES))
    for k, (e1, es) in errs.items():
        for s in SCALES:
            assert np.isfinite(es[s]), (k, s)
            assert es[s] <= 2 * e1, (tag, k, s, es[s], e1)


@pytest.mark.parametrize("path", NET_FIXTURES, **_ids)
def test_scaled_cotangents_through_the_plain_net(path):
    """s w back-propagated through the plain network for s = 1, 2^16 (GradScaler's initial
    scale) and 2^-24 (a relative loss averaged over a real grid), w the cotangent of
    test_plain_net_all_param_grads_match_oracle_autograd: g / s finite and
    err(s) <= 2 err(1) per parameter tensor against the fp64 oracle under the GPU's ReLU
    masks, err = max|g / s - g64| / max|g64|."""
    net = T.build("plain", path)
    taps = {}
    _tap_blocks(net, taps)
    x = T.inputs("plain", path)[0]
    w = None
    got = {}
    for s in (1.0,) + SCALES:
        net.zero_grad(set_to_none=True)
        y = net(x)
        if w is None:
            w = torch.randn(y.shape, generator=torch.Generator().manual_seed(29)).to(DEV)
        (y * (w * s)).sum().backward()
        got[s] = {k: p.grad / s for k, p in net.named_parameters()}
        for k, g in got[s].items():
            assert torch.isfinite(g).all(), (k, s)
    g64 = T.oracle_param_grads(path, taps, lambda yd: (yd * w.cpu().double()).sum())
    errs = {k: (T.rel_err(got[1.0][k], g64[k]), {s: T.rel_err(got[s][k], g64[k]) for s in SCALES})
            for k in got[1.0]}
    _report(os.path.basename(path)[:-4], errs)


def test_scaled_cotangents_through_the_generator():
    """The same two scales on the graph generator's gradients (the (12, 24) graph, hidden
    64, depth 1) against filmgen_ref in fp64."""
    from test_gpu_filmgen import _module, _stack
    case = (1, 64, 1, 1, 1, (12, 24))
    c = _stack(case)
    m = _module(1, 64, 1, c.out, c.idx, c.vals, c.mask, c.params)
    _, g64, s64 = c.ref[torch.float64]
    got = {}
    for s in (1.0,) + SCALES:
        sst = c.sst.to(DEV).requires_grad_()
        m.zero_grad(set_to_none=True)
        (m(sst) * (c.dy.to(DEV) * s)).sum().backward()
        got[s] = {k: p.grad / s for k, p in m.named_parameters()}
        got[s]["dsst"] = sst.grad / s
        for k, g in got[s].items():
            assert torch.isfinite(g).all(), (k, s)
    want = dict(g64, dsst=s64)
    errs = {k: (T.rel_err(got[1.0][k], want[k]), {s: T.rel_err(got[s][k], want[k]) for s in SCALES})
            for k in got[1.0]}
    _report("filmgen", errs)


def test_amp_iteration_matches_the_plain_iteration():
    """autocast(fp16) + GradScaler(init_scale = 2^16) + SGD, one iteration of the L2Sphere
    loss, next to the same iteration without AMP: the scaler does not skip the step, and
    per parameter tensor err = max|p_new - p_ref| / max|p_ref - p_old|, p_ref the fp64
    oracle's SGD step under the GPU's ReLU masks, obeys err(AMP) <= 2 err(plain)."""
    from msfno_amd.losses import L2Sphere
    from test_gpu_filmgen import _l2sphere_ref
    path, lr = SMALLEST, 0.05
    x, tar = T.inputs("plain", path)[0], T.target(path)
    loss_fn = L2Sphere()
    new, taps = {}, {}
    for amp in (False, True):
        net = T.build("plain", path)
        if not amp:
            _tap_blocks(net, taps)
        old = {k: p.detach().clone() for k, p in net.named_parameters()}
        opt = torch.optim.SGD(net.parameters(), lr=lr)
        if amp:
            scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
            with torch.autocast("cuda", dtype=torch.float16):
                loss = loss_fn(net(x), tar)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            assert scaler.get_scale() >= 2.0 ** 16   # no inf found: not backed off
            assert any(not torch.equal(p, old[k]) for k, p in net.named_parameters())
        else:
            loss_fn(net(x), tar).backward()
            opt.step()
        new[amp] = {k: p.detach().clone() for k, p in net.named_parameters()}
    g64 = T.oracle_param_grads(
        path, taps, lambda yd: _l2sphere_ref(yd, tar.cpu().double(), loss_fn).sum())
    for k in old:
        step = lr * g64[k]
        ref = old[k].cpu().double() - step
        size = step.abs().max().clamp_min(1e-300)
        e = {amp: float((new[amp][k].cpu().double() - ref).abs().max() / size)
             for amp in (False, True)}
        print(f"amp {k}: err(plain) {e[False]:.3e}  err(AMP) {e[True]:.3e}  "
              f"max|step| {float(size):.3e}")
        assert np.isfinite(e[True]) and e[True] <= 2 * e[False], (k, e)


# ---- 5. a weight changed between forward and backward is refused -----------------------

def _block_case(filmed):
    name = "c1_nl_film_middle.npz" if filmed else "c1_nl_plain_middle.npz"
    meta, params, arrays, _ = load([p for p in golden_files() if os.path.basename(p) == name][0])
    blk = make_block(meta, params)[0].to(DEV)
    film = (arrays["gamma"].to(DEV), arrays["beta"].to(DEV), float(meta["scale"])) if filmed else ()
    return blk, (arrays["x"].to(DEV),) + film, blk.mlp.fwd[0].weight


def _mlp_case():
    from msfno_amd.sfno import MLP
    torch.manual_seed(3)
    m = MLP(in_features=12, hidden_features=24, out_features=9).eval().to(DEV)
    return m, (torch.randn(2, 12, 6, 10, device=DEV),), m.fwd[2].weight


def _gcn_case():
    from test_gpu_filmgen import _module, _stack
    c = _stack((1, 64, 1, 1, 1, (12, 24)))
    m = _module(1, 64, 1, c.out, c.idx, c.vals, c.mask, c.params)
    return m, (c.sst.to(DEV),), m.conv_layers[0].weight


@pytest.mark.parametrize("fn,case", [("_BlockFn", lambda: _block_case(False)),
                                     ("_FilmedBlockFn", lambda: _block_case(True)),
                                     ("_MLPFn", _mlp_case), ("_GCNFn", _gcn_case)],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_weight_changed_between_forward_and_backward_is_refused(fn, case):
    """The backward of these Functions recomputes the forward from the module's weights as
    they are when it runs, so a weight changed in place after the forward must make
    backward() raise autograd's version error rather than return another function's
    gradient."""
    mod, args, weight = case()
    assert weight.requires_grad
    y = mod(*args)
    assert type(y.grad_fn).__name__.startswith(fn), type(y.grad_fn).__name__
    with torch.no_grad():
        weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    # an untouched forward still goes through
    y = mod(*args)
    y.sum().backward()
    assert weight.grad is not None and torch.isfinite(weight.grad).all()
