"""GPU tests of the native graph FiLM generator (msfno_amd/filmgen.py, csrc/graph.hip,
csrc/gcn.cpp).

Yardsticks: at depth 0 the reference's own GCN_custom (tests/golden/filmgen/filmgen_*.npz, written
by tests/golden/make_golden_filmgen.py); at depth >= 1, which the reference cannot execute,
the fp64 restatement tests/filmgen_ref.py.  Tolerance (derived, not chosen):
err_native <= 8 x err_f32 with err = max|. - y64| / max|y64| per tensor, err_f32 that of the
reference (goldens) or of the restatement (otherwise) evaluated in fp32 on the CPU; 8 = 4
(the split-precision engine keeps operands to 2^-22, fp32 to 2^-24) x 2 (another summation
order in the K = hidden products and the node mean)."""
import functools
import glob
import os
import types

import numpy as np
import pytest
import torch

import filmgen_ref as R
from conftest import GOLDEN
from workspace_guard import guard_intact, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "filmgen", "filmgen_*.npz")))
FEATURES = 256

# depth, hidden, Fin, B, film_layers, (H, W)
STACK_CASES = [
    (1, 64, 1, 1, 1, (12, 24)),
    (3, 100, 1, 3, 2, (12, 24)),
    (2, 64, 5, 2, 1, (12, 24)),
    (1, 512, 1, 1, 1, (12, 24)),   # the workload's width on a tiny graph
    (2, 64, 1, 1, 1, (45, 90)),    # ~2,700 nodes: several GEMM row tiles and reduction chunks
]
# the paths no case above takes: no residual layer at all (the pool rides on conv1, the
# backward has no dense product), and a row wider than one sweep of 256 float4 lanes
EDGE_CASES = [
    (0, 64, 1, 2, 1, (12, 24)),
    (1, 1028, 2, 1, 1, (12, 24)),
]


def _module(depth, hidden, fin, out, idx, vals, mask, params):
    from msfno_amd.filmgen import GCN_custom
    n = int(mask.sum())
    m = GCN_custom(1, DEV, depth, in_features=fin, embed_dim=hidden, out_features=out,
                   adj=R.coo_tensor(idx, vals, n), nan_mask=mask)
    m.load_state_dict(params)
    return m


def _check(name, got, want64, err_f32):
    err = R.rel_err(got, want64)
    print(f"{name}: err_native {err:.3e}  err_f32 {err_f32:.3e}  ratio "
          f"{err / err_f32 if err_f32 else float('inf') if err else 0.0:.2f}")
    assert err <= R.PARAM_FACTOR * err_f32, (name, err, err_f32)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_goldens_at_depth_zero(path):
    z = np.load(path)
    params = {k.replace("__", "."): torch.from_numpy(z[k]) for k in z.files if "__" in k}
    hidden, L = int(z["hidden"]), int(z["film_layers"])
    m = _module(0, hidden, 1, 2 * L * FEATURES, z["coo_idx"].astype(np.int64), z["coo_val"],
                z["mask"], params)
    with torch.no_grad():
        y = m(torch.from_numpy(z["sst"]).to(DEV))
    assert y.shape == (1, 2 * L * FEATURES)
    _check("y", y[0], torch.from_numpy(z["y64"]), float(z["err_f32"]))


@functools.lru_cache(maxsize=None)
def _stack(case, seed=7, strongly_unsymmetric=False):
    depth, hidden, fin, B, L, (H, W) = case
    mask = R.make_mask(H, W, seed)
    n = int(mask.sum())
    idx, vals = R.make_adjacency(n, seed)
    if strongly_unsymmetric:  # links to higher-numbered nodes only, besides the self-loops
        keep = idx[1] >= idx[0]
        idx, vals = idx[:, keep], vals[keep]
    out = 2 * L * FEATURES
    params = R.make_params(depth, fin, hidden, out, seed)
    g = torch.Generator().manual_seed(seed + 1)
    sst = torch.randn(B, H, W, generator=g) if fin == 1 else torch.randn(B, fin, H, W, generator=g)
    dy = torch.randn(B, out, generator=g)
    A = R.coo_tensor(idx, vals, n).coalesce().to_dense()  # duplicates summed as the module does
    tm = torch.from_numpy(mask)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = R.grads({k: v.to(dt) for k, v in params.items()}, A.to(dt), tm, sst.to(dt),
                           depth, dy.to(dt))
    return types.SimpleNamespace(mask=mask, idx=idx, vals=vals, params=params, sst=sst, dy=dy,
                                 A=A, ref=ref, out=out)


def _native_grads(m, sst, dy):
    s = sst.to(DEV).requires_grad_()
    m.zero_grad()
    y = m(s)
    (y * dy.to(DEV)).sum().backward()
    return y.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, s.grad.clone()


@pytest.mark.parametrize("case", STACK_CASES + EDGE_CASES, ids=lambda c: "d{}_h{}_f{}_b{}_l{}_{}x{}".format(
    *c[:5], *c[5]))
def test_stack_forward_and_gradients_against_the_restatement(case):
    depth, hidden, fin = case[:3]
    c = _stack(case)
    m = _module(depth, hidden, fin, c.out, c.idx, c.vals, c.mask, c.params)
    y, grads, dsst = _native_grads(m, c.sst, c.dy)
    y64, g64, s64 = c.ref[torch.float64]
    y32, g32, s32 = c.ref[torch.float32]
    _check("y", y, y64, R.rel_err(y32, y64))
    assert sorted(grads) == sorted(R.param_names(depth))
    for k in R.param_names(depth):
        _check(k, grads[k], g64[k], R.rel_err(g32[k], g64[k]))
    _check("dsst", dsst, s64, R.rel_err(s32, s64))
    land = ~torch.from_numpy(c.mask)
    assert dsst.shape == c.sst.shape
    assert (dsst.cpu().reshape(dsst.shape[0], -1, *c.mask.shape)[:, :, land] == 0).all()


def test_backward_uses_the_transposed_adjacency():
    case = (1, 64, 1, 1, 1, (12, 24))
    c = _stack(case, strongly_unsymmetric=True)
    y64, g64, s64 = c.ref[torch.float64]
    _, g32, s32 = c.ref[torch.float32]
    p64 = {k: v.double() for k, v in c.params.items()}
    _, gw, sw = R.grads(p64, c.A.double(), torch.from_numpy(c.mask), c.sst.double(), 1,
                        c.dy.double(), wrong_adjoint=True)
    m = _module(1, 64, 1, c.out, c.idx, c.vals, c.mask, c.params)
    _, grads, dsst = _native_grads(m, c.sst, c.dy)
    # the two candidates are far apart where A^T acts: dsst and the conv1 gradients
    for name, right, wrong, f32, got in (("dsst", s64, sw, s32, dsst),
                                         ("conv1.weight", g64["conv1.weight"], gw["conv1.weight"],
                                          g32["conv1.weight"], grads["conv1.weight"])):
        tol = R.PARAM_FACTOR * R.rel_err(f32, right)
        assert R.rel_err(wrong, right) > 100 * tol, name
        _check(name, got, right, R.rel_err(f32, right))


def test_rows_of_a_batch_equal_the_single_sample_results_bitwise():
    case = STACK_CASES[1]
    depth, hidden, fin = case[:3]
    c = _stack(case)
    m = _module(depth, hidden, fin, c.out, c.idx, c.vals, c.mask, c.params)
    sst = c.sst.to(DEV)
    assert not torch.equal(sst[0], sst[1]) and not torch.equal(sst[1], sst[2])
    with torch.no_grad():
        yb = m(sst)
        for b in range(sst.shape[0]):
            assert torch.equal(m(sst[b:b + 1])[0], yb[b]), b


def test_two_calls_are_bit_identical():
    case = STACK_CASES[1]
    depth, hidden, fin = case[:3]
    c = _stack(case)
    m = _module(depth, hidden, fin, c.out, c.idx, c.vals, c.mask, c.params)
    y1, g1, s1 = _native_grads(m, c.sst, c.dy)
    y2, g2, s2 = _native_grads(m, c.sst, c.dy)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_workspace_contents_do_not_matter_and_its_end_is_respected():
    case = STACK_CASES[2]
    depth, hidden, fin, B = case[:4]
    c = _stack(case)
    m = _module(depth, hidden, fin, c.out, c.idx, c.vals, c.mask, c.params)
    sst, dy = c.sst.to(DEV), c.dy.to(DEV)
    res = []
    for fill in (0x00, 0xFF):  # 0xFF: every float a NaN
        for train in (False, True):
            nbytes = m.workspace_size(B, train)
            assert nbytes > 0
            ws = guarded(nbytes, fill)
            y, saved = m.native_forward(sst, train=train, ws=ws[:nbytes])
            guard_intact(ws, nbytes)
            out = [y]
            if train:
                grads, dsst = m.native_backward(dy, saved, sst.shape)
                guard_intact(ws, nbytes)
                out += grads + [dsst]
            res.append(out)
    for a, b in zip(res[:2], res[2:]):
        for t, u in zip(a, b):
            assert torch.isfinite(u).all() and torch.equal(t, u)
    assert torch.equal(res[0][0], res[1][0])  # with and without train
    for train in (False, True):
        short = torch.empty(m.workspace_size(B, train) - 1, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="workspace"):
            m.native_forward(sst, train=train, ws=short)
    short = torch.empty(m.workspace_size(B, True) - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        m.native_backward(dy, short, sst.shape)


def _wrapper(c, depth, hidden, L, features=FEATURES):
    from msfno_amd.filmgen import Film_wrapper
    cfg = types.SimpleNamespace(batch_size=1, model_depth=depth, embed_dim=hidden, film_layers=L,
                                film_gen_type=None, assets=None)
    n = int(c.mask.sum())
    fw = Film_wrapper(DEV, cfg, num_film_features=features, adj=R.coo_tensor(c.idx, c.vals, n),
                      nan_mask=c.mask)
    return fw


def test_graph_capture_replays_bitwise():
    case = STACK_CASES[0]
    depth, hidden, _, _, L, _ = case
    c = _stack(case)
    fw = _wrapper(c, depth, hidden, L)
    fw.film_gen.load_state_dict(c.params)
    static = c.sst.to(DEV).clone()
    other = torch.randn(c.sst.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
    with torch.no_grad():
        want0, want1 = fw(static).clone(), fw(other).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fw(static)  # warm-up
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fw(static)
        graph.replay()
        torch.cuda.synchronize()
        assert out.shape == (1, 2, L, FEATURES) and torch.equal(out, want0)
        static.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want1) and not torch.equal(want0, want1)


def test_end_to_end_generator_gradients_through_the_filmed_network():
    """Film_wrapper as film_gen of a small FourierNeuralOperatorNet_Filmed, everything else
    frozen: L2Sphere loss, one backward; generator gradients against fp64 autograd of
    restatement o oracle network.  Bound per tensor: max(8 err_f32, the network's own 1e-4 of
    tests/test_gpu_net.py), relative to max|grad|."""
    from msfno_amd.losses import L2Sphere
    from oracle import sfno_ref
    from test_gpu_net import _build
    from test_oracle_net import NET_FIXTURES, load_net, net_cfg
    meta, params, x, _, _ = load_net(NET_FIXTURES[0])
    C = meta["C"]
    depth, hidden, L = 2, 64, 1
    case = (depth, hidden, 1, x.shape[0], L, (12, 24))
    c = _stack(case)
    g = torch.Generator().manual_seed(21)
    gp = R.make_params(depth, 1, hidden, 2 * L * C, 21)
    gp["head_film.weight"] *= 0.1   # FiLM of the size the network tests use
    gp["head_film.bias"] *= 0.1
    net = _build(meta, params, filmed=True, film_layers=L)
    fw = _wrapper(c, depth, hidden, L, features=C)
    fw.film_gen.load_state_dict(gp)
    net.film_gen = fw
    for name, p in net.named_parameters():
        p.requires_grad_("film_gen" in name)
    xd, sst = x.to(DEV), c.sst.to(DEV)
    # under no_grad: the generator's tensor passed as sst with film_gen = None
    with torch.no_grad():
        y_gen = net(xd, sst, 0.8)
        film = fw(sst)
        net.film_gen = None
        y_film = net(xd, film, 0.8)
        net.film_gen = fw
    assert torch.equal(y_gen, y_film)
    tar = torch.randn(y_gen.shape, generator=g)
    loss_fn = L2Sphere()
    loss = loss_fn(net(xd, sst, 0.8), tar.to(DEV))
    loss.backward()
    got = {k: p.grad for k, p in fw.film_gen.named_parameters()}
    # fp64 (and fp32, for err_f32) autograd of restatement o oracle network o the same loss
    cfg = net_cfg(meta)
    want = {}
    for dt in (torch.float64, torch.float32):
        pd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in params.items()}
        ps = {k: v.to(dt).requires_grad_() for k, v in gp.items()}
        f = R.forward(ps, c.A.to(dt), torch.from_numpy(c.mask), c.sst.to(dt), depth)
        f = f.reshape(x.shape[0], 2, L, C)
        yd = sfno_ref.net_forward(pd, x.to(dt), cfg, sfno_ref.make_net_transforms(cfg, dt),
                                  film=(f[:, 0], f[:, 1]), scale=0.8)
        _l2sphere_ref(yd, tar.to(dt), loss_fn).sum().backward()
        want[dt] = {k: v.grad for k, v in ps.items()}
    for k in R.param_names(depth):
        assert got[k] is not None, k
        bound = max(R.PARAM_FACTOR * R.rel_err(want[torch.float32][k], want[torch.float64][k]),
                    1e-4)
        err = R.rel_err(got[k], want[torch.float64][k])
        print(f"{k}: err_native {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


def _l2sphere_ref(prd, tar, loss_fn):
    """The loss module's own math in torch ops of prd's dtype (relative L2 under the
    module's latitude weights), for the fp64 side of the end-to-end test."""
    from msfno_amd.losses import sphere_weights
    H = prd.shape[-2]
    w = torch.from_numpy(np.asarray(sphere_weights(loss_fn.kind, H))).to(prd.dtype)
    num = (w[:, None] * (prd - tar) ** 2).sum(dim=(-1, -2))
    den = (w[:, None] * tar ** 2).sum(dim=(-1, -2))
    out = num / den if loss_fn.relative else num
    return out if loss_fn.squared else out.sqrt()
