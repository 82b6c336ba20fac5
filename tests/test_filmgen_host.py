"""Host-side checks of the graph FiLM generator (msfno_amd/filmgen.py): the declaration,
binding and export of its three entry points, the C-ABI refusals (all before any launch),
the host CSR builder against scipy, the modules' state-dict keys and initial values, the
merge of a reference generator checkpoint by load_filmed_checkpoint, and the fixtures."""
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

import filmgen_ref as R
from conftest import GOLDEN, REPO

SYMBOLS = ("msfno_gcn_workspace_size", "msfno_gcn_forward", "msfno_gcn_backward")
FIXTURE_CAP = 576 * 1024  # the cap tests/test_loss_host.py applies to its fixtures


def test_entry_points_are_declared_bound_and_exported():
    from msfno_amd import _native as N
    import msfno_amd
    assert hasattr(msfno_amd, "filmgen")
    header = open(os.path.join(REPO, "include", "msfno.h")).read()
    declared = set(re.findall(r"\b(msfno_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in SYMBOLS:
        assert s in declared and s in bound and hasattr(N.lib(), s), s
    assert N.lib().msfno_abi_version() == 6
    assert f"#define MSFNO_GCN_MAX_DEPTH {N.GCN_MAX_DEPTH}" in header


def _structs(N, depth=2, Nn=50, p=4096, **over):
    g = N.GcnGraph()
    g.N, g.nnz = Nn, 100
    for k in ("row_ptr", "col", "val", "t_row_ptr", "t_col", "t_val"):
        setattr(g, k, p)
    d = N.GcnDesc()
    d.Fin, d.hidden, d.depth, d.out = 1, 64, depth, 32
    gr = N.GcnGrads()
    for s in (d, gr):
        s.conv1_w = s.conv1_b = s.head_w = s.head_b = p
        for i in range(depth):
            s.conv_w[i] = s.conv_b[i] = p
    for k, v in over.items():
        obj, field = k.split("__")
        setattr({"g": g, "d": d, "gr": gr}[obj], field, v)
    return g, d, gr


def test_c_abi_refusals_come_before_any_launch():
    """Every refusal is decided on the arguments alone: the pointers here are never
    dereferenced (this test runs without a GPU)."""
    from msfno_amd import _native as N
    lib = N.lib()
    B, Nn, p = 2, 50, 4096
    size = lib.msfno_gcn_workspace_size(B, Nn, 1, 64, 2, 32, 0)
    train = lib.msfno_gcn_workspace_size(B, Nn, 1, 64, 2, 32, 1)
    assert 0 < size < train
    for bad in ((0, Nn, 1, 64, 2, 32), (B, 0, 1, 64, 2, 32), (B, Nn, 0, 64, 2, 32),
                (B, Nn, 1, 0, 2, 32), (B, Nn, 1, 64, -1, 32), (B, Nn, 1, 64, 2, 0),
                (B, Nn, 1, 66, 2, 32), (B, Nn, 17, 64, 2, 32), (B, Nn, 1, 64, 17, 32),
                (B, (1 << 21), 1, 64, 2, 32)):
        assert lib.msfno_gcn_workspace_size(*bad, 0) == 0, bad
        assert lib.msfno_gcn_workspace_size(*bad, 1) == 0, bad

    def fwd(x=p, y=p, B=B, ws=p, nbytes=train, tr=1, **over):
        g, d, _ = _structs(N, **over)
        return lib.msfno_gcn_forward(g, d, x, y, B, tr, ws, nbytes, None)

    def bwd(dy=p, dx=p, B=B, ws=p, nbytes=train, **over):
        g, d, gr = _structs(N, **over)
        return lib.msfno_gcn_backward(g, d, dy, gr, dx, B, ws, nbytes, None)

    assert lib.msfno_gcn_forward(None, None, p, p, B, 0, p, size, None) == N.MSFNO_EINVAL
    for kw in (dict(x=None), dict(y=None), dict(ws=None), dict(B=0), dict(g__N=0),
               dict(g__row_ptr=None), dict(g__col=None), dict(g__val=None), dict(g__nnz=-1),
               dict(d__conv1_w=None), dict(d__head_b=None),
               dict(d__Fin=0), dict(d__out=0), dict(d__depth=-1), dict(ws=4100),
               dict(d__conv1_w=4100)):
        assert fwd(**kw) == N.MSFNO_EINVAL, kw
    for kw in (dict(dy=None), dict(ws=None), dict(B=0), dict(g__N=0), dict(g__t_row_ptr=None),
               dict(g__t_col=None), dict(g__row_ptr=None), dict(gr__conv1_w=None),
               dict(gr__head_b=None)):
        assert bwd(**kw) == N.MSFNO_EINVAL, kw
    for kw in (dict(d__hidden=66), dict(d__Fin=17), dict(d__depth=17)):
        assert fwd(nbytes=1 << 40, **kw) == N.MSFNO_EUNSUPPORTED, kw
        assert bwd(nbytes=1 << 40, **kw) == N.MSFNO_EUNSUPPORTED, kw
    assert fwd(nbytes=train - 1) == N.MSFNO_EWORKSPACE
    assert fwd(nbytes=size - 1, tr=0) == N.MSFNO_EWORKSPACE
    assert bwd(nbytes=train - 1) == N.MSFNO_EWORKSPACE
    # the transposed arrays may be absent for the forward
    assert fwd(nbytes=0, g__t_row_ptr=None, g__t_col=None, g__t_val=None) == N.MSFNO_EWORKSPACE
    with pytest.raises(NotImplementedError, match="hidden"):
        N.check(fwd(d__hidden=66), "msfno_gcn_forward")
    with pytest.raises(ValueError, match="workspace"):
        N.check(fwd(nbytes=0), "msfno_gcn_forward")


def test_csr_and_transposed_csr_agree_with_scipy():
    import scipy.sparse as sp
    from msfno_amd.filmgen import build_csr
    n = 40
    idx, vals = R.make_adjacency(n, 3)
    coo = R.coo_tensor(idx, vals, n)
    assert coo._nnz() > coo.coalesce()._nnz()          # duplicates present
    want = sp.coo_matrix((vals.astype(np.float64), (idx[0], idx[1])), shape=(n, n)).tocsr()
    want.sum_duplicates()
    want.sort_indices()
    assert want.indptr[3] == want.indptr[2]            # the empty row
    assert abs(want - want.T).max() > 0.1              # unsymmetric
    for adj in (coo, coo.coalesce().to_sparse_csr()):
        c = build_csr(adj)
        for pre, m in (("", want), ("t_", want.T.tocsr())):
            m.sort_indices()
            assert c[pre + "row_ptr"].dtype == torch.int32 and c[pre + "col"].dtype == torch.int32
            assert c[pre + "val"].dtype == torch.float32
            assert np.array_equal(c[pre + "row_ptr"].numpy(), m.indptr)
            assert np.array_equal(c[pre + "col"].numpy(), m.indices)
            assert np.allclose(c[pre + "val"].numpy(), m.data, rtol=1e-6, atol=0)
    with pytest.raises(TypeError):
        build_csr(coo.to_dense())
    with pytest.raises(ValueError):
        build_csr(torch.sparse_coo_tensor(torch.zeros(2, 1, dtype=torch.long), torch.ones(1), (3, 4)))


def test_grid_adjacency_is_the_row_normalised_four_neighbour_graph():
    from msfno_amd.filmgen import grid_adjacency
    mask = np.ones((3, 4), dtype=bool)
    mask[1, 1] = False
    A = grid_adjacency(mask).to_dense()
    n = int(mask.sum())
    assert A.shape == (n, n) and torch.allclose(A.sum(1), torch.ones(n))
    node = -np.ones((3, 4), dtype=int)
    node[mask] = np.arange(n)
    r = node[0, 0]  # self, south (1,0), east (0,1), west wraps to (0,3); no north
    assert set(torch.nonzero(A[r]).flatten().tolist()) == {node[0, 0], node[1, 0], node[0, 1],
                                                           node[0, 3]}
    assert torch.allclose(A[r][A[r] > 0], torch.full((4,), 0.25))
    r = node[1, 0]  # east is land; west wraps to (1,3)
    assert set(torch.nonzero(A[r]).flatten().tolist()) == {node[1, 0], node[0, 0], node[2, 0],
                                                           node[1, 3]}
    B = grid_adjacency(mask, wrap=False).to_dense()
    assert set(torch.nonzero(B[node[0, 0]]).flatten().tolist()) == {node[0, 0], node[1, 0],
                                                                    node[0, 1]}
    assert grid_adjacency(mask).layout == torch.sparse_coo


def _graph(seed=5, shape=(6, 8)):
    mask = R.make_mask(*shape, seed)
    n = int(mask.sum())
    idx, vals = R.make_adjacency(n, seed)
    return mask, R.coo_tensor(idx, vals, n)


def test_state_dict_keys_shapes_and_initial_values():
    from msfno_amd.filmgen import GCN_custom, GraphConvolution
    mask, adj = _graph()
    m = GCN_custom(4, "cpu", 3, in_features=2, embed_dim=32, out_features=24, adj=adj,
                   nan_mask=mask)
    sd = m.state_dict()
    assert list(sd) == R.param_names(3)
    assert sd["conv1.weight"].shape == (2, 32) and sd["conv_layers.2.weight"].shape == (32, 32)
    assert sd["head_film.weight"].shape == (24, 32) and sd["head_film.bias"].shape == (24,)
    assert (sd["head_film.weight"] == 1).all() and (sd["head_film.bias"] == 0).all()
    gain = torch.nn.init.calculate_gain("leaky_relu", 0.01)
    for k, v in sd.items():
        if k.endswith("bias"):
            assert (v == 0).all(), k
        elif k.startswith("conv"):
            bound = gain * (6.0 / (v.shape[0] + v.shape[1])) ** 0.5
            assert v.abs().max() <= bound and v.abs().max() > 0.5 * bound and v.std() > 0, k
    assert GraphConvolution(3, 5, bias=False).bias is None
    assert m.num_nodes == int(mask.sum()) and m._row_ptr.numel() == m.num_nodes + 1
    for bad in (dict(embed_dim=30), dict(in_features=17), dict(depth=17)):
        kw = dict(depth=1, in_features=1, embed_dim=32)
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            GCN_custom(1, "cpu", kw.pop("depth"), adj=adj, nan_mask=mask, **kw)
    with pytest.raises(ValueError, match="GPU"):
        m(torch.zeros(1, 2, *mask.shape))                           # no CPU path


def test_assets_are_read_under_the_reference_names(tmp_path):
    from msfno_amd.filmgen import GCN_custom
    mask, adj = _graph()
    torch.save(adj, tmp_path / "adj_coarsen_2_sparse.pt")
    np.save(tmp_path / "nan_mask_coarsen_2_notflatten.npy", mask)
    a = GCN_custom(1, "cpu", 0, embed_dim=8, out_features=4, coarse_level=2, assets=str(tmp_path))
    b = GCN_custom(1, "cpu", 0, embed_dim=8, out_features=4, adj=adj, nan_mask=mask)
    for k in ("_row_ptr", "_col", "_val", "_t_row_ptr", "_t_col", "_t_val", "_cells"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def _cfg(kind=None, L=2):
    return types.SimpleNamespace(batch_size=1, model_depth=2, embed_dim=16, film_layers=L,
                                 film_gen_type=kind, assets=None)


def test_film_wrapper_shapes_and_unsupported_types(monkeypatch):
    from msfno_amd.filmgen import Film_wrapper, GCN_custom
    mask, adj = _graph()
    fw = Film_wrapper("cpu", _cfg(), adj=adj, nan_mask=mask)
    assert isinstance(fw.film_gen, GCN_custom) and fw.film_gen.out_features == 2 * 2 * 256
    assert [k for k, _ in fw.named_parameters()][0] == "film_gen.conv1.weight"
    assert len(list(fw.get_parameters())) == 2 * 3 + 2
    # the reshape, with the native call replaced by a recognisable tensor
    monkeypatch.setattr(GCN_custom, "forward",
                        lambda self, sst: torch.arange(3 * 1024.0).reshape(3, 1024))
    out = fw(torch.zeros(3, *mask.shape))
    assert out.shape == (3, 2, 2, 256)
    assert out[1, 1, 0, 5] == 1024 + 512 + 5
    for kind in ("gcn", "transformer", "mae"):
        with pytest.raises(NotImplementedError, match=kind):
            Film_wrapper("cpu", _cfg(kind), adj=adj, nan_mask=mask)


@pytest.mark.parametrize("prefixed", [False, True], ids=["bare", "film_gen_prefix"])
def test_load_filmed_checkpoint_merges_a_reference_generator_checkpoint(prefixed):
    from msfno_amd.filmgen import Film_wrapper
    from msfno_amd.rollout import load_filmed_checkpoint
    from msfno_amd.sfno import FourierNeuralOperatorNet_Filmed
    from test_oracle_net import NET_FIXTURES, load_net
    meta, params, _, _, _ = load_net(NET_FIXTURES[0])
    mask, adj = _graph()
    fw = Film_wrapper("cpu", _cfg(L=1), num_film_features=meta["C"], adj=adj, nan_mask=mask)
    net = FourierNeuralOperatorNet_Filmed(
        "cpu", None, film_layers=1, advanced_logging=False, model_depth=None, film_gen=fw,
        filter_type=meta["filter"], img_size=(meta["nlat"], meta["nlon"]),
        scale_factor=meta["scale_factor"], in_chans=meta["in_chans"], out_chans=meta["out_chans"],
        embed_dim_sfno=meta["C"], num_layers=meta["num_layers"], spectral_layers=3)
    assert "film_gen.film_gen.conv1.weight" in net.state_dict()
    gen = R.make_params(2, 1, 16, 2 * meta["C"], 9)         # reference key names
    state = {("film_gen." + k if prefixed else k): v for k, v in gen.items()}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # the SFNO half loads non-strictly
        load_filmed_checkpoint(net, {"model_state": dict(params)}, {"model_state": state})
    for k, v in gen.items():
        assert torch.equal(net.film_gen.film_gen.state_dict()[k], v), k
    # strict: a generator checkpoint with a key too many is not merged silently
    with pytest.raises(RuntimeError):
        fw.load_state_dict({**{"film_gen." + k: v for k, v in gen.items()},
                            "film_gen.extra": torch.zeros(1)})
    trainable = {k for k, p in net.named_parameters() if p.requires_grad}
    assert trainable == {"film_gen.film_gen." + k for k in gen}


def test_fixtures_exist_and_are_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "filmgen", "filmgen_*.npz")))
    assert len(files) == 4
    hid, layers = set(), set()
    for f in files:
        assert os.path.getsize(f) <= FIXTURE_CAP, f
        z = np.load(f)
        hid.add(int(z["hidden"]))
        layers.add(int(z["film_layers"]))
        n = int(z["mask"].sum())
        assert z["mask"].shape == (12, 24) and 0 < n < 12 * 24
        deg = np.bincount(np.unique(z["coo_idx"][0].astype(np.int64) * n + z["coo_idx"][1])
                          // n, minlength=n)
        assert deg.max() >= 100 and deg[1] == 1 and deg[2] == 0
        assert 0 < float(z["err_f32"]) < 1e-6
        assert z["y32"].shape == z["y64"].shape == (2 * int(z["film_layers"]) * 256,)
    assert hid == {64, 100} and layers == {1, 2}


def test_restatement_matches_the_reference_goldens():
    """The yardstick of depth >= 1 agrees with the reference where the reference runs."""
    for f in sorted(glob.glob(os.path.join(GOLDEN, "filmgen", "filmgen_*.npz"))):
        z = np.load(f)
        n = int(z["mask"].sum())
        p = {k.replace("__", "."): torch.from_numpy(z[k]).double() for k in z.files if "__" in k}
        A = R.coo_tensor(z["coo_idx"].astype(np.int64), z["coo_val"],
                         n).coalesce().to_dense().double()
        y = R.forward(p, A, torch.from_numpy(z["mask"]), torch.from_numpy(z["sst"]).double(), 0)
        assert R.rel_err(y[0], torch.from_numpy(z["y64"])) < 1e-13
