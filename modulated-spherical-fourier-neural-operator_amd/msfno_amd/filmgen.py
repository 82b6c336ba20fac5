"""The graph-convolution FiLM generator: SST field -> (gamma, beta) of the filmed blocks.

Mirror of the reference's default generator for ``--model-version film``
(MSFNO/Models/gcn/gcn.py:96-167 ``GCN_custom``, layers.py:8-43 ``GraphConvolution``,
sfnonet.py:863-912 ``Film_wrapper``) with its constructor arguments and state-dict keys, so
that ``rollout.load_filmed_checkpoint`` merges a reference generator checkpoint strictly.
Forward and backward run in libmsfno (msfno_gcn_forward / msfno_gcn_backward,
include/msfno.h); there is no eager path.

Per sample b, with A the sparse adjacency over the N ocean cells of ``nan_mask`` (row-major
order) and leaky = LeakyReLU(0.01):

    x0      = sst[b][mask]                                  (N, Fin)
    h_1     = leaky(A (x0 W0) + b0)
    h_{l+1} = h_l + leaky(A (h_l W_l) + b_l),  l = 1..depth
    y       = mean_nodes(h_last) Wh^T + bh                  (out,)

Differences from the reference, all of them where its code does not run: the reference's
``GraphConvolution.forward`` takes ``input[0]`` and fails at depth >= 1 (the activation is
2-D after the first layer); the math here is the per-sample form its commented einsum lines
state (layers.py:37-39), for any batch and depth, returning (B, out).  At B = 1 and depth 0
it is the reference's output after ``Film_wrapper``'s reshape.  The PyG ``gcn`` variant and
the ViT / MAE generators are not mirrored.

Sizes: ``embed_dim % 4 == 0``, ``in_features <= 16``, ``depth <= 16`` and ``B * N <= 2**21``;
anything else raises NotImplementedError (at construction where the size is known then).
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as N

MAX_IN_FEATURES = 16
MAX_ROWS = 1 << 21


def build_csr(adj):
    """Host CSR of ``adj`` and of its transpose.

    ``adj``: a square torch sparse COO or CSR tensor (duplicates are summed, as ``coalesce``
    does; explicit zeros are kept).  Returns a dict of CPU tensors: ``row_ptr`` (N + 1,
    int32), ``col`` (nnz, int32, ascending within a row), ``val`` (nnz, fp32) and the same
    three for the transpose under ``t_row_ptr``, ``t_col``, ``t_val``.  Nothing is assumed
    about symmetry, normalisation or empty rows."""
    if not isinstance(adj, torch.Tensor) or adj.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise TypeError("adj must be a torch sparse COO or CSR tensor")
    if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
        raise ValueError(f"adj must be square, got {tuple(adj.shape)}")
    coo = adj.detach().cpu().to_sparse_coo().coalesce()
    n = coo.shape[0]
    if n >= 2 ** 31 or coo._nnz() >= 2 ** 31:
        raise NotImplementedError("the graph kernels index with int32")
    row = coo.indices()[0].numpy().astype(np.int64)
    col = coo.indices()[1].numpy().astype(np.int64)
    val = coo.values().to(torch.float32).numpy()

    def csr(r, c, v):
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
        return (torch.from_numpy(ptr.astype(np.int32)), torch.from_numpy(c.astype(np.int32)),
                torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))

    # coalesce sorts by (row, col); a stable sort by col then gives (col, row)
    order = np.argsort(col, kind="stable")
    out = dict(zip(("row_ptr", "col", "val"), csr(row, col, val)))
    out.update(zip(("t_row_ptr", "t_col", "t_val"), csr(col[order], row[order], val[order])))
    return out


def grid_adjacency(nan_mask, wrap=True):
    """A 4-neighbour ocean graph for users without the reference's asset file.

    Nodes are the True cells of ``nan_mask`` (H, W) in row-major order; a node is linked to
    itself and to its ocean neighbours to the north, south, east and west, the east-west
    links wrapping around in longitude when ``wrap``; every row is divided by its number of
    links (a row-normalised adjacency with self-loops).  Returned as a torch sparse COO
    (N, N) fp32 tensor.  The reference loads its adjacency from
    ``adj_coarsen_<level>_sparse.pt``, which is not in its repository: this is this
    project's construction, not the reference's."""
    mask = np.asarray(nan_mask, dtype=bool)
    if mask.ndim != 2:
        raise ValueError("nan_mask must be (H, W)")
    H, W = mask.shape
    node = np.full((H, W), -1, dtype=np.int64)
    node[mask] = np.arange(int(mask.sum()))
    ii, jj = np.nonzero(mask)
    rows, cols = [node[ii, jj]], [node[ii, jj]]
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        i2, j2 = ii + di, jj + dj
        ok = (i2 >= 0) & (i2 < H)
        if wrap:
            j2 = j2 % W
        else:
            ok &= (j2 >= 0) & (j2 < W)
        i2c, j2c = np.clip(i2, 0, H - 1), np.clip(j2, 0, W - 1)
        ok &= mask[i2c, j2c]
        rows.append(node[ii[ok], jj[ok]])
        cols.append(node[i2c[ok], j2c[ok]])
    r, c = np.concatenate(rows), np.concatenate(cols)
    n = int(mask.sum())
    # a 2- or 1-column grid reaches the same neighbour twice: one link
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    deg = np.bincount(r, minlength=n).astype(np.float64)
    v = (1.0 / deg[r]).astype(np.float32)
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, c])), torch.from_numpy(v),
                                   (n, n)).coalesce()


class GraphConvolution(nn.Module):
    """The parameters of one graph convolution (layers.py:8-43): ``weight`` (in, out),
    input-major, xavier-uniform under the leaky_relu gain at 0.01; ``bias`` zeros.  It runs
    as a layer of ``GCN_custom`` (one native call for the whole stack), not on its own."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(in_features, out_features))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight, gain=nn.init.calculate_gain("leaky_relu", 0.01))

    def forward(self, input, adj):
        raise NotImplementedError("GraphConvolution runs natively only as a layer of GCN_custom")

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.in_features} -> {self.out_features})"


_GRAPH_FIELDS = ("row_ptr", "col", "val", "t_row_ptr", "t_col", "t_val")


class GCN_custom(nn.Module):
    """gcn.py:96-167.  State-dict keys ``conv1.*``, ``conv_layers.{i}.*``, ``head_film.*``;
    the head starts as ones / zeros like the reference's.  The graph comes from ``assets``
    (the reference's ``adj_coarsen_<level>_sparse.pt`` and
    ``nan_mask_coarsen_<level>_notflatten.npy``) or from ``adj`` (torch sparse COO or CSR)
    and ``nan_mask`` (H, W) directly; its CSR and transposed CSR are built once, on the
    host, and follow the module across ``.to(device)`` as non-persistent buffers.
    ``forward(sst)``: sst (B, H, W) or (B, in_features, H, W) -> (B, out_features), any B
    (``batch_size`` is kept for signature compatibility only)."""

    def __init__(self, batch_size, device, depth, in_features=1, embed_dim=512, out_features=256,
                 coarse_level=4, assets=None, adj=None, nan_mask=None):
        super().__init__()
        if embed_dim < 4 or embed_dim % 4 != 0:
            raise NotImplementedError(f"embed_dim {embed_dim}: the graph kernels need a multiple of 4")
        if not 1 <= in_features <= MAX_IN_FEATURES:
            raise NotImplementedError(f"in_features {in_features}: 1..{MAX_IN_FEATURES} only")
        if not 0 <= depth <= N.GCN_MAX_DEPTH:
            raise NotImplementedError(f"depth {depth}: 0..{N.GCN_MAX_DEPTH} only")
        self.batch_size = batch_size
        self.device = device
        self.in_features = in_features
        self.hidden_size = embed_dim
        self.out_features = out_features
        self.perceptive_field = depth
        self.conv1 = GraphConvolution(in_features, embed_dim)
        self.conv_layers = nn.ModuleList(
            [GraphConvolution(embed_dim, embed_dim) for _ in range(depth)])
        self.activation = nn.LeakyReLU()
        self.head_film = nn.Linear(embed_dim, out_features)
        self.head_film.weight = nn.Parameter(torch.ones_like(self.head_film.weight))
        self.head_film.bias = nn.Parameter(torch.zeros_like(self.head_film.bias))
        if assets is not None:
            if adj is not None or nan_mask is not None:
                raise ValueError("give either assets or adj and nan_mask")
            adj = torch.load(os.path.join(assets, f"adj_coarsen_{coarse_level}_sparse.pt"),
                             map_location="cpu")
            nan_mask = np.load(os.path.join(assets,
                                            f"nan_mask_coarsen_{coarse_level}_notflatten.npy"))
        if adj is None or nan_mask is None:
            raise ValueError("GCN_custom needs assets, or adj and nan_mask")
        mask = np.asarray(nan_mask.cpu() if isinstance(nan_mask, torch.Tensor) else nan_mask,
                          dtype=bool)
        if mask.ndim != 2:
            raise ValueError("nan_mask must be (H, W)")
        self.nan_mask = mask
        self.num_nodes = int(mask.sum())
        if self.num_nodes < 1 or tuple(adj.shape) != (self.num_nodes, self.num_nodes):
            raise ValueError(f"adj {tuple(adj.shape)} does not match the {self.num_nodes} "
                             "True cells of nan_mask")
        for k, v in build_csr(adj).items():
            self.register_buffer("_" + k, v, persistent=False)
        self.nnz = int(self._col.numel())
        self.register_buffer("_cells", torch.from_numpy(np.flatnonzero(mask.ravel())),
                             persistent=False)
        if device is not None:
            self.to(device)

    # ---- native call -------------------------------------------------------------------
    def _params(self):
        ps = [self.conv1.weight, self.conv1.bias]
        for c in self.conv_layers:
            ps += [c.weight, c.bias]
        return ps + [self.head_film.weight, self.head_film.bias]

    def _graph(self, device):
        if self._row_ptr.device != device:
            raise ValueError(f"the graph is on {self._row_ptr.device}, sst on {device}: "
                             "move the module with .to(device)")
        g = N.GcnGraph()
        g.N, g.nnz = self.num_nodes, self.nnz
        for k in _GRAPH_FIELDS:
            setattr(g, k, getattr(self, "_" + k).data_ptr())
        return g

    @staticmethod
    def _fill(struct, tensors):
        """conv1.w, conv1.b, (w, b) per layer, head.w, head.b -> the C struct's fields."""
        struct.conv1_w, struct.conv1_b = tensors[0].data_ptr(), tensors[1].data_ptr()
        for i in range((len(tensors) - 4) // 2):
            struct.conv_w[i] = tensors[2 + 2 * i].data_ptr()
            struct.conv_b[i] = tensors[3 + 2 * i].data_ptr()
        struct.head_w, struct.head_b = tensors[-2].data_ptr(), tensors[-1].data_ptr()
        return struct

    def _desc(self, keep):
        d = N.GcnDesc()
        d.Fin, d.hidden = self.in_features, self.hidden_size
        d.depth, d.out = self.perceptive_field, self.out_features
        return self._fill(d, [N.f32(p, keep) for p in self._params()])

    def _nodes(self, sst):
        """sst (B, H, W) or (B, Fin, H, W) -> x0 (B, N, Fin) fp32 contiguous."""
        H, W = self.nan_mask.shape
        if sst.dim() == 3:
            sst = sst[:, None]
        if sst.dim() != 4 or tuple(sst.shape[1:]) != (self.in_features, H, W):
            raise ValueError(f"sst {tuple(sst.shape)}: expected (B, {H}, {W}) or "
                             f"(B, {self.in_features}, {H}, {W})")
        B = sst.shape[0]
        if B * self.num_nodes > MAX_ROWS:
            raise NotImplementedError(f"B * N = {B * self.num_nodes} > {MAX_ROWS}")
        x = N.require_device_f32(sst.detach(), "sst").reshape(B, self.in_features, H * W)
        return x.index_select(2, self._cells).transpose(1, 2).contiguous()

    @N.on_input_device
    def workspace_size(self, B, train=False):
        return N.lib().msfno_gcn_workspace_size(B, self.num_nodes, self.in_features,
                                                self.hidden_size, self.perceptive_field,
                                                self.out_features, int(train))

    @N.on_input_device
    def native_forward(self, sst, train=False, ws=None):
        """(y, saved): y (B, out) fp32; ``saved`` is what native_backward needs (the
        workspace holding every layer's input and pre-activation), None without train.
        ``ws``: the caller's workspace (uint8, at least ``workspace_size(B, train)``), else
        one is allocated."""
        x0 = self._nodes(sst)
        B, dev = x0.shape[0], x0.device
        keep = []
        g, d = self._graph(dev), self._desc(keep)
        if ws is None:
            ws = torch.empty(self.workspace_size(B, train), dtype=torch.uint8, device=dev)
        elif ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous():
            raise ValueError(f"ws must be contiguous uint8 on {dev}")
        nbytes = ws.numel()
        y = torch.empty(B, d.out, dtype=torch.float32, device=dev)
        N.check(N.lib().msfno_gcn_forward(g, d, x0.data_ptr(), y.data_ptr(), B, int(train),
                                          ws.data_ptr(), nbytes, N.stream_of(dev)),
                "GCN_custom.forward")
        return y, (ws if train else None)

    @N.on_input_device
    def native_backward(self, dy, saved, sst_shape=None):
        """Gradients of every parameter (in ``_params`` order) and, with ``sst_shape``, of
        sst: scattered to the mask's cells, zeros on land."""
        dy = N.require_device_f32(dy, "dy")
        B, dev = dy.shape[0], dy.device
        keep = []
        g, d = self._graph(dev), self._desc(keep)
        grads = [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in self._params()]
        gr = self._fill(N.GcnGrads(), grads)
        dx0 = (torch.empty(B, g.N, d.Fin, dtype=torch.float32, device=dev)
               if sst_shape is not None else None)
        N.check(N.lib().msfno_gcn_backward(g, d, dy.data_ptr(), gr, N.ptr(dx0), B,
                                           saved.data_ptr(), saved.numel(), N.stream_of(dev)),
                "GCN_custom.backward")
        dsst = None
        if dx0 is not None:
            H, W = self.nan_mask.shape
            dsst = torch.zeros(B, d.Fin, H * W, dtype=torch.float32, device=dev)
            dsst.index_copy_(2, self._cells, dx0.transpose(1, 2).contiguous())
            dsst = dsst.reshape(sst_shape)
        return grads, dsst

    def forward(self, sst):
        if torch.is_grad_enabled():
            params = self._params()
            if sst.requires_grad or any(p.requires_grad for p in params):
                return _GCNFn.apply(sst, self, *params)
        return self.native_forward(sst)[0].to(sst.dtype if sst.is_floating_point()
                                              else torch.float32)


class _GCNFn(torch.autograd.Function):
    """Native generator forward; backward to sst and to every parameter (they ride along as
    trailing inputs, as in ``_MLPFn``)."""

    @staticmethod
    def forward(ctx, sst, gcn, *params):
        ctx.gcn, ctx.sst_shape, ctx.sst_dtype = gcn, sst.shape, sst.dtype
        y, saved = gcn.native_forward(sst, train=True)
        ctx.save_for_backward(saved, *params)  # the parameters: autograd checks their versions
        return y.to(sst.dtype)

    @staticmethod
    def backward(ctx, dy):
        saved, *params = ctx.saved_tensors
        need_sst = ctx.needs_input_grad[0]
        grads, dsst = ctx.gcn.native_backward(dy, saved, ctx.sst_shape if need_sst else None)
        if dsst is not None:
            dsst = dsst.to(ctx.sst_dtype)
        out = tuple(g.to(p.dtype) if ctx.needs_input_grad[2 + i] else None
                    for i, (g, p) in enumerate(zip(grads, params)))
        return (dsst, None) + out


class Film_wrapper(nn.Module):
    """sfnonet.py:863-912 for the default generator: child ``film_gen`` is a ``GCN_custom``
    with ``2 * cfg.film_layers * num_film_features`` outputs (so a filmed network's keys are
    ``film_gen.film_gen.conv1.weight`` ...), and forward reshapes its output to
    (B, 2, cfg.film_layers, num_film_features).  ``cfg``: batch_size, model_depth,
    embed_dim, film_layers, film_gen_type, and ``assets`` (the directory holding ``gcn/``)
    unless ``adj`` and ``nan_mask`` are given.  The reference's other generator types raise
    NotImplementedError."""

    def __init__(self, device, cfg, num_film_features=256, adj=None, nan_mask=None):
        super().__init__()
        self.device, self.cfg = device, cfg
        self.num_film_features = num_film_features
        kind = getattr(cfg, "film_gen_type", None)
        if kind in ("gcn", "transformer", "mae"):
            raise NotImplementedError(
                f"film_gen_type {kind!r} is not implemented: only the default graph generator "
                "(GCN_custom) is")
        assets = None if adj is not None else os.path.join(cfg.assets, "gcn")
        self.film_gen = GCN_custom(cfg.batch_size, device, depth=cfg.model_depth,
                                   embed_dim=cfg.embed_dim,
                                   out_features=num_film_features * cfg.film_layers * 2,
                                   assets=assets, adj=adj, nan_mask=nan_mask)

    def get_parameters(self):
        return self.film_gen.parameters()

    def forward(self, sst):
        x = self.film_gen(sst)
        return x.reshape(sst.shape[0], 2, self.cfg.film_layers, self.num_film_features)
