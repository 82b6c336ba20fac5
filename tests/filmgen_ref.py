"""Restatement of the graph FiLM generator's math in plain torch with a dense adjacency,
written from the formulas (not from any implementation), for any dtype:

    x0      = sst[b][mask]                                   (N, Fin), row-major mask order
    h_1     = leaky(A (x0 W0) + b0)
    h_{l+1} = h_l + leaky(A (h_l W_l) + b_l),  l = 1..depth
    y       = mean_nodes(h_last) Wh^T + bh

and the shared fixtures of the filmgen tests: masks, the unsymmetric adjacency with a hub
row, a self-loop-only row and an empty row, parameters, and the error measure."""
import numpy as np
import torch

SLOPE = 0.01
PARAM_FACTOR = 8  # err_native <= 8 err_f32: 4 (x3h operands to 2^-22 vs 2^-24) x 2 (order)


def param_names(depth):
    names = ["conv1.weight", "conv1.bias"]
    for i in range(depth):
        names += [f"conv_layers.{i}.weight", f"conv_layers.{i}.bias"]
    return names + ["head_film.weight", "head_film.bias"]


class WrongAdjoint(torch.autograd.Function):
    """A @ S whose backward multiplies by A where A^T belongs: the mistake the transpose
    test must be able to see."""

    @staticmethod
    def forward(ctx, A, S):
        ctx.save_for_backward(A)
        return A @ S

    @staticmethod
    def backward(ctx, g):
        (A,) = ctx.saved_tensors
        return None, A @ g


def forward(params, A, mask, sst, depth, wrong_adjoint=False):
    """params: dict by state-dict key; A dense (N, N); mask (H, W) bool tensor;
    sst (B, H, W) or (B, Fin, H, W).  Returns y (B, out)."""
    if wrong_adjoint:
        dense = A

        class _A:
            def __matmul__(self, S):
                return WrongAdjoint.apply(dense, S)
        A = _A()
    if sst.dim() == 3:
        sst = sst[:, None]
    B, Fin = sst.shape[:2]
    x = sst.reshape(B, Fin, -1)[:, :, mask.reshape(-1)].transpose(1, 2)  # (B, N, Fin)
    leaky = torch.nn.functional.leaky_relu
    h = leaky(A @ (x @ params["conv1.weight"]) + params["conv1.bias"], SLOPE)
    for i in range(depth):
        w, b = params[f"conv_layers.{i}.weight"], params[f"conv_layers.{i}.bias"]
        h = h + leaky(A @ (h @ w) + b, SLOPE)
    return h.mean(dim=-2) @ params["head_film.weight"].T + params["head_film.bias"]


def grads(params, A, mask, sst, depth, dy, wrong_adjoint=False):
    """(y, {name: dL/dparam}, dL/dsst) for L = sum(y * dy), by autograd in the tensors' dtype."""
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    s = sst.detach().clone().requires_grad_(True)
    y = forward(ps, A, mask, s, depth, wrong_adjoint)
    (y * dy).sum().backward()
    return y.detach(), {k: v.grad for k, v in ps.items()}, s.grad


def rel_err(a, ref):
    """max |a - ref| / max |ref| (the measure of the fixtures' err_f32)."""
    ref = ref.double()
    return float((a.double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-300))


def make_mask(H, W, seed):
    """(H, W) bool: ocean with rectangular land holes, about two thirds ocean."""
    rng = np.random.default_rng(seed)
    mask = np.ones((H, W), dtype=bool)
    while mask.mean() > 0.68:
        h, w = rng.integers(1, max(2, H // 3)), rng.integers(1, max(2, W // 3))
        i, j = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
        mask[i:i + h, j:j + w] = False
    return mask


def make_adjacency(n, seed, empty_row=True, hub_degree=None):
    """Unsymmetric, unnormalised COO (indices (2, nnz) int64, values fp32) over n nodes:
    self-loops and a few random out-links per row, row 0 a hub linked to min(n, 128) or
    ``hub_degree`` nodes, row 1 only its self-loop, row 2 empty (if asked), some duplicate
    entries (summed by coalesce)."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(n):
        k = int(rng.integers(1, 6))
        c = rng.choice(n, size=min(k, n), replace=False)
        rows += [r] * (len(c) + 1)
        cols += [r] + list(c)
    rows, cols = np.array(rows), np.array(cols)
    keep = (rows != 0) & (rows != 1) & ~((rows == 2) & empty_row)
    rows, cols = rows[keep], cols[keep]
    hub = rng.choice(n, size=min(n, hub_degree or 128), replace=False)
    rows = np.concatenate([rows, np.zeros(len(hub), dtype=np.int64), [1]])
    cols = np.concatenate([cols, hub, [1]])
    dup = rng.choice(len(rows), size=max(1, len(rows) // 20), replace=False)
    dup = dup[(rows[dup] != 1)]
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    vals = rng.uniform(-0.5, 1.0, size=len(rows)).astype(np.float32)
    vals[rows == 0] *= 4.0 / len(hub)  # the hub row sums to O(1)
    return np.stack([rows, cols]).astype(np.int64), vals


def coo_tensor(idx, vals, n):
    return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), (n, n))


def make_params(depth, fin, hidden, out, seed):
    """Random parameters under the module's state-dict keys (fp32): conv weights at the
    xavier scale, biases and the head random so that no column repeats."""
    g = torch.Generator().manual_seed(seed)
    p = {"conv1.weight": torch.randn(fin, hidden, generator=g) * (2.0 / (fin + hidden)) ** 0.5,
         "conv1.bias": 0.1 * torch.randn(hidden, generator=g)}
    for i in range(depth):
        p[f"conv_layers.{i}.weight"] = torch.randn(hidden, hidden, generator=g) * (1.0 / hidden) ** 0.5
        p[f"conv_layers.{i}.bias"] = 0.1 * torch.randn(hidden, generator=g)
    p["head_film.weight"] = torch.randn(out, hidden, generator=g) * (1.0 / hidden) ** 0.5
    p["head_film.bias"] = 0.1 * torch.randn(out, generator=g)
    return p
