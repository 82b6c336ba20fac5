"""The spectral MLP of the non-linear filter (csrc/gemm_x6c.hip, run_filter of
csrc/block_fwd.cpp) over depth, hidden width, ragged channels, column tiles and batch: the
cases of spectral_mlp_cases.py, whose docstring names the thresholds each one crosses.

Every case runs SpectralAttentionS2 on the native transforms (msfno_filter_forward: forward
transform, the chain, inverse transform, no norms) and is compared with
oracle.sfno_ref.spectral_attention_s2 in fp64:

  * default switches (the x3h 3M chain, the x6 3M chain where the range test of run_filter
    sends a deep chain, and the 4M chain where C > Hs): the bar of
    test_gpu_ring_refill.py, |got - want64|max < max(2 e32, 1e-6 max(1, |want64|max)) with
    e32 the error of the same oracle in fp32; three runs in one process are bit-equal (a
    stand-alone filter attaches no weight cache, so each run builds its images anew: the
    reuse of cached images is test_abi_exact_weight_cache's);
  * the A/B engines (ENGINES), one child process per setting, since the switches are read
    once per process: the bar of test_gpu_variants.py, 1e-4 max(1, |want64|max);
  * through the C ABI: refusals of 0 and 9 layers, exact workspaces and weight caches
    behind a guard (the protocol of test_gpu_workspace_guard.py).

test_spectral_mlp_cases_host.py shows on the CPU that the first bar fails for a dropped
k-tail, row tail or column tile, a skipped layer, a stale ping-pong buffer and a ReLU on
the imaginary part.

The case C16-f2-L8 is the regression test of the range test: on the x3h chain, which every
3M chain took before, its error was 7.2e-2 on outputs of 37 (6839 x the fp32 oracle's)."""
import functools
import json
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

import spectral_mlp_cases as M  # noqa: E402
from test_gpu_ring_refill import _bar, _thrice  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _filter(c, layers=None):
    """SpectralAttentionS2 of case `c` on the native transforms, the case's weights loaded."""
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno.sfnonet import SpectralFilterLayer
    sht = RealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    isht = InverseRealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    sht.weights = sht.weights * 1e5      # as oracle.sfno_ref.make_transforms
    isht.pct = isht.pct / 1e5
    f = SpectralFilterLayer(sht, isht, c.C, filter_type="non-linear", hidden_size_factor=c.factor,
                            spectral_layers=c.layers if layers is None else layers).filter
    if layers is None:
        ws, wout = M.weights(c)
        assert f.hidden_size == M.hidden(c) and len(f.w) == len(ws)
        with torch.no_grad():
            for p, w in zip(f.w, ws):
                p.copy_(w)
            f.wout.copy_(wout)
    return f.eval().to(DEV), (sht, isht)


def _run(c):
    """(output, three runs bit-equal) of case `c` under this process's switches."""
    f, keep = _filter(c)
    x = M.input_of(c).to(DEV)
    with torch.no_grad():
        got, same = _thrice(lambda: f(x).cpu())
    del keep
    return got, same


@functools.lru_cache(maxsize=None)
def _default(c):
    return _run(c)


# ---- a. forward, every case, default switches -----------------------------------------------

@pytest.mark.parametrize("case", M.CASES, ids=M.IDS)
def test_forward_matches_fp64_oracle(case):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    got, same = _default(case)
    assert got.shape == M.want64(case).shape and torch.isfinite(got).all()
    assert same, f"{M.case_id(case)}: three runs on the same input differ"
    _bar(got, M.want64(case), M.want32(case), f"{M.case_id(case)} [{M.chain_of(case.C, M.hidden(case))} "
         f"{M.engine_of(case.C, M.hidden(case), case.layers)}]")


def test_512_tile_boundary_batch_prefix():
    """B 127 takes the 64-row kernels in every layer (508 tiles), B 128 the 128-row ones
    (512): the first 127 fields of the latter against the former, at the bar of the former
    (its e32 and |y|max)."""
    lo, hi = M.BOUNDARY
    got_lo, got_hi = _default(lo)[0], _default(hi)[0]
    diff = got_hi[:lo.B].double() - got_lo.double()
    _bar(M.want64(lo) + diff, M.want64(lo), M.want32(lo), "B 128 [:127] vs B 127")


# ---- b. refusals ---------------------------------------------------------------------------

def _abi(c, f):
    """(lib, desc, forward plan, inverse plan, x on the device, keep-alive) of filter `f`."""
    from msfno_amd import _native as N
    x = M.input_of(c).to(DEV).contiguous()
    fwd, inv = f._transforms()
    pf, pi = fwd._plan(x.device), inv._plan(x.device)
    d, keep = f.native_desc(c.C)
    return N.lib(), d, pf, pi, x, (keep, fwd, inv)


def _forward_call(L, d, pf, pi, x, y, B):
    from msfno_amd import _native as N

    def call(ws, ws_bytes):
        return L.msfno_filter_forward(d, pf.handle, pi.handle, x.data_ptr(), y.data_ptr(), B, ws,
                                      ws_bytes, N.stream_of(x.device))
    return call


@pytest.mark.parametrize("layers", [0, M.MAX_LAYERS + 1])
def test_abi_refuses_layer_counts_outside_1_to_8(layers):
    from msfno_amd import _native as N
    c = M.DEPTH[1]
    f, keep_t = _filter(c)
    L, d, pf, pi, x, keep = _abi(c, f)
    nbytes = L.msfno_block_workspace_size(d, pf.handle, pi.handle, c.B)
    bad = N.BlockDesc.from_buffer_copy(d)
    bad.spectral_layers = layers
    y = torch.full(x.shape, NAN, dtype=torch.float32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert _forward_call(L, bad, pf, pi, x, y, c.B)(ws.data_ptr(), nbytes) == N.MSFNO_EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a refused call wrote its output"
    # the descriptor it was copied from is served
    assert _forward_call(L, d, pf, pi, x, y, c.B)(ws.data_ptr(), nbytes) == N.MSFNO_OK
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    del keep, keep_t


def test_python_refuses_nine_layers():
    c = M.DEPTH[1]
    f, keep = _filter(c, layers=M.MAX_LAYERS + 1)
    with pytest.raises(NotImplementedError):
        f(M.input_of(c).to(DEV))
    del keep


# ---- c. workspace and weight cache -----------------------------------------------------------

@pytest.mark.parametrize("case", M.WORKSPACE_CASES, ids=[M.case_id(c) for c in M.WORKSPACE_CASES])
def test_abi_exact_workspace(case):
    from test_gpu_workspace_guard import _run_guarded
    c = case
    f, keep_t = _filter(c)
    L, d, pf, pi, x, keep = _abi(c, f)
    outs = {"y": torch.full(x.shape, NAN, dtype=torch.float32, device=DEV)}
    nbytes = L.msfno_block_workspace_size(d, pf.handle, pi.handle, c.B)
    got = _run_guarded(nbytes, outs, _forward_call(L, d, pf, pi, x, outs["y"], c.B))["y"].cpu()
    _bar(got, M.want64(c), M.want32(c), f"{M.case_id(c)} exact workspace")
    del keep, keep_t


@pytest.mark.parametrize("case", [M.DEEPEST, M.LAST_X3H], ids=["nine_images_x6c", "five_images_x3h"])
def test_abi_exact_weight_cache(case):
    """The weight images (eight layers: all nine slots; the deepest x3h chain: five, and the
    x3h layer scales behind the first) in a cache of exactly msfno_block_wcache_size bytes:
    filled by a call with wcache_valid 0, reused by one with wcache_valid 1, the two outputs
    bit-equal, the guard behind the cache untouched."""
    from msfno_amd import _native as N
    from test_gpu_workspace_guard import _run_guarded
    from workspace_guard import guard_intact, guarded
    c = case
    assert M.engine_of(c.C, M.hidden(c), c.layers) == ("x6c" if c is M.DEEPEST else "x3h")
    f, keep_t = _filter(c)
    L, d, pf, pi, x, keep = _abi(c, f)
    plain = L.msfno_block_workspace_size(d, pf.handle, pi.handle, c.B)
    wbytes = L.msfno_block_wcache_size(d)
    assert wbytes > 0
    wc = guarded(wbytes, 0xFF, DEV)
    d.wcache, d.wcache_valid = wc.data_ptr(), 0
    nbytes = L.msfno_block_workspace_size(d, pf.handle, pi.handle, c.B)
    assert nbytes < plain                # the images left the workspace
    outs = {"y": torch.full(x.shape, NAN, dtype=torch.float32, device=DEV)}
    call = _forward_call(L, d, pf, pi, x, outs["y"], c.B)
    built = _run_guarded(nbytes, outs, call)["y"]
    guard_intact(wc, wbytes)
    d.wcache_valid = 1
    ws = guarded(nbytes, 0xFF, DEV)
    outs["y"].fill_(NAN)
    assert call(ws.data_ptr(), nbytes) == N.MSFNO_OK, L.msfno_last_error()
    guard_intact(ws, nbytes)
    guard_intact(wc, wbytes)
    assert torch.equal(outs["y"], built), "the cached images give another result"
    _bar(built.cpu(), M.want64(c), M.want32(c), f"{M.case_id(c)} exact weight cache")
    del keep, keep_t


# ---- d. the other engines ---------------------------------------------------------------------

ENGINE_IDS = [M.case_id(c) for c in M.ENGINE_CASES]


def _env_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@functools.lru_cache(maxsize=None)
def _engine_child(env_id):
    """The engine cases in one child process under the switch: {id: (output, repeatable)}"""
    import tempfile
    env = {k: v for k, v in os.environ.items()
           if k not in {k2 for e in M.ENGINES for k2 in e}}
    env.update(next(e for e in M.ENGINES if _env_id(e) == env_id))
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "engine.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=HERE,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        same = json.loads(str(z["same"]))
        return {i: (torch.from_numpy(z[i]), same[i]) for i in ENGINE_IDS}


@pytest.mark.parametrize("env", M.ENGINES, ids=_env_id)
def test_engine_matches_fp64_oracle(env):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    res = _engine_child(_env_id(env))
    bad = {}
    for cid, c in zip(ENGINE_IDS, M.ENGINE_CASES):
        got, same = res[cid]
        want = M.want64(c)
        e = (got.double() - want).abs().max().item()
        e32 = (M.want32(c) - want).abs().max().item()
        ymax = max(1.0, want.abs().max().item())
        print(f"{_env_id(env)} {cid}: max-abs vs fp64 {e:.3e}  cpu-fp32 {e32:.3e}  "
              f"ratio {e / e32:.2f}  (|y|max {ymax:.3f})")
        if not (same and e < 1e-4 * ymax):
            bad[cid] = (e, same)
    assert not bad, bad


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import conftest  # noqa: F401  (puts the package on sys.path)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    res = {i: _run(c) for i, c in zip(ENGINE_IDS, M.ENGINE_CASES)}
    np.savez(sys.argv[1], same=json.dumps({i: s for i, (_, s) in res.items()}),
             **{i: y.numpy() for i, (y, _) in res.items()})
