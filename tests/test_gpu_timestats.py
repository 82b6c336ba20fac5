"""Statistics over time on the device (msfno_amd/timestats.py, csrc/timestats.hip) against
the restatements of tests/timestats_util.py.

Shapes (B, S, H, W), each for what it exercises: (1,1,1,1) and (1,1,1,3), P below one
vector; (2,3,5,7), P = 35, every slab on another 16-byte phase; (3,2,4,8), everything
aligned; (1,2,3,2731), P = 8193, a block boundary and a one-element tail.  1 and 3 updates
(calls of B elements) everywhere, 64 on (2,3,5,7) only.

Accuracy is held to the rounding bounds of the recurrence stated in timestats_util (per pixel,
N valid updates, A = max |a|: mean N eps A, m2 / N  eps (8 A sigma + N sigma^2), c_pt likewise);
everything that can be bitwise is: counts, lo / hi, order, phase, stride, skipped updates,
graph replay, the drivers against a hand-written loop."""
import datetime as dt

import numpy as np
import pytest
import torch

import timestats_util as TU
import verify_util as VU

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x5A5A5A5A
CONFIGS = ("field", "field-clim-minmax", "error", "error-clim")


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _dev(x):
    return x.to(DEV)


def _new(cfg, shape):
    from msfno_amd import timestats as T
    _, S, H, W = shape
    if cfg.startswith("field"):
        return T.FieldStats(S, H, W, minmax=cfg.endswith("minmax"), device=DEV)
    return T.ErrorMaps(S, H, W, anomalies=cfg.endswith("clim"), device=DEV)


def _feed(st, cfg, p, t, c, skip=False):
    """One update of (B, S, H, W) device fields; the climatology one slab per (b, s)."""
    if cfg == "field":
        st.update(t, skip_nan=skip)
    elif cfg == "field-clim-minmax":
        st.update(t, clim=c, skip_nan=skip)
    elif cfg == "error":
        st.update(p, t, skip_nan=skip)
    else:
        st.update(p, t, clim=c, skip_nan=skip)


def _run(cfg, shape, P, T, C, skip=False, singles=False, omit=()):
    """The state after the updates P, T, C (updates, B, S, H, W), as calls of B elements or,
    with ``singles``, one call per element, leaving out the flat update indices ``omit``."""
    st = _new(cfg, shape)
    P, T, C = _dev(P), _dev(T), _dev(C)
    B = shape[0]
    for u in range(P.shape[0]):
        if not singles:
            assert not omit
            _feed(st, cfg, P[u], T[u], C[u], skip)
            continue
        for b in range(B):
            if u * B + b not in omit:
                _feed(st, cfg, P[u, b:b + 1], T[u, b:b + 1], C[u, b:b + 1], skip)
    return st


def _state(st):
    torch.cuda.synchronize()
    return st._count.cpu().clone(), st._planes.cpu().contiguous().clone()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_same(a, b, what, where=None):
    """States (count, planes) bitwise equal, on the pixels ``where`` (S, H, W) if given."""
    ca, pa, cb, pb = a[0], _bits(a[1]), b[0], _bits(b[1])
    if where is not None:
        ca, cb, pa, pb = ca[where], cb[where], pa[:, where], pb[:, where]
    assert torch.equal(ca, cb), f"{what}: counts differ"
    assert torch.equal(pa, pb), f"{what}: planes differ"


def _check_accuracy(cfg, state, p, t, c, valid, what):
    """The state against fp64 over the flat updates p, t, c (N, S, H, W) fp32 on the host."""
    count, pl = state
    p64, t64, c64 = p.double(), t.double(), c.double()
    if cfg.startswith("field"):
        a32, a64 = (t, t64) if cfg == "field" else (t - c, t64 - c64)
        TU.check_moments(count, pl[0], pl[1], a64, valid, what)
        if cfg.endswith("minmax"):
            inf = torch.tensor(float("inf"))
            v = torch.ones_like(a32, dtype=torch.bool) if valid is None else valid
            lo = torch.where(v, a32, inf).min(0).values
            hi = torch.where(v, a32, -inf).max(0).values
            assert torch.equal(_bits(pl[2]), _bits(lo)) and torch.equal(_bits(pl[3]), _bits(hi))
        return
    d = p64 - t64
    TU.check_moments(count, pl[0], pl[1], d, valid, f"{what} d")
    n, mabs, _ = TU.moments64(d.abs(), valid)
    has = n > 0
    TU.assert_within(torch.where(has, pl[2].double(), torch.full_like(mabs, float("nan"))), mabs,
                     TU.mean_bound(n, TU.amax(d, valid)), f"{what} mean_abs")
    if cfg.endswith("clim"):
        TU.check_moments(count, pl[3], pl[4], p64 - c64, valid, f"{what} pa")
        TU.check_moments(count, pl[5], pl[6], t64 - c64, valid, f"{what} ta")
        TU.check_cov(pl[7], p64 - c64, t64 - c64, valid, what)


# ---- 1. accuracy ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", TU.FAMILIES)
@pytest.mark.parametrize("shape,updates", TU.CASES, ids=_ids)
def test_accuracy_against_fp64(shape, updates, family):
    P, T, C = TU.problem(shape, updates, family)
    for cfg in CONFIGS:
        st = _run(cfg, shape, P, T, C)
        _check_accuracy(cfg, _state(st), TU.flat(P), TU.flat(T), TU.flat(C), None, cfg)


def test_accessors_follow_the_formulas():
    shape = (2, 3, 5, 7)
    P, T, C = TU.problem(shape, 3, "300")
    fs = _run("field-clim-minmax", shape, P, T, C)
    cnt, pl = _state(fs)
    n = cnt.float()

    def close(a, b):       # plain torch on the planes: a few roundings of the device's ops
        return torch.allclose(a.cpu(), b, rtol=1e-6, atol=0)

    assert torch.equal(fs.count.cpu(), cnt.long()) and (cnt == 6).all()
    assert torch.equal(fs.mean.cpu(), pl[0]) and close(fs.var(), pl[1] / n)
    assert close(fs.var(ddof=1), pl[1] / (n - 1)) and close(fs.std, (pl[1] / n).sqrt())
    assert torch.equal(fs.min.cpu(), pl[2]) and torch.equal(fs.max.cpu(), pl[3])
    em = _run("error-clim", shape, P, T, C)
    cnt, pl = _state(em)
    assert torch.equal(em.bias.cpu(), pl[0]) and torch.equal(em.mae.cpu(), pl[2])
    assert close(em.mse, pl[1] / n + pl[0] ** 2)
    assert close(em.rmse, (pl[1] / n + pl[0] ** 2).sqrt())
    assert close(em.error_std, (pl[1] / n).sqrt())
    pear = pl[7] / (pl[4].sqrt() * pl[6].sqrt())
    assert close(em.acc(centred=True), pear)
    assert ((em.acc(centred=True).cpu().abs() <= 1 + 1e-5)).all()
    fresh = _new("error-clim", shape)
    assert torch.isnan(fresh.bias).all() and torch.isnan(fresh.acc()).all()


# ---- 2. order and determinism --------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 2, 4, 8)], ids=_ids)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_order_and_determinism_bitwise(cfg, shape):
    P, T, C = TU.problem(shape, 3, "scales")
    ref = _state(_run(cfg, shape, P, T, C))
    _assert_same(_state(_run(cfg, shape, P, T, C)), ref, "two runs")
    _assert_same(_state(_run(cfg, shape, P, T, C, singles=True)), ref,
                 "B one-element calls against one call of B")
    if "clim" not in cfg:
        return
    # the climatology stack in reversed slab order, the map remapped to match
    B, S, H, W = shape
    st = _new(cfg, shape)
    back = list(range(B * S - 1, -1, -1))
    for u in range(3):
        stack = _dev(C[u].reshape(B * S, H, W).flip(0).contiguous())
        args = (_dev(T[u]),) if cfg.startswith("field") else (_dev(P[u]), _dev(T[u]))
        # a host map on even updates, a device map on odd ones
        slab = back if u % 2 == 0 else torch.tensor(back, dtype=torch.int32, device=DEV)
        st.update(*args, clim=stack, clim_slab=slab)
    _assert_same(_state(st), ref, "reversed climatology stack")


# ---- 3. phase and stride -------------------------------------------------------------------
def _poisoned(n, dtype=torch.float32):
    return torch.full((n,), POISON, dtype=torch.int32, device=DEV).view(dtype)


def _place(chunks, off, stride, pad=9, dtype=torch.float32):
    """``chunks`` (a list of flat host tensors of one length) at ``off + i * stride`` of a
    poisoned buffer with ``pad`` words behind; returns (buffer, the view at ``off``)."""
    n = chunks[0].numel()
    buf = _poisoned(off + (len(chunks) - 1) * stride + n + pad, dtype)
    for i, ch in enumerate(chunks):
        buf[off + i * stride: off + i * stride + n] = _dev(ch.reshape(-1).to(dtype))
    return buf, buf[off:]


def _untouched(buf, off, nchunks, stride, n):
    """Every word of ``buf`` outside the chunks still holds the poison."""
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for i in range(nchunks):
        keep[off + i * stride: off + i * stride + n] = False
    words = buf.view(torch.int32).cpu()
    return bool((words[keep] == POISON).all())


def _raw_update(kind, flags, in0, in1, bs0, bs1, clim, slab, B, S, P, skip, count, state, ps):
    from msfno_amd import _native as N
    return N.lib().msfno_tstats_update(
        kind, flags, N.ptr(in0), N.ptr(in1), bs0, bs1, N.ptr(clim), N.ptr(slab), B, S, P, skip,
        N.ptr(count), N.ptr(state), ps, torch.cuda.current_stream().cuda_stream)


PHASES = [((1, 1, 1, 1, 1), 0, 0), ((2, 2, 2, 2, 2), 0, 0), ((3, 3, 3, 3, 3), 0, 0),
          ((1, 2, 3, 2, 3), 0, 0), ((3, 0, 1, 1, 2), 0, 0),
          ((0, 0, 0, 0, 0), 1, 0),      # a batch stride of S P + 1
          ((0, 0, 0, 0, 0), 0, 3),      # a plane stride of S P + 3
          ((2, 1, 0, 3, 1), 1, 3)]


@pytest.mark.parametrize("offs,dbs,dps", PHASES, ids=_ids)
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 2, 4, 8), (1, 2, 3, 2731)], ids=_ids)
@pytest.mark.parametrize("cfg", ["field-clim-minmax", "error-clim"])
def test_phase_and_stride_bitwise(cfg, shape, offs, dbs, dps):
    """Inputs, state and count as views at element offsets (in0, in1, clim, state, count) into
    poisoned buffers, batch stride S P + dbs, plane stride S P + dps: the bits of the aligned
    run, and not a word written outside the state."""
    from msfno_amd import timestats as TS
    B, S, H, W = shape
    Pn = H * W
    SP = S * Pn
    P, T, C = TU.problem(shape, 3, "300")
    ref = _state(_run(cfg, shape, P, T, C))
    field = cfg.startswith("field")
    kind, flags = (TS.FIELD, TS.MINMAX) if field else (TS.ERROR, TS.ANOM)
    K = ref[1].shape[0]
    o0, o1, oc, os_, on = offs
    fresh = [torch.zeros(SP) for _ in range(K)]
    if field:
        fresh[2].fill_(float("inf"))
        fresh[3].fill_(float("-inf"))
    sbuf, state = _place(fresh, os_, SP + dps)
    cbuf, count = _place([torch.zeros(SP, dtype=torch.int32)], on, 0, dtype=torch.int32)
    slab = torch.arange(B * S, dtype=torch.int32, device=DEV)
    guards = []
    for u in range(3):
        a0 = T[u] if field else P[u]
        b0, in0 = _place(list(a0.reshape(B, SP)), o0, SP + dbs)
        b1, in1 = (None, None) if field else _place(list(T[u].reshape(B, SP)), o1, SP + dbs)
        bc, clim = _place([C[u].reshape(-1)], oc, 0)
        rc = _raw_update(kind, flags, in0, in1, SP + dbs, SP + dbs, clim, slab, B, S, Pn, 0,
                         count, state, SP + dps)
        assert rc == 0
        guards.append((b0, o0, B, SP + dbs, SP))
        if b1 is not None:
            guards.append((b1, o1, B, SP + dbs, SP))
        guards.append((bc, oc, 1, 0, B * SP))
    torch.cuda.synchronize()
    got_planes = torch.stack([state[k * (SP + dps): k * (SP + dps) + SP].cpu() for k in range(K)])
    got = (count[:SP].cpu().reshape(S, H, W), got_planes.reshape(K, S, H, W))
    _assert_same(got, ref, f"offsets {offs}, batch stride +{dbs}, plane stride +{dps}")
    assert _untouched(sbuf, os_, K, SP + dps, SP), "a word outside the planes was written"
    assert _untouched(cbuf, on, 1, 0, SP), "a word outside the count was written"
    for g in guards:
        assert _untouched(*g), "an input buffer was written"


# ---- 4. missing values ---------------------------------------------------------------------
def _subset(shape, seed=9):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape[1:], generator=g) < 0.25
    m.view(-1)[0] = True
    m.view(-1)[-1] = True
    return m


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 3, 2731)], ids=_ids)
@pytest.mark.parametrize("cfg,which", [("error-clim", "t"), ("error-clim", "c"), ("error", "t"),
                                       ("field-clim-minmax", "t"), ("field-clim-minmax", "c"),
                                       ("field", "t")])
def test_skipped_updates_leave_the_bits_of_a_run_without_them(cfg, which, shape):
    """Update k has NaN in the truth (the field itself for FIELD) or in the climatology on a
    scattered subset.  With skip_nan the subset has bitwise the state of a run that never saw
    update k, the other pixels that of the run without NaNs, and the counts differ by one;
    without skip_nan exactly those pixels are NaN."""
    B = shape[0]
    P, T, C = TU.problem(shape, 3, "300")
    k = 1 * B + (B - 1)                          # the last element of the second call
    sub = _subset(shape)
    T2, C2 = T.clone(), C.clone()
    (T2 if which == "t" else C2)[1, B - 1][sub] = float("nan")
    clean = _state(_run(cfg, shape, P, T, C))
    without = _state(_run(cfg, shape, P, T, C, singles=True, omit=(k,)))
    got = _state(_run(cfg, shape, P, T2, C2, skip=True))
    _assert_same(got, without, "skipped pixels", where=sub)
    _assert_same(got, clean, "other pixels", where=~sub)
    assert torch.equal(clean[0] - got[0], sub.to(torch.int32))
    # and against fp64 over the valid updates
    valid = torch.ones(TU.flat(T).shape, dtype=torch.bool)
    valid[k] = ~sub
    _check_accuracy(cfg, got, TU.flat(P), TU.flat(T), TU.flat(C), valid, f"{cfg} skip")
    # without skip_nan: the moment planes that the NaN reaches are NaN on those pixels (the
    # climatology does not enter d, nor the truth pa), everything else is clean
    raw = _state(_run(cfg, shape, P, T2, C2))
    _assert_same(raw, clean, "other pixels, no skip", where=~sub)
    assert torch.equal(raw[0], clean[0])
    poisoned = {("field", "t"): (0, 1), ("field-clim-minmax", "t"): (0, 1),
                ("field-clim-minmax", "c"): (0, 1), ("error", "t"): (0, 1, 2),
                ("error-clim", "t"): (0, 1, 2, 5, 6, 7),
                ("error-clim", "c"): (3, 4, 5, 6, 7)}[(cfg, which)]
    moment_planes = 2 if cfg.startswith("field") else raw[1].shape[0]
    for k in range(moment_planes):
        if k in poisoned:
            assert torch.isnan(raw[1][k][sub]).all(), k
        else:
            assert torch.equal(_bits(raw[1][k]), _bits(clean[1][k])), k
    assert not torch.isnan(raw[1][:, ~sub]).any()


def test_nan_in_the_forecast_is_never_skipped():
    shape = (2, 3, 5, 7)
    P, T, C = TU.problem(shape, 3, "300")
    sub = _subset(shape, seed=10)
    P2 = P.clone()
    P2[1, 1][sub] = float("nan")
    clean = _state(_run("error-clim", shape, P, T, C))
    for skip in (True, False):
        got = _state(_run("error-clim", shape, P2, T, C, skip=skip))
        assert torch.equal(got[0], clean[0])                      # counted
        for k in (0, 1, 2, 3, 4, 7):                               # d and pa planes, c_pt
            assert torch.isnan(got[1][k][sub]).all(), k
        assert torch.equal(_bits(got[1][5]), _bits(clean[1][5]))   # ta never saw p
        _assert_same(got, clean, "other pixels", where=~sub)


# ---- 5. merge -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,updates", [((2, 3, 5, 7), 4), ((1, 2, 3, 2731), 3),
                                           ((1, 1, 1, 3), 2), ((2, 3, 5, 7), 64)], ids=_ids)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_merge_of_two_parts_is_the_whole(cfg, shape, updates):
    P, T, C = TU.problem(shape, updates, "300")
    h = max(1, updates // 3)                                       # unequal parts
    a = _run(cfg, shape, P[:h], T[:h], C[:h])
    b = _run(cfg, shape, P[h:], T[h:], C[h:])
    b_before = _state(b)
    na = _state(a)[0]
    a.merge(b)
    got = _state(a)
    _assert_same(_state(b), b_before, "the source of a merge")
    assert torch.equal(got[0], na + b_before[0])
    _check_accuracy(cfg, got, TU.flat(P), TU.flat(T), TU.flat(C), None, f"{cfg} merged")
    # a fresh state is the unit, on either side, bit for bit
    a.merge(_new(cfg, shape))
    _assert_same(_state(a), got, "merging a fresh state in")
    f = _new(cfg, shape)
    f.merge(a)
    _assert_same(_state(f), got, "merging into a fresh state")


@pytest.mark.parametrize("cfg", ["field-clim-minmax", "error-clim"])
def test_merge_with_counts_that_differ_per_pixel(cfg):
    shape = (2, 3, 5, 7)
    B = shape[0]
    P, T, C = TU.problem(shape, 4, "300")
    T2 = T.clone()
    subs = [_subset(shape, seed=s) for s in (11, 12)]
    T2[0, 1][subs[0]] = float("nan")
    T2[3, 0][subs[1]] = float("nan")
    T2[2, :, 0, 0, 0] = float("nan")               # all of the second part at one pixel ...
    T2[3, :, 0, 0, 0] = float("nan")
    T2[0, :, 1, 2, 3] = float("nan")               # ... and all of the first at another
    T2[1, :, 1, 2, 3] = float("nan")
    a = _run(cfg, shape, P[:2], T2[:2], C[:2], skip=True)
    b = _run(cfg, shape, P[2:], T2[2:], C[2:], skip=True)
    sa, sb = _state(a), _state(b)
    a.merge(b)
    got = _state(a)
    valid = ~torch.isnan(TU.flat(T2))
    assert torch.equal(got[0], valid.sum(0).to(torch.int32))
    assert sb[0][0, 0, 0] == 0 and sa[0][1, 2, 3] == 0 and got[0].min() > 0
    _check_accuracy(cfg, got, TU.flat(P), TU.flat(T), TU.flat(C), valid, f"{cfg} merged")
    here = torch.zeros(shape[1:], dtype=torch.bool)
    here[0, 0, 0] = True
    _assert_same(got, sa, "src without an update: dst keeps its bits", where=here)
    here = torch.zeros(shape[1:], dtype=torch.bool)
    here[1, 2, 3] = True
    _assert_same(got, sb, "dst without an update: it takes src's bits", where=here)


def test_climatology_window_is_the_three_way_merge():
    from msfno_amd import timestats as TS
    shape = (2, 3, 5, 7)
    _, S, H, W = shape
    _, T, _ = TU.problem(shape, 3, "300")
    cl = TS.Climatology(5, S, H, W, device=DEV)
    for u in range(3):
        cl.update(_dev(T[u]), [u, u + 1])         # bins 0..3; bin 4 stays empty
    cl.update(_dev(T[0, :1]), [None])              # a dropped element
    win = cl.window(1)
    torch.cuda.synchronize()
    for j in range(5):
        want = TS.FieldStats(S, H, W, device=DEV).load_state_dict(cl[j].state_dict())
        want.merge(cl[(j - 1) % 5]).merge(cl[(j + 1) % 5])
        _assert_same(_state(win[j]), _state(want), f"bin {j}")
    assert [int(cl[j].count.max()) for j in range(5)] == [1, 2, 2, 1, 0]
    assert [int(win[j].count.max()) for j in range(5)] == [3, 5, 5, 3, 2]
    # a whole stack merges member by member
    twice = TS.Climatology(5, S, H, W, device=DEV).load_state_dict(cl.state_dict())
    twice.merge(cl)
    for j in range(5):
        want = TS.FieldStats(S, H, W, device=DEV).load_state_dict(cl[j].state_dict())
        want.merge(cl[j])
        _assert_same(_state(twice[j]), _state(want), f"stack merge, bin {j}")


# ---- 6. graph -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["field-clim-minmax", "error-clim"])
def test_recorded_update_replays_bitwise(cfg):
    """One update recorded with torch.cuda.graph and replayed three times, with new data
    written into the static inputs, equals three eager updates: the running count lives on
    the device.  A single-branch graph; no queue setting is touched."""
    shape = (2, 3, 5, 7)
    P, T, C = TU.problem(shape, 3, "scales")
    ref = _state(_run(cfg, shape, P, T, C))
    st = _new(cfg, shape)
    sp, stt, sc = _dev(P[0].clone()), _dev(T[0].clone()), _dev(C[0].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _feed(st, cfg, sp, stt, sc)                # warm-up: the slab map is built here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    st.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _feed(st, cfg, sp, stt, sc)
    torch.cuda.synchronize()
    assert int(st.count.sum()) == 0               # recording runs nothing
    for u in range(3):
        sp.copy_(_dev(P[u]))
        stt.copy_(_dev(T[u]))
        sc.copy_(_dev(C[u]))
        graph.replay()
    _assert_same(_state(st), ref, "three replays against three eager updates")


# ---- 7. consistency with verification ----------------------------------------------------
def test_maps_sum_to_the_verification_scores():
    """For a batch of B cases the latitude-weighted pixel mean of each map is the mean over
    the cases of what verification.field_sums / finish give.  Tolerance: the map's own bound
    (timestats_util: mean N eps A; the uncentred moments m2 / N + mean^2 by the variance bound
    plus (2 |mean| + db) db for the mean's bound db, the cross moment likewise), weighted and
    averaged like the map, plus the verify tests' 1e-5 of the magnitude sum."""
    from msfno_amd import timestats as TS
    from msfno_amd import verification as V
    shape = (3, 4, 9, 14)
    B, C, H, W = shape
    prd, tar, clim, w, want = VU.problem(shape)
    em = TS.ErrorMaps(C, H, W, anomalies=True, device=DEV)
    em.update(_dev(prd), _dev(tar), clim=_dev(clim), clim_slab=list(range(B * C)))
    sums = V.field_sums(_dev(prd), _dev(tar), _dev(w), _dev(clim),
                        list(range(B * C))).cpu().double()
    sc = V.finish(sums, w, W, batch_mean=True)
    n = W * w.double().sum()
    mag = want["full"][1].sum(0) / (n * B)                 # (C, 6) magnitude sums per case
    wl = w.double()[None, :, None]

    def pix(m):
        return (wl * m.cpu().double()).sum(dim=(-1, -2)) / n

    p64, t64 = prd.double(), tar.double()
    c64 = clim.double().reshape(B, C, H, W)
    cnt = torch.full((C, H, W), B)
    stats = {}
    for name, a in (("d", p64 - t64), ("pa", p64 - c64), ("ta", t64 - c64)):
        _, mean, var = TU.moments64(a)
        A = TU.amax(a)
        stats[name] = (mean, var, A, TU.mean_bound(cnt, A), TU.var_bound(cnt, A, var))

    def second(name):                                       # bound of m2 / N + mean^2
        mean, _, _, db, vb = stats[name]
        return vb + (2 * mean.abs() + db) * db

    md, _, Ad, dbd, _ = stats["d"]
    cross_b = TU.cov_bound(cnt, stats["pa"][2], stats["pa"][1], stats["ta"][2], stats["ta"][1]) \
        + stats["pa"][0].abs() * stats["ta"][3] + stats["ta"][0].abs() * stats["pa"][3] \
        + stats["pa"][3] * stats["ta"][3]
    pa2, ta2, cross = em.moments()
    rows = [("bias", em.bias, sc.bias, dbd, V.ERR), ("mse", em.mse, sc.mse, second("d"), V.SE),
            ("mae", em.mae, sc.mae, dbd, V.AE),
            ("pa2", pa2, sums.sum(0)[:, V.PA2] / (n * B), second("pa"), V.PA2),
            ("ta2", ta2, sums.sum(0)[:, V.TA2] / (n * B), second("ta"), V.TA2),
            ("cross", cross, sums.sum(0)[:, V.CROSS] / (n * B), cross_b, V.CROSS)]
    for name, m, ref, bound, k in rows:
        got = pix(m)
        tol = pix(bound) + 1e-5 * mag[:, k]
        err = (got - ref.double()).abs()
        print(f"{name}: worst error / tolerance = {(err / tol).max().item():.3g}")
        assert (err <= tol).all(), name
    # acc() against the per-pixel uncentred ACC in fp64: first-order propagation of the
    # three moments' bounds through cross / sqrt(pa2 ta2), and 16 eps for the fp32 quotient
    pa2_64 = stats["pa"][1] + stats["pa"][0] ** 2
    ta2_64 = stats["ta"][1] + stats["ta"][0] ** 2
    cr_64 = TU.moments64(p64 - c64, None, t64 - c64)[5] + stats["pa"][0] * stats["ta"][0]
    acc64 = cr_64 / (pa2_64 * ta2_64).sqrt()
    tol = cross_b / (pa2_64 * ta2_64).sqrt() \
        + acc64.abs() * 0.5 * (second("pa") / pa2_64 + second("ta") / ta2_64) + 16 * TU.EPS
    err = (em.acc().cpu().double() - acc64).abs()
    print(f"acc: worst error / tolerance = {(err / tol).max().item():.3g}")
    assert (err <= tol).all()


# ---- 8. drivers -----------------------------------------------------------------------------
def _recording(r, rec):
    run = r.run

    def recording(*args, **kwargs):
        for i, y in run(*args, **kwargs):
            rec.append(y.clone())
            yield i, y

    r.run = recording


@pytest.mark.parametrize("regrid", [False, True], ids=["native", "regrid"])
def test_verify_maps_is_the_hand_written_loop(regrid):
    """steps = 5, every = 2 over two successive batches: 3 lead slots, count 2 B each, and the
    bits of updating by hand with the very outputs run() yielded (recorded: a second run need
    not give the same bits)."""
    from test_gpu_ensemble import _rollout
    from msfno_amd import regrid as G
    from msfno_amd import timestats as TS
    r, x0, stds = _rollout(True)
    B, C, H, W = x0.shape
    R = G.Regridder(G.Grid(H, W), G.Grid(max(H // 3, 2), max(W // 3, 2))) if regrid else None
    Ho, Wo = R.out_shape if regrid else (H, W)
    rec = []
    _recording(r, rec)
    g = torch.Generator().manual_seed(3)
    clim = torch.randn(C, Ho, Wo, generator=g).to(DEV)
    batches = []
    maps = None
    for k in range(2):
        truths = [(torch.randn(B, C, Ho, Wo, generator=g).to(DEV), clim) for _ in range(3)]
        xk = x0 + 0.01 * k * stds
        maps = r.verify_maps(xk, truths, 5, every=2, maps=maps, regrid=R)
        batches.append(truths)
    assert len(rec) == 10 and len(maps) == 3 and maps.anomalies
    want = TS.LeadTimeMaps(3, C, Ho, Wo, anomalies=True, device=DEV)
    for k in range(2):
        for slot, i in enumerate((0, 2, 4)):
            y = rec[5 * k + i]
            want[slot].update(y if R is None else R(y), *batches[k][slot])
    for slot in range(3):
        assert (maps[slot].count == 2 * B).all()
        _assert_same(_state(maps[slot]), _state(want[slot]), f"lead slot {slot}")
    assert torch.isfinite(maps[2].rmse).all() and (maps[2].acc().abs() <= 1 + 1e-5).all()
    with pytest.raises(ValueError, match="anomalies=True"):
        r.verify_maps(x0, [(t, clim) for t, _ in batches[0]], 5, every=2,
                      maps=TS.LeadTimeMaps(3, C, Ho, Wo, device=DEV), regrid=R)
    with pytest.raises(ValueError, match="lead times"):
        r.verify_maps(x0, batches[0], 7, every=2, maps=maps, regrid=R)


def test_statistics_is_the_hand_written_loop():
    from test_gpu_ensemble import _rollout
    from msfno_amd import timestats as TS
    r, x0, _ = _rollout(True)
    B, C, H, W = x0.shape
    rec = []
    _recording(r, rec)
    stats = r.statistics(x0, 6, TS.FieldStats(C, H, W, minmax=True, device=DEV))
    assert len(rec) == 6 and (stats.count == 6 * B).all()
    want = TS.FieldStats(C, H, W, minmax=True, device=DEV)
    for y in rec:
        want.update(y)
    _assert_same(_state(stats), _state(want), "statistics")
    assert (stats.min <= stats.max).all() and torch.isfinite(stats.std).all()


def test_climatology_save_resume_and_skill_score():
    """3 "years" of 8 bins (with a 29 February that is dropped), saved after year 2 and
    continued in a new object: the bits of the uninterrupted one.  Its as_clim output goes
    straight into verification.field_sums and reproduces the skill score of the fp64
    climatology: within the verify tests' 2e-5 se / ta2 plus what the mean's bound N eps A
    can move ta2 by, d(ta2) <= sum w (2 |t - c| dc + dc^2), through se / ta2^2."""
    from msfno_amd import timestats as TS
    from msfno_amd import verification as V
    C, H, W, nb = 3, 5, 7, 8
    g = torch.Generator().manual_seed(8)
    years = [(280.0 + 10 * torch.randn(nb, C, H, W, generator=g)).float() for _ in range(3)]

    def feed(cl, x):
        cl.update(_dev(x[0:3]), [0, 1, 2])             # one call per element
        cl.update(_dev(x[2:4]), [None, 3])             # a dropped element
        cl.update(_dev(x[4:6]), [4, 5])
        cl.update(_dev(x[6:7].expand(2, C, H, W)), [6, 6])   # one call, a shared bin
        cl.update(_dev(x[7]), [7])

    whole = TS.Climatology(nb, C, H, W, device=DEV)
    for x in years:
        feed(whole, x)
    first = TS.Climatology(nb, C, H, W, device=DEV)
    for x in years[:2]:
        feed(first, x)
    saved = {k: (v.cpu() if isinstance(v, torch.Tensor) else v)
             for k, v in first.state_dict().items()}
    resumed = TS.Climatology(nb, C, H, W, device=DEV).load_state_dict(saved)
    feed(resumed, years[2])
    torch.cuda.synchronize()
    assert torch.equal(resumed._count.cpu(), whole._count.cpu())
    assert torch.equal(_bits(resumed._planes.cpu()), _bits(whole._planes.cpu()))
    assert [int(whole[j].count.max()) for j in range(nb)] == [3, 3, 3, 3, 3, 3, 6, 3]
    # the skill score of a batch whose elements fall into bins 5, 2, 5
    bins = [5, 2, 5]
    B = len(bins)
    tar = (280.0 + 10 * torch.randn(B, C, H, W, generator=g)).float()
    prd = (tar + 3 * torch.randn(B, C, H, W, generator=g)).float()
    w = (torch.rand(H, generator=g) + 0.1).float()
    clim, slab = whole.as_clim(bins)
    assert tuple(clim.shape) == (2 * C, H, W) and slab.dtype == torch.int32 and slab.is_cuda
    sums = V.field_sums(_dev(prd), _dev(tar), _dev(w), clim, slab)
    skill = V.finish(sums.cpu().double(), w, W).skill
    stack = torch.stack([y.double() for y in years])            # (3, nb, C, H, W)
    c64 = stack.mean(0)                                           # bin 6: pairs, the same mean
    cl64 = torch.stack([c64[j] for j in bins])
    ref, _ = VU.sums(prd.double(), tar.double(), w.double(), cl64.reshape(B * C, H, W),
                     list(range(B * C)))
    want = VU.scores(ref, w, W, torch.ones(B, C, dtype=torch.bool))["skill"]
    ncase = torch.tensor([whole[j].count.max().item() for j in bins]).double()
    A = torch.stack([stack[:, j].abs().amax(dim=0) for j in bins])
    dc = ncase[:, None, None, None] * TU.EPS * A                   # N eps A
    wl = w.double()[None, None, :, None]
    dta2 = (wl * (2 * (tar.double() - cl64).abs() * dc + dc * dc)).sum(dim=(-1, -2))
    ratio = ref[..., V.SE] / ref[..., V.TA2]
    tol = 2e-5 * ratio + ratio * dta2 / ref[..., V.TA2] * 1.001
    err = (skill - want).abs()
    print(f"skill: worst error / tolerance = {(err / tol).max().item():.3g}")
    assert (err <= tol).all()
    # and hour_of_year_bin drives update: 28 February 18 UTC, 29 February (dropped), 1 March
    cl = TS.Climatology(1460, 1, 1, 3, device=DEV)
    days = [dt.datetime(2020, 2, 28, 18), dt.datetime(2020, 2, 29, 0), dt.datetime(2020, 3, 1, 0)]
    cl.update(torch.ones(3, 1, 1, 3, device=DEV), [cl.hour_of_year_bin(d) for d in days])
    assert int(cl._count.sum()) == 6 and int(cl[235].count.sum()) == 3 \
        and int(cl[236].count.sum()) == 3


# ---- 9. refusals ----------------------------------------------------------------------------
def test_every_einval_case_fails_before_a_launch():
    from msfno_amd import _native as N
    from msfno_amd import timestats as TS
    lib = N.lib()
    B, S, Pn = 2, 3, 35
    SP = S * Pn
    x = torch.randn(B, SP, device=DEV)
    y = torch.randn(B, SP, device=DEV)
    clim = torch.randn(B * S, Pn, device=DEV)
    slab = torch.arange(B * S, dtype=torch.int32, device=DEV)
    count = _poisoned(SP, torch.int32)
    state = _poisoned(8 * SP)
    count2, state2 = _poisoned(SP, torch.int32), _poisoned(8 * SP)
    F_, E_, MM, AN = TS.FIELD, TS.ERROR, TS.MINMAX, TS.ANOM
    stream = torch.cuda.current_stream().cuda_stream

    def upd(kind=E_, flags=AN, in0=x, in1=y, clim=clim, slab=slab, B=B, S=S, P=Pn, count=count,
            state=state, ps=SP):
        return _raw_update(kind, flags, in0, in1, SP, SP, clim, slab, B, S, P, 0, count, state,
                           ps)

    def mrg(kind=E_, flags=AN, dc=count, ds=state, dps=SP, sc=count2, ss=state2, sps=SP, n=SP):
        return lib.msfno_tstats_merge(kind, flags, N.ptr(dc), N.ptr(ds), dps, N.ptr(sc),
                                      N.ptr(ss), sps, n, stream)

    cases = [
        (lambda: upd(in0=None), "in0"), (lambda: upd(count=None), "count"),
        (lambda: upd(state=None), "state"), (lambda: upd(B=0), "B, S or P"),
        (lambda: upd(S=0), "B, S or P"), (lambda: upd(P=0), "B, S or P"),
        (lambda: upd(kind=2), "kind"), (lambda: upd(flags=4), "flag"),
        (lambda: upd(flags=AN | MM), "flag"),                       # MINMAX on ERROR
        (lambda: upd(kind=F_, flags=AN, in1=None), "flag"),         # ANOM on FIELD
        (lambda: upd(in1=None), "in1"),                             # missing for ERROR
        (lambda: upd(kind=F_, flags=MM), "in1"),                    # given for FIELD
        (lambda: upd(clim=None), "clim_slab"), (lambda: upd(slab=None), "clim_slab"),
        (lambda: upd(flags=0), "iff clim"),                         # planes without a flag
        (lambda: upd(flags=AN, clim=None, slab=None), "iff clim"),
        (lambda: upd(ps=SP - 1), "plane_stride"),
        (lambda: mrg(dc=None), "dst_count"), (lambda: mrg(ds=None), "dst_state"),
        (lambda: mrg(sc=None), "src_count"), (lambda: mrg(ss=None), "src_state"),
        (lambda: mrg(n=0), "N"), (lambda: mrg(kind=-1), "kind"),
        (lambda: mrg(kind=E_, flags=MM), "flag"),
        (lambda: mrg(dps=SP - 1), "dst_plane_stride"),
        (lambda: mrg(sps=SP - 1), "src_plane_stride"),
        (lambda: lib.msfno_tstats_planes(2, 0), "kind"),
        (lambda: lib.msfno_tstats_planes(E_, MM), "flag"),
        (lambda: lib.msfno_tstats_planes(F_, AN), "flag"),
    ]
    for i, (call, word) in enumerate(cases):
        assert call() == N.MSFNO_EINVAL, i
        msg = lib.msfno_last_error().decode()
        assert word in msg, (i, word, msg)
    torch.cuda.synchronize()
    for buf in (count, state, count2, state2):
        assert (buf.view(torch.int32) == POISON).all(), "a refused call wrote to a state"
    assert [lib.msfno_tstats_planes(*kf) for kf in ((F_, 0), (F_, MM), (E_, 0), (E_, AN))] \
        == [2, 4, 3, 8]
    assert TS.planes(E_, AN) == 8
    # the Python layer refuses a map that would leave a slab without its climatology
    em = TS.ErrorMaps(S, 5, 7, anomalies=True, device=DEV)
    p4 = x.reshape(B, S, 5, 7)
    for bad in ([0, 1, 2, -1, 4, 5], torch.tensor([0, 1, 2, 3, 4, 6], dtype=torch.int32,
                                                   device=DEV)):
        with pytest.raises(ValueError, match="clim_slab"):
            em.update(p4, p4, clim=clim.reshape(B * S, 5, 7), clim_slab=bad)
    assert int(em.count.sum()) == 0
