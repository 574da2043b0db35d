"""The trace generators and the virtual peers (include/hermeskv_workload.h) against tests/peer_model.py, byte for
byte.

The mirrored round tests replay whatever messages these kernels emit on the device and on the oracle twin alike,
so a wrong message -- a timestamp read from a stale place, a dedup that keeps another occurrence, a Zipf with less
skew -- is applied identically on both sides and passes there. Here every kernel's output is compared with the
model's: the C entry points are called directly (hermes_amd.workload._L), output buffers are pre-filled with 0xA5
and the bytes the contract leaves untouched are compared too. The peers' timestamps are checked on tables whose
versions differ (the protocol rounds of tests/inline_cases.py ran on them), in LOG, freshly converted INLINE, and
INLINE after twelve launches without an export, where an inline key's log copy is stale.

tests/test_peer_model_cpu.py shows the model is not vacuous and that exact equality is safe at these shapes.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS, gen_keys  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests import peer_cases as PC  # noqa: E402
from tests import peer_model as PM  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
FILL = 0xA5
GUARD = 64       # elements past every buffer's used part, which must stay FILL


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def engine_path():
    """the multi-kernel engine for every batch launch: the single-workgroup kernel has no inline instance"""
    from hermes_amd import kvs
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    yield
    kvs.HermesKV.default_flags = 0


def _wl():
    from hermes_amd import workload as WL
    return WL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(nbytes):
    return torch.full((int(nbytes),), FILL, dtype=torch.uint8, device="cuda")


def _host(t, dtype=np.uint8):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _zipf(WL, z):
    return WL.HkvZipf(z.theta, z.zetan, z.alpha, z.eta, z.half_pow, z.n)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        pytest.fail(f"{what}: {len(bad)} of {len(got)} rows differ, first {bad[:8].tolist()}: "
                    f"device {got[bad[0]].reshape(-1)[:24].tolist()} model {want[bad[0]].reshape(-1)[:24].tolist()}")


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("W,ln,n,theta,write_pm,rmw_pm,with_id", PC.TRACE_CASES)
def test_gen_trace(W, ln, n, theta, write_pm, rmw_pm, with_id):
    WL = _wl()
    z = PM.zipf_params(n, theta)
    N = W * ln
    tk, to, ti = _filled((N + GUARD) * 8), _filled(N + GUARD), _filled((N + GUARD) * 4) if with_id else None
    hz = _zipf(WL, z)
    WL.check(WL._L.hkv_wl_gen_trace(WL._ptr(tk), WL._ptr(to), WL._ptr(ti), W, ln, ctypes.byref(hz), write_pm, rmw_pm,
                                    ctypes.c_uint64(PC.SEED), WL._s()), "gen_trace")
    key, op, ids = PM.gen_trace(W, ln, z, write_pm, rmw_pm, PC.SEED, gen_keys(n))
    if with_id:
        got = _host(ti, "<u4")
        _same(got[:N], ids, "ids")
        assert (got[N:] == 0xA5A5A5A5).all()
    _same(_host(tk, "<u8")[:N], key, "keys")
    _same(_host(to)[:N], op, "opcodes")
    assert (_host(tk)[N * 8:] == FILL).all() and (_host(to)[N:] == FILL).all(), "written past the trace"
    if rmw_pm:
        assert (op == PM.OP_RMW).sum() > 0.05 * N and (op == PM.OP_PUT).sum() > 0.05 * N
    if n == 3:
        assert set(ids.tolist()) == {0, 1, 2}


@pytest.mark.parametrize("W,pp,peers,big,rmw_pm,rounds", PC.PEER_ROUND_CASES)
def test_gen_peer_round(W, pp, peers, big, rmw_pm, rounds):
    WL = _wl()
    s = L.BIG if big else L.DEFAULT
    n = PC.PEER_ROUND_KEYS
    z = PM.zipf_params(n, 0.99)
    keys = gen_keys(n)
    R = len(peers)
    hz = _zipf(WL, z)
    scratch = torch.empty(int(WL._L.hkv_wl_peer_round_scratch(W, pp, R)), dtype=torch.uint8, device="cuda")
    peer_t = _dev(np.array(peers, np.uint8))
    outs = []
    for rnd in rounds:
        ri, rv, pc = _filled(W * R * pp * s.op), _filled(W * R * pp * 16), _filled(W * R * 4)
        WL.check(WL._L.hkv_wl_gen_peer_round(WL._ptr(ri), WL._ptr(rv), WL._ptr(pc), W, pp, WL._ptr(peer_t), R, s.op,
                                             s.st_value, s.shift, ctypes.byref(hz), rmw_pm, rnd,
                                             ctypes.c_uint64(PC.SEED), WL._ptr(scratch), WL._s()), "gen_peer_round")
        invs, vals, counts = PM.gen_peer_round(W, pp, peers, s.op, s.st_value, s.shift, z, rmw_pm, rnd, PC.SEED, keys,
                                               fill=FILL)
        _same(_host(pc, "<i4").reshape(W, R), counts, f"round {rnd}: peer counts")
        _same(_host(ri).reshape(W * R * pp, s.op), invs.reshape(-1, s.op), f"round {rnd}: INVs")
        _same(_host(rv).reshape(W * R * pp, 16), vals.reshape(-1, 16), f"round {rnd}: VALs")
        assert counts.sum() < 0.9 * W * R * pp, "the dedup dropped nothing"
        if rmw_pm:
            live = invs.reshape(-1, s.op)[invs.reshape(-1, s.op)[:, 8] == PM.OP_INV]
            assert 0.3 < (live[:, 16] == 1).mean() < 0.7
        outs.append(invs)
    if len(outs) > 1:
        assert not np.array_equal(outs[0], outs[1]), "two round indices drew the same round"


@pytest.mark.parametrize("n", [1, 15, 16, 40, 16384, 16400])
def test_ack_offsets(n):
    """n = 16400: a second 16384-chunk, whose offsets carry the first chunk's sum. Pointers 16-byte aligned (the
    vector path) and offset by one int32 (the scalar path); seq 0 (no flag) and seq 3 (h_out[2] = 3)."""
    WL = _wl()
    rng = np.random.default_rng(n)
    h = torch.zeros(4, dtype=torch.int32).pin_memory()
    for n_peers in (1, 2, 7):
        for shift in (0, 1):
            for seq in (0, 3):
                counts = rng.integers(0, 50, size=n).astype(np.int32)
                counts[rng.integers(0, n)] = 50
                cbuf = np.full(n + 8, -7, np.int32)
                cbuf[shift:shift + n] = counts
                ct = _dev(cbuf)
                ot = _filled((n + 1 + 8) * 4)
                h[:] = -1
                WL.check(WL._L.hkv_wl_ack_offsets(ctypes.c_void_p(ct.data_ptr() + 4 * shift), n, n_peers,
                                                  ctypes.c_void_p(ot.data_ptr() + 4 * shift), WL._ptr(h), seq, WL._s()),
                         "ack_offsets")
                got = _host(ot, "<i4")
                off, total, mx = PM.ack_offsets(counts, n_peers)
                what = f"n_peers {n_peers} shift {shift} seq {seq}"
                _same(got[shift:shift + n + 1], off, what)
                assert (got[:shift] == -1515870811).all() and (got[shift + n + 1:] == -1515870811).all(), what
                assert h.tolist()[:3] == [total, mx, seq if seq else -1], (what, h.tolist())
                assert mx == 50 and np.array_equal(_host(ct, "<i4"), cbuf)


# ------------------------------------------------------------------------------------------- peer timestamps
def _table_after_rounds(state, rmw=False):
    """Geometry A after two protocol rounds (12 launches: local, two unique INV launches, two unique ACK launches,
    VALs; writes in flight, INVALID keys, versions above 0), device and twin, never exported. state "log": the
    table stays in the reference layout; "inline": the rounds run INLINE (an RMW table's local launches have no
    inline kernels: it stays in LOG here). Returns (g, o, T, the Mirror, the engine that runs the rounds)."""
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO["A"]
    g = HermesKV(n_keys, bkts, cap, machine_id=0, rmw=rmw)
    o = C.make_oracle("A", rmw=rmw)
    T = C.describe(o, "A")
    if state != "log":
        assert g.prefer_layout(INLINE)
    m = Mirror(g, o, f"peers {state}", table_check="deferred")
    eng = GpuEngine(m, layout=state != "log")
    return g, o, T, m, eng


def _run_rounds(eng, T, rmw=False):
    C.case_rounds(eng, T, C.Rec(T.inline_keys), rmw=rmw, rounds=2, big=(), check_after=())
    assert eng.m.launches == 12


def _sample_invs(T, rng, op_size, rmw_flags, peers=(1, 2)):
    """One INV per peer and key over every inline key, 400 other present keys, the absent keys and the collision
    fakes (same bucket and tag as a present key: the first tag match is another key's entry, a miss), shuffled;
    every byte the stamping must keep is random"""
    K, M, fakes = C.collision_keys(T)
    others = np.setdiff1d(T.keys[T.present], T.inline_keys)
    ks = np.concatenate([T.inline_keys, rng.choice(others, 400, replace=False), T.keys[~T.present], fakes,
                         np.array([K, M], np.uint64)])
    ks = np.unique(ks)
    keys = np.concatenate([ks for _ in peers])
    invs = rng.integers(0, 256, size=(len(keys), op_size), dtype=np.uint8)
    invs[:, :8] = keys.view(np.uint8).reshape(-1, 8)
    invs[:, 9] = np.repeat(np.array(peers, np.uint8), len(ks))
    invs[:, 16] = rng.integers(0, 2, size=len(keys)) if rmw_flags else 0
    perm = rng.permutation(len(keys))
    invs = invs[perm]
    vals = rng.integers(0, 256, size=(len(keys), 16), dtype=np.uint8)
    vals[:, :8] = invs[:, :8]
    strata = {"inline": np.isin(keys[perm], T.inline_keys), "absent": np.isin(keys[perm], T.keys[~T.present]),
              "fake": np.isin(keys[perm], fakes)}
    return invs, vals, strata


def _locate(WL, g, invs):
    n, op = invs.shape
    d = _dev(invs.reshape(-1))
    phys = torch.full((n + GUARD,), -6510615555426900571, dtype=torch.int64, device="cuda")   # 0xA5 bytes
    WL.check(WL._L.hkv_wl_peer_locate(g.h, WL._ptr(d), n, op, WL._ptr(phys), WL._s()), "peer_locate")
    torch.cuda.synchronize()
    assert (phys[n:] == -6510615555426900571).all() and np.array_equal(_host(d).reshape(n, op), invs)
    return phys


def _ts_at(WL, g, invs, vals, phys, words, rnd, merged=False):
    """hkv_wl_peer_ts_at (or the merged hkv_wl_refill_plan_peer_ts) over the INVs back to back; returns the
    stamped (invs, vals) with the guard elements checked"""
    n, op = invs.shape
    di, dv = _filled((n + GUARD) * op), _filled((n + GUARD) * 16)
    di[:n * op] = _dev(invs.reshape(-1))
    dv[:n * 16] = _dev(vals.reshape(-1))
    if merged:
        W, S, tl = 4, 250, 64
        states = torch.full((W * S,), int(L.Resp.GET_COMPLETE), dtype=torch.uint8, device="cuda")
        tkey = torch.arange(W * tl, dtype=torch.int64, device="cuda")
        top = torch.full((W * tl,), int(L.Op.GET), dtype=torch.uint8, device="cuda")
        cursor = torch.zeros(W, dtype=torch.int32, device="cuda")
        counters = torch.zeros(4096, dtype=torch.int64, device="cuda")
        opc, patch = torch.zeros(W * S, dtype=torch.uint8, device="cuda"), _filled(W * S * 16)
        WL.check(WL._L.hkv_wl_refill_plan_peer_ts(WL._ptr(states), W, S, g.sizes.st_value, g.sizes.shift, WL._ptr(tkey),
                                                  WL._ptr(top), tl, WL._ptr(cursor), 0, 0, WL._ptr(counters),
                                                  WL._ptr(opc), WL._ptr(patch), g.h, WL._ptr(di), WL._ptr(dv),
                                                  WL._ptr(phys), n, op, WL._ptr(words), rnd, WL._s()),
                 "refill_plan_peer_ts")
        torch.cuda.synchronize()
        assert (opc == int(L.Op.GET)).all() and (cursor == S % tl).all(), "the plan half did not run"
    else:
        WL.check(WL._L.hkv_wl_peer_ts_at(g.h, WL._ptr(di), WL._ptr(dv), WL._ptr(phys), n, op, WL._ptr(words), rnd,
                                         WL._s()), "peer_ts_at")
    gi, gv = _host(di).reshape(-1, op), _host(dv).reshape(-1, 16)
    assert (gi[n:] == FILL).all() and (gv[n:] == FILL).all(), "written past the INVs"
    return gi[:n], gv[:n]


def _ts_rows(WL, g, invs, vals, words, rnd, rng):
    """hkv_wl_peer_ts: the INVs laid out in rows with ragged counts (0 and a full row among them); returns the
    rows' (invs, vals, live mask)"""
    n, op = invs.shape
    S = 300
    counts = [0, S]
    left = n - S
    while left > 0:
        c = int(min(left, rng.integers(1, S + 1)))
        counts.append(c)
        left -= c
    counts = np.array(counts, np.int32)
    W = len(counts)
    where = np.concatenate([w * S + np.arange(c) for w, c in enumerate(counts)])
    ri, rv = np.full((W * S, op), FILL, np.uint8), np.full((W * S, 16), FILL, np.uint8)
    ri[where], rv[where] = invs, vals
    di, dv = _dev(ri.reshape(-1)), _dev(rv.reshape(-1))
    WL.check(WL._L.hkv_wl_peer_ts(g.h, WL._ptr(di), WL._ptr(dv), WL._ptr(_dev(counts)), W, S, op, WL._ptr(words), rnd,
                                  WL._s()), "peer_ts")
    gi, gv = _host(di).reshape(-1, op), _host(dv).reshape(-1, 16)
    live = np.zeros(W * S, bool)
    live[where] = True
    assert (gi[~live] == FILL).all() and (gv[~live] == FILL).all(), "a slot past its row's count was written"
    return gi[where], gv[where]


@pytest.mark.parametrize("state", ["log", "fresh", "stale"])
def test_peer_timestamps(state):
    """(a) a LOG table, (b) an INLINE table freshly converted (log and lines byte-equal), (c) an INLINE table twelve
    launches after its conversion and never exported: the inline keys' log copies are stale. peer_locate, peer_ts_at
    and the merged call must not convert the table; hkv_wl_peer_ts asks for LOG and does."""
    WL = _wl()
    rng = np.random.default_rng(7)
    g, o, T, m, eng = _table_after_rounds("log" if state == "log" else "inline")
    invs, vals, strata = _sample_invs(T, rng, 56, rmw_flags=True)
    n = len(invs)
    assert min(v.sum() for v in strata.values()) >= 4 and strata["inline"].sum() >= 1000
    phys_before = _locate(WL, g, invs)                  # taken before the rounds
    assert g.layout()["conversions"] == 0
    _run_rounds(eng, T)
    if state == "fresh":
        m.check_table("before the conversion")          # the export sends the table to LOG ...
        g.apply_layout()                                # ... and this converts it again
        torch.cuda.synchronize()
    lay0 = g.layout()
    assert lay0["state"] == (LOG if state == "log" else INLINE)
    assert lay0["conversions"] == {"log": 0, "fresh": 3, "stale": 1}[state], lay0
    ver, phys = PM.peer_versions(o, invs)
    want_i, want_v = PM.stamp(invs, PM.OP_INV, ver), PM.stamp(vals, PM.OP_VAL, ver)
    # the sample is not trivial: versions moved, on inline keys too; absent keys and fakes miss
    moved = (phys >= 0) & (ver > 2)
    assert moved.sum() >= 200 and (moved & strata["inline"]).sum() >= 50, (moved.sum(), (moved & strata["inline"]).sum())
    assert (phys[strata["absent"] | strata["fake"]] == -1).all() and (ver[strata["fake"]] == 2).all()
    assert len(np.unique(ver)) >= 4

    located = _locate(WL, g, invs)
    lp = _host(located, "<u8")[:n]
    assert np.array_equal(lp == np.uint64(PM.M64), phys < 0), "peer_locate: which keys are absent"
    assert np.array_equal(lp[phys >= 0] & np.uint64((1 << 40) - 1), phys[phys >= 0].astype(np.uint64)), "log offsets"
    perm = located.clone()
    perm[:n] = located[:n][torch.from_numpy(rng.permutation(n)).cuda()]
    none = torch.full_like(located, -1)
    for what, ph in (("located", located), ("permuted", perm), ("all absent", none), ("before the rounds", phys_before)):
        gi, gv = _ts_at(WL, g, invs, vals, ph, None, 3)
        _same(gi, want_i, f"{state}, peer_ts_at, {what}: INVs")
        _same(gv, want_v, f"{state}, peer_ts_at, {what}: VALs")
    gi, gv = _ts_at(WL, g, invs, vals, located, None, 3, merged=True)
    _same(gi, want_i, f"{state}, merged: INVs")
    _same(gv, want_v, f"{state}, merged: VALs")
    lay = g.layout()    # (inline_launches counts the live-view calls that ran on the lines)
    assert (lay["state"], lay["conversions"]) == (lay0["state"], lay0["conversions"]), \
        f"peer_locate / peer_ts_at / the merged call converted the table: {lay0} -> {lay}"
    assert lay["inline_launches"] > lay0["inline_launches"] or state == "log"
    gi, gv = _ts_rows(WL, g, invs, vals, None, 3, rng)
    _same(gi, want_i, f"{state}, peer_ts rows: INVs")
    _same(gv, want_v, f"{state}, peer_ts rows: VALs")
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == lay0["conversions"] + (state != "log"), (lay0, lay)
    m.check_table("the end")        # and nothing above wrote the table
    assert g.take_error_flags() == 0


def test_peer_timestamps_rmw_build():
    """An RMW build: + 2 for an RMW, + 4 for a plain write; every word of d_peer_ts, the untouched ones included;
    a second call with the next round number replaces the words it names. A sender of 9 records no word."""
    WL = _wl()
    rng = np.random.default_rng(11)
    g, o, T, m, eng = _table_after_rounds("log", rmw=True)
    _run_rounds(eng, T, rmw=True)
    invs, vals, strata = _sample_invs(T, rng, 56, rmw_flags=True, peers=(1, 2, 7, 9))
    n = len(invs)
    ver, phys = PM.peer_versions(o, invs)
    plain, rmw = invs[:, 16] == 0, invs[:, 16] == 1
    log = o.log_bytes()
    cur = np.array([int.from_bytes(bytes(log[p + 24:p + 28]), "little") if p >= 0 else 0 for p in phys])
    hit = phys >= 0
    assert (ver[hit & plain] == cur[hit & plain] + 4).all() and (ver[hit & rmw] == cur[hit & rmw] + 2).all()
    assert (hit & plain).sum() > 500 and (hit & rmw).sum() > 500 and len(np.unique(cur[hit])) >= 4
    want_i, want_v = PM.stamp(invs, PM.OP_INV, ver), PM.stamp(vals, PM.OP_VAL, ver)
    nw = int(WL._L.hkv_wl_peer_ts_words(g.h))
    assert nw == (T.cap // 64 + 1) * 8
    w1 = PM.peer_ts_words(np.zeros(nw, np.uint64), invs, ver, phys, 64, 4)
    assert np.count_nonzero(w1) == (hit & (invs[:, 9] < 8)).sum() and not w1.reshape(-1, 8)[:, [0, 3, 4, 5, 6]].any()
    half = np.sort(rng.choice(n, n // 2, replace=False))
    w2 = PM.peer_ts_words(w1, invs[half], ver[half], phys[half], 64, 5)
    assert (w2 != w1).sum() == (hit & (invs[:, 9] < 8))[half].sum()
    located = _locate(WL, g, invs)
    lh = torch.full((len(half) + GUARD,), -1, dtype=torch.int64, device="cuda")
    lh[:len(half)] = located[:n][torch.from_numpy(half).cuda()]
    for how in ("rows", "at", "merged"):
        words = torch.zeros(nw, dtype=torch.int64, device="cuda")
        for rnd, sel, ww, ph in ((4, slice(None), w1, located), (5, half, w2, lh)):
            if how == "rows":
                gi, gv = _ts_rows(WL, g, invs[sel], vals[sel], words, rnd, rng)
            else:
                gi, gv = _ts_at(WL, g, invs[sel], vals[sel], ph, words, rnd, merged=how == "merged")
            _same(gi, want_i[sel], f"{how}, round {rnd}: INVs")
            _same(gv, want_v[sel], f"{how}, round {rnd}: VALs")
            _same(_host(words, "<u8").reshape(-1, 8), ww.reshape(-1, 8), f"{how}, round {rnd}: peer_ts words")
    m.check_table("the end")
    assert g.take_error_flags() == 0


# ---------------------------------------------------------------------------------------------- peer answers
def _answer_layouts(WL, g, o, invs, inv_count, peers, ack_size, words_dev, words, rnd, rng):
    """hkv_wl_peer_acks (rows and d_out_off), _pm and _queue over invs [W][C][op] against the model; returns all
    answers of the rows layout"""
    W, Cs, op = invs.shape
    R = len(peers)
    kw = dict(oracle=o, words=words, rnd=rnd) if words is not None else {}
    di, dc, dp = _dev(invs.reshape(-1)), _dev(inv_count), _dev(np.array(peers, np.uint8))
    wp = WL._ptr(words_dev)
    # rows
    stride = Cs * R
    out, cnt = _filled((W * stride + GUARD) * ack_size), _filled(W * 4)
    WL.check(WL._L.hkv_wl_peer_acks(g.h, WL._ptr(di), WL._ptr(dc), W, Cs, op, WL._ptr(out), ack_size, stride,
                                    WL._ptr(cnt), WL._ptr(dp), R, wp, rnd, None, WL._s()), "peer_acks")
    want = np.full((W * stride + GUARD, ack_size), FILL, np.uint8)
    want, wc = PM.peer_acks_rows(invs, inv_count, peers, ack_size, stride, want, **kw)
    _same(_host(out).reshape(-1, ack_size), want, "peer_acks rows")
    _same(_host(cnt, "<i4"), wc, "peer_acks rows: ack_count")
    rows = want
    # packed at d_out_off
    off, total, _ = PM.ack_offsets(inv_count, R)
    out, cnt = _filled((total + GUARD) * ack_size), _filled(W * 4)
    WL.check(WL._L.hkv_wl_peer_acks(g.h, WL._ptr(di), WL._ptr(dc), W, Cs, op, WL._ptr(out), ack_size, stride,
                                    WL._ptr(cnt), WL._ptr(dp), R, wp, rnd, WL._ptr(_dev(off)), WL._s()), "peer_acks")
    want = np.full((total + GUARD, ack_size), FILL, np.uint8)
    want, wc = PM.peer_acks_packed(invs, inv_count, peers, ack_size, off, want, **kw)
    _same(_host(out).reshape(-1, ack_size), want, "peer_acks packed")
    _same(_host(cnt, "<i4"), wc, "peer_acks packed: ack_count")
    out = _filled((total + GUARD) * ack_size)     # and without d_ack_count, which the header allows with d_out_off
    WL.check(WL._L.hkv_wl_peer_acks(g.h, WL._ptr(di), WL._ptr(dc), W, Cs, op, WL._ptr(out), ack_size, stride,
                                    None, WL._ptr(dp), R, wp, rnd, WL._ptr(_dev(off)), WL._s()), "peer_acks")
    _same(_host(out).reshape(-1, ack_size), want, "peer_acks packed, no ack_count")
    # peer-major
    ioff, T_, mx = PM.ack_offsets(inv_count, 1)
    out, cnt = _filled((R * T_ + GUARD) * ack_size), _filled(W * 4)
    WL.check(WL._L.hkv_wl_peer_acks_pm(g.h, WL._ptr(di), WL._ptr(dc), W, Cs, op, WL._ptr(out), ack_size, mx,
                                       WL._ptr(cnt), WL._ptr(dp), R, wp, rnd, WL._ptr(_dev(ioff)), WL._s()),
             "peer_acks_pm")
    want = np.full((R * T_ + GUARD, ack_size), FILL, np.uint8)
    want, wc = PM.peer_acks_pm(invs, inv_count, peers, ack_size, ioff, want, **kw)
    _same(_host(out).reshape(-1, ack_size), want, "peer_acks_pm")
    _same(_host(cnt, "<i4"), wc, "peer_acks_pm: ack_count")
    # queues: 5 answers queued already in some rows, VALs outstanding in some
    q = stride + 5
    aq_n = rng.choice(np.array([0, 5], np.int32), size=W)
    vq_n = rng.choice(np.array([0, 2], np.int32), size=W)
    aq_n[:4], vq_n[:4] = [0, 0, 5, 5], [0, 2, 0, 2]
    out, cnt, dq = _filled((W * q + GUARD) * ack_size), _filled(W * 4), _dev(aq_n)
    WL.check(WL._L.hkv_wl_peer_acks_queue(g.h, WL._ptr(di), WL._ptr(dc), W, Cs, op, WL._ptr(out), ack_size, q,
                                          WL._ptr(dq), WL._ptr(_dev(vq_n)), WL._ptr(cnt), WL._ptr(dp), R, wp, rnd,
                                          WL._s()), "peer_acks_queue")
    want = np.full((W * q + GUARD, ack_size), FILL, np.uint8)
    want, wq, wc = PM.peer_acks_queue(invs, inv_count, peers, ack_size, q, aq_n, vq_n, want, **kw)
    _same(_host(out).reshape(-1, ack_size), want, "peer_acks_queue")
    _same(_host(dq, "<i4"), wq, "peer_acks_queue: aq_n")
    _same(_host(cnt, "<i4"), wc, "peer_acks_queue: ack_count")
    assert (wc == 0).any() and (wc > 0).any()
    assert np.array_equal(_host(di).reshape(invs.shape), invs), "the INVs were written"
    return rows


def _ragged(rng, W, Cs):
    c = rng.integers(0, Cs + 1, size=W).astype(np.int32)
    c[0], c[1], c[2] = 0, Cs, 1
    return c


@pytest.mark.parametrize("peers", [[1, 2], [1, 2, 3, 4, 5, 6, 7]])
def test_peer_answers(peers):
    """without RMWs: 16-byte ACKs, the INV's header with opcode ACK and sender = the peer"""
    WL = _wl()
    from hermes_amd.kvs import HermesKV
    rng = np.random.default_rng(len(peers))
    g = HermesKV(*C.GEO["A"], machine_id=0)
    W, Cs = 40, 56
    invs = rng.integers(0, 256, size=(W, Cs, 56), dtype=np.uint8)
    invs[:, :, 8] = PM.OP_INV
    rows = _answer_layouts(WL, g, None, invs, _ragged(rng, W, Cs), peers, 16, None, None, 9, rng)
    live = rows[rows[:, 8] != FILL]
    assert (live[:, 8] == PM.OP_ACK).all() and set(np.unique(live[:, 9]).tolist()) == set(peers)


@pytest.mark.parametrize("peers", [[1, 2], [1, 2, 3, 4, 5, 6, 7]])
def test_peer_answers_rmw_build(peers):
    """RMW build, op-sized answers: the peers wrote keys S1 this round and keys S0 the round before (words with an
    older tag, which read as empty); the local INVs are plain writes and RMWs on S1, S0, untouched and absent keys,
    below and above the peers' words."""
    WL = _wl()
    from hermes_amd.kvs import HermesKV
    rng = np.random.default_rng(100 + len(peers))
    rnd = 6
    g = HermesKV(*C.GEO["A"], machine_id=0, rmw=True)
    o = C.make_oracle("A", rmw=True)
    T = C.describe(o, "A")
    present, absent = T.keys[T.present], T.keys[~T.present]
    S0, S1, S2 = present[:300], present[300:900], present[900:1100]

    def peer_writes(ks):
        x = np.zeros((len(ks) * len(peers), 56), np.uint8)
        x[:, :8] = np.tile(ks, len(peers)).view(np.uint8).reshape(-1, 8)
        x[:, 9] = x[:, 11] = np.repeat(np.array(peers, np.uint8), len(ks))
        x[:, 16] = rng.integers(0, 2, size=len(x))
        return x

    nw = int(WL._L.hkv_wl_peer_ts_words(g.h))
    words_dev = torch.zeros(nw, dtype=torch.int64, device="cuda")
    words = np.zeros(nw, np.uint64)
    for ks, r in ((S0, rnd - 1), (S1, rnd)):
        x = peer_writes(ks)
        ver, phys = PM.peer_versions(o, x)
        words = PM.peer_ts_words(words, x, ver, phys, 64, r)
        ph = torch.full((len(x) + GUARD,), -1, dtype=torch.int64, device="cuda")
        _ts_at(WL, g, x, np.zeros((len(x), 16), np.uint8), ph, words_dev, r)
    _same(_host(words_dev, "<u8").reshape(-1, 8), words.reshape(-1, 8), "the peers' words")
    W, Cs = 40, 56
    pool = np.concatenate([S0, S1, S2, absent])
    invs = rng.integers(0, 256, size=(W, Cs, 56), dtype=np.uint8)
    k = rng.choice(pool, W * Cs)
    invs[:, :, :8] = k.view(np.uint8).reshape(W, Cs, 8)
    invs[:, :, 8], invs[:, :, 9], invs[:, :, 11] = PM.OP_INV, 0, 0
    invs[:, :, 16] = rng.integers(0, 2, size=(W, Cs))
    # the peers' writes took versions 2 (an RMW) or 4 (a plain write) on this fresh table: 0, 2, 3, 4, 6 lie below, at
    # and above them (at an equal version the cid decides: the peer's is larger than ours, 0)
    invs[:, :, 12:16] = rng.choice(np.array([0, 2, 3, 4, 6], "<u4"), size=(W, Cs)).view(np.uint8).reshape(W, Cs, 4)
    ic = _ragged(rng, W, Cs)
    rows = _answer_layouts(WL, g, o, invs, ic, peers, 56, words_dev, words, rnd, rng)
    live = rows[rows[:, 8] != FILL]
    n_ab, n_ack = int((live[:, 8] == PM.OP_INV_ABORT).sum()), int((live[:, 8] == PM.OP_ACK).sum())
    assert n_ab > 100 and n_ack > 100 and n_ab + n_ack == len(live), (n_ab, n_ack, len(live))
    # an RMW INV of version 0 on a key of S0 is below the peer's word of the round before: only the round tag makes
    # its answer an ACK
    sent = (np.arange(Cs)[None, :] < ic[:, None]) & np.isin(k.reshape(W, Cs), S0) & (invs[:, :, 16] == 1) & \
        (invs[:, :, 12:16] == 0).all(axis=2)
    assert sent.sum() > 10
    for w, j in np.argwhere(sent)[:10]:
        x = invs[w, j]
        pw = int(words[(o.lookup(PM.key_of(x)) // 64) * 8 + peers[-1]])
        assert pw >> 41 == PM.round_tag(rnd - 1) and (pw & 0xFFFFFFFFFF) > 0
        y = rows[w * Cs * len(peers) + j * len(peers) + len(peers) - 1]
        assert y[8] == PM.OP_ACK and y[9] == peers[-1] and np.array_equal(y[:8], x[:8])
    ab = live[live[:, 8] == PM.OP_INV_ABORT]
    assert np.isin(ab[:, :8].copy().view("<u8").reshape(-1), S1).all() and (ab[:, 9] == ab[:, 11]).all()


# ----------------------------------------------------------------------------------------------------- Round
def _bench_round(monkeypatch, inline):
    """the bench round of test_whole_round_checked_once_per_step under a deferred Mirror that never exports"""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.workload import Round, zipf_params
    c = PC.ROUND
    if not inline:
        monkeypatch.setenv("HKV_INLINE", "0")
    g = HermesKV(c["n_keys"], c["bkts"], c["cap"], machine_id=0, skew=3)
    o = OracleKVS(c["bkts"], c["cap"], 0, skew=3)
    o.populate(c["n_keys"], g.sizes.kvs_value)
    m = Mirror(g, o, f"round inline={inline}", table_check="deferred", expect_inline=inline)
    r = Round(g, c["W"], L.membership(3, 0), c["peers"], zipf_params(c["n_keys"], c["theta"]), c["write_pm"],
              seed=PC.SEED, max_steps=c["max_steps"], trace_len=c["trace_len"], retry_stalled=True)
    assert r.inline == inline and r.fused and r.pack_remote
    return g, o, m, r


def _next_slab(r, o, slabs):
    """(device INVs, device VALs, model INVs, model VALs) of the slab the next step applies, the model's stamped
    from the twin as it stands"""
    k = r.clock % len(r.remote_packed)
    pi, pv, _, total, _, _ = r.remote_packed[k]
    model = slabs[k]
    assert total == len(model)
    ver, phys = PM.peer_versions(o, model)
    want_i = PM.stamp(model, PM.OP_INV, ver)
    want_v = PM.stamp(model[:, :16], PM.OP_VAL, ver)
    return _host(pi)[:total * 56].reshape(-1, 56).copy(), _host(pv)[:total * 16].reshape(-1, 16).copy(), want_i, want_v, \
        ver, phys


@pytest.mark.parametrize("inline", [True, False])
def test_round_stamps_the_next_slab_from_the_live_table(inline, monkeypatch):
    """After every step the packed slab the next round applies (remote_packed[clock % n]) carries peer_versions of
    the twin as it stands: the generator, the packing and the merged end-of-step stamping against the model, on a
    table that is never exported -- INLINE, the inline keys' log copies are stale from the first step on."""
    c = PC.ROUND
    g, o, m, r = _bench_round(monkeypatch, inline)
    keys = gen_keys(c["n_keys"])
    slabs = PC.round_slabs(keys)
    log0 = o.log_bytes()[:c["cap"]].copy()      # the image the table is converted with
    _, _, _, _, inline_keys, _ = C.census(o.index_bytes().copy(), log0, c["cap"])
    moved_inline = 0
    for step in range(c["steps"]):
        r.step()
        gi, gv, want_i, want_v, ver, phys = _next_slab(r, o, slabs)
        _same(gi, want_i, f"step {step}: the next slab's INVs")
        _same(gv, want_v, f"step {step}: the next slab's VALs")
        il = np.isin(want_i[:, :8].copy().view("<u8").reshape(-1), inline_keys)
        v0 = log0[np.maximum(phys, 0)[:, None] + np.arange(24, 28)[None, :]].copy().view("<u4").reshape(-1)
        moved_inline += int((il & (phys >= 0) & (ver - 2 != v0)).sum())
        assert g.layout()["state"] == (INLINE if inline else LOG)
    assert m.launches == c["steps"] * 5     # local, one INV launch per peer, the ACK rows launch, VAL
    assert moved_inline >= 100, moved_inline
    lay = g.layout()
    assert lay["conversions"] == (1 if inline else 0), lay
    assert r.stats()["committed"] > 0 and g.take_error_flags() == 0


def test_round_restamps_after_a_write_between_steps(monkeypatch):
    """The end-of-step launch stamps the next round's timestamps a round early. A launch on the table between two
    steps (here PUTs on keys of the next slab, mirrored on the twin) makes them stale: the step must read them again,
    so its INV launches carry the live table's versions. Back-to-back steps do not repeat the stamping."""
    c = PC.ROUND
    g, o, m, r = _bench_round(monkeypatch, True)
    slabs = PC.round_slabs(gen_keys(c["n_keys"]))
    stamps, carried = [], []
    pts, local = r.peer_timestamps_packed, r.local_batch

    def counted(k, n_peers=None):
        stamps.append(r.clock)
        pts(k, n_peers)

    def snap():   # the slab as the step's INV launches will carry it
        pi, _, _, total, _, _ = r.remote_packed[r.clock % len(r.remote_packed)]
        carried.append(_host(pi)[:total * 56].reshape(-1, 56).copy())
        local()
    r.peer_timestamps_packed, r.local_batch = counted, snap
    r.step()
    r.step()
    assert stamps == [0] and m.launches == 10    # the first step has no refill before it; the second reuses its stamps
    gi, _, cached, _, _, _ = _next_slab(r, o, slabs)
    _same(gi, cached, "the slab stamped at the end of the step")
    # PUTs on 200 keys of the next slab, through the table's own batch path (and the Mirror, so the twin follows)
    ks = np.unique(cached[:, :8].copy().view("<u8").reshape(-1))[:200]
    ops = np.zeros(len(ks), dtype=L.op_dtype())
    ops["key"], ops["opcode"], ops["state"], ops["val_len"] = ks, int(L.Op.PUT), int(L.Bucket.NEW), g.sizes.st_value
    ops["value"] = ord("z")
    t = _dev(ops.view(np.uint8).reshape(-1).copy())
    g.batch(L.BatchType.local_ops, t, 1, len(ks), 56, L.membership(3, 0))
    torch.cuda.synchronize()
    assert (_host(t).reshape(-1, 56)[:, 9] == int(L.Resp.PUT_SUCCESS)).sum() > 100
    _, _, live, _, _, _ = _next_slab(r, o, slabs)
    assert ((live != cached).any(axis=1)).sum() > 100, "the PUTs raised no version of the slab"
    launches = m.launches
    r.step()
    assert stamps == [0, 2], "the step after the write did not read the timestamps again"
    _same(carried[-1], live, "the INVs the step after the write carried")
    assert m.launches == launches + 5
    r.step()
    assert stamps == [0, 2] and m.launches == launches + 10
    assert g.take_error_flags() == 0
