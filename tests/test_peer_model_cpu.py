"""tests/peer_model.py is not vacuous, and the exact comparisons of tests/test_virtual_peers_gpu.py are safe.

* The model's Zipf has the shape of Gray's generator: the shares of ids 0 and 1 and of PUTs are within 4 binomial
  standard deviations of 1/zetan, (half_pow - 1)/zetan and the write fraction; every branch of the draw is hit at
  its thresholds.
* No power-law draw the GPU module compares exactly lies within 1e-10 (relative) of an integer: device pow, a
  contracted eta*u - eta + 1 and alpha = 100 move the value by about 1e-14, so no draw can fall on the other side.
* The dedup of the peer rounds keeps each (peer, id) pair's first draw, and drops enough to be exercised.
* The CPU baseline's generators (oracle/hkv_oracle_bench.c), which bench.py's cpu_baseline leg calls "the same
  generators", equal the model byte for byte (the op's pad after an INV's value apart, which the baseline leaves zero).
* On the oracle alone, the peers' own writes move the versions of inline keys that later slabs of the Round check
  name, so a version read from an inline key's stale log copy is a wrong one there.
"""
import math

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle import cpu_baseline as CB
from oracle.oracle import OracleKVS, gen_keys
from tests import inline_cases as C
from tests import peer_cases as PC
from tests import peer_model as PM


def _within(share, p, n, what):
    sd = math.sqrt(p * (1 - p) / n)
    print(f"{what}: {share:.4f} against {p:.4f} (sd {sd:.4f})")
    assert abs(share - p) <= 4 * sd, what


@pytest.mark.parametrize("n", [3000, 60000])
def test_zipf_shape(n):
    z = PM.zipf_params(n, 0.99)
    _, op, ids = PM.gen_trace(40, 1024, z, 200, 0, PC.SEED, gen_keys(n))
    N = len(ids)
    _within(float((ids == 0).mean()), 1 / z.zetan, N, "id 0")
    _within(float((ids == 1).mean()), (z.half_pow - 1) / z.zetan, N, "id 1")
    _within(float((op == PM.OP_PUT).mean()), 0.2, N, "PUT")
    assert set(np.unique(op).tolist()) == {PM.OP_GET, PM.OP_PUT} and ids.max() < n
    # the power law falls: the ids below n/100 take most of the draws
    assert (ids < n // 100).mean() > 0.4


def test_zipf_params_against_the_product():
    """the model's constants are bit for bit the ones Round hands the device (hermes_amd.workload.zipf_params): the
    Round checks of the GPU module feed the device the product's and the model its own"""
    from hermes_amd.workload import zipf_params
    for n, theta in [(3, 0.99), (3000, 0.99), (60000, 0.99), (1_000_000, 0.99), (3000, 0.0)]:
        a, b = PM.zipf_params(n, theta), zipf_params(n, theta)
        for f in PM.Zipf._fields:
            assert getattr(a, f) == getattr(b, f), (n, theta, f)


def test_zipf_thresholds():
    for n in (3, 3000):
        z = PM.zipf_params(n, 0.99)
        t1, t2 = 1 / z.zetan, z.half_pow / z.zetan
        below = lambda x: np.nextafter(np.nextafter(x, 0.0), 0.0)   # noqa: E731  (two ulps: u * zetan rounds)
        above = lambda x: np.nextafter(np.nextafter(x, 1.0), 1.0)   # noqa: E731
        u = np.array([0.0, below(t1), above(t1), below(t2), above(t2), np.nextafter(1.0, 0.0)])
        assert PM.zipf_branch(z, u).tolist() == [1, 1, 2, 2, 3, 3]
        ids = PM.zipf_draw(z, u)
        assert ids[:4].tolist() == [0, 0, 1, 1]
        assert 1 <= ids[4] <= 2 and ids[4] < n      # the power law starts where the two hottest ids end
        assert ids[5] == n - 1                      # the largest u: n * 1^alpha = n, clamped
    z3 = PM.zipf_params(3, 0.99)
    got = set(PM.zipf_draw(z3, PM.unit_double(PM.trace_randoms(3, 100, PC.SEED)[0])).tolist())
    assert got == {0, 1, 2}
    # theta = 0: uniform, floor(u * n), clamped
    zu = PM.zipf_params(8, 0.0)
    assert PM.zipf_draw(zu, np.array([0.0, 0.124, 0.125, 0.99999, np.nextafter(1.0, 0.0)])).tolist() == [0, 0, 1, 7, 7]
    ids = PM.zipf_draw(PM.zipf_params(3000, 0.0), PM.unit_double(PM.trace_randoms(8, 256, PC.SEED)[0]))
    assert ids.max() < 3000 and len(np.unique(ids)) > 1400


@pytest.mark.parametrize("n", [3, 3000, 60000, 1_000_000])
def test_second_branch_is_a_shortcut_of_the_power_law(n):
    """Gray's generator is continuous at its thresholds: over [1/zetan, half_pow/zetan) the power law runs from
    about 1.1 to 2, so it truncates to id 1 as the `uz < half_pow` branch answers. A draw without that branch
    (only slower) is therefore no wrong draw, and no test of ids can tell the two apart; the `uz < 1` branch is not
    one (the power law gives more than 1 below 1/zetan as well, where the id is 0). At half_pow/zetan the power
    law passes 2: the two agree there too."""
    z = PM.zipf_params(n, 0.99)
    lo, hi = 1 / z.zetan, z.half_pow / z.zetan
    u = np.linspace(lo, hi, 20001)[:-1]
    x = PM.zipf_power(z, u)
    print(n, float(x.min()), float(x.max()))
    assert x.min() > 1.05 and x.max() < 2.0 and (np.diff(x) > 0).all()
    assert PM.zipf_power(z, np.array([np.nextafter(lo, 0.0)]))[0] > 1.05
    assert abs(PM.zipf_power(z, np.array([hi]))[0] - 2.0) < 1e-6


def test_splitmix64_known_answers():
    """Vigna's splitmix64.c from state 0: the first outputs of the published generator"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(PM.splitmix64(np.uint64((k * 0x9E3779B97F4A7C15) & PM.M64))[0]) for k in range(3)]
    assert got == want
    assert PM.unit_double(np.uint64(PM.M64)) == np.nextafter(1.0, 0.0) and PM.unit_double(np.uint64(0)) == 0.0


def test_rounding_margin():
    """Exact equality is asked of the device: every power-law draw compared there is at least 1e-10 (relative)
    from an integer. A seed or shape that fails this is replaced, never given a tolerance."""
    draws = PC.all_draws()
    c = PC.ROUND   # the Round check's own trace and peer rounds, and the baseline comparison below
    z = PM.zipf_params(c["n_keys"], c["theta"])
    shape = (c["W"], c["per_peer"], len(c["peers"]))
    for k in range(c["max_steps"]):
        draws.append((f"Round peers {k}", z, PC.peer_units(*shape, k, PC.round_peer_seed())))
    for n in (3000, 60000):
        for k in range(CB.BENCH_PEER_ROUNDS):
            draws.append((f"baseline peers n={n} round {k}", PM.zipf_params(n, 0.99), PC.peer_units(*shape, k, PC.SEED)))
        draws.append((f"baseline trace n={n}", PM.zipf_params(n, 0.99), PM.unit_double(PM.trace_randoms(40, 1024, PC.SEED)[0])))
    for what, z, u in draws:
        m = PC.power_law_margin(z, u)
        print(f"{what}: {m:.3g}")
        assert m >= 1e-10, what


def test_peer_round_dedup_properties():
    W, P, R, n = 40, 50, 2, 3000
    z = PM.zipf_params(n, 0.99)
    ids, flags, keep = PM.peer_draws(W, P, R, z, 0, 0, PC.SEED)
    invs, vals, counts = PM.gen_peer_round(W, P, [1, 2], 56, 31, 0, z, 0, 0, PC.SEED, gen_keys(n), fill=0xA5)
    assert counts.sum() == keep.sum() and not flags.any()
    dropped = 1 - keep.mean()
    print(f"dropped {dropped:.3f}")
    assert dropped >= 0.20
    order = np.arange(W)[:, None] * P + np.arange(P)[None, :]
    for r in range(R):
        kept = ids[:, r][keep[:, r]]
        assert len(np.unique(kept)) == len(kept), "a key twice for one peer"
        first = {int(i): int(o) for i, o in zip(kept, order[keep[:, r]])}
        d_ids, d_ord = ids[:, r][~keep[:, r]], order[~keep[:, r]]
        assert all(first[int(i)] < int(o) for i, o in zip(d_ids, d_ord)), "a dropped draw without an earlier kept one"
    # per worker: peer 1's INVs, then peer 2's, then the caller's bytes
    tot = counts.sum(axis=1)
    for w in range(W):
        assert (invs[w, :counts[w, 0], 9] == 1).all() and (invs[w, counts[w, 0]:tot[w], 9] == 2).all()
        assert (invs[w, tot[w]:] == 0xA5).all() and (vals[w, tot[w]:] == 0xA5).all()
        assert (vals[w, :tot[w], 8] == PM.OP_VAL).all() and (vals[w, :tot[w], :8] == invs[w, :tot[w], :8]).all()
    # another round index draws other keys; the RMW flag is drawn per element
    ids5, _, _ = PM.peer_draws(W, P, R, z, 0, 5, PC.SEED)
    assert (ids5 != ids).mean() > 0.5
    _, f, _ = PM.peer_draws(W, P, R, z, 500, 0, PC.SEED)
    assert 0.4 < f.mean() < 0.6


@pytest.mark.parametrize("n", [3000, 60000])
def test_cpu_baseline_generators_equal_the_model(n):
    """hko_bench_rounds' trace and peer-round loops (now hko_bench_gen_trace / hko_bench_gen_peer_rounds): the
    baseline's shape is peers 1 + r, no RMW flags, 16 round indices, default sizes. One difference is modelled, not
    hidden: the baseline writes the value's 31 bytes and leaves the op's 7 pad bytes zero, the device fills them;
    no batch reads past val_len."""
    z = PM.zipf_params(n, 0.99)
    keys = gen_keys(n)
    W, R, P = 40, 2, 50
    key, op, ids = CB.bench_gen_trace(z, W, 1024, 200, PC.SEED)
    mk, mo, mi = PM.gen_trace(W, 1024, z, 200, 0, PC.SEED, keys)
    assert np.array_equal(ids, mi) and np.array_equal(key, mk) and np.array_equal(op, mo)
    s = L.DEFAULT
    invs, vals, counts = CB.bench_gen_peer_rounds(z, W, R, P, CB.BENCH_PEER_ROUNDS, s.op, s.st_value, PC.SEED)
    pad = L.OP_VALUE_OFF + s.st_value       # the baseline leaves the op's pad after the value zero, the device fills it
    for k in range(CB.BENCH_PEER_ROUNDS):
        mi_, mv, mc = PM.gen_peer_round(W, P, [1, 2], s.op, s.st_value, s.shift, z, 0, k, PC.SEED, keys, fill=0)
        assert (mi_[:, :, pad:][mi_[:, :, 8] == PM.OP_INV] != 0).all() and not invs[k][:, :, pad:].any()
        mi_[:, :, pad:] = 0
        assert np.array_equal(counts[k], mc.sum(axis=1)), f"round {k}: counts"
        assert np.array_equal(invs[k], mi_), f"round {k}: INVs"
        assert np.array_equal(vals[k], mv), f"round {k}: VALs"
    assert not np.array_equal(invs[0], invs[5])


def test_peer_versions_on_the_oracle():
    """the +2 / +4 steps, absent keys and tag collisions, on a table whose versions differ"""
    for rmw in (False, True):
        o = C.make_oracle("A", rmw=rmw)
        T = C.describe(o, "A")
        K, M, fakes = C.collision_keys(T)
        log = o.log_bytes()
        present = T.keys[T.present][:6]
        for i, k in enumerate(present):     # versions 0, 10, 20, ...
            log[o.lookup(int(k)) + 24:o.lookup(int(k)) + 28] = np.frombuffer((10 * i).to_bytes(4, "little"), np.uint8)
        ks = np.concatenate([present, T.keys[~T.present][:2], fakes])
        invs = np.zeros((len(ks), 56), np.uint8)
        invs[:, :8] = ks.view(np.uint8).reshape(-1, 8)
        invs[:, 9] = invs[:, 11] = 1
        invs[::2, 16] = 1                   # RMW flag on every other INV
        ver, phys = PM.peer_versions(o, invs)
        step = [2 if (not rmw or i % 2 == 0) else 4 for i in range(6)]
        assert ver.tolist() == [10 * i + step[i] for i in range(6)] + [2, 2, 2, 2]
        assert (phys[:6] >= 0).all() and (phys[6:] == -1).all()
        out = PM.stamp(invs, PM.OP_INV, ver)
        assert (out[:, 8] == PM.OP_INV).all() and np.array_equal(out[:, 12:16].copy().view("<u4").reshape(-1), ver)
        keep = np.ones(56, bool)
        keep[[8, 12, 13, 14, 15]] = False
        assert np.array_equal(out[:, keep], invs[:, keep])
        if rmw:
            w = PM.peer_ts_words(np.zeros(8 * (T.cap // 64 + 1), np.uint64), invs, ver, phys, 64, 4)
            i = (int(phys[1]) // 64) * 8 + 1
            assert int(w[i]) == (5 << 41) | (0 << 40) | (14 << 8) | 1 and np.count_nonzero(w) == 6
            # peer 1's answer to a local RMW INV below / above its word, and with the word of another round
            x = np.zeros(56, np.uint8)
            x[:8] = invs[1, :8]
            x[8], x[9], x[10], x[11], x[16], x[17] = PM.OP_INV, 0, 31, 0, 1, 2
            x[12:16] = np.frombuffer((14).to_bytes(4, "little"), np.uint8)   # (14, 0) < (14, 1)
            y = PM.peer_answer(x, 1, 56, oracle=o, words=w, rnd=4)
            assert y[8] == PM.OP_INV_ABORT and y[9] == 1 and y[11] == 1 and y[16] == 0 and y[17] == 2
            assert int.from_bytes(bytes(y[12:16]), "little") == 14 and (y[18:] == ord("b")).all()
            assert PM.peer_answer(x, 1, 56, oracle=o, words=w, rnd=5)[8] == PM.OP_ACK   # an older round's word
            x[12] = 16
            y = PM.peer_answer(x, 1, 56, oracle=o, words=w, rnd=4)
            assert y[8] == PM.OP_ACK and y[9] == 1 and np.array_equal(y[:8], x[:8]) and (y[16:] == 0).all()


def test_ack_offsets_model():
    off, total, mx = PM.ack_offsets([3, 0, 5], 2)
    assert off.tolist() == [0, 6, 6, 16] and total == 16 and mx == 5


def test_round_check_has_moving_inline_keys():
    """The Round check of the GPU module, on the oracle alone and with the peers' writes only (the local writes
    of the real round move more): after each round's slab is applied, the next slab names inline keys whose
    version is no longer the one the table was converted with."""
    c = PC.ROUND
    o = OracleKVS(c["bkts"], c["cap"], 0)
    o.populate(c["n_keys"], L.DEFAULT.kvs_value)
    keys = gen_keys(c["n_keys"])
    _, _, _, _, inline_keys, _ = C.census(o.index_bytes().copy(), o.log_bytes()[:c["cap"]].copy(), c["cap"])
    slabs = PC.round_slabs(keys)
    mb = L.membership(3, 0)
    v0 = {}
    moved = []
    for k in range(c["steps"]):
        invs = slabs[k % len(slabs)]
        kk = invs[:, :8].copy().view("<u8").reshape(-1)
        il = np.isin(kk, inline_keys)
        ver, phys = PM.peer_versions(o, invs)
        for key, v in zip(kk.tolist(), (ver - 2).tolist()):
            v0.setdefault(key, v)
        moved.append(int(sum(il[i] and phys[i] >= 0 and int(ver[i]) - 2 != v0[int(kk[i])] for i in range(len(kk)))))
        n = len(invs)
        nb = (n + 249) // 250
        e = np.zeros((nb * 250, 56), np.uint8)
        e[:n] = PM.stamp(invs, PM.OP_INV, ver)
        cnt = np.minimum(250, n - 250 * np.arange(nb)).astype(np.int32)
        ev = e.reshape(-1).view(np.dtype((np.void, 56))).copy()
        o.batch_multi(int(L.BatchType.invs), ev, nb, 250, cnt, mb)
        assert (ev.view(np.uint8).reshape(-1, 56)[:n, 8] == int(L.Resp.INV_SUCCESS)).mean() > 0.9
    print("inline keys with a moved version per slab:", moved)
    assert moved[0] == 0 and all(m >= 20 for m in moved[1:]), moved
