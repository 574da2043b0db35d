"""The serial-order checker (tests/serial_order.py) against histories whose answer is known.

The history maker restates the thread programs of `capi_threads contend` (tools/capi_threads.c) on an
OracleKVS: five workers (a 250-op local batch, half of it on 48 hot keys, then the peers' ACKs of its
own writes), two peers (64 INVs on hot keys, then the VALs of their previous round's INVs) and a
bulk sender (300 INVs on one hot key, every fourth round 4,200 over the hot keys). A random scheduler
starts a thread's call, applies it to the oracle and ends it as three separate steps, so a call's
interval contains its linearisation point and overlaps other threads' calls.

The checker must find an order for such a history within 4*T*N applications, and must rule out --
by exhausting the search, not by hitting that cap -- the same history with a stale read, a torn
call, a lost update or a real-time violation put into it.
"""
import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import gen
from tests.serial_order import Call, NoSerialOrder, call_keys, contention, find_serial_order

T, HOT, NKEYS, ROUNDS = 8, 48, 20_000, 30
LOCAL, INVS, ACKS, VALS = (int(L.BatchType.local_ops), int(L.BatchType.invs), int(L.BatchType.acks),
                           int(L.BatchType.vals))
MB = L.membership(3, 0)
BARRIER = "barrier"
WANTED = {(LOCAL, int(L.Resp.GET_COMPLETE)), (LOCAL, int(L.Resp.GET_STALL)), (LOCAL, int(L.Resp.PUT_SUCCESS)),
          (LOCAL, int(L.Resp.PUT_STALL)), (ACKS, int(L.Resp.ACK_SUCCESS)), (ACKS, int(L.Resp.LAST_ACK_SUCCESS)),
          (INVS, int(L.Resp.INV_SUCCESS)), (VALS, int(L.Resp.VAL_SUCCESS))}


def fresh_oracle():
    o = OracleKVS(1 << 15, 2 << 20, machine_id=0)
    o.populate(NKEYS, L.DEFAULT.kvs_value)
    return o


def _values(a, who, r):
    """31 value bytes that name their writer: (thread, round, index)"""
    n = len(a)
    v = np.full((n, 31), ord("a") + who, np.uint8)
    v[:, 0], v[:, 1], v[:, 2], v[:, 3] = who, r, np.arange(n) & 255, np.arange(n) >> 8
    return v


def _worker(k, rng, keys, rounds):
    for r in range(rounds):
        ops = np.zeros(250, L.op_dtype())
        ids = np.where(rng.random(250) < 0.5, rng.integers(0, HOT, 250), rng.integers(0, NKEYS, 250))
        put = rng.random(250) < 0.3
        ops["key"], ops["state"] = keys[ids], int(L.Bucket.NEW)
        ops["opcode"] = np.where(put, int(L.Op.PUT), int(L.Op.GET))
        ops["val_len"] = np.where(put, 31, 0)
        ops["value"] = np.where(put[:, None], _values(ops, k, r), 0)
        yield LOCAL, ops, None
        won = np.flatnonzero(ops["state"] == int(L.Resp.PUT_SUCCESS))
        if len(won):
            ops["state"][won] = int(L.Bucket.IN_PROGRESS_PUT)   # inv_modify_elem_after_send
            acks = np.zeros(2 * len(won), L.msg_dtype())
            acks["key"] = np.repeat(ops["key"][won], 2)
            acks["opcode"] = int(L.Op.ACK)
            acks["sender"] = np.tile(np.array([1, 2], np.uint8), len(won))
            acks["ts_cid"] = np.repeat(ops["ts_cid"][won], 2)
            acks["ts_ver"] = np.repeat(ops["ts_ver"][won], 2)
            yield ACKS, acks, ops
        if r == rounds // 2:
            yield BARRIER


def _invs(n, ids, keys, sender, rng, who, r):
    a = np.zeros(n, L.op_dtype())
    a["key"], a["opcode"], a["state"], a["ts_cid"] = keys[ids], int(L.Op.INV), sender, sender
    a["ts_ver"] = 2 * rng.integers(0, r + 3, n)
    a["val_len"], a["value"] = 31, _values(a, who, r)
    return a


def _peer(k, rng, keys, rounds):
    prev = None
    for r in range(rounds):
        a = _invs(64, rng.integers(0, HOT, 64), keys, k - 4, rng, k, r)
        sent = gen.bytecopy(a)
        yield INVS, a, None
        if prev is not None:
            v = np.zeros(len(prev), L.msg_dtype())
            v["key"], v["opcode"], v["sender"] = prev["key"], int(L.Op.VAL), prev["ts_cid"]
            v["ts_cid"], v["ts_ver"] = prev["ts_cid"], prev["ts_ver"]
            yield VALS, v, None
        prev = sent
        if r == rounds // 2:
            yield BARRIER


def _bulk(k, rng, keys, rounds):
    for r in range(rounds):
        if r % 4 != 3:
            a = _invs(300, np.full(300, rng.integers(0, HOT)), keys, 1 + r % 2, rng, k, r)
        else:
            a = _invs(4200, rng.integers(0, HOT, 4200), keys, 1 + r % 2, rng, k, r)
        yield INVS, a, None
        if r == rounds // 2:
            yield BARRIER


def make_history(seed, rounds=ROUNDS):
    """(calls, true order as (thread, call) pairs, final log) of one scheduled run on a fresh oracle"""
    rng = np.random.default_rng(seed)
    keys = gen_keys(NKEYS)
    o = fresh_oracle()
    progs = [(_worker if k < 5 else _peer if k < 7 else _bulk)(k, np.random.default_rng([seed, k]), keys, rounds)
             for k in range(T)]
    calls = [[] for _ in range(T)]
    order, now = [], 0
    state = ["idle"] * T       # idle -> started -> applied -> idle; or waiting at the barrier; or done
    cur = [None] * T
    while any(s != "done" for s in state):
        runnable = [k for k in range(T) if state[k] not in ("done", BARRIER)]
        if not runnable:       # everyone is at the barrier (or done): the idle gap
            state = ["idle" if s == BARRIER else s for s in state]
            continue
        k = int(rng.choice(runnable))
        if state[k] == "idle":
            nxt = next(progs[k], None)
            if nxt is None:
                state[k] = "done"
            elif nxt == BARRIER:
                state[k] = BARRIER
            else:
                t, a, rw = nxt
                cur[k] = (t, a, rw, gen.bytecopy(a), gen.bytecopy(rw) if rw is not None else None, now)
                now += 1
                state[k] = "started"
        elif state[k] == "started":
            t, a, rw = cur[k][:3]
            o.batch(t, a, MB, rw=rw)
            order.append((k, len(calls[k])))
            state[k] = "applied"
        else:
            t, a, rw, ain, rwin, start = cur[k]
            u8 = lambda x: None if x is None else x.view(np.uint8).reshape(-1).copy()  # noqa: E731
            calls[k].append(Call(t, len(a), a.dtype.itemsize, u8(ain), u8(a), u8(rwin), u8(rw), start, now))
            now += 1
            state[k] = "idle"
    return calls, order, o.log_bytes().copy()


def sequential(calls, order):
    """the same calls with times that allow the true order only"""
    out = [list(c) for c in calls]
    for i, (k, c) in enumerate(order):
        out[k][c] = out[k][c]._replace(start=2 * i, end=2 * i + 1)
    return out


@pytest.fixture(scope="module")
def hist():
    return make_history(1)


@pytest.fixture(scope="module")
def walk(hist):
    """The true order replayed once: per call, the entries of its hot keys before and after it."""
    calls, order, _ = hist
    o = fresh_oracle()
    log = o.log_bytes()
    hot = {int(key): o.lookup(int(key)) for key in gen_keys(NKEYS)[:HOT]}
    steps = []
    for k, c in order:
        call = calls[k][c]
        keys = sorted(set(np.ascontiguousarray(call.ein.reshape(-1, call.esz)[:, :8]).view("<u8").reshape(-1).tolist())
                      & hot.keys())
        before = {key: log[hot[key]:hot[key] + 64].copy() for key in keys}
        e = gen.bytecopy(call.ein.view(np.dtype((np.void, call.esz))))
        rw = gen.bytecopy(call.rin.view(np.dtype((np.void, 56)))) if call.rin is not None else None
        o.batch(call.type, e, MB, rw=rw)
        assert np.array_equal(e.view(np.uint8).reshape(-1), call.eout)
        steps.append((k, c, before, {key: log[hot[key]:hot[key] + 64].copy() for key in keys}))
    return steps, hot


def _rejected(calls, final_log=None):
    with pytest.raises(NoSerialOrder) as ei:
        find_serial_order(calls, fresh_oracle(), MB, final_log)
    print(str(ei.value)[:2000])
    assert ei.value.exhausted, "the cap was hit: the history was not shown to have no order"
    assert ei.value.diffs
    return ei.value


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_finds_an_order_within_the_cap(seed, hist):
    """Largest figure observed over seeds 1-4 at ROUNDS 30 (448 calls): see MEASURED below; the cap is
    32 applications per call (4*T*N).

    MEASURED: 3.9 applications per call at most (seed 1: 1,744 of a cap of 14,336; seeds 2-4: 1,213, 1,120,
    1,120), 0.3-0.5 s each. Exhausting the whole space of seed 1's history (the lost update) took 6,130."""
    calls, order, final_log = hist if seed == 1 else make_history(seed)
    n = sum(len(c) for c in calls)
    got, applications = find_serial_order(calls, fresh_oracle(), MB, final_log)   # the cap is the default, 4*T*N
    print(f"seed {seed}: {n} calls, {applications} applications, {applications / n:.2f} per call, cap {4 * T * n}")
    assert len(got) == n and applications <= 4 * T * n
    for k in range(T):
        assert [c for j, c in got if j == k] == list(range(len(calls[k])))


def test_sequential_times_take_one_application_per_call(hist):
    calls, order, final_log = hist
    got, applications = find_serial_order(sequential(calls, order), fresh_oracle(), MB, final_log)
    assert got == order and applications == len(order)


def test_history_is_contended(hist):
    share, seen = contention(hist[0])
    print(f"{share:.2f} of the calls overlap a call of another thread that shares a key")
    assert share > 0.5
    assert WANTED <= seen, sorted(WANTED - seen)


def _with_output(calls, k, c, eout):
    out = [list(x) for x in calls]
    out[k][c] = out[k][c]._replace(eout=eout)
    return out


def test_rejects_a_stale_read(hist, walk):
    """One GET_COMPLETE on a hot key returns a value that key held earlier, overwritten by a call that
    had ended before the reading call started (values name their writer, so it never comes back)."""
    calls, order, final_log = hist
    steps, hot = walk
    held = {}   # hot key -> [(value, end of the call that wrote it)], oldest first
    for k, c, before, after in steps[:len(steps) // 3]:
        call = calls[k][c]
        for key in before:
            held.setdefault(key, [(before[key][33:64].tobytes(), -1)])
        if call.type == LOCAL:
            out = call.eout.reshape(call.n, 56)
            for i in np.flatnonzero((out[:, 8] == int(L.Op.GET)) & (out[:, 9] == int(L.Resp.GET_COMPLETE))).tolist():
                key = int(out[i, :8].copy().view("<u8")[0])
                vals = held.get(key, [])
                if len(vals) >= 2 and vals[-1][0] == out[i, 18:49].tobytes() and vals[-1][1] < call.start:
                    eout = call.eout.copy()
                    eout[i * 56 + 18:i * 56 + 49] = np.frombuffer(vals[-2][0], np.uint8)
                    print(f"stale: thread {k} call {c} element {i} returns the value before {vals[-1][0][:4].hex()}")
                    _rejected(_with_output(calls, k, c, eout), final_log)
                    return
        for key in after:
            v = after[key][33:64].tobytes()
            if held[key][-1][0] != v:
                held[key].append((v, call.end))
    pytest.fail("no GET_COMPLETE on a hot key that had changed")


def test_rejects_a_torn_call(hist, walk):
    """Call A is an INV batch raising hot keys k1 and k2; call B reads both and is made to show k1
    as it was before A and k2 as A left it: what a launch split by a stop looks like."""
    calls, order, final_log = hist
    steps, hot = walk
    raised = []   # (value A wrote to k2, k1, k1's valid entry before A) per pair of keys an INV batch raised
    for k, c, before, after in steps[:len(steps) // 2]:
        call = calls[k][c]
        if call.type == INVS:
            up = [key for key in after if after[key][23:28].tobytes() != before[key][23:28].tobytes()]
            raised += [(after[k2][33:64].tobytes(), k2, k1, before[k1]) for k1 in up for k2 in up
                       if k1 != k2 and before[k1][18] == int(L.State.VALID)]
        elif call.type == LOCAL:
            out = call.eout.reshape(call.n, 56)
            gets = {int(out[i, :8].copy().view("<u8")[0]): i for i in np.flatnonzero(out[:, 8] == int(L.Op.GET)).tolist()}
            puts = {int(out[i, :8].copy().view("<u8")[0]) for i in np.flatnonzero(out[:, 8] == int(L.Op.PUT)).tolist()}
            for val2, k2, k1, was in raised:
                if k1 in gets and k2 in gets and k1 not in puts and k2 not in puts and \
                        out[gets[k2], 9] == int(L.Resp.GET_COMPLETE) and out[gets[k2], 18:49].tobytes() == val2:
                    i = gets[k1]
                    eout = call.eout.copy()   # k1 as a GET that met the entry before A returns it
                    eout[i * 56 + 9] = int(L.Resp.GET_COMPLETE)
                    eout[i * 56 + 10] = was[17] - L.OP_META_SIZE
                    eout[i * 56 + 18:i * 56 + 49] = was[33:64]
                    assert not np.array_equal(eout, call.eout)
                    print(f"torn: thread {k} call {c} shows element {i} before and element {gets[k2]} after the "
                          f"INV batch that wrote {val2[:4].hex()}")
                    _rejected(_with_output(calls, k, c, eout), final_log)
                    return
    pytest.fail("no local batch reads two keys that one INV batch raised")


def test_rejects_a_lost_update(hist, walk):
    """every output is as recorded, but a raised hot key's entry in the final log is its previous image"""
    calls, order, final_log = hist
    steps, hot = walk
    for k, c, before, after in reversed(steps):
        for key in after:
            if after[key][23:28].tobytes() != before[key][23:28].tobytes():   # the key's last raise
                bad = final_log.copy()
                bad[hot[key]:hot[key] + 64] = before[key]
                _rejected(calls, bad)
                return
    pytest.fail("no key was raised")


def test_rejects_a_real_time_violation(hist):
    """sequential times in the true order, with the time slots of two adjacent calls that do not commute
    (a local batch and an INV batch sharing a key) exchanged"""
    calls, order, final_log = hist
    seq = sequential(calls, order)
    for i in range(len(order) - 1):
        (ka, ca), (kb, cb) = order[i], order[i + 1]
        a, b = seq[ka][ca], seq[kb][cb]
        if ka == kb or {a.type, b.type} != {LOCAL, INVS} or call_keys(a).isdisjoint(call_keys(b)):
            continue
        swapped = [list(x) for x in seq]
        swapped[ka][ca] = a._replace(start=b.start, end=b.end)
        swapped[kb][cb] = b._replace(start=a.start, end=a.end)
        # does the oracle itself reject the exchange? replay the exchanged order
        o = fresh_oracle()
        ok = True
        for k, c in order[:i] + [order[i + 1], order[i]]:
            call = calls[k][c]
            e = gen.bytecopy(call.ein.view(np.dtype((np.void, call.esz))))
            rw = gen.bytecopy(call.rin.view(np.dtype((np.void, 56)))) if call.rin is not None else None
            o.batch(call.type, e, MB, rw=rw)
            ok = ok and np.array_equal(e.view(np.uint8).reshape(-1), call.eout)
        if ok:
            continue
        err = _rejected(swapped, final_log)
        assert err.applications <= len(order)
        return
    pytest.fail("no adjacent local and INV batches that do not commute")
