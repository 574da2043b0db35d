"""Inputs of the inline-layout parity tests (tests/test_inline_parity_gpu.py), in one place so that a machine
without a GPU can prove they are not vacuous (tests/test_inline_cases_cpu.py runs every case on the oracle alone).

A case is a script of launches driven through an engine: OracleEngine here, the device-and-Mirror engine in the
GPU module. Later launches are built from earlier results (the ACKs answer the round's own local writes, the VALs
follow the INVs that were applied), so a case cannot be a list of arrays. Every launch names the layout it must
run in as a literal (inline=True / False), written from the launch kind: the GPU engine hands it to the Mirror,
the oracle engine ignores it. A Rec collects, per launch kind, the outcome codes seen on inline keys and on the
others.

Geometries (keys / buckets / log_cap), from the oracle's image after populate. Slots fill from slot 7 downward, so
the inline key -- the key in the bucket's lowest in-use slot -- is the bucket's most recently inserted one, in slot
0 of a full bucket:

  A   3000 /  512 / 2^18   2864 present,  136 absent (evicted or overwritten),  511 inline keys,  123 full buckets
  D  20000 / 2048 / 2^21  15358 present, 4642 absent,                          2048 inline keys, 1574 full buckets
  S   1000 / 1024 / 2^17   1000 present,    0 absent,                           656 inline keys,    0 full buckets
"""
from __future__ import annotations

import dataclasses

import numpy as np

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import gen

GEO = {"A": (3000, 512, 1 << 18), "D": (20000, 2048, 1 << 21), "S": (1000, 1024, 1 << 17)}

MISS = int(L.Resp.MISS)
SUCCESSES = [int(L.Resp.PUT_SUCCESS), int(L.Resp.RMW_SUCCESS), int(L.Resp.REPLAY_SUCCESS)]
# the local elements the batch function skips (hermesKV.c:709-730)
SKIPPED_LOCAL = SUCCESSES + [int(L.Bucket.IN_PROGRESS_PUT), int(L.Bucket.IN_PROGRESS_REPLAY),
                             int(L.Op.MEMBERSHIP_CHANGE), int(L.Resp.PUT_COMPLETE_SEND_VALS)]
MOVED_TO_VALID = 1     # Rec code of a VAL element whose key it moved to VALID (no opcode tells)


def census(index: np.ndarray, log: np.ndarray, cap: int):
    """From the exported image: every bucket's slots, its lowest in-use slot (-1: empty), the inline keys
    (the keys of the entries those slots name), and the census the base geometry promises."""
    slots = index.view("<u8").reshape(-1, 8)
    used = (slots & np.uint64(1)).astype(bool)
    n_used = used.sum(axis=1)
    first = np.where(n_used > 0, used.argmax(axis=1), -1)
    nz = np.nonzero(first >= 0)[0]
    phys = ((slots[nz, first[nz]] >> np.uint64(24)) & np.uint64(cap - 1)).astype(np.int64)
    keys = log[(phys[:, None] + np.arange(8, 16)[None, :])].copy().view("<u8").reshape(-1)
    return slots, first, nz, phys, keys, n_used


@dataclasses.dataclass
class Table:
    """What a case needs to know of a populated table, all from the oracle's image."""
    name: str
    n_keys: int
    bkts: int
    cap: int
    keys: np.ndarray          # gen_keys(n_keys)
    present: np.ndarray       # bool per key: the lookup finds it
    slots: np.ndarray         # [bkts][8]
    first: np.ndarray         # lowest in-use slot per bucket, -1: empty
    n_used: np.ndarray
    inline_buckets: np.ndarray
    inline_keys: np.ndarray   # one per non-empty bucket, in inline_buckets' order
    log: np.ndarray

    def bucket(self, keys):
        return ((np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFFFFFF)) & np.uint64(self.bkts - 1)).astype(np.int64)

    def slot_keys(self, buckets, slot):
        """the keys of the entries that `slot` of each of `buckets` names"""
        phys = ((self.slots[buckets, slot] >> np.uint64(24)) & np.uint64(self.cap - 1)).astype(np.int64)
        return self.log[phys[:, None] + np.arange(8, 16)[None, :]].copy().view("<u8").reshape(-1)

    def is_inline(self, keys):
        return np.isin(keys, self.inline_keys)


def make_oracle(name: str, rmw: bool = False, skew: int = 0, machine_id: int = 0) -> OracleKVS:
    n_keys, bkts, cap = GEO[name]
    o = OracleKVS(bkts, cap, machine_id, rmw, skew=skew)
    o.populate(n_keys, L.DEFAULT.kvs_value)
    return o


def describe(o: OracleKVS, name: str) -> Table:
    n_keys, bkts, cap = GEO[name]
    keys = gen_keys(n_keys)
    present = np.array([o.lookup(int(k)) is not None for k in keys])
    log = o.log_bytes()[:cap].copy()
    slots, first, nz, _, ikeys, n_used = census(o.index_bytes().copy(), log, cap)
    return Table(name, n_keys, bkts, cap, keys, present, slots, first, n_used, nz, ikeys, log)


class Rec:
    """Per launch kind, the outcome codes seen on inline keys and on the others."""

    def __init__(self, inline_keys):
        self.inline_keys = np.asarray(inline_keys)
        self.seen: dict = {}

    def add(self, kind, keys, codes):
        keys, codes = np.asarray(keys), np.asarray(codes)
        il = np.isin(keys, self.inline_keys)
        for flag in (True, False):
            self.seen.setdefault((kind, flag), set()).update(np.unique(codes[il == flag]).tolist())

    def codes(self, kind, inline):
        return self.seen.get((kind, inline), set())


class OracleEngine:
    """Runs a case's launches on the oracle alone, arrays in place."""

    def __init__(self, o: OracleKVS, machine_id: int = 0):
        self.o, self.sizes, self.machine_id = o, L.DEFAULT, machine_id

    def check_table(self, what):
        pass

    def _packed(self, btype, flat, live, off, n_batches, mb, rw, rw_stride, ns):
        """batches back to back in flat [n][esz] (live: the positions that are elements), as rows to the oracle"""
        off = np.asarray(off, np.int64)
        nl = int(off[-1])
        bat = np.repeat(np.arange(n_batches), np.diff(off))
        sel = np.nonzero(live[:nl])[0]
        cnt = np.bincount(bat[sel], minlength=n_batches).astype(np.int32)
        width = max(int(cnt.max()), 1)
        esz = flat.shape[1]
        rows = np.zeros((n_batches, width, esz), np.uint8)
        pos = np.arange(width)[None, :] < cnt[:, None]
        rows[pos] = flat[sel]
        e = rows.reshape(-1).view(np.dtype((np.void, esz))).copy()
        self.o.batch_multi(int(btype), e, n_batches, width, cnt, mb, rw, rw_stride, ns)
        flat[sel] = e.view(np.uint8).reshape(n_batches, width, esz)[pos]

    def launch(self, btype, elems, n_batches, stride, mb, counts=None, offsets=None, rw=None, rw_stride=0, ns=None,
               unique=False, rows=None, vals=False, inline=None):
        esz = elems.dtype.itemsize
        raw = elems.view(np.uint8).reshape(-1, esz)
        if rows is not None:
            n_rows, row_stride, skip = rows
            for r in range(n_rows):
                if r == skip:
                    continue
                flat = raw[r * row_stride:r * row_stride + stride]
                self._packed(btype, flat, flat[:, 8] != 0, offsets, n_batches, mb, rw, rw_stride, None)
        elif offsets is not None:
            self._packed(btype, raw[:stride], np.ones(stride, bool), offsets, n_batches, mb, rw, rw_stride, ns)
        else:
            self.o.batch_multi(int(btype), elems, n_batches, stride, counts, mb, rw, rw_stride, ns)


# ---------------------------------------------------------------------------------------------- batch builders
def cat(parts):
    """np.concatenate that keeps a structured dtype's itemsize (and the pad bytes)"""
    dt = parts[0].dtype
    assert all(p.dtype == dt for p in parts)
    return np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts]).view(dt)


def live_mask(n_batches, stride, counts):
    if counts is None:
        return np.ones(n_batches * stride, bool)
    return (np.arange(stride)[None, :] < np.asarray(counts)[:, None]).reshape(-1)


def key_states(o: OracleKVS, keys) -> np.ndarray:
    """each key's state byte in the oracle's table (0: absent)"""
    log = o.log_bytes()
    out = np.zeros(len(keys), np.uint8)
    for i, k in enumerate(keys):
        off = o.lookup(int(k))
        if off is not None:
            out[i] = log[off + 18]
    return out


def distinct_keys(rng, must, others, n):
    """n distinct keys: all of `must`, the rest drawn from `others`, shuffled"""
    must = np.unique(np.asarray(must, np.uint64))
    extra = np.setdiff1d(np.asarray(others, np.uint64), must)
    take = rng.choice(extra, size=max(n - len(must), 0), replace=False)
    out = np.concatenate([must, take])
    rng.shuffle(out)
    assert len(np.unique(out)) == len(out)
    return out


def split_counts(rng, n, n_batches):
    """ragged batch sizes that add up to n"""
    cuts = np.sort(rng.integers(0, n + 1, size=n_batches - 1))
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int32)


def lay_out(a, counts, packed):
    """`a` holds the batches back to back. packed: as it is, with offsets; else rows [W][max count] with counts.
    Returns (elems, stride, counts, offsets, where): where = a's elements' positions in elems."""
    W = len(counts)
    if packed:
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        return a, len(a), None, off, np.arange(len(a))
    M = max(int(counts.max()), 1)
    out = np.zeros(W * M, dtype=a.dtype)
    where = np.concatenate([w * M + np.arange(c) for w, c in enumerate(counts)]).astype(np.int64)
    out.view(np.uint8).reshape(W * M, -1)[where] = a.view(np.uint8).reshape(len(a), -1)
    return out, M, counts.astype(np.int32), None, where


def run_local(eng, rec, rng, pool, W, S, mb, tsp, rmw=False, skew=0, ragged=True, inline=None):
    """One local launch of fresh ops on `pool`. Returns (ops after -- the workers' read_write_ops --, the elements
    that were run: live and not skipped)."""
    loc = gen.local_ops(rng, pool, W * S, eng.sizes, rmw, tsp)
    if skew:   # refilled GETs carry (0, 0) (inline-util.h:268-272); some PUTs version 0
        z = rng.random(W * S) < 0.3
        loc["ts_ver"][z] = 0
        loc["ts_cid"][z & (loc["opcode"] == int(L.Op.GET))] = 0
    counts = rng.integers(S // 2, S + 1, size=W).astype(np.int32) if ragged else None
    ran = live_mask(W, S, counts) & ~np.isin(loc["state"], SKIPPED_LOCAL)
    eng.launch(L.BatchType.local_ops, loc, W, S, mb, counts=counts, inline=inline)
    gen.harvest_ts(tsp, loc)
    rec.add("local", loc["key"][ran], loc["state"][ran])
    return loc, ran


def run_memb(eng, rec, rng, pool, W, S, mb_fail, tsp, rmw, inline=None):
    mem = gen.memb_ops(rng, pool, W * S, eng.sizes, rmw, tsp)
    eng.launch(L.BatchType.local_ops_after_membership_change, mem, W, S, mb_fail, inline=inline)
    rec.add("memb", mem["key"], mem["state"])
    return mem


def run_unique_invs(eng, rec, rng, keys, W, mb, tsp, sender, rmw=False, packed=False, memb=True, inline=None):
    """One unique INV launch: one INV per key of `keys` (distinct) from `sender`, in W ragged batches, with
    membership-change INVs (node_suspected). Returns (the INVs that were run, after; node_suspected)."""
    assert len(np.unique(keys)) == len(keys)
    a = gen.invs(rng, keys, len(keys), eng.sizes, rmw, tsp, machine_num=3)
    a["key"] = keys
    a["state"] = sender
    if not memb:
        a["opcode"] = int(L.Op.INV)
    run = a["opcode"] != int(L.Op.MEMBERSHIP_CHANGE)
    elems, stride, counts, off, where = lay_out(a, split_counts(rng, len(a), W), packed)
    ns = np.full(W, -1, np.int32)
    eng.launch(L.BatchType.invs, elems, W, stride, mb, counts=counts, offsets=off, ns=ns, unique=True, inline=inline)
    out = elems[where][run]
    rec.add("inv", out["key"], np.where(out["state"] == MISS, MISS, out["opcode"]))
    return out, ns


def first_successes(loc, ran):
    """the elements of a local launch that began a write, the first per key"""
    idx = np.nonzero(ran & np.isin(loc["state"], SUCCESSES))[0]
    _, first = np.unique(loc["key"][idx], return_index=True)
    return np.sort(idx[first])


def build_acks(rng, loc, idx, W, S, sender, noise_keys, sizes, rmw, tsp):
    """A peer's ACKs to the writes loc[idx] began -- each in the batch of the worker that holds the op, with the
    op's timestamp -- among gen.acks noise on noise_keys (distinct, none of them a written key), shuffled within
    each batch. Returns (the batches back to back, counts)."""
    noise_keys = np.asarray(noise_keys, np.uint64)
    assert len(np.unique(noise_keys)) == len(noise_keys) and not np.isin(noise_keys, loc["key"][idx]).any()
    sf = "state" if rmw else "sender"
    parts, counts = [], []
    for w, nk in enumerate(np.array_split(noise_keys, W)):
        mine = idx[idx // S == w]
        a = np.zeros(len(mine) + len(nk), dtype=L.op_dtype(sizes) if rmw else L.msg_dtype())
        a["key"][:len(mine)] = loc["key"][mine]
        a["ts_ver"][:len(mine)] = loc["ts_ver"][mine]
        a["ts_cid"][:len(mine)] = loc["ts_cid"][mine]
        a["opcode"][:len(mine)] = int(L.Op.ACK)
        a[sf][:len(mine)] = sender
        if len(nk):
            n = gen.acks(rng, nk, len(nk), sizes, rmw, tsp, machine_num=3)
            n["key"] = nk
            a.view(np.uint8).reshape(len(a), -1)[len(mine):] = n.view(np.uint8).reshape(len(n), -1)
        a = a[rng.permutation(len(a))]
        parts.append(a)
        counts.append(len(a))
    return cat(parts), np.array(counts, np.int32)


def run_unique_acks(eng, rec, rng, loc, idx, W, S, mb, tsp, sender, noise_keys, rmw=False, packed=False, inline=None):
    """One unique ACK launch of build_acks, read_write_ops = the local buffers `loc` (updated in place)."""
    a, counts = build_acks(rng, loc, idx, W, S, sender, noise_keys, eng.sizes, rmw, tsp)
    elems, stride, counts, off, where = lay_out(a, counts, packed)
    st_before = loc["state"].copy()
    eng.launch(L.BatchType.acks, elems, W, stride, mb, counts=counts, offsets=off, rw=loc, rw_stride=S, unique=True,
               inline=inline)
    out = elems[where]
    run = out["state" if rmw else "sender"] != int(L.Op.MEMBERSHIP_CHANGE)
    rec.add("ack", out["key"][run], out["opcode"][run])
    done = loc["state"] != st_before
    rec.add("rw", loc["key"][done], loc["state"][done])
    return out


def run_vals(eng, rec, rng, pool, applied, W, M, mb, tsp, inline=None):
    """One VAL launch (keys repeat): the VALs of INVs that were applied (same key, timestamp and sender) among
    gen.vals noise on `pool`. Records which elements' keys the launch moved to VALID. Returns (VALs before, after)."""
    n = W * M
    v = gen.vals(rng, pool, n, eng.sizes, False, tsp, machine_num=3)
    ok = applied[applied["opcode"] == int(L.Resp.INV_SUCCESS)] if len(applied) else applied
    k = min(len(ok), n // 2)
    if k:
        pick, pos = rng.choice(len(ok), k, replace=False), rng.choice(n, k, replace=False)
        for f, g in (("key", "key"), ("ts_ver", "ts_ver"), ("ts_cid", "ts_cid"), ("sender", "state")):
            v[f][pos] = ok[g][pick]
    uk = np.unique(v["key"])
    before = key_states(eng.o, uk)
    vin = gen.bytecopy(v)
    eng.launch(L.BatchType.vals, v, W, M, mb, inline=inline)
    after = key_states(eng.o, uk)
    moved = uk[(after == int(L.State.VALID)) & (before != int(L.State.VALID))]
    rec.add("val", uk, np.where(np.isin(uk, moved), MOVED_TO_VALID, 0))
    return vin, v


# ---------------------------------------------------------------------------------------------- the cases
def case_rounds(eng, T: Table, rec: Rec, skew=0, rmw=False, rounds=6, big=(1, 3), check_after=(1, 4), memb_from=None,
                seed=20261019):
    """Protocol rounds (3a; with rmw: 3d). Per round: one local launch (W=5, S=48, ragged; in the rounds `big`
    W=40, S=250), two unique INV launches standing for peers 1 and 2 (packed in alternate rounds, membership-change
    INVs, node_suspected), each peer's ACKs to the round's writes as a unique ACK launch with rw = the local
    buffers, one VAL launch of 5 x 96; from round memb_from on an after-membership-change launch. The table is
    checked after the rounds in check_after only. Without RMWs every launch runs INLINE; with them the local and
    the after-membership-change launches have no inline kernels."""
    rng = np.random.default_rng(seed + skew + (7 if rmw else 0))
    tsp = gen.TsPool(rng)
    mb, mb_fail = L.membership(3, 0), L.membership(3, 0, alive=0b011)
    suspected = 0
    for rnd in range(rounds):
        W, S = (40, 250) if rnd in big else (5, 48)
        pool = gen.key_pool(rng, T.keys, hot=24 if rnd % 2 else 200)
        loc, ran = run_local(eng, rec, rng, pool, W, S, mb, tsp, rmw=rmw, skew=skew, inline=not rmw)
        idx = first_successes(loc, ran)
        applied = []
        for peer in (1, 2):
            keys = distinct_keys(rng, pool, T.keys, 400)
            out, ns = run_unique_invs(eng, rec, rng, keys, 5, mb, tsp, peer, rmw=rmw, packed=rnd % 2 == 1, inline=True)
            applied.append(out)
            suspected += int((ns >= 0).sum())
        for peer in (1, 2):
            noise = np.setdiff1d(distinct_keys(rng, pool, T.keys, 300), loc["key"][idx])
            run_unique_acks(eng, rec, rng, loc, idx, W, S, mb, tsp, peer, noise, rmw=rmw, packed=rnd % 2 == 0,
                            inline=True)
        run_vals(eng, rec, rng, pool, cat(applied), 5, 96, mb, tsp, inline=True)
        if memb_from is not None and rnd >= memb_from:
            run_memb(eng, rec, rng, pool, W, S, mb_fail, tsp, rmw, inline=False)
        if rnd in check_after:
            eng.check_table(f"round {rnd}")
    assert suspected >= rounds, "membership-change INVs set their batches' node_suspected"


def collision_keys(T: Table):
    """An inline key K whose bucket holds two keys or more, a bucket-mate M that is not the inline key, and their
    fakes: the same bucket and tag (bit 40 is in neither), absent."""
    b = T.inline_buckets[np.nonzero(T.n_used[T.inline_buckets] >= 2)[0][0]]
    K = T.inline_keys[np.nonzero(T.inline_buckets == b)[0][0]]
    M = T.slot_keys(np.array([b]), 7)[0]          # the bucket's first inserted key: slot 7, never the lowest of two
    assert T.first[b] < 7 and M != K and T.bucket([M])[0] == b
    fakes = np.array([int(K) ^ (1 << 40), int(M) ^ (1 << 40)], dtype=np.uint64)
    return np.uint64(K), np.uint64(M), fakes


def case_collisions(eng, T: Table, rec: Rec, seed=11):
    """3b: tag collisions and hot inline keys. Three pools (K, M and their fakes alone; among 300 others; K and its
    fake alone), per pool a local launch 8 x 250, a unique INV launch and each peer's unique ACK launch over the
    pool's keys padded with other keys to 256 elements or more, VALs 8 x 900; the table checked after each pool.
    Every element on a fake comes out MISS."""
    rng = np.random.default_rng(seed)
    tsp = gen.TsPool(rng)
    mb = L.membership(3, 0)
    K, M, fakes = collision_keys(T)
    assert all(eng.o.lookup(int(f)) is None for f in fakes)
    four = np.array([K, M, fakes[0], fakes[1]], dtype=np.uint64)
    others = np.setdiff1d(T.keys[100:400], four)
    W, S = 8, 250
    for p, pool in enumerate((four, np.concatenate([four, others]), np.array([K, fakes[0]], dtype=np.uint64))):
        loc, ran = run_local(eng, rec, rng, pool, W, S, mb, tsp, ragged=False, inline=True)
        fk = np.isin(loc["key"], fakes) & ran
        assert fk.sum() > 100 and (loc["state"][fk] == MISS).all(), f"pool {p}: local elements on the fakes"
        idx = first_successes(loc, ran)
        keys = distinct_keys(rng, pool, T.keys, max(len(pool), 280))
        out, _ = run_unique_invs(eng, rec, rng, keys, W, mb, tsp, 1, inline=True)
        fk = np.isin(out["key"], fakes)
        assert (out["state"][fk] == MISS).all() and (out["state"][~fk] != MISS).all(), f"pool {p}: INVs on the fakes"
        for peer in (1, 2):
            noise = np.setdiff1d(distinct_keys(rng, pool, T.keys, max(len(pool), 280)), loc["key"][idx])
            acks = run_unique_acks(eng, rec, rng, loc, idx, W, S, mb, tsp, peer, noise, inline=True)
            fk = np.isin(acks["key"], fakes) & (acks["sender"] != int(L.Op.MEMBERSHIP_CHANGE))
            assert (acks["sender"][fk] == MISS).all(), f"pool {p}: ACKs on the fakes"
        _, v = run_vals(eng, rec, rng, pool, out, 8, 900, mb, tsp, inline=True)
        fk = np.isin(v["key"], fakes)
        assert fk.sum() > 100 and (v["sender"][fk] == MISS).all(), f"pool {p}: VALs on the fakes"
        eng.check_table(f"pool {p}")


def dense_strata(T: Table):
    """Geometry D's four strata: evicted (or overwritten) keys; the inline keys of full buckets (slot 0); the
    slot-7 keys of full buckets; the inline keys of buckets that are not full."""
    full = T.n_used[T.inline_buckets] == 8
    fb = T.inline_buckets[full]
    return {"evicted": T.keys[~T.present], "inline_full": T.inline_keys[full], "slot7_full": T.slot_keys(fb, 7),
            "inline_part": T.inline_keys[~full]}


def case_dense(eng, T: Table, rec: Rec, seed=31):
    """3c: twice a local launch 40 x 250 on 200 keys of each stratum, one unique INV launch of 3000 distinct keys
    (500 of them evicted), VALs 8 x 900; then the table is checked. Every element on an evicted key is MISS."""
    rng = np.random.default_rng(seed)
    tsp = gen.TsPool(rng)
    mb = L.membership(3, 0)
    strata = dense_strata(T)
    assert all(len(v) >= 200 for v in strata.values()), {k: len(v) for k, v in strata.items()}
    evicted = strata["evicted"]
    for rep in range(2):
        pool = np.concatenate([rng.choice(v, 200, replace=False) for v in strata.values()])
        rng.shuffle(pool)
        loc, ran = run_local(eng, rec, rng, pool, 40, 250, mb, tsp, inline=True)
        ev = np.isin(loc["key"], evicted) & ran
        assert ev.sum() > 500 and (loc["state"][ev] == MISS).all(), "local elements on evicted keys"
        must = np.concatenate([pool[~np.isin(pool, evicted)], rng.choice(evicted, 500, replace=False)])
        keys = distinct_keys(rng, must, T.keys[T.present], 3000)
        out, _ = run_unique_invs(eng, rec, rng, keys, 8, mb, tsp, 1 + rep, inline=True)
        ev = np.isin(out["key"], evicted)
        assert ev.sum() >= 450 and (out["state"][ev] == MISS).all() and (out["state"][~ev] != MISS).all()
        _, v = run_vals(eng, rec, rng, pool, out, 8, 900, mb, tsp, inline=True)
        ev = np.isin(v["key"], evicted)
        assert ev.sum() > 500 and (v["sender"][ev] == MISS).all(), "VALs on evicted keys"
    eng.check_table("dense")


def rows_setup(n_rows, skip):
    """(machines, this machine, the sender of each row). Without a skip row the rows are the peers of machine 0
    (eight rows: seven peers, and the first one's ACKs once more); with one, row r is machine r and the skip row
    this machine's own."""
    if skip < 0:
        machines = min(n_rows + 1, 8)
        return machines, 0, [1 + r % (machines - 1) for r in range(n_rows)]
    return n_rows, skip, list(range(n_rows))


def case_ack_rows(eng, T: Table, rec: Rec, n_rows, skip, inline, reps=2, seed=53):
    """3e: `reps` times a local launch 8 x 250 and then its ACKs from every peer as one rows launch of 16-B ACKs
    (row r = one sender's ACKs, position j of every row on one key, holes, a row stride past the total, the VAL
    callbacks' output wanted). The table is checked after the last."""
    rng = np.random.default_rng(seed + 10 * n_rows + skip)
    tsp = gen.TsPool(rng)
    machines, me, senders = rows_setup(n_rows, skip)
    assert eng.machine_id == me
    mb = L.membership(machines, me)
    W, S = 8, 250
    for rep in range(reps):
        pool = gen.key_pool(rng, T.keys, hot=40 if rep else 300)
        loc, ran = run_local(eng, rec, rng, pool, W, S, mb, tsp, ragged=False, inline=True)
        idx = first_successes(loc, ran)
        noise = np.setdiff1d(distinct_keys(rng, pool, T.keys, 320), loc["key"][idx])
        a, counts = build_acks(rng, loc, idx, W, S, 0, noise, eng.sizes, False, tsp)
        total = len(a) + 3                       # three positions past the last offset: in no batch
        row_stride = total + 5
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        elems = np.zeros((n_rows - 1) * row_stride + total, dtype=L.msg_dtype())
        for r in range(n_rows):
            row = gen.bytecopy(a)
            keep = row["sender"] != int(L.Op.MEMBERSHIP_CHANGE)
            row["sender"][keep] = senders[r]
            row["opcode"][rng.random(len(a)) < 0.15] = 0          # holes
            elems[r * row_stride:r * row_stride + len(a)] = row
        st_before = loc["state"].copy()
        eng.launch(L.BatchType.acks, elems, W, total, mb, offsets=off, rw=loc, rw_stride=S, unique=True,
                   rows=(n_rows, row_stride, skip), vals=True, inline=inline)
        done = loc["state"] != st_before
        rec.add("rw", loc["key"][done], loc["state"][done])
    eng.check_table("rows")


def case_inv_rows(eng, T: Table, rec: Rec, n_rows=3, reps=2, seed=59):
    """3e for INVs: rows of 56-B INVs, row r from peer r + 1, position j of every row on one key, holes."""
    rng = np.random.default_rng(seed)
    tsp = gen.TsPool(rng)
    mb = L.membership(n_rows + 1, 0)
    W = 8
    for rep in range(reps):
        keys = distinct_keys(rng, gen.key_pool(rng, T.keys, hot=100), T.keys, 300)
        counts = split_counts(rng, len(keys), W)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        total = len(keys) + 3
        row_stride = total + 5
        elems = np.zeros((n_rows - 1) * row_stride + total, dtype=L.op_dtype(eng.sizes))
        holes = []
        for r in range(n_rows):
            row = gen.invs(rng, keys, len(keys), eng.sizes, False, tsp, machine_num=n_rows + 1)
            row["key"] = keys
            row["state"] = r + 1
            row["opcode"] = int(L.Op.INV)
            row["opcode"][rng.random(len(keys)) < 0.15] = 0
            holes.append(row["opcode"] == 0)
            elems[r * row_stride:r * row_stride + len(keys)] = row
        eng.launch(L.BatchType.invs, elems, W, total, mb, offsets=off, unique=True, rows=(n_rows, row_stride, -1),
                   inline=True)
        for r in range(n_rows):
            out = elems[r * row_stride:r * row_stride + len(keys)][~holes[r]]
            rec.add("inv", out["key"], np.where(out["state"] == MISS, MISS, out["opcode"]))
    eng.check_table("inv rows")
