"""Inputs of tests/test_local_fused_blocks_gpu.py: local launches of the direct path shaped around the fused pass's
64-element blocks (two waves stage 32 elements each, one wave resolves all 64 and stores the first writers' entry
images), in one place so that tests/test_local_fused_blocks_cpu.py can show on the oracle alone that every case
produces the outcome it is meant to.

A case drives an engine as tests/inline_cases.py's do (OracleBlockEngine here, the device-and-Mirror engine in the
GPU module) and returns the facts the CPU test asserts. Launches take `patch` ([n][16], the pending header writes of
include/hermeskv.h) besides what inline_cases' engines take. All cases run on geometry S with keys that no earlier
launch of the case has written, so that a key's first PUT is its first writer (F) of the launch.
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L
from tests import gen
from tests import inline_cases as C

GET, PUT, INV = int(L.Op.GET), int(L.Op.PUT), int(L.Op.INV)
NEW = int(L.Bucket.NEW)
MISS, PUT_SUCCESS, GET_COMPLETE = int(L.Resp.MISS), int(L.Resp.PUT_SUCCESS), int(L.Resp.GET_COMPLETE)
GET_STALL, PUT_STALL, REPLAY_SUCCESS = int(L.Resp.GET_STALL), int(L.Resp.PUT_STALL), int(L.Resp.REPLAY_SUCCESS)
BLOCK = 64
EDGE = (0, 31, 32, 63)           # first and last position of each wave's half of a block
# n, batches, stride
SIZES = [(1, 1, 1), (31, 1, 31), (32, 1, 32), (33, 1, 33), (63, 1, 63), (64, 1, 64), (65, 1, 65), (127, 1, 127),
         (129, 3, 43), (200, 2, 100)]
FIRST_WRITERS = (0, 1, 16, 17, 33, 64)   # per block: none, one, one store step, past it, past a wave's worth, all
DEFERRED = (1, 2, 64)


def apply_patches(ops: np.ndarray, patch: np.ndarray, st_value: int):
    """the valid patches written into ops ([n][esz] bytes) in place: key, opcode, state NEW, val_len, flags; the
    timestamp cleared where byte 13 says so; the value filled where byte 12 is not 0"""
    for i in np.nonzero(patch[:, 14])[0]:
        o, p = ops[i], patch[i]
        o[0:8] = p[0:8]
        o[8], o[9], o[10] = p[8], NEW, p[9]
        if p[13]:
            o[11:16] = 0
        o[16:18] = p[10:12]
        if p[12]:
            o[18:18 + st_value] = p[12]


class OracleBlockEngine(C.OracleEngine):
    def launch(self, btype, elems, n_batches, stride, mb, patch=None, **kw):
        if patch is not None:
            apply_patches(elems.view(np.uint8).reshape(len(elems), -1), patch, self.sizes.st_value)
        super().launch(btype, elems, n_batches, stride, mb, **kw)


class Supply:
    """Keys of the table nobody has handed out yet: inline keys, the others, and (inline key, bucket-mate) pairs."""

    def __init__(self, T: C.Table):
        full = np.zeros(len(T.inline_buckets), bool)
        full[np.nonzero(T.n_used[T.inline_buckets] >= 2)[0][:8]] = True    # eight pairs are set aside
        b = T.inline_buckets[full]
        mates = T.slot_keys(b, 7)    # a bucket's first inserted key: never the lowest slot of two
        self.pairs = list(zip(T.inline_keys[full].tolist(), mates.tolist()))
        paired = np.concatenate([T.inline_keys[full], mates])
        il = T.is_inline(T.keys)
        free = T.present & ~np.isin(T.keys, paired)
        self.inl, self.oth = T.keys[il & free].tolist(), T.keys[~il & free].tolist()

    def pair(self):
        return self.pairs.pop()

    def take(self, n):
        """n fresh keys, inline keys and others alternating"""
        out = [(self.inl if j % 2 == 0 else self.oth).pop() for j in range(n)]
        return np.array(out, dtype=np.uint64)


def missing_keys(rng, o, n):
    k = rng.integers(1, 2**63, size=n, dtype=np.int64).astype(np.uint64)
    assert all(o.lookup(int(x)) is None for x in k)
    return k


def blank_ops(n, sizes, rng):
    a = np.zeros(n, dtype=L.op_dtype(sizes))
    a["state"] = NEW
    a["val_len"] = sizes.st_value >> sizes.shift
    a["flags"] = rng.integers(0, 1 << 16, size=n)
    a["value"] = rng.integers(1, 256, size=(n, sizes.st_value))
    return a


def ragged_counts(W, S):
    """a count that ends inside wave 0's half of a block, and a batch with count 0"""
    if W == 1:
        return np.array([min(20, S - 1)], np.int32)
    return np.array([17, 0, S] if W == 3 else [S, 20], np.int32)


def edge_patches(rng, ops, pool, sizes):
    """hand-made patches at positions 0, 31, 32 and 63 of every block, and at a few others: the slots hold finished
    ops (as a refill finds them), the patches put GETs and PUTs on the pool's keys there"""
    n = len(ops)
    pos = np.array([i for i in range(n) if i % BLOCK in EDGE or rng.random() < 0.1])
    patch = np.zeros((n, 16), np.uint8)
    ops["state"][pos] = rng.choice([GET_COMPLETE, int(L.Resp.PUT_COMPLETE)], size=len(pos))
    put = rng.random(len(pos)) < 0.5
    patch[pos, 0:8] = rng.choice(pool, size=len(pos)).astype("<u8").view(np.uint8).reshape(-1, 8)
    patch[pos, 8] = np.where(put, PUT, GET)
    patch[pos, 9] = sizes.st_value >> sizes.shift
    patch[pos, 10:12] = rng.integers(0, 256, size=(len(pos), 2))
    patch[pos, 12] = np.where(put, rng.integers(1, 256, size=len(pos)), 0)
    patch[pos, 13] = ~put
    patch[pos, 14] = 1
    return patch, pos


def case_block_edges(eng, T: C.Table, skew=0, seed=5):
    """Every size of SIZES, with and without counts, with and without patches: random GETs and PUTs (skipped states
    among them) on ten fresh keys and two absent ones. Facts per launch: (n, ragged, patched, ops after, live mask,
    patched positions, ops before with the patches applied)."""
    rng = np.random.default_rng(seed + skew)
    tsp = gen.TsPool(rng)
    mb = L.membership(3, 0)
    sup = Supply(T)
    facts = []
    for n, W, S in SIZES:
        for ragged in (False, True):
            for patched in (False, True):
                pool = np.concatenate([sup.take(10 if n > 1 else 2), missing_keys(rng, eng.o, 2)])
                ops = gen.local_ops(rng, pool, n, eng.sizes, False, tsp)
                if skew:
                    z = rng.random(n) < 0.3
                    ops["ts_ver"][z] = 0
                    ops["ts_cid"][z & (ops["opcode"] == GET)] = 0
                counts = ragged_counts(W, S) if ragged else None
                patch, pos = edge_patches(rng, ops, pool, eng.sizes) if patched else (None, np.zeros(0, np.int64))
                before = gen.bytecopy(ops)
                if patched:
                    apply_patches(before.view(np.uint8).reshape(n, -1), patch, eng.sizes.st_value)
                eng.launch(L.BatchType.local_ops, ops, W, S, mb, counts=counts, patch=patch, inline=True)
                facts.append((n, ragged, patched, gen.bytecopy(ops), C.live_mask(W, S, counts), pos, before))
        eng.check_table(f"edges n {n}")
    return facts


def case_first_writer_position(eng, T: C.Table, skew=0, seed=7):
    """One key per launch of 64 elements, its first PUT at position 0, 31, 32 or 63: GETs and skipped PUTs before it,
    GETs and PUTs after it, in both halves. For an inline key and for its bucket-mate that is not inline. Facts per
    launch: (position, key is inline, opcodes, states before, states after)."""
    rng = np.random.default_rng(seed + skew)
    mb = L.membership(3, 0)
    sup = Supply(T)
    facts = []
    for p in EDGE:
        pair = sup.pair()
        for which in (0, 1):
            ops = blank_ops(BLOCK, eng.sizes, rng)
            ops["key"] = pair[which]
            ops["opcode"] = np.where(np.arange(BLOCK) % 2 == 0, GET, PUT)
            ops["opcode"][p] = PUT
            early = (np.arange(BLOCK) < p) & (ops["opcode"] == PUT)
            ops["state"][early] = int(L.Bucket.IN_PROGRESS_PUT)     # skipped: no writer before p
            before = ops["state"].copy()
            eng.launch(L.BatchType.local_ops, ops, 1, BLOCK, mb, inline=True)
            facts.append((p, bool(T.is_inline([pair[which]])[0]), ops["opcode"].copy(), before, ops["state"].copy()))
    eng.check_table("first writer positions")
    return facts


def case_first_writers_per_block(eng, T: C.Table, skew=0, seed=9):
    """A 64-element block with 0, 1, 16, 17, 33 and 64 first PUTs on distinct fresh keys, GETs on four keys nobody
    writes elsewhere. Facts per launch: (first writers asked for, PUT positions, states after)."""
    rng = np.random.default_rng(seed + skew)
    mb = L.membership(3, 0)
    sup = Supply(T)
    readers = sup.take(4)
    facts = []
    for k in FIRST_WRITERS:
        ops = blank_ops(BLOCK, eng.sizes, rng)
        ops["opcode"] = GET
        ops["key"] = rng.choice(readers, size=BLOCK)
        pos = np.sort(rng.choice(BLOCK, size=k, replace=False))
        if k == 1:
            pos = np.array([40])          # alone, in wave 1's half
        ops["opcode"][pos] = PUT
        ops["key"][pos] = sup.take(k) if k else []
        eng.launch(L.BatchType.local_ops, ops, 1, BLOCK, mb, inline=True)
        facts.append((k, pos, ops["state"].copy()))
    eng.check_table("first writers per block")
    return facts


def case_deferred(eng, T: C.Table, skew=0, seed=13):
    """A unique INV launch from peers 1 and 2 leaves 300 keys INVALID; then, with peer 2 out of the membership, blocks
    with 1, 2 and 64 elements on INVALID keys in both halves (GETs replay where peer 2 wrote last and stall where
    peer 1 did; PUTs write), among GETs on VALID keys. Facts per launch: (elements asked for, key states before per
    element, opcodes, states after)."""
    rng = np.random.default_rng(seed + skew)
    mb, mb_fail = L.membership(3, 0), L.membership(3, 0, alive=0b011)
    sup = Supply(T)
    keys = sup.take(300)
    invs = blank_ops(len(keys), eng.sizes, rng)
    invs["key"] = keys
    invs["opcode"] = INV
    invs["state"] = np.where(np.arange(len(keys)) % 2 == 0, 2, 1)      # the sender
    invs["ts_ver"] = 1000
    invs["ts_cid"] = invs["state"]
    ns = np.full(4, -1, np.int32)
    eng.launch(L.BatchType.invs, invs, 4, 75, mb, ns=ns, unique=True, inline=True)
    assert (C.key_states(eng.o, keys) == int(L.State.INVALID)).all()
    from2, from1 = list(keys[0::2]), list(keys[1::2])
    valid = sup.take(6)
    facts = []
    for d in DEFERRED:
        ops = blank_ops(2 * BLOCK, eng.sizes, rng)
        ops["opcode"] = GET
        ops["key"] = rng.choice(valid, size=2 * BLOCK)
        ops["ts_ver"] = 0
        pos = {1: [33], 2: [5, 60]}.get(d, list(range(BLOCK)))
        for j, p in enumerate(pos):
            src = from2 if j % 2 == 0 else from1
            # in the full block keys repeat (a replay or a write, then that key's later elements) and a third are PUTs
            ops["key"][p] = src.pop() if d < BLOCK or j < 40 else ops["key"][pos[j - 40]]
            if d == BLOCK and j % 3 == 2:
                ops["opcode"][p] = PUT
        st0 = C.key_states(eng.o, ops["key"])
        eng.launch(L.BatchType.local_ops, ops, 1, 2 * BLOCK, mb_fail, inline=True)
        facts.append((d, st0, ops["opcode"].copy(), ops["state"].copy()))
    eng.check_table("deferred")
    return facts


def case_misses_and_skipped(eng, T: C.Table, skew=0, seed=17):
    """Absent keys (GET and PUT) and skipped elements at fixed positions of both halves of a block, two blocks and a
    partial third. Facts: (miss positions, skipped positions, ops before, ops after)."""
    rng = np.random.default_rng(seed + skew)
    mb = L.membership(3, 0)
    sup = Supply(T)
    n = 2 * BLOCK + 9
    ops = blank_ops(n, eng.sizes, rng)
    ops["key"] = rng.choice(sup.take(8), size=n)
    ops["opcode"] = rng.choice([GET, PUT], size=n)
    miss = np.array([3, 7, 35, 39, 64, 127, 130])
    skipped = np.array([10, 31, 32, 50, 63, 100, 136])
    ops["key"][miss] = missing_keys(rng, eng.o, len(miss))
    ops["state"][skipped] = rng.choice(C.SKIPPED_LOCAL, size=len(skipped))
    before = gen.bytecopy(ops)
    eng.launch(L.BatchType.local_ops, ops, 1, n, mb, inline=True)
    eng.check_table("misses and skipped")
    return miss, skipped, before, gen.bytecopy(ops)
