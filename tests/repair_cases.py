"""Scripted launches that put a repair's source and target tables into the states an install has to handle, numpy
only. Each script drives `apply(btype, elems, membership)` (in place), so the same launches run on an oracle
alone (tests/test_repair_cpu.py) or on a device table and its oracle twin (tests/test_repair_gpu.py).

Source (machine 0) ends with VALID, INVALID, WRITE and INVALID_WRITE keys at mixed timestamps; the target script
(machine 2) makes keys newer than, equal to and older than the source's, two keys in WRITE at a timestamp the
source holds too, and the target is populated with fewer ids, so some source keys are absent from it.
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L

SRC_ID, DST_ID, N_MACH = 0, 2, 5
BATCH = 200          # elements per launch: below MAX_BATCH_KVS_OPS_SIZE (250)
# id ranges of the scripts (all below the smallest table used, 1000 keys)
PUT = (40, 120)      # source: local PUTs, WRITE at (2, 0)
INV1 = (100, 400)    # source: INVs from machine 1 at (4, 1); 100..119 were in WRITE: INVALID_WRITE
VAL1 = (200, 400)    # source: VALs of those: VALID at (4, 1)
NEWER = (300, 360)   # target: INVs from machine 3 at (6, 3) (300..329 made VALID): newer than the source's
EQUAL = (360, 420)   # target: the same INVs from machine 1 at (4, 1) (360..389 made VALID): equal
TW = (500, 502)      # target: local PUTs, WRITE at (2, DST_ID); the source has them from machine DST_ID's INVs,
                     # 500 still INVALID (the target stays WRITE), 501 made VALID (the VAL validates the target)


def _fill(a, ids, salt):
    a["value"] = ((np.asarray(ids)[:, None] * 7 + salt + np.arange(a["value"].shape[1])[None, :]) % 251).astype(np.uint8)


def invs(keys, ids, sender, ts, sizes, salt):
    a = np.zeros(len(ids), dtype=L.op_dtype(sizes))
    a["key"] = keys[ids]
    a["opcode"] = int(L.Op.INV)
    a["state"] = sender
    a["ts_ver"], a["ts_cid"] = ts
    a["val_len"] = sizes.st_value >> sizes.shift
    _fill(a, ids, salt)
    return a


def vals(keys, ids, sender, ts):
    a = np.zeros(len(ids), dtype=L.msg_dtype())
    a["key"] = keys[ids]
    a["opcode"] = int(L.Op.VAL)
    a["sender"] = sender
    a["ts_ver"], a["ts_cid"] = ts
    return a


def puts(keys, ids, sizes, salt):
    a = np.zeros(len(ids), dtype=L.op_dtype(sizes))
    a["key"] = keys[ids]
    a["opcode"] = int(L.Op.PUT)
    a["state"] = int(L.Bucket.NEW)
    a["val_len"] = sizes.st_value >> sizes.shift
    _fill(a, ids, salt)
    return a


def make_records(keys, states, ts_ver, ts_cid, sizes, salt):
    """records [n][E] written by hand: key, state, timestamp and value, every other byte zero"""
    keys = np.asarray(keys, np.uint64)
    rec = np.zeros(len(keys), dtype=L.entry_dtype(sizes))
    rec["key"] = keys
    rec["state"] = states
    rec["ts_ver"], rec["ts_cid"] = ts_ver, ts_cid
    rec["value"] = ((np.arange(len(keys))[:, None] * 5 + salt + np.arange(sizes.st_value)[None, :]) % 253).astype(np.uint8)
    return rec.view(np.uint8).reshape(len(keys), sizes.entry)


def collision_records(T, oracle, ts_ver):
    """Records at (ts_ver, 1) for K, M and both fakes of tests/inline_cases.collision_keys -- the fakes are absent
    and share a present key's bucket and tag -- and eight ordinary present keys; every third record INVALID.
    Returns (records, K, M, fakes)."""
    from tests import inline_cases as C
    K, M, fakes = C.collision_keys(T)
    assert all(oracle.lookup(int(f)) is None for f in fakes)
    others = np.setdiff1d(T.keys[T.present][:12], [K, M])[:8]
    keys = np.concatenate([np.array([K, M], dtype=np.uint64), fakes, others.astype(np.uint64)])
    assert len(np.unique(keys)) == len(keys) == 12
    states = np.where(np.arange(len(keys)) % 3 == 0, int(L.State.INVALID), int(L.State.VALID))
    return make_records(keys, states, ts_ver, 1, L.DEFAULT, 23), K, M, fakes


def _chunks(apply, btype, elems, mb):
    for lo in range(0, len(elems), BATCH):
        part = elems[lo:lo + BATCH].copy()
        apply(btype, part, mb)


def source_script(apply, keys, sizes):
    mb = L.membership(N_MACH, SRC_ID)
    r = np.arange
    _chunks(apply, L.BatchType.local_ops, puts(keys, r(*PUT), sizes, 1), mb)
    _chunks(apply, L.BatchType.invs, invs(keys, r(*INV1), 1, (4, 1), sizes, 2), mb)
    _chunks(apply, L.BatchType.vals, vals(keys, r(*VAL1), 1, (4, 1)), mb)
    _chunks(apply, L.BatchType.invs, invs(keys, r(*TW), DST_ID, (2, DST_ID), sizes, 5), mb)
    _chunks(apply, L.BatchType.vals, vals(keys, r(TW[0] + 1, TW[1]), DST_ID, (2, DST_ID)), mb)


def target_script(apply, keys, sizes):
    mb = L.membership(N_MACH, DST_ID)
    r = np.arange
    _chunks(apply, L.BatchType.invs, invs(keys, r(*NEWER), 3, (6, 3), sizes, 3), mb)
    _chunks(apply, L.BatchType.vals, vals(keys, r(NEWER[0], NEWER[0] + 30), 3, (6, 3)), mb)
    _chunks(apply, L.BatchType.invs, invs(keys, r(*EQUAL), 1, (4, 1), sizes, 2), mb)
    _chunks(apply, L.BatchType.vals, vals(keys, r(EQUAL[0], EQUAL[0] + 30), 1, (4, 1)), mb)
    _chunks(apply, L.BatchType.local_ops, puts(keys, r(*TW), sizes, 5), mb)
