"""Upsert (include/hermeskv.h, "Upsert") restated in numpy on the oracle's own memory, written from the header's
text, not from the kernels: the reference's insert (mica_insert_one, mica.c:78-146) acting on OracleKVS's index, log
and log head, the entry image an inserted record stands for, and the call as the header defines it -- the install,
then for each missed record in record order the insert and that record's INV and VAL as one-element batches through
OracleKVS.batch. The device is held against it byte for byte (tests/test_upsert_gpu.py), and the definition is
checked on the oracle alone (tests/test_upsert_cpu.py).
"""
from __future__ import annotations

import ctypes

import numpy as np

from hermes_amd import layout as L
from tests import repair_model as RM

RESULT = ("raised", "equal", "older", "inserted", "replaced", "evictions", "log_head")


def _set_head(oracle, head: int) -> None:
    from oracle.oracle import lib
    lib().hko_set_log_head.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib().hko_set_log_head(oracle.h, head)


def _log_with_slack(oracle, sizes: L.Sizes) -> np.ndarray:
    """the oracle's log with the one entry of slack behind log_cap (an entry that starts just below the capacity
    runs into it), writable"""
    from oracle.oracle import lib
    return np.ctypeslib.as_array(lib().hko_log(oracle.h), shape=(oracle.log_cap + sizes.entry,))


def mica_insert(oracle, image: np.ndarray, sizes: L.Sizes = L.DEFAULT) -> tuple[int, int]:
    """mica_insert_one of one entry image (E bytes, the key in bytes 8..15) on the oracle's memory. Returns
    (replaced, evicted), each 0 or 1: the insert took an in-use slot by tag match; it found no slot."""
    image = np.asarray(image, np.uint8).reshape(-1)
    E, cap = sizes.entry, oracle.log_cap
    assert len(image) == E
    key = int(image[8:16].copy().view("<u8")[0])
    bkt = (key & 0xFFFFFFFF) & (oracle.num_bkts - 1)          # the 32-bit bkt field
    tag = key >> 48
    views = getattr(oracle, "_upsert_views", None)            # (the oracle's memory never moves: mapped once)
    if views is None:
        views = oracle._upsert_views = (oracle.index_bytes().view("<u8"), _log_with_slack(oracle, sizes))
    slots = views[0][bkt * 8:bkt * 8 + 8]
    use, replaced, evicted = -1, 0, 0
    for i in range(8):
        s = int(slots[i])
        if ((s >> 1) & 0x7FFFFF) == tag or not (s & 1):       # the last slot that has the tag or is empty
            use, replaced = i, s & 1
    if use < 0:
        use, evicted = tag & 7, 1
    head = oracle.log_head()
    slots[use] = np.uint64(1 | (tag << 1) | ((head << 24) & 0xFFFFFFFFFFFFFFFF))
    phys = head & (cap - 1)
    views[1][phys:phys + E] = image
    head = (head + E + 7) & ~7                                 # len_to_copy, rounded up to 8: E
    if ((cap - head) & 0xFFFFFFFFFFFFFFFF) <= sizes.kvs_value + 32:   # the unsigned test: fires once
        head = (head + cap) & ~(cap - 1)
    _set_head(oracle, head)
    return replaced, evicted


def populate_image(key_first: int, key: int, value, sizes: L.Sizes = L.DEFAULT) -> np.ndarray:
    """the entry spacetime_populate_fixed_len(kv, ., KVS_VALUE_SIZE) builds (spacetime.c:17-68), fields the
    reference leaves uninitialised zero; value: ST_VALUE_SIZE bytes, or one fill byte"""
    e = np.zeros(1, dtype=L.entry_dtype(sizes))
    e["key_first"], e["key"] = key_first, key
    e["opcode"] = int(L.Op.PUT)
    e["val_len"] = sizes.kvs_value >> sizes.shift
    e["state"] = int(L.State.VALID)
    e["rmw_lwid"] = L.LWID_EMPTY << 1
    e["obi"] = L.OBI_EMPTY
    e["ts_cid"] = L.CID_EMPTY
    e["value"] = value
    return e.view(np.uint8).reshape(-1)


def record_images(records: np.ndarray, sizes: L.Sizes = L.DEFAULT) -> np.ndarray:
    """[n][E]: the image an upsert inserts for each record -- populate's, with bytes 0..7 zero, the record's key
    and value"""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry)
    out = np.tile(populate_image(0, 0, 0, sizes), (len(records), 1))
    out[:, 8:16] = records[:, 8:16]
    out[:, 33:] = records[:, 33:]
    return out


def upsert_model(oracle, records: np.ndarray, sizes: L.Sizes, membership: bytes) -> dict:
    """hkv_table_upsert of the records on the oracle, step by step as the header states it; returns
    hkv_upsert_result as a dict"""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry)
    # step 1: the install; the missed set against the table as it was before the call
    missed = [i for i, r in enumerate(records)
              if oracle.lookup(int(r[8:16].copy().view("<u8")[0])) is None]
    counts = RM.install_counts(oracle, records, sizes)
    assert counts["missed"] == len(missed)
    RM.apply_records(oracle, records, sizes, membership)
    # step 2: each missed record in record order -- the insert, then its INV and (VALID) its VAL, one-element batches
    replaced = evictions = 0
    inv, val = RM.records_to_batches(records, sizes)           # record i's INV is inv[i]; its VAL, if VALID, val[at[i]]
    valid = records[:, 18] == int(L.State.VALID)
    at = np.cumsum(valid) - 1
    images = record_images(records[missed], sizes) if missed else ()
    for i, image in zip(missed, images):
        r, e = mica_insert(oracle, image, sizes)
        replaced, evictions = replaced + r, evictions + e
        oracle.batch(L.BatchType.invs, inv[i:i + 1], membership)
        if valid[i]:
            oracle.batch(L.BatchType.vals, val[at[i]:at[i] + 1], membership)
    return {"raised": counts["raised"], "equal": counts["equal"], "older": counts["older"], "inserted": len(missed),
            "replaced": replaced, "evictions": evictions, "log_head": oracle.log_head()}
