"""Replica repair (include/hermeskv.h, "Replica repair") restated in numpy, on tests/census_model.py: what an extract
of a table image holds, the two reference batches that define an install, and the install's counts. Written from
the header's text, not from the kernels, so the device can be held against it and the definition can be checked
on the oracle alone (tests/test_repair_cpu.py).

An image is census_model's (index, log, log_head, cap, sizes).
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L
from tests import census_model as CM

COUNTS = ("raised", "equal", "older", "missed")


def sort_records(records: np.ndarray, sizes: L.Sizes) -> np.ndarray:
    """records [n][E] ordered by key (an extract writes them in no particular order)"""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry)
    keys = records[:, 8:16].copy().view("<u8").reshape(-1)
    return records[np.argsort(keys, kind="stable")]


def _in_range(image, bkt_lo, bkt_hi):
    index, log, head, cap, sizes = image
    entries, bkt, _, _ = CM.live_entries(index, log, head, cap, sizes)
    n_bkts = len(np.asarray(index).reshape(-1)) // 64
    lo, hi = 0 if bkt_lo is None else bkt_lo, n_bkts if bkt_hi is None else bkt_hi
    return entries, (bkt >= lo) & (bkt < hi)


def extract_model(image, bkt_lo: int | None = None, bkt_hi: int | None = None, min_ts: int = 0) -> np.ndarray:
    """records [n][E] sorted by key: one record -- the entry under the digest's mask -- per live slot of the
    buckets [bkt_lo, bkt_hi) (default: all) whose (version << 8 | cid) is at least min_ts"""
    sizes = image[4]
    entries, in_range = _in_range(image, bkt_lo, bkt_hi)
    ent = entries.copy().view(L.entry_dtype(sizes)).reshape(-1)
    take = in_range & (L.ts64(ent["ts_ver"], ent["ts_cid"]) >= np.uint64(min_ts))
    return sort_records(entries[take] & CM.digest_mask(sizes)[None, :], sizes)


def scanned_model(image, bkt_lo: int | None = None, bkt_hi: int | None = None) -> int:
    """hkv_extract_result.scanned_keys: the range's live slots, whatever their timestamp"""
    return int(_in_range(image, bkt_lo, bkt_hi)[1].sum())


def records_to_batches(records: np.ndarray, sizes: L.Sizes):
    """(INVs as op_dtype, VALs as msg_dtype): the `invs` batch of one INV per record (opcode ST_OP_INV, the
    record's key, timestamp and value, sender = ts cid, val_len ST_VALUE_SIZE as the worker's INVs carry it, RMW
    flag 0) and the `vals` batch of one VAL per record whose state is VALID"""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry).copy().view(L.entry_dtype(sizes)).reshape(-1)
    inv = np.zeros(len(rec), dtype=L.op_dtype(sizes))
    inv["key"] = rec["key"]
    inv["opcode"] = int(L.Op.INV)
    inv["state"] = rec["ts_cid"]            # the sender
    inv["val_len"] = sizes.st_value >> sizes.shift
    inv["ts_cid"], inv["ts_ver"] = rec["ts_cid"], rec["ts_ver"]
    inv["flags"] = 0
    inv["value"] = rec["value"]
    v = rec[rec["state"] == int(L.State.VALID)]
    val = np.zeros(len(v), dtype=L.msg_dtype())
    val["key"] = v["key"]
    val["opcode"] = int(L.Op.VAL)
    val["sender"] = v["ts_cid"]
    val["ts_cid"], val["ts_ver"] = v["ts_cid"], v["ts_ver"]
    return inv, val


def apply_records(oracle, records: np.ndarray, sizes: L.Sizes, membership: bytes) -> None:
    """the install by its definition: the two batches through OracleKVS.batch, one after the other"""
    inv, val = records_to_batches(records, sizes)
    if len(inv):
        oracle.batch(L.BatchType.invs, inv, membership)
    if len(val):
        oracle.batch(L.BatchType.vals, val, membership)


def install_counts(oracle, records: np.ndarray, sizes: L.Sizes = L.DEFAULT) -> dict:
    """raised / equal / older / missed of the records against the oracle's table as it is now (OracleKVS.lookup:
    call before the batches run)"""
    from oracle.oracle import lib
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry).copy().view(L.entry_dtype(sizes)).reshape(-1)
    log = np.ctypeslib.as_array(lib().hko_log(oracle.h), shape=(oracle.log_cap + sizes.entry,))
    out = dict.fromkeys(COUNTS, 0)
    ts = L.ts64(rec["ts_ver"], rec["ts_cid"]).tolist()
    ver_lo, cid_at = 24, 23          # entry bytes of ts version (4, little-endian) and ts cid
    for key, mine in zip(rec["key"].tolist(), ts):
        off = oracle.lookup(key)
        if off is None:
            out["missed"] += 1
            continue
        theirs = (int.from_bytes(log[off + ver_lo:off + ver_lo + 4].tobytes(), "little") << 8) | int(log[off + cid_at])
        out["raised" if mine > theirs else "equal" if mine == theirs else "older"] += 1
    return out
