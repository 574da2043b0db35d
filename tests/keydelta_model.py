"""The key-level delta repair of include/hermeskv.h ("Key-level delta repair") restated in numpy, on
tests/census_model.py, tests/repair_model.py and tests/delta_model.py. Written from the header's text, not from the
kernels: a summary is 16 bytes of its record, the six classes compare a summary with the entry the reference's
lookup finds, and a fetch is that entry under the digest's mask, by position.

An image is census_model's (index, log, log_head, cap, sizes).
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L
from tests import census_model as CM
from tests import delta_model as DM
from tests import repair_model as RM

SUMMARY = np.dtype([("key", "<u8"), ("ts_ver", "<u4"), ("ts_cid", "u1"), ("state", "u1"), ("zero", "u1", (2,))])
assert SUMMARY.itemsize == 16
CLASSES = ("missed", "newer", "validate", "same", "state_only", "older")
NEEDED = ("missed", "newer", "validate")
VALID = int(L.State.VALID)


def summaries_of_records(records: np.ndarray, sizes: L.Sizes) -> np.ndarray:
    """one summary per record, in the records' order: a function of the record's bytes alone"""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, sizes.entry).copy().view(L.entry_dtype(sizes)).reshape(-1)
    out = np.zeros(len(rec), SUMMARY)
    out["key"], out["ts_ver"], out["ts_cid"], out["state"] = rec["key"], rec["ts_ver"], rec["ts_cid"], rec["state"]
    return out


def sort_summaries(s: np.ndarray) -> np.ndarray:
    """summaries as sorted 16-byte rows (the device writes them in no particular order)"""
    s = np.ascontiguousarray(s).view(np.uint8).reshape(-1, 16)
    return s[np.lexsort(s.T[::-1])]


def summaries_model(image, part_bits: int = 0, mask=None, rng: tuple | None = None, min_ts: int = 0) -> np.ndarray:
    """the summaries (SUMMARY array, by key) of the records the masked extract would emit: the live keys of the
    buckets `rng` = (lo, hi) (default: all) whose partition key & (2^part_bits - 1) has a non-zero mask byte (mask
    None: every partition) and whose timestamp is at least min_ts"""
    lo, hi = (None, None) if rng is None else rng
    assert (1 << part_bits) <= DM.num_buckets(image)
    rec = RM.extract_model(image, lo, hi, min_ts) if mask is None else \
        DM.extract_parts_model(image, part_bits, mask, lo, hi, min_ts)
    return summaries_of_records(rec, image[4])


def lookup_image(image, key: int):
    """the reference's lookup on an image: the first in-use slot of the key's bucket that carries its tag, the
    window check, the 8-byte key compare; the entry's offset in the log, or None"""
    index, log, head, cap, sizes = image
    slots = np.asarray(index, np.uint8).reshape(-1).view("<u8").reshape(-1, 8)
    key = int(key)
    bkt = (key & 0xFFFFFFFFFFFF) & (len(slots) - 1)
    tag = key >> 48
    for s in slots[bkt].tolist():
        if s & 1 and ((s >> 1) & 0x7FFFFF) == tag:
            off = s >> 24
            if (head - off) % (1 << 64) >= cap:
                return None
            phys = off & (cap - 1)
            k = int(np.asarray(log[phys + 8:phys + 16]).copy().view("<u8")[0])
            return phys if k == key else None
    return None


def classify(s_ts: int, s_state: int, e_ts: int | None, e_state: int | None) -> str:
    """a summary (packed timestamp, state) against the entry the lookup found (None: no entry)"""
    if e_ts is None:
        return "missed"
    if s_ts != e_ts:
        return "newer" if s_ts > e_ts else "older"
    if s_state == e_state:
        return "same"
    return "validate" if s_state == VALID else "state_only"


def need_model(oracle, summaries: np.ndarray, sizes: L.Sizes = L.DEFAULT):
    """(counts by class plus needed, the needed keys sorted (uint64, a key as often as it was summarised), the
    class of every summary) of the summaries against the oracle's table as it is now (OracleKVS.lookup)"""
    from oracle.oracle import lib
    log = np.ctypeslib.as_array(lib().hko_log(oracle.h), shape=(oracle.log_cap + sizes.entry,))
    s = np.ascontiguousarray(summaries).view(SUMMARY).reshape(-1)
    cls = []
    for key, ver, cid, st in zip(s["key"].tolist(), s["ts_ver"].tolist(), s["ts_cid"].tolist(), s["state"].tolist()):
        off = oracle.lookup(key)
        if off is None:
            cls.append("missed")
            continue
        e_ts = (int.from_bytes(log[off + 24:off + 28].tobytes(), "little") << 8) | int(log[off + 23])
        cls.append(classify((ver << 8) | cid, st, e_ts, int(log[off + 18])))
    cls = np.array(cls, dtype=object)
    counts = {c: int((cls == c).sum()) for c in CLASSES}
    need = np.isin(cls, NEEDED) if len(cls) else np.zeros(0, bool)
    counts["needed"] = int(need.sum())
    return counts, np.sort(s["key"][need].astype(np.uint64)), cls


def fetch_model(image, keys) -> np.ndarray:
    """records [n][E] by position: key i's entry under the digest's mask, or zero but for the key bytes 8..15"""
    sizes = image[4]
    E = sizes.entry
    log = np.asarray(image[1], np.uint8).reshape(-1)
    if len(log) < image[3] + E:
        log = np.concatenate([log, np.zeros(image[3] + E - len(log), np.uint8)])
    keys = np.asarray(keys, np.uint64).reshape(-1)
    out = np.zeros((len(keys), E), np.uint8)
    keep = CM.digest_mask(sizes)
    for i, k in enumerate(keys.tolist()):
        off = lookup_image((image[0], log, image[2], image[3], sizes), k)
        if off is None:
            out[i, 8:16] = np.array([k], "<u8").view(np.uint8)
        else:
            out[i] = log[off:off + E] & keep
    return out
