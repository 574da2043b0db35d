"""The partitioned census and the masked extract of include/hermeskv.h ("Partitioned census and delta repair")
restated in numpy on tests/census_model.py and tests/repair_model.py. Written from the header's text, not from the
kernels: partition p of P = 2^part_bits holds the live keys with key & (P - 1) == p, a row is the census's
digest_sum, digest_xor, keys and not-VALID count over them, and the masked extract is the extract filtered by the
key's partition (which, for P <= num_bkts, is its bucket's).

An image is census_model's (index, log, log_head, cap, sizes).
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L
from tests import census_model as CM
from tests import repair_model as RM

ROW = ("digest_sum", "digest_xor", "keys", "not_valid")


def num_buckets(image) -> int:
    return len(np.asarray(image[0]).reshape(-1)) // 64


def part_rows_model(image, part_bits: int) -> np.ndarray:
    """rows [P][4] uint64: (digest_sum, digest_xor, keys, not_valid) of every partition"""
    index, log, head, cap, sizes = image
    P = 1 << part_bits
    assert P <= num_buckets(image), "part_bits <= log2(num_bkts)"
    entries, *_ = CM.live_entries(index, log, head, cap, sizes)
    rows = np.zeros((P, 4), np.uint64)
    if not len(entries):
        return rows
    ent = entries.copy().view(L.entry_dtype(sizes)).reshape(-1)
    part = (ent["key"].astype(np.uint64) & np.uint64(P - 1)).astype(np.int64)
    h = CM.entry_hashes(entries, sizes)
    np.add.at(rows[:, 0], part, h)
    np.bitwise_xor.at(rows[:, 1], part, CM.mix64(h + np.uint64(CM.G)))
    np.add.at(rows[:, 2], part, np.uint64(1))
    np.add.at(rows[:, 3], part, (ent["state"] != int(L.State.VALID)).astype(np.uint64))
    return rows


def fold(rows: np.ndarray) -> dict:
    """the rows folded over the partitions: what the census reports in digest_sum, digest_xor, keys, offenders"""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    return {"digest_sum": int(rows[:, 0].sum(dtype=np.uint64)), "digest_xor": int(np.bitwise_xor.reduce(rows[:, 1])),
            "keys": int(rows[:, 2].sum(dtype=np.uint64)), "offenders": int(rows[:, 3].sum(dtype=np.uint64))}


def census_fold(census: dict) -> dict:
    return {k: census[k] for k in ("digest_sum", "digest_xor", "keys", "offenders")}


def _selected(records: np.ndarray, part_bits: int, mask) -> np.ndarray:
    keys = records[:, 8:16].copy().view("<u8").reshape(-1)
    return np.asarray(mask).reshape(-1)[(keys & np.uint64((1 << part_bits) - 1)).astype(np.int64)] != 0


def extract_parts_model(image, part_bits: int, mask, lo: int | None = None, hi: int | None = None,
                        min_ts: int = 0) -> np.ndarray:
    """repair_model.extract_model filtered by key & (P - 1): the records, sorted by key, of the live keys of the
    buckets [lo, hi) whose partition has a non-zero mask byte and whose timestamp is at least min_ts"""
    assert len(np.asarray(mask).reshape(-1)) == 1 << part_bits <= num_buckets(image)
    rec = RM.extract_model(image, lo, hi, min_ts)
    return rec[_selected(rec, part_bits, mask)]


def scanned_parts_model(image, part_bits: int, mask, lo: int | None = None, hi: int | None = None) -> int:
    """scanned_keys of the masked extract: the live slots of the selected buckets of the range, whatever their
    timestamp"""
    return int(_selected(RM.extract_model(image, lo, hi), part_bits, mask).sum())


def diff_model(rows_a: np.ndarray, rows_b: np.ndarray, mask=None):
    """(mask uint8[P], count) of hkv_part_rows_diff_async; mask given: accumulate"""
    d = (np.asarray(rows_a, np.uint64) != np.asarray(rows_b, np.uint64)).any(axis=1).astype(np.uint8)
    out = d if mask is None else (np.asarray(mask, np.uint8) | d)
    return out, int((out != 0).sum())
