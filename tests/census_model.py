"""The table census and digest of include/hermeskv.h ("Table census and digest") restated in numpy over a table
image in the reference's byte layout: (index, log, log_head, log_cap, sizes). Written from the header's text and
hermes_amd.layout.entry_dtype, not from the kernel, so the device result, two replicas and two layouts can be
held against it.

A slot is live when it is in use (bit 0) and log_head - offset < log_cap, offset = slot >> 24 (the lookup's window
check, unsigned); its entry, at log[offset & (log_cap - 1)], is a live key.
"""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
FIELDS = ("keys", "dead_slots", "by_state", "obi_set", "not_valid_by_cid", "max_ts", "digest_sum", "digest_xor",
          "from_lines", "offenders")


def mix64(x: np.ndarray) -> np.ndarray:
    """the splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)"""
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def digest_mask(sizes: L.Sizes) -> np.ndarray:
    """the bytes of an entry the digest keeps: key, state, ts cid, ts version, value"""
    dt = L.entry_dtype(sizes)
    keep = np.zeros(sizes.entry, np.uint8)
    for name in ("key", "state", "ts_cid", "ts_ver", "value"):
        sub, off = dt.fields[name][0], dt.fields[name][1]
        keep[off:off + sub.itemsize] = 0xFF
    assert np.nonzero(keep)[0].tolist() == list(range(8, 16)) + [18, 23] + list(range(24, 28)) + \
        list(range(33, 33 + sizes.st_value))
    return keep


def entry_hashes(entries: np.ndarray, sizes: L.Sizes) -> np.ndarray:
    """h of every entry of entries [n][E] (uint8)"""
    m = (entries & digest_mask(sizes)[None, :]).copy().view("<u8").reshape(len(entries), sizes.entry // 8)
    assert not m[:, 0].any()
    e = np.zeros(len(entries), np.uint64)
    for i in range(1, sizes.entry // 8):
        e += mix64(m[:, i] + np.uint64(((i + 1) * G) & M64))
    return mix64(e)


def live_entries(index: np.ndarray, log: np.ndarray, log_head: int, cap: int, sizes: L.Sizes):
    """(entries [n][E] of the live slots in bucket and slot order, their (bucket, slot), in-use slots that are
    not live)"""
    E = sizes.entry
    log = np.asarray(log, np.uint8).reshape(-1)
    if len(log) < cap + E:   # an entry never runs past the log's slack; the image may come without it
        log = np.concatenate([log, np.zeros(cap + E - len(log), np.uint8)])
    slots = np.asarray(index, np.uint8).reshape(-1).view("<u8").reshape(-1, 8)
    used = (slots & np.uint64(1)).astype(bool)
    off = slots >> np.uint64(24)
    live = used & ((np.uint64(log_head) - off) < np.uint64(cap))
    bkt, slot = np.nonzero(live)
    phys = (off[bkt, slot] & np.uint64(cap - 1)).astype(np.int64)
    entries = log[phys[:, None] + np.arange(E)[None, :]]
    return entries, bkt, slot, int((used & ~live).sum())


def census_model(index, log, log_head: int, cap: int, sizes: L.Sizes = L.DEFAULT, inline: bool = False) -> dict:
    """hkv_census of the image as a dict of Python integers (and lists). inline: the image is that of a table in
    INLINE state, whose library reads every bucket's lowest in-use slot's entry from its line (from_lines)."""
    entries, bkt, slot, dead = live_entries(index, log, log_head, cap, sizes)
    n = len(entries)
    ent = entries.copy().view(L.entry_dtype(sizes)).reshape(-1)
    state, obi, cid = ent["state"].astype(np.int64), ent["obi"], ent["ts_cid"].astype(np.int64)
    ts = (ent["ts_ver"].astype(np.uint64) << np.uint64(8)) | cid.astype(np.uint64)
    h = entry_hashes(entries, sizes)
    not_valid = state != int(L.State.VALID)
    si = np.where((state >= 1) & (state <= 5), state, 0)
    ci = np.where(cid < 8, cid, 8)
    from_lines = 0
    if inline:
        used = (np.asarray(index, np.uint8).reshape(-1).view("<u8").reshape(-1, 8) & np.uint64(1)).astype(bool)
        first = np.where(used.any(axis=1), used.argmax(axis=1), -1)
        from_lines = int((slot == first[bkt]).sum())
    return {"keys": n, "dead_slots": dead,
            "by_state": np.bincount(si, minlength=8).tolist(),
            "obi_set": int((obi != L.OBI_EMPTY).sum()),
            "not_valid_by_cid": np.bincount(ci[not_valid], minlength=9).tolist(),
            "max_ts": int(ts.max()) if n else 0,
            "digest_sum": int(h.sum(dtype=np.uint64)) if n else 0,
            "digest_xor": int(np.bitwise_xor.reduce(mix64(h + np.uint64(G)))) if n else 0,
            "from_lines": from_lines, "offenders": int(not_valid.sum())}


def offender_keys(index, log, log_head: int, cap: int, sizes: L.Sizes = L.DEFAULT) -> np.ndarray:
    """the keys (uint64, sorted) of the live keys that are not VALID"""
    entries, *_ = live_entries(index, log, log_head, cap, sizes)
    ent = entries.copy().view(L.entry_dtype(sizes)).reshape(-1)
    return np.sort(ent["key"][ent["state"] != int(L.State.VALID)].astype(np.uint64))


def oracle_image(o, sizes: L.Sizes = L.DEFAULT):
    """(index, log, log_head, cap, sizes) of an OracleKVS, copied. The log comes with the one entry of slack behind
    log_cap that the oracle (like the device table) allocates: an entry that starts just below the capacity runs
    into it (320-byte entries in a wrapped log), and OracleKVS.log_bytes() ends at the capacity."""
    from oracle.oracle import lib
    log = np.ctypeslib.as_array(lib().hko_log(o.h), shape=(o.log_cap + sizes.entry,)).copy()
    return o.index_bytes().copy(), log, o.log_head(), o.log_cap, sizes


def digest(c: dict) -> tuple:
    return c["digest_sum"], c["digest_xor"]


def assert_not_vacuous(seq: list) -> None:
    """somewhere in a sequence of censuses: three states or more at once, two writers or more of keys that are
    not VALID at once, and an op buffer index"""
    assert max(sum(1 for x in c["by_state"] if x) for c in seq) >= 3, [c["by_state"] for c in seq]
    assert max(sum(1 for x in c["not_valid_by_cid"] if x) for c in seq) >= 2, [c["not_valid_by_cid"] for c in seq]
    assert max(c["obi_set"] for c in seq) > 0
