"""Upsert on the oracle alone (include/hermeskv.h, "Upsert"; tests/upsert_model.py): (a) the model's insert is the
reference's -- populate's images inserted in reverse id order give hko_populate's index, log, head and evictions
byte for byte; (b) the definition carries a scripted table's replicated state into an empty table of another
geometry, a second upsert inserts nothing, a key caught mid-write arrives INVALID, and two records of one bucket
and tag leave only the later one reachable; (c) the ABI of the call (no GPU needed: the refusals come before any
device work).
"""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, cityhash128, gen_keys
from tests import census_model as CM
from tests import repair_cases as RC
from tests import repair_model as RM
from tests import upsert_model as UM

S = L.DEFAULT
MB = L.membership(RC.N_MACH, RC.DST_ID)


# ------------------------------------------------------------------ (a) the model is the reference's insert
@pytest.mark.parametrize("n_keys,bkts,cap,big", [
    (5000, 16384, 1 << 20, False),
    (20000, 2048, 1 << 21, False),     # evictions
    (3000, 4096, 1 << 17, False),      # the log wraps
    (1500, 256, 1 << 20, True),        # 320-B entries
])
def test_model_insert_is_populate(n_keys, bkts, cap, big):
    sizes = L.BIG if big else S
    ref = OracleKVS(bkts, cap, 0, False, big, 4 if big else 0)
    ref.populate(n_keys, sizes.kvs_value)
    o = OracleKVS(bkts, cap, 0, False, big, 4 if big else 0)
    replaced = evictions = 0
    for i in range(n_keys - 1, -1, -1):
        first, second = cityhash128(int(i).to_bytes(4, "little"))
        r, e = UM.mica_insert(o, UM.populate_image(first, second, ord("a") + i % 20, sizes), sizes)
        replaced, evictions = replaced + r, evictions + e
    assert o.log_head() == ref.log_head()
    assert evictions == ref.evictions()
    assert np.array_equal(o.index_bytes(), ref.index_bytes())
    assert np.array_equal(CM.oracle_image(o, sizes)[1], CM.oracle_image(ref, sizes)[1])
    if (n_keys, bkts) == (20000, 2048):
        assert evictions > 0
    if cap == 1 << 17:
        assert o.log_head() > cap


# ------------------------------------------------------------------ (b) the definition on the oracle alone
@pytest.fixture(scope="module")
def source():
    """5000 keys in 16384 buckets after tests/repair_cases.source_script: VALID, INVALID, WRITE, INVALID_WRITE"""
    o = OracleKVS(16384, 1 << 20, RC.SRC_ID)
    o.populate(5000, S.kvs_value)
    RC.source_script(lambda bt, e, mb: o.batch_multi(bt, e, 1, len(e), None, mb), gen_keys(5000), S)
    image = CM.oracle_image(o, S)
    rec = RM.extract_model(image)
    rec = rec[np.random.default_rng(11).permutation(len(rec))]
    return o, CM.census_model(*image), rec


def test_upsert_into_empty_table(source):
    """the source's records into an empty table of a quarter of the buckets: nothing replaced or evicted (asserted,
    the geometry was picked for it), so every key arrives and the census agrees in the replicated fields, with the
    keys the source caught mid-write INVALID on both sides of the comparison"""
    o, census, rec = source
    t = OracleKVS(4096, 1 << 19, RC.DST_ID)
    out = UM.upsert_model(t, rec, S, MB)
    assert out == {"raised": 0, "equal": 0, "older": 0, "inserted": len(rec), "replaced": 0, "evictions": 0,
                   "log_head": len(rec) * S.entry}
    got = CM.census_model(*CM.oracle_image(t, S))
    # a key caught mid-write (WRITE, INVALID_WRITE) arrives INVALID: fold the source's states the same way
    quiet = rec.copy()
    quiet[:, 18] = np.where(quiet[:, 18] == int(L.State.VALID), int(L.State.VALID), int(L.State.INVALID))
    h = CM.entry_hashes(quiet, S)
    assert got["keys"] == census["keys"] == len(rec)
    assert got["digest_sum"] == int(h.sum(dtype=np.uint64))
    assert got["digest_xor"] == int(np.bitwise_xor.reduce(CM.mix64(h + np.uint64(CM.G))))
    want_states = np.bincount(quiet[:, 18], minlength=8).tolist()
    assert got["by_state"] == want_states
    # a second upsert inserts nothing and counts everything equal
    image = CM.oracle_image(t, S)
    again = UM.upsert_model(t, rec, S, MB)
    assert again == {"raised": 0, "equal": len(rec), "older": 0, "inserted": 0, "replaced": 0, "evictions": 0,
                     "log_head": out["log_head"]}
    after = CM.oracle_image(t, S)
    assert np.array_equal(image[0], after[0]) and np.array_equal(image[1], after[1])


def test_quiet_source_census_equal():
    """a quiet source (every key VALID): source and target censuses are equal in digest_sum, digest_xor, keys and
    by_state outright"""
    o = OracleKVS(16384, 1 << 20, RC.SRC_ID)
    o.populate(5000, S.kvs_value)
    keys = gen_keys(5000)
    ids = np.arange(100, 300)
    o.batch_multi(L.BatchType.invs, RC.invs(keys, ids, 1, (4, 1), S, 2), 1, len(ids), None, L.membership(RC.N_MACH, 0))
    o.batch_multi(L.BatchType.vals, RC.vals(keys, ids, 1, (4, 1)), 1, len(ids), None, L.membership(RC.N_MACH, 0))
    image = CM.oracle_image(o, S)
    t = OracleKVS(4096, 1 << 19, RC.DST_ID)
    out = UM.upsert_model(t, RM.extract_model(image), S, MB)
    assert out["replaced"] == out["evictions"] == 0 and out["inserted"] == 5000
    a, b = CM.census_model(*image), CM.census_model(*CM.oracle_image(t, S))
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert a[f] == b[f], f


def test_mid_write_key_arrives_invalid(source):
    o, _, rec = source
    keys = gen_keys(5000)
    k = int(keys[RC.PUT[0]])                       # the source's own PUT, still in WRITE at (2, SRC_ID)
    r = rec[rec[:, 8:16].copy().view("<u8").reshape(-1) == k]
    assert len(r) == 1 and r[0, 18] == int(L.State.WRITE)
    t = OracleKVS(1024, 1 << 17, RC.DST_ID)
    out = UM.upsert_model(t, r, S, MB)
    assert out["inserted"] == 1
    e = CM.oracle_image(t, S)[1][:S.entry].view(L.entry_dtype(S))[0]
    assert e["key"] == k and e["state"] == int(L.State.INVALID)
    assert e["rmw_lwid"] >> 1 == RC.SRC_ID and e["ts_cid"] == RC.SRC_ID and e["ts_ver"] == r.view(L.entry_dtype(S))[0]["ts_ver"]
    assert e["key_first"] == 0 and np.array_equal(e["value"], r[0, 33:])


def test_same_bucket_and_tag_replaces():
    """two records whose keys share bucket and tag: the later insert takes the earlier one's slot"""
    a = (0x1234 << 48) | (7 << 20) | 5
    b = (0x1234 << 48) | (9 << 20) | 5             # bits 20.. are above a 1024-bucket mask: same bucket, same tag
    rec = RC.make_records(np.array([a, b], np.uint64), [int(L.State.VALID)] * 2, 4, 1, S, 9)   # (versions are even: odd is the seqlock's "locked")
    t = OracleKVS(1024, 1 << 17, RC.DST_ID)
    out = UM.upsert_model(t, rec, S, MB)
    assert out["inserted"] == 2 and out["replaced"] == 1 and out["evictions"] == 0
    assert t.lookup(a) is None and t.lookup(b) == S.entry
    assert CM.census_model(*CM.oracle_image(t, S))["keys"] == 1


# ------------------------------------------------------------------ (c) ABI
def test_abi():
    from hermes_amd import lib
    r = lib.raw()
    assert r.hkv_upsert_result_bytes() == 64 == ctypes.sizeof(lib.HkvUpsertResult)
    assert r.hkv_abi_version() == 10
    res = (ctypes.c_uint8 * 64)(*([0xA5] * 64))
    rec = (ctypes.c_uint8 * 128)(*([0x5A] * 128))
    rc = r.hkv_table_upsert(None, ctypes.cast(rec, ctypes.c_void_p), 2,
                            ctypes.cast(res, ctypes.POINTER(lib.HkvUpsertResult)), None)
    assert rc < 0 and b"upsert" in r.hkv_last_error()
    assert bytes(res) == b"\xA5" * 64 and bytes(rec) == b"\x5A" * 128, "a refused call wrote"
