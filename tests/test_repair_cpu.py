"""Replica repair on the oracle alone: the definition of include/hermeskv.h ("Replica repair") -- an install is the
reference applying one INV per record and then one VAL per record whose source state was VALID -- carries a table's
replicated state to a table of another geometry, is idempotent, never moves a key backwards and misses unknown
keys; an extract's records hash to the source's digest and its filters partition it. Then the ABI of the two calls
(no GPU needed: the refusals come before any device work).
"""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import census_model as CM
from tests import repair_cases as RC
from tests import repair_model as RM

S = L.DEFAULT
N_KEYS = 5000


class _Done(Exception):
    pass


def _table(bkts, cap, n_keys=N_KEYS, machine_id=0):
    o = OracleKVS(bkts, cap, machine_id)
    o.populate(n_keys, S.kvs_value)
    return o


@pytest.fixture(scope="module")
def table_a():
    """5000 keys in 16384 buckets after the first three launches of tests/scripted.py (local ops, INVs, ACKs):
    VALID, INVALID and WRITE keys"""
    from tests.scripted import run_scripted
    o = _table(16384, 1 << 20)
    n = [0]

    def runner(btype, elems, mb, rw=None, node_suspected=None):
        o.batch_multi(btype, elems, 1, len(elems), None, mb, rw=rw, node_suspected=node_suspected)
        n[0] += 1
        if n[0] == 3:
            raise _Done

    with pytest.raises(_Done):
        run_scripted(runner, gen_keys(N_KEYS), S, False)
    image = CM.oracle_image(o, S)
    census = CM.census_model(*image)
    assert sum(1 for x in census["by_state"] if x) >= 3, census["by_state"]
    return o, image, census, RM.extract_model(image)


def _entries_by_key(image):
    entries, *_ = CM.live_entries(*image)
    ent = entries.copy().view(L.entry_dtype(image[4])).reshape(-1)
    return {int(e["key"]): e for e in ent}


def _expected_digest(records, image_b_before):
    """the digest B must have after the install: every key B holds and the records carry takes the record's key,
    timestamp and value and is VALID when the source was, INVALID otherwise; B's other keys keep their entries"""
    want = {int(r[8:16].copy().view("<u8")[0]): r.copy() for r in records}
    for r in want.values():
        if r[18] != int(L.State.VALID):
            r[18] = int(L.State.INVALID)
    sizes = image_b_before[4]
    entries, *_ = CM.live_entries(*image_b_before)
    masked = entries & CM.digest_mask(sizes)[None, :]
    exp = np.stack([want.get(int(m[8:16].copy().view("<u8")[0]), m) for m in masked])
    h = CM.entry_hashes(exp, sizes)
    return int(h.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(CM.mix64(h + np.uint64(CM.G))))


def test_geometry_independence_idempotence(table_a):
    """A's records into B, the same keys freshly populated in an eighth of the buckets. State is part of the
    digest and a key the source caught mid-write arrives INVALID, so B's digest is A's with those keys' state byte
    INVALID (equal to A's outright once A is quiet: test_quiet_source_digest_equal)."""
    _, image_a, census_a, records = table_a
    _independence_idempotence(image_a, census_a, records, _table(2048, 1 << 19), S)


def _independence_idempotence(image_a, census_a, records, b, S):
    mb = L.membership(5, 0)
    image_b0 = CM.oracle_image(b, S)
    counts = RM.install_counts(b, records, S)
    assert counts["raised"] > 0 and counts["equal"] > 0 and counts["older"] == 0
    RM.apply_records(b, records, S, mb)
    image_b = CM.oracle_image(b, S)
    census_b = CM.census_model(*image_b)
    ea, eb = _entries_by_key(image_a), _entries_by_key(image_b)
    assert counts["missed"] == len(set(ea) - set(eb))     # (keys B's fuller buckets evicted at populate)
    assert CM.digest(census_b) == _expected_digest(records, image_b0)
    if set(ea) == set(eb) and census_a["offenders"] == 0:
        assert CM.digest(census_b) == CM.digest(census_a)
    n_valid = n_not = 0
    for k, a in ea.items():
        if k not in eb:
            continue
        e = eb[k]
        assert (int(e["ts_ver"]), int(e["ts_cid"])) == (int(a["ts_ver"]), int(a["ts_cid"]))
        assert np.array_equal(e["value"], a["value"])
        if int(a["state"]) == int(L.State.VALID):
            assert int(e["state"]) == int(L.State.VALID)
            n_valid += 1
        else:   # caught mid-write at the source: INVALID at the source's timestamp
            assert int(e["state"]) == int(L.State.INVALID)
            n_not += 1
    assert n_valid > 0 and n_not > 0
    assert census_b["by_state"][int(L.State.VALID)] == n_valid + len(set(eb) - set(ea))
    assert census_b["by_state"][int(L.State.INVALID)] == n_not
    # idempotence: the same records again change no byte
    before = (b.index_bytes().copy(), image_b[1])
    again = RM.install_counts(b, records, S)
    assert again["raised"] == 0 and again["equal"] == counts["raised"] + counts["equal"]
    RM.apply_records(b, records, S, mb)
    assert np.array_equal(b.index_bytes(), before[0]) and np.array_equal(CM.oracle_image(b, S)[1], before[1])


@pytest.mark.parametrize("ecl", [1, 2, 5, 8, 16])
def test_geometry_independence_idempotence_value_sizes(ecl):
    """The same at the five big-object sizes of tests/test_value_sizes_gpu.py: a source of 1500 keys in 2048
    buckets whose log wraps (the capacity is the largest power of two below 1500 entries, so the highest ids, populated
    first, are dead slots), scripted by tests/repair_cases.py over its lowest ids, into a fresh target of the same ids in
    512 buckets and a log that does not wrap."""
    sizes = L.Sizes(True, ecl)
    n = 1500
    cap = 1 << ((n * sizes.entry).bit_length() - 1)
    assert cap < n * sizes.entry
    a = OracleKVS(2048, cap, RC.SRC_ID, False, True, ecl)
    a.populate(n, sizes.kvs_value)
    keys = gen_keys(n)
    assert a.lookup(int(keys[n - 1])) is None and cap // sizes.entry - 8 > RC.TW[1]   # the script's ids are live
    RC.source_script(lambda bt, e, mb: a.batch_multi(bt, e, 1, len(e), None, mb), keys, sizes)
    image_a = CM.oracle_image(a, sizes)
    census_a = CM.census_model(*image_a)
    assert census_a["dead_slots"] > 0 and 0 < census_a["keys"] < n
    assert sum(1 for x in census_a["by_state"] if x) >= 4, census_a["by_state"]
    records = RM.extract_model(image_a)
    assert len(records) == census_a["keys"] and records.shape[1] == sizes.entry
    b = OracleKVS(512, 1 << (n * sizes.entry + 2048).bit_length(), 0, False, True, ecl)
    b.populate(n, sizes.kvs_value)
    _independence_idempotence(image_a, census_a, records, b, sizes)


def test_quiet_source_digest_equal():
    """a source with every key VALID (the quiet group a resync is for): B's digest equals A's, in other buckets"""
    keys = gen_keys(N_KEYS)
    a = _table(16384, 1 << 20)
    mb = L.membership(5, 0)
    ids = np.arange(100, 400)
    inv = RC.invs(keys, ids, 1, (4, 1), S, 9)
    a.batch(L.BatchType.invs, inv, mb)
    a.batch(L.BatchType.vals, RC.vals(keys, ids, 1, (4, 1)), mb)
    census_a = CM.census_model(*CM.oracle_image(a, S))
    assert census_a["by_state"][int(L.State.VALID)] == census_a["keys"] and census_a["max_ts"] == (4 << 8) | 1
    b = _table(1 << 15, 1 << 19)
    fresh = CM.census_model(*CM.oracle_image(b, S))
    assert CM.digest(fresh) != CM.digest(census_a)
    RM.apply_records(b, RM.extract_model(CM.oracle_image(a, S)), S, mb)
    assert CM.digest(CM.census_model(*CM.oracle_image(b, S))) == CM.digest(census_a)


def test_older_records_change_nothing(table_a):
    _, _, _, records = table_a
    keys = gen_keys(N_KEYS)
    b = _table(2048, 1 << 19)
    mb = L.membership(5, 0)
    # B moves every key the source wrote past the source's timestamps
    rec = records.copy().view(L.entry_dtype(S)).reshape(-1)
    written = rec[rec["ts_ver"] > 0]
    assert len(written) >= 5
    ids = np.nonzero(np.isin(keys, written["key"]))[0]
    b.batch(L.BatchType.invs, RC.invs(keys, ids, 3, (40, 3), S, 4), mb)
    only = RM.sort_records(written.view(np.uint8).reshape(-1, S.entry), S)
    counts = RM.install_counts(b, only)
    assert counts["older"] > 0 and counts["raised"] == counts["equal"] == 0
    before = (b.index_bytes().copy(), CM.oracle_image(b, S)[1])
    RM.apply_records(b, only, S, mb)
    assert np.array_equal(b.index_bytes(), before[0]) and np.array_equal(CM.oracle_image(b, S)[1], before[1])


def test_missing_key_is_a_miss(table_a):
    _, _, _, records = table_a
    b = _table(2048, 1 << 19, n_keys=200)      # ids 0..199 only
    keys = gen_keys(N_KEYS)
    rec = records.copy().view(L.entry_dtype(S)).reshape(-1)
    absent = rec[np.isin(rec["key"], keys[200:])][:50]
    assert len(absent) == 50
    only = absent.view(np.uint8).reshape(-1, S.entry)
    assert RM.install_counts(b, only) == {"raised": 0, "equal": 0, "older": 0, "missed": 50}
    inv, val = RM.records_to_batches(only, S)
    before = (b.index_bytes().copy(), CM.oracle_image(b, S)[1])
    b.batch(L.BatchType.invs, inv, L.membership(5, 0))
    assert (inv["state"] == int(L.Resp.MISS)).all()
    RM.apply_records(b, only, S, L.membership(5, 0))
    assert np.array_equal(b.index_bytes(), before[0]) and np.array_equal(CM.oracle_image(b, S)[1], before[1])


@pytest.mark.parametrize("rounds", [0, 2])
def test_tag_collision_records_miss(rounds):
    """the inputs of tests/test_repair_gpu.py::test_install_tag_collisions on the oracle alone, on a fresh table and
    after two protocol rounds: the two fakes' records miss (their INVs come back MISS), K and M take the records'
    timestamp"""
    from tests import inline_cases as C
    o = C.make_oracle("S")
    T = C.describe(o, "S")
    if rounds:
        C.case_rounds(C.OracleEngine(o), T, C.Rec(T.inline_keys), rounds=rounds, big=(1,), check_after=())
    ver = (CM.census_model(*CM.oracle_image(o, S))["max_ts"] >> 8) + 10
    records, K, M, fakes = RC.collision_records(T, o, ver)
    assert RM.install_counts(o, records) == {"raised": len(records) - 2, "equal": 0, "older": 0, "missed": 2}
    inv, _ = RM.records_to_batches(records, S)
    probe = inv.copy()
    o.batch(L.BatchType.invs, probe, L.membership(3, 0))
    miss = probe["state"] == int(L.Resp.MISS)
    assert miss.sum() == 2 and set(inv["key"][miss].tolist()) == set(fakes.tolist())
    ent = _entries_by_key(CM.oracle_image(o, S))
    for k in (K, M):
        assert (int(ent[int(k)]["ts_ver"]), int(ent[int(k)]["ts_cid"])) == (ver, 1)


def test_digest_link_and_batches(table_a):
    _, image, census, records = table_a
    assert len(records) == census["keys"]
    assert int(CM.entry_hashes(records, S).sum(dtype=np.uint64)) == census["digest_sum"]
    assert not (records & ~CM.digest_mask(S)[None, :]).any()          # every other byte is zero
    k = records[:, 8:16].copy().view("<u8").reshape(-1)
    assert (np.diff(k.astype(np.uint64)) > 0).all()                    # sorted, no key twice
    inv, val = RM.records_to_batches(records, S)
    rec = records.copy().view(L.entry_dtype(S)).reshape(-1)
    assert len(inv) == len(records) and len(val) == int((rec["state"] == int(L.State.VALID)).sum()) < len(inv)
    assert (inv["opcode"] == int(L.Op.INV)).all() and (inv["state"] == rec["ts_cid"]).all()
    assert (inv["flags"] == 0).all() and (inv["val_len"] == S.st_value).all()
    assert np.array_equal(inv["value"], rec["value"]) and (val["opcode"] == int(L.Op.VAL)).all()


def test_filters_partition(table_a):
    _, image, census, records = table_a
    whole = {r.tobytes() for r in records}
    assert len(whole) == len(records)
    # bucket ranges
    cuts = [0, 1000, 1001, 9000, 16384]
    parts = [RM.extract_model(image, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
    sets = [{r.tobytes() for r in p} for p in parts]
    assert sum(len(s) for s in sets) == len(whole) and set().union(*sets) == whole
    assert sum(RM.scanned_model(image, lo, hi) for lo, hi in zip(cuts, cuts[1:])) == census["keys"]
    # min_ts: at least t, and its complement
    t = (2 << 8) | 0
    hi_part = {r.tobytes() for r in RM.extract_model(image, min_ts=t)}
    rec = records.copy().view(L.entry_dtype(S)).reshape(-1)
    lo_part = {r.tobytes() for r, x in zip(records, L.ts64(rec["ts_ver"], rec["ts_cid"])) if int(x) < t}
    assert 0 < len(hi_part) < len(whole) and hi_part | lo_part == whole and not (hi_part & lo_part)
    assert RM.scanned_model(image) == census["keys"]


# ------------------------------------------------------------------ ABI (fails on a library older than ABI 10)
def test_abi_of_the_repair_calls():
    from hermes_amd import lib
    from hermes_amd.lib import HkvExtractResult, HkvInstallResult
    r = lib.raw()
    assert r.hkv_abi_version() == 10 == lib.ABI_VERSION
    assert r.hkv_extract_result_bytes() == ctypes.sizeof(HkvExtractResult) == 16
    assert r.hkv_install_result_bytes() == ctypes.sizeof(HkvInstallResult) == 32
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    rc = r.hkv_table_extract_async(None, 0, 0, 0, p, 1, p, None)
    assert rc < 0 and r.hkv_last_error()
    first = r.hkv_last_error()
    rc = r.hkv_table_install_async(None, p, 1, p, None)
    assert rc < 0 and r.hkv_last_error() and b"install" in r.hkv_last_error() and b"extract" in first
    assert not any(buf)
