"""The key-level delta repair on the oracle alone (include/hermeskv.h, "Key-level delta repair"): the ABI of the
three calls against the built library (no GPU needed: the refusals come before any device work), and the
definition -- a key is needed exactly when installing its record would miss or would change a byte the digest keeps
-- checked record by record on the tables tests/test_repair_cpu.py uses.
"""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import census_model as CM
from tests import delta_model as DM
from tests import keydelta_model as KM
from tests import repair_model as RM

S = L.DEFAULT
N_KEYS = 5000
MB = L.membership(5, 0)


# ------------------------------------------------------------------ ABI (fails on a library without the three calls)
def test_abi_of_the_key_level_calls():
    from hermes_amd import lib
    r = lib.raw()
    assert r.hkv_abi_version() == 10 == lib.ABI_VERSION
    assert r.hkv_key_summary_bytes() == 16 == KM.SUMMARY.itemsize
    assert r.hkv_need_result_bytes() == 64
    assert r.hkv_fetch_result_bytes() == 16
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    seen = []
    for name, call in (("summaries", lambda: r.hkv_table_summaries_async(None, 0, None, 0, 0, 0, p, 1, p, None)),
                       ("need", lambda: r.hkv_table_need_async(None, p, 1, p, 1, p, None)),
                       ("fetch", lambda: r.hkv_table_fetch_async(None, p, 1, p, p, None))):
        rc = call()
        msg = r.hkv_last_error()
        assert rc < 0 and msg and name.encode() in msg, (name, rc, msg)
        seen.append(msg)
    assert len(set(seen)) == 3
    assert not any(buf)


def test_python_bindings_exist():
    from hermes_amd import kvs, replica_group
    for name in ("summaries", "need", "fetch"):
        assert callable(getattr(kvs.HermesKV, name))
    assert callable(replica_group.key_delta_resync) and callable(replica_group.group_key_delta_resync)
    assert kvs.SUMMARY_DTYPE.itemsize == 16 and kvs.SUMMARY_DTYPE == KM.SUMMARY


# ------------------------------------------------------------------ the definition, on the oracle alone
class _Done(Exception):
    pass


def _table(bkts, cap, n_keys=N_KEYS, machine_id=0):
    o = OracleKVS(bkts, cap, machine_id)
    o.populate(n_keys, S.kvs_value)
    return o


def _clone(o, bkts, cap):
    """an oracle with the same index, log and head (the image copied into a fresh table of the same geometry)"""
    from oracle.oracle import lib
    c = OracleKVS(bkts, cap, 0)
    c.populate(N_KEYS, S.kvs_value)
    assert c.log_head() == o.log_head()
    c.index_bytes()[:] = o.index_bytes()
    np.ctypeslib.as_array(lib().hko_log(c.h), shape=(cap + S.entry,))[:] = \
        np.ctypeslib.as_array(lib().hko_log(o.h), shape=(cap + S.entry,))
    return c


@pytest.fixture(scope="module")
def pair():
    """tests/test_repair_cpu.py's tables: a source of 5000 keys in 16384 buckets after the first three launches of
    tests/scripted.py, and a target of the same ids freshly populated in an eighth of the buckets (so some source
    keys are absent from it, its fuller buckets having evicted them)"""
    from tests.scripted import run_scripted
    src = _table(16384, 1 << 20)
    n = [0]

    def runner(btype, elems, mb, rw=None, node_suspected=None):
        src.batch_multi(btype, elems, 1, len(elems), None, mb, rw=rw, node_suspected=node_suspected)
        n[0] += 1
        if n[0] == 3:
            raise _Done

    with pytest.raises(_Done):
        run_scripted(runner, gen_keys(N_KEYS), S, False)
    dst = _table(2048, 1 << 19)
    return src, CM.oracle_image(src, S), dst


def _digest_bytes(o):
    """every live key's digest-masked entry, by key -- what the digest sees of the table"""
    image = CM.oracle_image(o, S)
    entries, *_ = CM.live_entries(*image)
    m = entries & CM.digest_mask(S)[None, :]
    return {int(r[8:16].copy().view("<u8")[0]): r.tobytes() for r in m}


def test_needed_is_exactly_what_an_install_would_miss_or_change(pair):
    """record by record: the key is in need_model's set exactly when applying records_to_batches of its single
    record to a copy of the target misses or changes a digest-masked byte"""
    _, image_src, dst = pair
    records = RM.extract_model(image_src)
    summ = KM.summaries_of_records(records, S)
    counts, need_keys, cls = KM.need_model(dst, summ, S)
    assert counts["missed"] > 0 and counts["newer"] > 0 and counts["same"] > 0, counts
    assert counts["needed"] == counts["missed"] + counts["newer"] + counts["validate"] == len(need_keys)
    assert sum(counts[c] for c in KM.CLASSES) == len(records)
    need = set(need_keys.tolist())
    # one scratch copy of the target, restored after every record that changed it
    twin = _clone(dst, 2048, 1 << 19)
    from oracle.oracle import lib
    log = np.ctypeslib.as_array(lib().hko_log(twin.h), shape=((1 << 19) + S.entry,))
    base_index, base_log = twin.index_bytes().copy(), log.copy()
    keep = CM.digest_mask(S)
    checked = dict.fromkeys(KM.CLASSES, 0)
    # every record of the classes that are rare here, and every fifth of the rest
    rare = {c for c in KM.CLASSES if counts[c] < 200}
    for i, (r, c) in enumerate(zip(records, cls)):
        if c not in rare and i % 5:
            continue
        key = int(summ["key"][i])
        off = twin.lookup(key)
        inv, val = RM.records_to_batches(r[None, :], S)
        twin.batch(L.BatchType.invs, inv, MB)
        missed = int(inv["state"][0]) == int(L.Resp.MISS)
        assert missed == (off is None)
        if len(val):
            twin.batch(L.BatchType.vals, val, MB)
        changed = False
        if off is not None:
            changed = bool(((log[off:off + S.entry] ^ base_log[off:off + S.entry]) & keep).any())
            log[off:off + S.entry] = base_log[off:off + S.entry]
        assert np.array_equal(twin.index_bytes(), base_index)
        assert (key in need) == (missed or changed), (key, c, missed, changed)
        checked[c] += 1
    assert all(checked[c] > 0 for c in KM.CLASSES if counts[c]), (checked, counts)
    assert np.array_equal(log, base_log)


def test_needed_records_repair_what_all_records_repair(pair):
    """applying the needed records gives the same partition rows as applying all records of the differing
    partitions"""
    _, image_src, dst = pair
    part_bits = 8
    rows_src = DM.part_rows_model(image_src, part_bits)
    mask, count = DM.diff_model(rows_src, DM.part_rows_model(CM.oracle_image(dst, S), part_bits))
    assert 0 < count
    all_rec = DM.extract_parts_model(image_src, part_bits, mask)
    summ = KM.summaries_model(image_src, part_bits, mask)
    assert len(summ) == len(all_rec)
    _, need_keys, _ = KM.need_model(dst, summ, S)
    needed = KM.fetch_model(image_src, need_keys)
    assert 0 < len(needed) < len(all_rec)
    a, b = _clone(dst, 2048, 1 << 19), _clone(dst, 2048, 1 << 19)
    RM.apply_records(a, all_rec, S, MB)
    RM.apply_records(b, needed, S, MB)
    rows_a = DM.part_rows_model(CM.oracle_image(a, S), part_bits)
    rows_b = DM.part_rows_model(CM.oracle_image(b, S), part_bits)
    assert np.array_equal(rows_a, rows_b)
    assert _digest_bytes(a) == _digest_bytes(b)
    # and nothing is left to need
    again, keys_again, _ = KM.need_model(b, summ, S)
    assert again["newer"] == again["validate"] == 0 and again["missed"] == len(keys_again)


def test_a_summary_is_a_function_of_its_record(pair):
    _, image_src, _ = pair
    records = RM.extract_model(image_src)
    summ = KM.summaries_model(image_src)
    assert len(summ) == len(records)
    raw = summ.view(np.uint8).reshape(-1, 16)
    assert np.array_equal(raw[:, 0:8], records[:, 8:16])         # key
    assert np.array_equal(raw[:, 8:12], records[:, 24:28])       # ts version
    assert np.array_equal(raw[:, 12], records[:, 23])            # ts cid
    assert np.array_equal(raw[:, 13], records[:, 18])            # state
    assert not raw[:, 14:16].any()
    assert len({r.tobytes() for r in raw}) == len(raw)
    # the filters select the summaries of the records they select
    t = (2 << 8) | 0
    assert np.array_equal(KM.summaries_model(image_src, rng=(1000, 9000), min_ts=t),
                          KM.summaries_of_records(RM.extract_model(image_src, 1000, 9000, t), S))
    # the fetch of a summary's key gives its record back; an absent key a zero record but for the key
    keys = np.concatenate([summ["key"][:50], np.array([0x1234567812345678], np.uint64), summ["key"][:3]])
    got = KM.fetch_model(image_src, keys)
    assert np.array_equal(got[:50], records[:50]) and np.array_equal(got[51:], records[:3])
    assert got[50, 8:16].copy().view("<u8")[0] == 0x1234567812345678 and not got[50, :8].any() and not got[50, 16:].any()


def test_image_lookup_is_the_oracles(pair):
    src, image_src, dst = pair
    image_dst = CM.oracle_image(dst, S)
    keys = gen_keys(N_KEYS)
    absent = 0
    for k in keys[::7].tolist():
        assert KM.lookup_image(image_src, k) == src.lookup(k)
        assert KM.lookup_image(image_dst, k) == dst.lookup(k)
        absent += dst.lookup(k) is None
    assert absent > 0
