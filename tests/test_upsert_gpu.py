"""Upsert on the device (hkv_table_upsert: k_table_install with its missed flags, the scan, the sort, k_pop_buckets,
k_ups_log) against tests/upsert_model.py on the oracle twin, byte for byte: index, log over log_cap, log head, the
result's counts, the census and the error flags, in every case. Empty and populated targets, full buckets and
evictions inside one call, a log that wraps mid-call, record counts around the block sizes, a scripted pair, tag
collisions, big objects, the grid-stride loop, an INLINE table, refusals, and resync / delta_resync / group_resync
with insert=True.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS, gen_keys  # noqa: E402
from tests import census_model as CM  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests import repair_cases as RC  # noqa: E402
from tests import repair_model as RM  # noqa: E402
from tests import upsert_model as UM  # noqa: E402
from tests.gen import bytecopy  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0xA5
VALID, INVALID = int(L.State.VALID), int(L.State.INVALID)
# the scripted pair of tests/test_repair_gpu.py
GEOM = {False: dict(src=(5000, 16384, 1 << 20), dst=(4700, 2048, 1 << 19)),
        True: dict(src=(2000, 1024, 1 << 20), dst=(1800, 512, 1 << 20))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_pair(n_keys, num_bkts, log_cap, machine_id=RC.DST_ID, rmw=False, ecl=0):
    from hermes_amd.kvs import HermesKV
    sizes = L.Sizes(True, ecl) if ecl else L.DEFAULT
    g = HermesKV(n_keys, num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl, populate=n_keys > 0)
    o = OracleKVS(num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl)
    if n_keys:
        o.populate(n_keys, sizes.kvs_value)
    return g, o, sizes


def both(g, o):
    def apply(btype, elems, mb):
        eo = bytecopy(elems)
        g.batch_host(btype, elems, mb)
        o.batch_multi(btype, eo, 1, len(eo), None, mb)
    return apply


def assert_tables_equal(g, o, what):
    assert np.array_equal(g.index_bytes(), o.index_bytes()), f"{what}: index differs"
    gl, ol = g.log_bytes(), o.log_bytes()[: g.cfg.log_cap]
    if not np.array_equal(gl, ol):
        bad = np.nonzero(gl != ol)[0]
        e = g.sizes.entry
        pytest.fail(f"{what}: log differs in entries {np.unique(bad // e)[:8]}, bytes-in-entry {np.unique(bad % e)[:16]}")


def hand_records(keys, sizes, salt, ver=4, cid=1):
    """VALID and INVALID records at (ver, cid); every seventh at (0, 255), a key never written, every eleventh at
    (0, 3), older than a fresh entry"""
    i = np.arange(len(keys))
    states = np.where(i % 3 == 0, INVALID, VALID)
    v = np.where((i % 7 == 6) | (i % 11 == 10), 0, ver)
    c = np.where(i % 7 == 6, 255, np.where(i % 11 == 10, 3, cid))
    return RC.make_records(keys, states, v, c, sizes, salt)


def upsert_both(g, o, records, sizes, what, n=None, ev0=None):
    """the records through the device and through the model on the twin; everything compared; returns the result"""
    n = len(records) if n is None else n
    ev0 = o.evictions() if ev0 is None else ev0
    dev = torch.from_numpy(records.copy()).cuda()      # all of them: n says how many are applied
    want = UM.upsert_model(o, records[:n], sizes, L.membership(RC.N_MACH, g.machine_id))
    keys0 = g.num_keys
    got = g.upsert(dev, n=n)
    assert got == want, f"{what}: {got} != model {want}"
    assert np.array_equal(dev.cpu().numpy(), records), f"{what}: the upsert wrote its records"
    assert g.log_head == o.log_head() == want["log_head"]
    assert g.num_keys == keys0 + want["inserted"]
    assert g.evictions == ev0 + want["evictions"]
    assert_tables_equal(g, o, what)
    model = CM.census_model(*CM.oracle_image(o, sizes))
    census = g.census().host()
    assert census == model, (what, census, model)
    assert g.take_error_flags() == 0
    return got, ev0 + want["evictions"]


# ------------------------------------------------------------------ 1. empty and tiny tables
@pytest.mark.parametrize("n", [1, 40])
def test_into_empty_table(n):
    g, o, sizes = make_pair(0, 64, 1 << 16)
    rec = hand_records(gen_keys(40)[:n], sizes, 3)
    got, _ = upsert_both(g, o, rec, sizes, f"{n} records into an empty table")
    assert got["inserted"] == n and got["log_head"] == n * 64
    assert g.layout()["conversions"] == 0
    # nothing was lost, so the same records again insert nothing and leave the table as it is
    assert got["replaced"] == got["evictions"] == 0
    image = (g.index_bytes(), g.log_bytes())
    again, _ = upsert_both(g, o, rec, sizes, "the same records again")
    assert again["inserted"] == again["raised"] == 0 and again["equal"] + again["older"] == n
    assert np.array_equal(g.index_bytes(), image[0]) and np.array_equal(g.log_bytes(), image[1])


def test_two_missed_records_share_bucket_and_tag():
    """in-call replacement: two records of one call whose keys share bucket and tag, among ordinary ones -- the
    later insert takes the earlier one's slot, in record order"""
    g, o, sizes = make_pair(0, 1024, 1 << 17)
    a = (0x1234 << 48) | (7 << 20) | 5
    b = (0x1234 << 48) | (9 << 20) | 5             # bits 20.. lie above the bucket mask: same bucket, same tag
    keys = np.concatenate([gen_keys(30)[:15], np.array([a], np.uint64), gen_keys(30)[15:], np.array([b], np.uint64)])
    got, _ = upsert_both(g, o, hand_records(keys, sizes, 13), sizes, "two keys of one bucket and tag")
    assert got["inserted"] == 32 and got["replaced"] == 1 and got["evictions"] == 0
    assert g.lookup_offset(a) is None and o.lookup(a) is None
    assert g.lookup_offset(b) == o.lookup(b) == 31 * 64


def test_sixteen_buckets_full_and_evicting():
    """200 records into 16 empty buckets: about 12 per bucket, so buckets fill and evict inside one call and the
    order inside a bucket decides every slot"""
    g, o, sizes = make_pair(0, 16, 1 << 16)
    got, _ = upsert_both(g, o, hand_records(gen_keys(200), sizes, 5), sizes, "200 records into 16 buckets")
    assert got["inserted"] == 200 and got["evictions"] > 0 and got["replaced"] == 0


def test_log_wraps_mid_call():
    """1500 records of 64 B into a log of 65536 B: the head wraps inside the call, later entries overwrite earlier
    ones and their slots go dead"""
    g, o, sizes = make_pair(0, 1024, 1 << 16)
    got, _ = upsert_both(g, o, hand_records(gen_keys(1500), sizes, 7), sizes, "1500 records, the log wraps")
    assert got["log_head"] > (1 << 16)
    c = g.census().host()
    assert c["dead_slots"] > 0 and c["keys"] < 1500
    assert not g.layout()["eligible"], "a wrapped log is not eligible for the inline layout"


@pytest.mark.parametrize("n", [1, 3, 4096, 4097])
def test_record_counts_around_block_sizes(n):
    n_keys, bkts, cap = GEOM[False]["dst"]
    g, o, sizes = make_pair(n_keys, bkts, cap)
    keys = gen_keys(n_keys + 4097)[n_keys:n_keys + n]
    got, _ = upsert_both(g, o, hand_records(keys, sizes, 9), sizes, f"{n} missing keys")
    assert got["inserted"] == n and got["raised"] == got["equal"] == got["older"] == 0


# ------------------------------------------------------------------ 2. the scripted pair
_sources = {}


def source_records(big):
    """the scripted source of tests/test_repair_gpu.py (an oracle: the records are its image's extract_model),
    shuffled, made once per size"""
    if big not in _sources:
        sizes = L.BIG if big else L.DEFAULT
        n_keys, bkts, cap = GEOM[big]["src"]
        o = OracleKVS(bkts, cap, RC.SRC_ID, False, big, 4 if big else 0)
        o.populate(n_keys, sizes.kvs_value)
        RC.source_script(lambda bt, e, mb: o.batch_multi(bt, e, 1, len(e), None, mb), gen_keys(n_keys), sizes)
        rec = RM.extract_model(CM.oracle_image(o, sizes))
        rec = rec[np.random.default_rng(7).permutation(len(rec))]
        rec.setflags(write=False)
        _sources[big] = rec
    return _sources[big]


def test_mixed_scripted_pair():
    """the scripted source into the scripted target, plus 300 records for keys neither table was populated with:
    raised, equal, older, inserted and replaced all occur; the same records again change nothing"""
    n_keys, bkts, cap = GEOM[False]["dst"]
    g, o, sizes = make_pair(n_keys, bkts, cap)
    RC.target_script(both(g, o), gen_keys(n_keys), sizes)
    extra = gen_keys(5600)[5200:5500].copy()
    # two of them share bucket and tag with a key the target holds (bit 30 lies between the two fields): each
    # insert takes that key's slot
    extra[:2] = gen_keys(n_keys)[[10, 11]] ^ np.uint64(1 << 30)
    assert all(o.lookup(int(k)) is None for k in extra[:2]) \
        and all(o.lookup(int(k)) is not None for k in gen_keys(n_keys)[[10, 11]])
    more = RC.make_records(extra, np.where(np.arange(300) % 4 == 0, INVALID, VALID), 6, 3, sizes, 31)
    rec = np.concatenate([source_records(False), more])
    rec = rec[np.random.default_rng(13).permutation(len(rec))]
    got, ev = upsert_both(g, o, rec, sizes, "the scripted pair")
    zero = [k for k in ("raised", "equal", "older", "inserted", "replaced") if not got[k]]
    assert not zero, f"counts that are zero: {zero}"
    # The same records again. Nothing is raised; but this target (5300 keys for 2048 buckets) lost keys in the first
    # call -- the model and the device both count replaced 2, evictions 8 -- and the records carry those ten keys,
    # so the definition has the second call insert exactly them again (measured: inserted 10, device == model byte
    # for byte). "Inserts nothing" holds where nothing was lost: test_resync_insert_rebuilds_from_empty.
    lost = got["replaced"] + got["evictions"]
    again, _ = upsert_both(g, o, rec, sizes, "the same records again", ev0=ev)
    assert again["raised"] == 0 and again["older"] == got["older"] and again["inserted"] == lost, (got, again)
    # and a third time: no fixed point -- each re-inserted key took the slot of the one that had taken its own, so
    # the two fakes and keys 10 and 11 keep alternating; the device follows the model through it byte for byte
    third, _ = upsert_both(g, o, rec, sizes, "a third time", ev0=ev + again["evictions"])
    assert third["raised"] == 0 and third["replaced"] >= 2 and third["inserted"] >= 2, third


def test_tag_collisions():
    """the fakes of tests/inline_cases.collision_keys share K's and M's bucket and tag: each insert replaces that
    slot, and K and M no longer look up -- the reference's lossy index, as on the oracle twin"""
    g, o, sizes = make_pair(*C.GEO["S"], machine_id=0)
    T = C.describe(o, "S")
    ver = (CM.census_model(*CM.oracle_image(o, sizes))["max_ts"] >> 8) + 10
    records, K, M, fakes = RC.collision_records(T, o, ver)
    got, _ = upsert_both(g, o, records, sizes, "collision records")
    assert got["inserted"] == 2 and got["replaced"] == 2 and got["evictions"] == 0 and got["raised"] == len(records) - 2
    for k in (K, M):
        assert o.lookup(int(k)) is None and g.lookup_offset(int(k)) is None
    for f in fakes:
        assert o.lookup(int(f)) is not None and g.lookup_offset(int(f)) == o.lookup(int(f))


# ------------------------------------------------------------------ 3. big objects
@pytest.mark.parametrize("populated", [False, True])
def test_big_objects_320(populated):
    n_keys, bkts, cap = GEOM[True]["dst"]
    g, o, sizes = make_pair(n_keys if populated else 0, bkts, cap, ecl=4)
    got, _ = upsert_both(g, o, source_records(True), sizes, "320-B records")
    assert got["inserted"] > 0 and (got["equal"] > 0) == populated


@pytest.mark.parametrize("populated", [False, True])
def test_big_objects_128(populated):
    """c = 1: the general instance, 128-B entries"""
    g, o, sizes = make_pair(1500 if populated else 0, 256, 1 << 19, ecl=1)
    assert sizes.entry == 128
    keys = gen_keys(2400)[900:2100]                 # 600 the populated table holds, 600 it lacks
    got, _ = upsert_both(g, o, hand_records(keys, sizes, 11), sizes, "128-B records")
    assert got["inserted"] >= 600 and (got["raised"] > 0) == populated


# ------------------------------------------------------------------ 4. the grid-stride loop
def test_grid_stride():
    """140000 records: more than the 131072 that 2048 blocks take in one step of 64 each"""
    g, o, sizes = make_pair(0, 1 << 16, 1 << 24)
    n = 140000
    keys = gen_keys(n)
    states = np.where(np.arange(n) % 5 == 0, INVALID, VALID)
    got, _ = upsert_both(g, o, RC.make_records(keys, states, 4, 2, sizes, 29), sizes, "140000 records")
    assert got["inserted"] == n


# ------------------------------------------------------------------ 5. an INLINE table
def _inline_twelve(name, geo="A"):
    """geometry A, INLINE, two protocol rounds of tests/inline_cases.py (twelve launches) and no export
    (tests/test_repair_gpu.py's fixture)"""
    from hermes_amd import kvs
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO[geo]
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE     # (the single-workgroup kernel has no inline instance)
    try:
        g = HermesKV(n_keys, bkts, cap)
        o = C.make_oracle(geo)
        T = C.describe(o, geo)
        assert g.prefer_layout(INLINE)
        m = Mirror(g, o, name, table_check="deferred")
        C.case_rounds(GpuEngine(m), T, C.Rec(T.inline_keys), rounds=2, big=(1,), check_after=())
    finally:
        kvs.HermesKV.default_flags = 0
    lay = g.layout()
    assert m.launches == 12 and lay["state"] == INLINE and lay["inline_launches"] == 12 and lay["conversions"] == 1, lay
    return g, o, T, m


def test_inline_table():
    from hermes_amd import kvs
    g, o, T, m = _inline_twelve("upsert inline")
    S = L.DEFAULT
    mb = L.membership(3, 0)
    present = T.keys[T.present]
    il = T.is_inline(present)
    pick = np.concatenate([present[il][:60], present[~il][:60]])
    head = CM.census_model(*CM.oracle_image(o, S))["max_ts"] >> 8
    states = np.where(np.arange(len(pick)) % 3 == 0, INVALID, VALID)
    records = RC.make_records(pick, states, head + 10, 1, S, 17)
    # every record present: an install, nothing converted, no counter moved
    before = g.layout()
    want = UM.upsert_model(o, records, S, mb)
    assert want["inserted"] == 0 and want["raised"] == 120
    assert g.upsert(torch.from_numpy(records.copy()).cuda()) == want
    assert g.layout() == before, "an upsert with nothing missed moved the layout or its counters"
    assert g.census().host() == CM.census_model(*CM.oracle_image(o, S), inline=True)
    assert g.layout() == before
    # 50 absent keys among present ones: the table goes to LOG, one conversion
    absent = gen_keys(T.n_keys + 50)[T.n_keys:]
    rec2 = np.concatenate([RC.make_records(absent, np.where(np.arange(50) % 2 == 0, INVALID, VALID), head + 12, 2, S, 19),
                           RC.make_records(pick[:40], [VALID] * 40, head + 14, 1, S, 21)])
    rec2 = rec2[np.random.default_rng(5).permutation(len(rec2))]
    want = UM.upsert_model(o, rec2, S, mb)
    assert want["inserted"] == 50 and want["raised"] == 40
    assert g.upsert(torch.from_numpy(rec2.copy()).cuda()) == want
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == before["conversions"] + 1 and lay["eligible"], lay
    assert lay["inline_launches"] == before["inline_launches"]
    # two more inline rounds through the Mirror, on the table as it is now (the new keys in the oracle twin)
    T2 = C.describe(o, "A")
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    try:
        C.case_rounds(GpuEngine(m), T2, C.Rec(T2.inline_keys), rounds=2, big=(1,), check_after=(), seed=4242)
    finally:
        kvs.HermesKV.default_flags = 0
    lay = g.layout()
    assert lay["state"] == INLINE and lay["conversions"] == before["conversions"] + 2, lay
    m.check_table("after the upserts and two more inline rounds")
    for k in absent:
        assert o.lookup(int(k)) is not None
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from hermes_amd import lib
    from hermes_amd.kvs import HermesKV
    r = lib.raw()

    def refused(rc, word):
        msg = r.hkv_last_error()
        assert rc < 0 and msg and b"upsert" in msg and word in msg, (rc, msg)

    rec = torch.full((64 * 64 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = (ctypes.c_uint8 * 64)(*([CANARY] * 64))
    pres = ctypes.cast(res, ctypes.POINTER(lib.HkvUpsertResult))
    g = HermesKV(1000, 1024, 1 << 17, rmw=True)
    refused(r.hkv_table_upsert(g.h, ctypes.c_void_p(rec.data_ptr()), 4, pres, None), b"RMW")
    g2 = HermesKV(1000, 1024, 1 << 17)
    img = (g2.index_bytes(), g2.log_bytes())
    refused(r.hkv_table_upsert(g2.h, ctypes.c_void_p(rec.data_ptr() + 8), 4, pres, None), b"aligned")
    refused(r.hkv_table_upsert(g2.h, None, 4, pres, None), b"null")
    refused(r.hkv_table_upsert(g2.h, ctypes.c_void_p(rec.data_ptr()), 4, None, None), b"null")
    refused(r.hkv_table_upsert(g2.h, ctypes.c_void_p(rec.data_ptr()), 1 << 31, pres, None), b"2^31")
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == CANARY).all() and bytes(res) == bytes([CANARY]) * 64, "a refused call wrote"
    assert np.array_equal(g2.index_bytes(), img[0]) and np.array_equal(g2.log_bytes(), img[1])
    assert g2.log_head == 1000 * 64 and g.take_error_flags() == 0 and g2.take_error_flags() == 0


# ------------------------------------------------------------------ 7. resync and delta_resync with insert=True
def _written_source(n_keys, bkts, cap, machine_id=0):
    """a populated pair with 600 keys written and validated at (4, 2)"""
    g, o, sizes = make_pair(n_keys, bkts, cap, machine_id=machine_id)
    keys = gen_keys(n_keys)
    mb = L.membership(3, machine_id)
    for lo in range(100, 700, 200):
        ids = np.arange(lo, lo + 200)
        both(g, o)(L.BatchType.invs, RC.invs(keys, ids, 2, (4, 2), sizes, 6), mb)
        both(g, o)(L.BatchType.vals, RC.vals(keys, ids, 2, (4, 2)), mb)
    return g, o, sizes


def test_resync_insert_rebuilds_from_empty():
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import resync
    n_keys, bkts, cap = 4000, 8192, 1 << 20
    src, so, sizes = _written_source(n_keys, bkts, cap)
    dst = HermesKV(n_keys, bkts // 2, cap, machine_id=1, populate=False)
    twin = OracleKVS(bkts // 2, cap, 1)
    chunk = bkts // 3 + 1
    # An extract writes its records in no particular order and the log is filled in record order, so the model
    # takes each chunk's records as resync() handed them to the device: the upsert is watched, not replaced.
    seen, upsert = [], dst.upsert

    def watched(records, n=None, stream=None):
        seen.append(records.tensor[:n * sizes.entry].cpu().numpy().reshape(n, sizes.entry).copy())
        return upsert(records, n=n, stream=stream)
    dst.upsert = watched
    got = resync(dst, src, chunk_buckets=chunk, insert=True)
    del dst.upsert
    assert len(seen) == 3
    want = dict.fromkeys(UM.RESULT[:6], 0)
    image = CM.oracle_image(so, sizes)
    for i, lo in enumerate(range(0, bkts, chunk)):
        assert np.array_equal(RM.sort_records(seen[i], sizes), RM.extract_model(image, lo, min(lo + chunk, bkts)))
        out = UM.upsert_model(twin, seen[i], sizes, L.membership(3, 1))
        for k in want:
            want[k] += out[k]
    assert {k: got[k] for k in want} == want and got["missed"] == 0
    assert want["inserted"] == got["records"] == src.census().keys and want["replaced"] == want["evictions"] == 0
    assert dst.log_head == twin.log_head()
    assert_tables_equal(dst, twin, "the rebuilt replica")
    assert dst.census().host() == CM.census_model(*CM.oracle_image(twin, sizes))
    a, b = src.census().host(), dst.census().host()
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert a[f] == b[f], f
    again = resync(dst, src, chunk_buckets=chunk, insert=True)
    assert again["inserted"] == 0 and again["raised"] == 0 and again["equal"] == got["records"]
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


def test_delta_resync_insert():
    """the source holds 300 keys the target lacks: without insert their partitions stay in unresolved (today's
    behaviour), with insert nothing is left -- the model says no key is lost to replaced / evictions here"""
    from hermes_amd.replica_group import delta_resync
    n_keys, bkts, cap = 4000, 8192, 1 << 20
    src, so, sizes = make_pair(n_keys + 300, bkts, cap, machine_id=0)
    dst, do, _ = make_pair(n_keys, bkts, cap, machine_id=1)
    only = gen_keys(n_keys + 300)[n_keys:]
    held = np.array([so.lookup(int(k)) is not None for k in only])
    parts = np.unique(only[held] & np.uint64((1 << 10) - 1))
    plain = delta_resync(dst, src, part_bits=10)
    assert plain["missed"] == int(held.sum()) > 250 and plain["differing_after"] == len(parts)
    assert "inserted" not in plain and set(plain["unresolved"]) <= set(parts.tolist())
    mask = np.isin(np.arange(bkts) & ((1 << 10) - 1), parts)
    image = CM.oracle_image(so, sizes)
    rec = RM.extract_model(image)
    rec = rec[mask[(rec[:, 8:16].copy().view("<u8").reshape(-1) & np.uint64(bkts - 1)).astype(np.int64)]]
    want = UM.upsert_model(do, rec, sizes, L.membership(3, 1))
    assert want["replaced"] == want["evictions"] == 0 and want["inserted"] == int(held.sum())
    got = delta_resync(dst, src, part_bits=10, insert=True)
    assert {k: got[k] for k in UM.RESULT[:6]} == {k: want[k] for k in UM.RESULT[:6]} and got["missed"] == 0
    assert got["differing_before"] == len(parts) and got["differing_after"] == 0 and got["unresolved"] == []
    assert CM.digest(dst.census().host()) == CM.digest(src.census().host())
    assert dst.census().host() == CM.census_model(*CM.oracle_image(do, sizes))
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


# ------------------------------------------------------------------ 8. group_resync(insert=True) over gloo
def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import group_census, group_resync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        n_keys = 4000
        g = HermesKV(n_keys, 8192 if rank == 0 else 4096, 1 << 20, machine_id=rank, populate=rank == 0)
        if rank == 0:
            keys = gen_keys(n_keys)
            mb = L.membership(3, 0)
            ids = np.arange(100, 300)
            g.batch_host(L.BatchType.invs, RC.invs(keys, ids, 2, (4, 2), L.DEFAULT, 6), mb)
            g.batch_host(L.BatchType.vals, RC.vals(keys, ids, 2, (4, 2)), mb)
        before = group_census(g, None)
        res = group_resync(g, None, 0, [1], chunk_buckets=8192 // 3 + 1, insert=True)
        after = group_census(g, None)
        again = group_resync(g, None, 0, [1], chunk_buckets=None, insert=True)
        q.put((rank, before, res, after, again, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, None, None, 0, repr(e)))


def test_group_resync_insert_over_gloo():
    """two ranks as fresh child processes sharing the GPU over gloo: rank 1 was created empty; after
    group_resync(insert=True) the group census agrees"""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_child, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    for rank, before, out, after, again, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert not before["live_ranks_agree"] and before["rows"][1][2] == 0 < before["rows"][0][2]
        assert after["live_ranks_agree"] and after["not_valid"] == [0, 0], after
        assert out["records"] == before["rows"][0][2]
        if rank == 1:
            assert out["inserted"] == out["records"] and out["missed"] == 0 and out["replaced"] == out["evictions"] == 0
            assert again["inserted"] == 0 and again["equal"] == out["records"]
        else:
            assert out["inserted"] == 0 and out["raised"] == 0
