"""Replica repair on the device (hkv_table_extract_async / hkv_table_install_async, k_table_extract /
k_table_install) against tests/repair_model.py and the oracle.

Extract: the records equal the numpy model of the table's image byte for byte -- fresh populates of every census
geometry (whole range, uneven bucket chunks, a min_ts filter, a short buffer over a canary), and an INLINE table
whose log copies have gone stale, where a reader of the log is shown to give other records. Install: index and log
equal, byte for byte, the oracle twin that applied the records as the header defines them (one INV per record, then
one VAL per record that was VALID), into other bucket counts, 64-B and 320-B entries, fresh and scripted targets,
the record counts around the block sizes; then into an INLINE table between inline rounds. Refusals, a loopback
group's resync, and group_resync over gloo.
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
from tests.gen import bytecopy  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_pair(n_keys, num_bkts, log_cap, big=False, machine_id=0, rmw=False, ecl=None):
    """ecl: big objects of that many extra cache lines (default: 4 with big, the default geometry without)"""
    from hermes_amd.kvs import HermesKV
    ecl = (4 if big else 0) if ecl is None else ecl
    sizes = L.Sizes(True, ecl) if ecl else L.DEFAULT
    g = HermesKV(n_keys, num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl, populate=n_keys > 0)
    o = OracleKVS(num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl)
    if n_keys:
        o.populate(n_keys, sizes.kvs_value)
    return g, o, sizes


def device_image(g, sizes):
    """the device table's own export (sends an INLINE table to LOG)"""
    cap = g.cfg.log_cap
    return g.index_bytes(), g.log_bytes(0, cap + sizes.entry), g.log_head, cap, sizes


def assert_extract(x, want, scanned, sizes, what):
    h = x.host()
    assert h["records"] == len(want), f"{what}: records {h['records']} != model {len(want)}"
    assert h["scanned_keys"] == scanned, f"{what}: scanned_keys {h['scanned_keys']} != model {scanned}"
    got = RM.sort_records(x.records_host(), sizes)
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: records differ from the model"


def assert_tables_equal(g, o, what):
    assert np.array_equal(g.index_bytes(), o.index_bytes()), f"{what}: index differs"
    gl, ol = g.log_bytes(), o.log_bytes()[: g.cfg.log_cap]
    if not np.array_equal(gl, ol):
        bad = np.nonzero(gl != ol)[0]
        e = g.sizes.entry
        pytest.fail(f"{what}: log differs in entries {np.unique(bad // e)[:8]}, bytes-in-entry {np.unique(bad % e)[:16]}")


def both(g, o):
    """apply(btype, elems, mb) of tests/repair_cases.py on a device table and its oracle twin"""
    def apply(btype, elems, mb):
        eo = bytecopy(elems)
        g.batch_host(btype, elems, mb)
        o.batch_multi(btype, eo, 1, len(eo), None, mb)
        assert np.array_equal(elems.view(np.uint8), eo.view(np.uint8))
    return apply


# ------------------------------------------------------------------ 1. extract, fresh populate
@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big", [
    (5000, 16384, 1 << 20, False),     # default-shaped: under one key per bucket
    (20000, 2048, 1 << 21, False),     # full buckets, evictions
    (3000, 4096, 1 << 17, False),      # the log wraps: dead slots are no records
    (1500, 256, 1 << 20, True),        # big objects, 320-byte records
    (0, 64, 1 << 16, False),           # no key
    (1, 64, 1 << 16, False),           # one key
    (40, 16, 1 << 16, False),          # 16 buckets: a quarter of one block's step
    (100, 32, 1 << 16, False),         # 32 buckets
    (60000, 1 << 18, 1 << 23, False),  # 512 block steps of 512 buckets
    (30000, 1 << 21, 1 << 22, False),  # 4096 block steps for a grid of at most 2048 blocks: the grid-stride loop
])
def test_extract_fresh_populate(n_keys, num_bkts, log_cap, big):
    g, o, sizes = make_pair(n_keys, num_bkts, log_cap, big=big)
    E = sizes.entry
    image = device_image(g, sizes)
    want = RM.extract_model(image)
    assert np.array_equal(want, RM.extract_model(CM.oracle_image(o, sizes))), "the device image is the oracle's"
    R = len(want)
    # the whole range; twice into one buffer and result: overwritten, not accumulated
    x = g.extract()
    assert_extract(x, want, RM.scanned_model(image), sizes, "whole")
    assert x.cap == n_keys
    y = g.extract(out=x.tensor, result=x.result)
    assert_extract(y, want, R, sizes, "second call into the same buffer")
    if R:
        assert int(CM.entry_hashes(RM.sort_records(x.records_host(), sizes), sizes).sum(dtype=np.uint64)) == \
            CM.census_model(*image)["digest_sum"] == g.census().digest_sum
    # three uneven chunks
    cuts = [0, num_bkts // 3 + 1, num_bkts - 5, num_bkts]
    seen = 0
    for lo, hi in zip(cuts, cuts[1:]):
        part = g.extract((lo, hi), cap=R)
        assert_extract(part, RM.extract_model(image, lo, hi), RM.scanned_model(image, lo, hi), sizes, f"[{lo}, {hi})")
        seen += part.records
    assert seen == R
    assert g.extract((7, 7)).host() == {"records": 0, "scanned_keys": 0}
    # a short buffer over a canary
    if R >= 4:
        buf = torch.full((R * E + 64,), CANARY, dtype=torch.uint8, device="cuda")
        z = g.extract(out=buf, cap=R - 3)
        assert z.host() == {"records": R, "scanned_keys": R} and z.written == R - 3
        got = z.records_host()
        have = {r.tobytes() for r in want}
        assert len({r.tobytes() for r in got}) == R - 3 and all(r.tobytes() in have for r in got)
        assert (buf[(R - 3) * E:].cpu().numpy() == CANARY).all(), "written past record_cap"
    # a write round over half the keys, then min_ts above the other half
    if n_keys >= 2:
        half = n_keys // 2
        nb = max(half // 500, 1)
        stride = half // nb
        ids = np.arange(nb * stride)
        inv = RC.invs(gen_keys(n_keys), ids, 1, (4, 1), sizes, 3)
        g.batch_host(L.BatchType.invs, inv, L.membership(3, 0), n_batches=nb, stride=stride)
        image = device_image(g, sizes)
    t = (4 << 8) | 1
    newer = RM.extract_model(image, min_ts=t)
    assert len(newer) < max(R, 1) and (n_keys < 1000 or 0 < len(newer))
    assert_extract(g.extract(min_ts=t), newer, RM.scanned_model(image), sizes, "min_ts")
    assert_extract(g.extract(min_ts=t + 1), RM.extract_model(image, min_ts=t + 1), RM.scanned_model(image), sizes,
                   "min_ts above every key")
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == 0
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 2. extract, INLINE with stale logs
def _inline_twelve(name, geo="A"):
    """geometry A (or `geo`), INLINE, two protocol rounds of tests/inline_cases.py (twelve launches) and no export"""
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


def test_extract_inline_with_stale_logs():
    g, o, T, m = _inline_twelve("extract inline")
    cap = T.cap
    before = g.layout()
    x = g.extract()
    chunked = [g.extract((lo, hi), cap=T.n_keys) for lo, hi in ((0, 100), (100, 101), (101, T.bkts))]
    assert g.layout() == before, "the extract moved the layout or its counters"
    image = CM.oracle_image(o, L.DEFAULT)
    want = RM.extract_model(image)
    assert_extract(x, want, RM.scanned_model(image), L.DEFAULT, "INLINE")
    assert len(want) == int(T.present.sum())
    for part, (lo, hi) in zip(chunked, ((0, 100), (100, 101), (101, T.bkts))):
        assert_extract(part, RM.extract_model(image, lo, hi), RM.scanned_model(image, lo, hi), L.DEFAULT, f"[{lo}, {hi})")
    # what a reader of index and log would have extracted: the inline keys' entries as they were when the table was
    # converted, every other entry current
    idx, log_now, head, _, _ = image
    _, _, _, phys, ikeys, _ = C.census(idx, T.log, cap)
    assert np.array_equal(ikeys, T.inline_keys)
    stale = log_now.copy()
    rows = phys[:, None] + np.arange(64)[None, :]
    stale[rows] = T.log[rows]
    assert not np.array_equal(RM.extract_model((idx, stale, head, cap, L.DEFAULT)), want)
    assert g.layout() == before
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 3. install into LOG, byte for byte
GEOM = {False: dict(src=(5000, 16384, 1 << 20), dst=(4700, 2048, 1 << 19)),
        True: dict(src=(2000, 1024, 1 << 20), dst=(1800, 512, 1 << 20))}
_sources = {}


def source_records(big):
    """the scripted source (an oracle: the records are its image's extract_model), shuffled, made once per size"""
    if big not in _sources:
        sizes = L.BIG if big else L.DEFAULT
        n_keys, bkts, cap = GEOM[big]["src"]
        o = OracleKVS(bkts, cap, RC.SRC_ID, False, big, 4 if big else 0)
        o.populate(n_keys, sizes.kvs_value)
        RC.source_script(lambda bt, e, mb: o.batch_multi(bt, e, 1, len(e), None, mb), gen_keys(n_keys), sizes)
        rec = RM.extract_model(CM.oracle_image(o, sizes))
        states = set(rec[:, 18].tolist())
        assert {int(L.State.VALID), int(L.State.INVALID), int(L.State.WRITE), int(L.State.INVALID_WRITE)} <= states
        rec = rec[np.random.default_rng(7).permutation(len(rec))]
        rec.setflags(write=False)
        _sources[big] = rec
    return _sources[big]


@pytest.mark.parametrize("big,scripted,n", [
    (False, False, None), (True, False, None),                       # fresh targets, every record
    (False, True, 1), (False, True, 3), (False, True, 1000), (False, True, 4096), (False, True, 4097),
    (False, True, None), (True, True, 3), (True, True, 1000), (True, True, None)])
def test_install_log_against_oracle(big, scripted, n):
    records = source_records(big)
    n = len(records) if n is None else n
    assert n <= len(records) and (n == len(records) or n in (1, 3, 4096, 4097) or n % 16)
    n_keys, bkts, cap = GEOM[big]["dst"]
    g, o, sizes = make_pair(n_keys, bkts, cap, big=big, machine_id=RC.DST_ID)
    if scripted:
        RC.target_script(both(g, o), gen_keys(n_keys), sizes)
    want = RM.install_counts(o, records[:n], sizes)
    if scripted and n == len(records):
        assert all(want[k] > 0 for k in RM.COUNTS), want
        e = o.lookup(int(gen_keys(n_keys)[RC.TW[0]]))
        assert CM.oracle_image(o, sizes)[1][e + 18] == int(L.State.WRITE)
    elif n == len(records):
        assert want["raised"] > 0 and want["equal"] > 0 and want["missed"] > 0, want
    dev = torch.from_numpy(records.copy()).cuda()          # all of them: n says how many are applied
    res = g.install(dev, n=n)
    torch.cuda.synchronize()
    RM.apply_records(o, records[:n], sizes, L.membership(RC.N_MACH, RC.DST_ID))
    assert res.host() == want
    assert np.array_equal(dev.cpu().numpy(), records), "the install wrote its records"
    assert_tables_equal(g, o, f"install of {n} records")
    got = g.census().host()
    model = CM.census_model(*CM.oracle_image(o, sizes))
    assert got == model, (got, model)
    if scripted and n == len(records):   # the target's WRITE at the equal timestamp: kept for an INVALID record,
        keys = gen_keys(n_keys)          # validated where the source was VALID
        log = CM.oracle_image(o, sizes)[1]
        assert log[o.lookup(int(keys[RC.TW[0]])) + 18] == int(L.State.WRITE)
        assert log[o.lookup(int(keys[RC.TW[0] + 1])) + 18] == int(L.State.VALID)
        again = g.install(dev, n=n).host()
        assert again["raised"] == 0 and again["equal"] == want["raised"] + want["equal"]
        assert_tables_equal(g, o, "the same records again")
    assert g.layout()["conversions"] == 0
    assert g.take_error_flags() == 0


def test_install_grid_stride():
    """140000 records: more than the 131072 that a grid of 2048 blocks takes in one step of 64 each, so blocks
    take a second step; hand-made records, VALID and INVALID, over a fresh target"""
    n_keys, n = 150000, 140000
    g, o, sizes = make_pair(n_keys, 1 << 16, 1 << 24, machine_id=1)
    keys = gen_keys(n_keys)
    ids = np.random.default_rng(3).permutation(n_keys)[:n]
    states = np.where(ids % 5 == 0, int(L.State.INVALID), int(L.State.VALID))
    records = RC.make_records(keys[ids], states, 4, 2, sizes, 29)
    want = RM.install_counts(o, records, sizes)
    assert want["raised"] > 130000 and want["raised"] + want["missed"] == n
    res = g.install(torch.from_numpy(records).cuda())
    RM.apply_records(o, records, sizes, L.membership(3, 1))
    assert res.host() == want
    assert_tables_equal(g, o, "install of 140000 records")
    assert g.take_error_flags() == 0


def test_install_from_extract_default_n():
    """install(Extract) with n omitted applies min(records, capacity) records, read on the host"""
    g, o, sizes = make_pair(3000, 4096, 1 << 18)
    h, ho, _ = make_pair(3000, 512, 1 << 18, machine_id=1)
    keys = gen_keys(3000)
    both(g, o)(L.BatchType.invs, RC.invs(keys, np.arange(50, 250), 1, (4, 1), sizes, 2), L.membership(3, 0))
    x = g.extract(min_ts=(4 << 8) | 1)
    res = h.install(x).host()
    rec = RM.extract_model(CM.oracle_image(o, sizes), min_ts=(4 << 8) | 1)
    want = RM.install_counts(ho, rec, sizes)
    RM.apply_records(ho, rec, sizes, L.membership(3, 1))
    assert res == want and want["raised"] == len(rec) - want["missed"] > 0
    assert_tables_equal(h, ho, "install of an extract")
    assert g.take_error_flags() == 0 and h.take_error_flags() == 0


# ------------------------------------------------------------------ 4. install into INLINE with stale logs
def test_install_inline_with_stale_logs():
    from hermes_amd import kvs
    g, o, T, m = _inline_twelve("install inline")
    present = T.keys[T.present]
    il = T.is_inline(present)
    pick = np.concatenate([present[il][:60], present[~il][:60]])
    assert int(T.is_inline(pick).sum()) == 60 and len(pick) == 120      # inline keys and keys read from the log
    head = CM.census_model(*CM.oracle_image(o, L.DEFAULT))["max_ts"] >> 8
    states = np.where(np.arange(len(pick)) % 3 == 0, int(L.State.INVALID), int(L.State.VALID))
    records = RC.make_records(pick, states, head + 10, 1, L.DEFAULT, 17)
    records = np.concatenate([records, RM.extract_model(CM.oracle_image(o, L.DEFAULT))[:200]])   # and equal ones
    _, uniq = np.unique(records[:, 8:16].copy().view("<u8").reshape(-1), return_index=True)
    records = records[np.sort(uniq)]
    want = RM.install_counts(o, records)
    assert want["raised"] == 120 and want["equal"] > 0 and want["missed"] == 0
    before = g.layout()
    res = g.install(torch.from_numpy(records.copy()).cuda())
    assert res.host() == want
    assert g.layout() == before, "the install moved the layout or its counters"
    RM.apply_records(o, records, L.DEFAULT, L.membership(3, 0))
    assert g.census().host() == CM.census_model(*CM.oracle_image(o, L.DEFAULT), inline=True)
    assert g.layout() == before
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    try:
        C.case_rounds(GpuEngine(m), T, C.Rec(T.inline_keys), rounds=2, big=(1,), check_after=(), seed=4242)
    finally:
        kvs.HermesKV.default_flags = 0
    lay = g.layout()
    assert lay["state"] == INLINE and lay["conversions"] == 1 and lay["inline_launches"] == 24, lay
    m.check_table("after the install and two more inline rounds")
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 4b. install: records for absent keys that collide
@pytest.mark.parametrize("layout", [LOG, INLINE])
def test_install_tag_collisions(layout):
    """Records for K (its bucket's inline key), M (a bucket-mate in slot 7) and their fakes -- absent keys with the
    same bucket and tag, tests/inline_cases.collision_keys -- among ordinary keys, all newer than the table, on the
    1000-key geometry: the fakes miss after the probe's tag match and window check, at the key compare; K and M
    are raised; index and log equal the oracle twin that ran records_to_batches. LOG: a fresh target. INLINE:
    between two inline rounds with no export, as test_install_inline_with_stale_logs."""
    from hermes_amd import kvs
    if layout == INLINE:
        g, o, T, m = _inline_twelve("install collisions", geo="S")
    else:
        g, o, _ = make_pair(*C.GEO["S"])
        T = C.describe(o, "S")
    ver = (CM.census_model(*CM.oracle_image(o, L.DEFAULT))["max_ts"] >> 8) + 10
    records, K, M, fakes = RC.collision_records(T, o, ver)
    want = RM.install_counts(o, records)
    assert want == {"raised": len(records) - 2, "equal": 0, "older": 0, "missed": 2}
    before = g.layout()
    res = g.install(torch.from_numpy(records.copy()).cuda())
    assert res.host() == want
    assert g.layout() == before, "the install moved the layout or its counters"
    RM.apply_records(o, records, L.DEFAULT, L.membership(3, 0))
    log = CM.oracle_image(o, L.DEFAULT)[1]
    for k in (K, M):
        e = o.lookup(int(k))
        assert int.from_bytes(log[e + 24:e + 28].tobytes(), "little") == ver and int(log[e + 23]) == 1
    if layout == INLINE:
        kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
        try:
            C.case_rounds(GpuEngine(m), T, C.Rec(T.inline_keys), rounds=2, big=(1,), check_after=(), seed=4242)
        finally:
            kvs.HermesKV.default_flags = 0
        lay = g.layout()
        assert lay["state"] == INLINE and lay["conversions"] == 1 and lay["inline_launches"] == 24, lay
        m.check_table("after the install and two more inline rounds")
    else:
        assert_tables_equal(g, o, "install of the collision records")
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    from hermes_amd import lib
    from hermes_amd.kvs import HermesKV
    r = lib.raw()
    E = 64

    def refused(rc, word):
        msg = r.hkv_last_error()
        assert rc < 0 and msg and word in msg, (rc, msg)

    def P(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)

    rec = torch.full((64 * E + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    g = HermesKV(1000, 1024, 1 << 17, rmw=True)
    refused(r.hkv_table_extract_async(g.h, 0, 1024, 0, P(rec), 64, P(res), None), b"RMW")
    refused(r.hkv_table_install_async(g.h, P(rec), 4, P(res), None), b"RMW")
    with pytest.raises(lib.HkvError):
        g.extract()
    g2 = HermesKV(1000, 1024, 1 << 17)
    img = (g2.index_bytes(), g2.log_bytes())
    refused(r.hkv_table_extract_async(g2.h, 0, 1024, 0, P(rec, 8), 64, P(res), None), b"aligned")
    refused(r.hkv_table_extract_async(g2.h, 0, 1024, 0, P(rec), 64, P(res, 8), None), b"aligned")
    refused(r.hkv_table_install_async(g2.h, P(rec, 8), 4, P(res), None), b"aligned")
    refused(r.hkv_table_install_async(g2.h, P(rec), 4, P(res, 8), None), b"aligned")
    refused(r.hkv_table_extract_async(g2.h, 0, 1025, 0, P(rec), 64, P(res), None), b"bucket range")
    refused(r.hkv_table_extract_async(g2.h, 9, 8, 0, P(rec), 64, P(res), None), b"bucket range")
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == CANARY).all() and (res.cpu().numpy() == -1).all(), "a refused call wrote"
    assert np.array_equal(g2.index_bytes(), img[0]) and np.array_equal(g2.log_bytes(), img[1])
    assert g.take_error_flags() == 0 and g2.take_error_flags() == 0


# ------------------------------------------------------------------ 6. loopback group
def test_resync_loopback_group():
    """Three replicas; replica 2 fails between rounds (ReplicaRound.fail(), the drop agreed through Hades) and
    the others run three more rounds: the census rows disagree. resync() from replica 0 in three bucket chunks
    brings replica 2's digest, key count and states to replica 0's, its image to its oracle twin's after the same
    batches, and a second resync raises nothing. (The replica fails with no write of its own in flight: a key it
    left in WRITE stays WRITE under a record of the same timestamp, by the install's definition.)"""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import LoopbackGroup, ReplicaRound, census_row, census_rows_agree, resync
    from hermes_amd.workload import zipf_params
    n_rep, n_keys, bkts, cap = 3, 4000, 8192, 1 << 20
    z = zipf_params(n_keys, 0.99)
    reps, mirrors = [], []
    for r in range(n_rep):
        g = HermesKV(n_keys, bkts, cap, machine_id=r)
        o = OracleKVS(bkts, cap, r)
        o.populate(n_keys, L.DEFAULT.kvs_value)
        mirrors.append(Mirror(g, o, f"replica {r}"))
        reps.append(ReplicaRound(g, 16, n_rep, r, z, 400, seed=77 + r, trace_len=512))
    grp = LoopbackGroup(reps, hades=True)
    for _ in range(2):
        grp.step()
    for r in reps:
        r.peer_failing()
    reps[2].fail()
    for _ in range(3):
        grp.step()
    torch.cuda.synchronize()
    assert grp.hades_changes and all(c[2][1] == 0b011 for c in grp.hades_changes)
    cs = [m.g.census() for m in mirrors]
    rows = [[int(x) & CM.M64 for x in census_row(c).cpu().tolist()] for c in cs]
    assert census_rows_agree(rows, (0, 1)) and not census_rows_agree(rows, (0, 2))
    src, dst, twin = mirrors[0].g, mirrors[2].g, mirrors[2].o
    chunk = bkts // 3 + 1
    want = dict.fromkeys(RM.COUNTS, 0)
    image0 = CM.oracle_image(mirrors[0].o, L.DEFAULT)
    for lo in range(0, bkts, chunk):
        rec = RM.extract_model(image0, lo, min(lo + chunk, bkts))
        for k, v in RM.install_counts(twin, rec).items():
            want[k] += v
        RM.apply_records(twin, rec, L.DEFAULT, L.membership(n_rep, 2))
    out = resync(dst, src, chunk_buckets=chunk)
    assert {k: out[k] for k in RM.COUNTS} == want and want["raised"] > 0 and want["missed"] == 0
    assert out["records"] == out["scanned_keys"] == cs[0].keys
    h0, h2 = src.census().host(), dst.census().host()
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert h0[f] == h2[f], f"{f}: replica 0 {h0[f]} != replica 2 {h2[f]}"
    mirrors[2].check_table("replica 2 after the resync")
    assert mirrors[0].g.census().host() == h0
    assert resync(dst, src, chunk_buckets=chunk)["raised"] == 0
    assert all(m.g.take_error_flags() == 0 for m in mirrors)


# ------------------------------------------------------------------ 7. group_resync over gloo
def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import group_census, group_resync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        n_keys = 4000
        bkts = 8192 if rank == 0 else 4096            # the stale rank has another geometry
        g = HermesKV(n_keys, bkts, 1 << 20, machine_id=rank)
        keys = gen_keys(n_keys)
        if rank == 0:                                  # writes only rank 0 saw
            mb = L.membership(3, 0)
            for lo in range(100, 700, 200):
                ids = np.arange(lo, lo + 200)
                g.batch_host(L.BatchType.invs, RC.invs(keys, ids, 2, (4, 2), L.DEFAULT, 6), mb)
                g.batch_host(L.BatchType.vals, RC.vals(keys, ids, 2, (4, 2)), mb)
        before = group_census(g, None)
        res = group_resync(g, None, 0, [1], chunk_buckets=8192 // 3 + 1)
        after = group_census(g, None)
        again = group_resync(g, None, 0, [1], chunk_buckets=None)
        q.put((rank, before, res, after, again, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, None, None, 0, repr(e)))


def test_group_resync_over_gloo():
    """two ranks as fresh child processes sharing the GPU over gloo: rank 1 missed INVs and VALs that rank 0
    applied; after group_resync the group census agrees"""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_child, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    for rank, before, out, after, again, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert not before["live_ranks_agree"] and before["rows"][0][2] == before["rows"][1][2] > 0
        assert after["live_ranks_agree"] and after["not_valid"] == [0, 0], after
        assert out["records"] == out["scanned_keys"] == before["rows"][0][2]
        if rank == 1:
            assert out["raised"] == 600 and out["missed"] == 0 and again["raised"] == 0 and again["equal"] == out["records"]
        else:
            assert all(out[k] == 0 for k in RM.COUNTS)
    assert res[0][1] == res[1][1] and res[0][3] == res[1][3]
