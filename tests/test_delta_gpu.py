"""The partitioned census and the delta repair on the device (hkv_table_census_parts_async,
hkv_part_rows_diff_async, hkv_table_extract_parts_async; k_table_census_parts, k_part_rows_diff, k_table_extract's
masked instances) against tests/delta_model.py.

The rows equal the numpy model of the table's image word for word and fold to the census -- fresh populates of the
census's geometries at part_bits 0, 1, a middle value and log2(num_bkts), from both mappings of the kernel;
mid-protocol states with keys that are not VALID, on RMW and big tables too; an INLINE table whose log copies have
gone stale. The masked extract equals the model's records byte for byte under every kind of mask, bucket sub-range
and min_ts, on LOG, INLINE and big tables. The rows' diff against numpy. Refusals. delta_resync on a loopback pair
of different geometry and residency, and group_delta_resync over gloo with two stale ranks.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS, gen_keys  # noqa: E402
from tests import census_model as CM  # noqa: E402
from tests import delta_model as DM  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests import repair_cases as RC  # noqa: E402
from tests import repair_model as RM  # noqa: E402
from tests.gen import bytecopy  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0xA5
CANARY64 = int(np.array([CANARY] * 8, np.uint8).view(np.int64)[0])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_pair(n_keys, num_bkts, log_cap, big=False, machine_id=0, rmw=False):
    from hermes_amd.kvs import HermesKV
    ecl = 4 if big else 0
    sizes = L.Sizes(True, ecl) if ecl else L.DEFAULT
    g = HermesKV(n_keys, num_bkts, log_cap, machine_id, rmw, big, ecl, populate=n_keys > 0)
    o = OracleKVS(num_bkts, log_cap, machine_id, rmw, big, ecl)
    if n_keys:
        o.populate(n_keys, sizes.kvs_value)
    return g, o, sizes


def device_image(g, sizes):
    """the device table's own export (sends an INLINE table to LOG)"""
    cap = g.cfg.log_cap
    return g.index_bytes(), g.log_bytes(0, cap + sizes.entry), g.log_head, cap, sizes


def both(g, o):
    """apply(btype, elems, mb) of tests/repair_cases.py on a device table and its oracle twin"""
    def apply(btype, elems, mb):
        eo = bytecopy(elems)
        g.batch_host(btype, elems, mb)
        o.batch_multi(btype, eo, 1, len(eo), None, mb)
        assert np.array_equal(elems.view(np.uint8), eo.view(np.uint8))
    return apply


def rows_over_canary(g, part_bits):
    """census_parts into a dirty buffer with a canary behind the P rows: (rows uint64 [P, 4], raw bytes)"""
    P = 1 << part_bits
    buf = torch.full((P * 4 + 8,), CANARY64, dtype=torch.int64, device="cuda")
    r = g.census_parts(part_bits, out=buf)
    assert r.tensor.shape == (P, 4) and r.part_bits == part_bits
    host = buf.cpu().numpy()
    assert (host[P * 4:] == CANARY64).all(), f"part_bits {part_bits}: written past P * 32 bytes"
    again = g.census_parts(part_bits, out=buf)       # the same buffer: overwritten, the same bytes
    assert again.tensor.cpu().numpy().tobytes() == host[:P * 4].tobytes(), f"part_bits {part_bits}: second call differs"
    return r.host().copy(), host[:P * 4].tobytes()


def assert_rows(g, image, part_bits, monkeypatch, what):
    """both mappings' rows equal the model's and fold to the device's census"""
    want = DM.part_rows_model(image, part_bits)
    monkeypatch.delenv("HKV_CENSUS_PARTS_MAPPING", raising=False)
    got, raw = rows_over_canary(g, part_bits)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f"{what}, part_bits {part_bits}: rows {bad[:8]} differ: {got[bad[:2]]} != {want[bad[:2]]}"
    monkeypatch.setenv("HKV_CENSUS_PARTS_MAPPING", "B")
    try:
        assert rows_over_canary(g, part_bits)[1] == raw, f"{what}, part_bits {part_bits}: mapping B differs from A"
    finally:
        monkeypatch.delenv("HKV_CENSUS_PARTS_MAPPING", raising=False)
    return got


def bits_of(num_bkts):
    top = num_bkts.bit_length() - 1
    return sorted({0, 1, min(4, top), top // 2, top})


# ------------------------------------------------------------------ 1. census_parts, fresh populate
@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big", [
    (5000, 16384, 1 << 20, False),     # default-shaped: under one key per bucket
    (20000, 2048, 1 << 21, False),     # full buckets, evictions
    (3000, 4096, 1 << 17, False),      # the log wraps: dead slots count nowhere
    (1500, 256, 1 << 20, True),        # big objects, 320-byte entries
    (0, 64, 1 << 16, False),           # no key
    (1, 64, 1 << 16, False),           # one key
    (40, 16, 1 << 16, False),          # 16 buckets: a quarter of one block's step
    (30000, 1 << 21, 1 << 22, False),  # part_bits 21: 32768 tiles for a grid of at most 2048 blocks; part_bits 4:
                                       # one tile, the stride range split over the blocks
])
def test_census_parts_fresh_populate(n_keys, num_bkts, log_cap, big, monkeypatch):
    g, o, sizes = make_pair(n_keys, num_bkts, log_cap, big=big, rmw=big)
    before = g.layout()
    census = g.census().host()
    image = device_image(g, sizes)
    assert CM.census_model(*image) == census
    if n_keys >= 1000:
        assert (census["dead_slots"] > 0) == (g.log_head > log_cap) and census["keys"] > 0
    for part_bits in bits_of(num_bkts):
        got = assert_rows(g, image, part_bits, monkeypatch, "fresh")
        assert DM.fold(got) == DM.census_fold(census), f"part_bits {part_bits}: the rows do not fold to the census"
    lay = g.layout()
    assert lay == before and lay["state"] == LOG and lay["conversions"] == 0 and lay["inline_launches"] == 0
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 2. mid-protocol states
@pytest.mark.parametrize("cfg", [dict(rmw=False, big=False), dict(rmw=True, big=False), dict(rmw=False, big=True)])
def test_census_parts_mid_protocol_states(cfg, monkeypatch):
    """tests/repair_cases.source_script on the device and its oracle twin: VALID, INVALID, WRITE and INVALID_WRITE
    keys at mixed timestamps; the rows equal the model on the twin's image, with keys that are not VALID in two
    partitions or more; where the table has no RMWs, masked extracts of that state too"""
    g, o, sizes = make_pair(1000, 4096, 1 << 22, big=cfg["big"], rmw=cfg["rmw"])
    RC.source_script(both(g, o), gen_keys(1000), sizes)
    image = CM.oracle_image(o, sizes)
    census = g.census().host()
    assert census == CM.census_model(*image) and census["offenders"] > 0
    for part_bits in (0, 3, 12):
        got = assert_rows(g, image, part_bits, monkeypatch, str(cfg))
        assert DM.fold(got) == DM.census_fold(census)
        if part_bits:
            assert (got[:, 3] > 0).sum() >= 2, "not_valid in two partitions or more"
    if not cfg["rmw"]:
        mask = (np.random.default_rng(5).random(8) < 0.5).astype(np.uint8)
        mask[3] = 1
        check_masked(g, image, sizes, 3, mask, "scripted", min_ts=(4 << 8) | 1)
    assert g.layout()["conversions"] == 0
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 3. INLINE with stale logs
def _inline_twelve(name, geo="A"):
    """geometry A, INLINE, two protocol rounds of tests/inline_cases.py (twelve launches) and no export"""
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


def test_census_parts_inline_with_stale_logs(monkeypatch):
    """the rows are read from the lines: they equal the model on the twin's image, and not the model on the image
    a reader of index and log would see"""
    g, o, T, m = _inline_twelve("census_parts inline")
    before = g.layout()
    image = CM.oracle_image(o, L.DEFAULT)
    census = g.census().host()
    assert census["from_lines"] == len(T.inline_keys) > 0 and census["offenders"] >= 8
    idx, log_now, head, cap, _ = image
    _, _, _, phys, ikeys, _ = C.census(idx, T.log, cap)
    stale = log_now.copy()
    at = phys[:, None] + np.arange(64)[None, :]
    stale[at] = T.log[at]
    for part_bits in (0, 4, 9):
        got = assert_rows(g, image, part_bits, monkeypatch, "INLINE")
        assert DM.fold(got) == DM.census_fold(census)
        assert not np.array_equal(got, DM.part_rows_model((idx, stale, head, cap, L.DEFAULT), part_bits))
    assert g.layout() == before, "census_parts moved the layout or its counters"
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 4. the masked extract
def assert_extract(x, want, scanned, sizes, what):
    h = x.host()
    assert h["records"] == len(want), f"{what}: records {h['records']} != model {len(want)}"
    assert h["scanned_keys"] == scanned, f"{what}: scanned_keys {h['scanned_keys']} != model {scanned}"
    got = RM.sort_records(x.records_host(), sizes)
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: records differ from the model"


def check_masked(g, image, sizes, part_bits, mask, what, min_ts=0):
    """the masked extract against the model: the whole range, an uneven sub-range, min_ts, and a short buffer"""
    E = sizes.entry
    n_bkts = DM.num_buckets(image)
    dmask = torch.from_numpy(mask.copy()).cuda()
    rows = g.census_parts(part_bits).host()
    want = DM.extract_parts_model(image, part_bits, mask)
    cap = max(len(want), 1)
    buf = torch.full((cap * E + 64,), CANARY, dtype=torch.uint8, device="cuda")
    x = g.extract(out=buf, cap=len(want), part_bits=part_bits, part_mask=dmask)
    assert_extract(x, want, DM.scanned_parts_model(image, part_bits, mask), sizes, f"{what}: whole")
    assert len(want) == int(rows[mask != 0, 2].sum()), f"{what}: records != the selected rows' keys"
    assert (buf[len(want) * E:].cpu().numpy() == CANARY).all(), f"{what}: written past the records"
    lo, hi = n_bkts // 3 + 1, n_bkts - 5
    if lo < hi:
        part = g.extract((lo, hi), cap=cap, part_bits=part_bits, part_mask=dmask)
        assert_extract(part, DM.extract_parts_model(image, part_bits, mask, lo, hi),
                       DM.scanned_parts_model(image, part_bits, mask, lo, hi), sizes, f"{what}: [{lo}, {hi})")
        if min_ts:
            part = g.extract((lo, hi), min_ts, cap=cap, part_bits=part_bits, part_mask=dmask)
            assert_extract(part, DM.extract_parts_model(image, part_bits, mask, lo, hi, min_ts),
                           DM.scanned_parts_model(image, part_bits, mask, lo, hi), sizes, f"{what}: [{lo}, {hi}) min_ts")
    if min_ts:
        newer = DM.extract_parts_model(image, part_bits, mask, min_ts=min_ts)
        assert_extract(g.extract(min_ts=min_ts, cap=cap, part_bits=part_bits, part_mask=dmask), newer,
                       DM.scanned_parts_model(image, part_bits, mask), sizes, f"{what}: min_ts")
    R = len(want)
    if R >= 4:      # a short buffer over a canary
        buf.fill_(CANARY)
        z = g.extract(out=buf, cap=R - 3, part_bits=part_bits, part_mask=dmask)
        assert z.host() == {"records": R, "scanned_keys": R} and z.written == R - 3
        have = {r.tobytes() for r in want}
        got = z.records_host()
        assert len({r.tobytes() for r in got}) == R - 3 and all(r.tobytes() in have for r in got)
        assert (buf[(R - 3) * E:].cpu().numpy() == CANARY).all(), f"{what}: written past record_cap"
    assert np.array_equal(dmask.cpu().numpy(), mask), "the extract wrote its mask"


def masks_of(part_bits, image, seed):
    P = 1 << part_bits
    rng = np.random.default_rng(seed)
    rows = DM.part_rows_model(image, part_bits)
    one = np.zeros(P, np.uint8)
    one[int(np.argmax(rows[:, 2]))] = 1                       # the fullest partition
    mixed = np.zeros(P, np.uint8)
    pick = rng.permutation(P)[:max(P // 3, 1)]
    mixed[pick] = np.where(np.arange(len(pick)) % 2 == 0, 0x80, 0x01)
    return {"zeros": np.zeros(P, np.uint8), "ones": np.ones(P, np.uint8), "one": one,
            "half": (rng.random(P) < 0.5).astype(np.uint8), "0x80 and 0x01": mixed}


@pytest.mark.parametrize("kind", ["log", "big", "inline"])
def test_extract_parts_against_model(kind):
    if kind == "inline":
        g, o, T, m = _inline_twelve("extract_parts inline")
        sizes, part_bits = L.DEFAULT, 7
        image = CM.oracle_image(o, sizes)
        min_ts = (CM.census_model(*image)["max_ts"] >> 8) << 8         # the newest version only
    else:
        big = kind == "big"
        g, o, sizes = make_pair(1500, 256, 1 << 20, big=True) if big else make_pair(5000, 16384, 1 << 20)
        part_bits = 6 if big else 10
        n_keys = 1500 if big else 5000
        ids = np.arange(0, n_keys // 2, 3)
        mb = L.membership(3, 0)
        for at in range(0, len(ids), RC.BATCH):                       # a write round over a sixth of the keys
            both(g, o)(L.BatchType.invs, RC.invs(gen_keys(n_keys), ids[at:at + RC.BATCH], 1, (4, 1), sizes, 3), mb)
        image = CM.oracle_image(o, sizes)
        min_ts = (4 << 8) | 1
    before = g.layout()
    unmasked = RM.extract_model(image)
    for name, mask in masks_of(part_bits, image, 21).items():
        check_masked(g, image, sizes, part_bits, mask, f"{kind}, {name}", min_ts=min_ts)
        n = len(DM.extract_parts_model(image, part_bits, mask))
        if name == "zeros":
            buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
            x = g.extract(out=buf, part_bits=part_bits, part_mask=torch.from_numpy(mask).cuda())
            assert x.host() == {"records": 0, "scanned_keys": 0} and (buf.cpu().numpy() == CANARY).all()
        elif name == "ones":
            assert n == len(unmasked)
            assert_extract(g.extract(), unmasked, RM.scanned_model(image), sizes, "unmasked")
        else:
            assert 0 < n < len(unmasked), (name, n)
    assert g.layout() == before, "the masked extract moved the layout or its counters"
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 5. the rows' diff
@pytest.mark.parametrize("part_bits", [0, 5, 12, 20])   # one row; a part of a block; 16 blocks; the grid-stride loop
def test_part_rows_diff_against_numpy(part_bits):
    from hermes_amd.replica_group import part_diff
    P = 1 << part_bits
    rng = np.random.default_rng(part_bits)
    a = rng.integers(-(1 << 63), (1 << 63) - 1, size=(P, 4), dtype=np.int64)
    b = a.copy()
    if P > 1:
        change = rng.permutation(P)[:max(P // 7, 1)]
        b[change, rng.integers(0, 4, len(change))] ^= np.int64(1) << rng.integers(0, 63, len(change))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want, n = DM.diff_model(a.view(np.uint64), b.view(np.uint64))
    mask, count = part_diff(da, db)
    assert mask.dtype == torch.uint8 and mask.shape == (P,) and count.shape == (1,)
    assert np.array_equal(mask.cpu().numpy(), want) and int(count.cpu()[0]) == n == (0 if P == 1 else max(P // 7, 1))
    # a single word of a single row, the highest bit of the last word
    c = a.copy()
    c[P - 1, 3] ^= np.int64(-(1 << 63))
    m1, c1 = part_diff(da, torch.from_numpy(c).cuda())
    w1 = np.zeros(P, np.uint8)
    w1[P - 1] = 1
    assert np.array_equal(m1.cpu().numpy(), w1) and int(c1.cpu()[0]) == 1
    for w in range(4):      # every word counts
        d = a.copy()
        d[0, w] += 1
        assert int(part_diff(da, torch.from_numpy(d).cuda())[1].cpu()[0]) == 1
    # accumulate: or-ed into what is there, bytes other than 1 kept; the count is of the result
    prior = np.zeros(P, np.uint8)
    prior[::3] = 0x80
    acc = torch.from_numpy(prior.copy()).cuda()
    m2, c2 = part_diff(da, db, mask=acc)
    want2, n2 = DM.diff_model(a.view(np.uint64), b.view(np.uint64), mask=prior)
    assert m2.data_ptr() == acc.data_ptr()
    assert np.array_equal(acc.cpu().numpy(), want2) and int(c2.cpu()[0]) == n2
    # equal rows: nothing, and accumulate leaves the mask as it is
    m3, c3 = part_diff(da, da.clone())
    assert not m3.cpu().numpy().any() and int(c3.cpu()[0]) == 0
    assert np.array_equal(da.cpu().numpy(), a) and np.array_equal(db.cpu().numpy(), b), "the diff wrote its rows"


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from hermes_amd import lib
    from hermes_amd.kvs import HermesKV
    r = lib.raw()
    E = 64

    def refused(rc, *words):
        msg = r.hkv_last_error()
        assert rc < 0 and msg and all(w in msg for w in words), (rc, msg)

    def P(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)

    rec = torch.full((64 * E + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    rows = torch.full((4 * 2048 + 8,), -1, dtype=torch.int64, device="cuda")
    sel = torch.ones(2048, dtype=torch.uint8, device="cuda")
    g = HermesKV(1000, 1024, 1 << 17, rmw=True)
    refused(r.hkv_table_extract_parts_async(g.h, 4, P(sel), 0, 1024, 0, P(rec), 64, P(res), None), b"extract_parts", b"RMW")
    with pytest.raises(lib.HkvError):
        g.extract(part_bits=4, part_mask=sel)
    assert r.hkv_table_census_parts_async(g.h, 10, P(rows), None) == 0      # an RMW table is accepted, as by the census
    torch.cuda.synchronize()
    assert (rows[4 * 1024:].cpu().numpy() == -1).all()
    rows.fill_(-1)
    g2 = HermesKV(1000, 1024, 1 << 17)
    img = (g2.index_bytes(), g2.log_bytes())
    refused(r.hkv_table_census_parts_async(g2.h, 11, P(rows), None), b"census_parts", b"part_bits")
    refused(r.hkv_table_census_parts_async(g2.h, 40, P(rows), None), b"census_parts", b"part_bits")
    refused(r.hkv_table_census_parts_async(g2.h, 4, P(rows, 8), None), b"census_parts", b"aligned")
    refused(r.hkv_table_census_parts_async(g2.h, 4, None, None), b"census_parts")
    refused(r.hkv_table_extract_parts_async(g2.h, 11, P(sel), 0, 1024, 0, P(rec), 64, P(res), None), b"extract_parts", b"part_bits")
    refused(r.hkv_table_extract_parts_async(g2.h, 4, None, 0, 1024, 0, P(rec), 64, P(res), None), b"extract_parts", b"mask")
    refused(r.hkv_table_extract_parts_async(g2.h, 4, P(sel), 0, 1025, 0, P(rec), 64, P(res), None), b"extract_parts", b"bucket range")
    refused(r.hkv_table_extract_parts_async(g2.h, 4, P(sel), 0, 1024, 0, P(rec, 8), 64, P(res), None), b"extract_parts", b"aligned")
    refused(r.hkv_table_extract_parts_async(g2.h, 4, P(sel), 0, 1024, 0, P(rec), 64, P(res, 8), None), b"extract_parts", b"aligned")
    refused(r.hkv_part_rows_diff_async(P(rows, 8), P(rows), 4, P(sel), P(res), 0, None), b"part_rows_diff", b"aligned")
    refused(r.hkv_part_rows_diff_async(P(rows), None, 4, P(sel), P(res), 0, None), b"part_rows_diff")
    with pytest.raises(lib.HkvError):
        g2.census_parts(11)
    for bits in (40, 63, -1):      # refused by the library, with its message, before 2^bits rows are allocated
        with pytest.raises(lib.HkvError, match="census_parts.*part_bits"):
            g2.census_parts(bits)
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == CANARY).all() and (res.cpu().numpy() == -1).all() and (rows.cpu().numpy() == -1).all()
    assert (sel.cpu().numpy() == 1).all(), "a refused call wrote"
    assert np.array_equal(g2.index_bytes(), img[0]) and np.array_equal(g2.log_bytes(), img[1])
    assert g.take_error_flags() == 0 and g2.take_error_flags() == 0


# ------------------------------------------------------------------ 7. delta_resync, loopback
N_KEYS, PART_BITS = 5000, 10


def _raise(apply, ids, ts, salt, machine_id, sizes=L.DEFAULT, n_keys=N_KEYS, vals=True):
    """INV (and VAL) launches from machine ts[1] that move the keys `ids` to timestamp ts, VALID (INVALID
    without the VALs)"""
    keys = gen_keys(n_keys)
    mb = L.membership(3, machine_id)
    for at in range(0, len(ids), RC.BATCH):
        part = np.asarray(ids[at:at + RC.BATCH])
        apply(L.BatchType.invs, RC.invs(keys, part, ts[1], ts, sizes, salt), mb)
        if vals:
            apply(L.BatchType.vals, RC.vals(keys, part, ts[1], ts), mb)


def assert_tables_equal(g, o, what):
    assert np.array_equal(g.index_bytes(), o.index_bytes()), f"{what}: index differs"
    assert np.array_equal(g.log_bytes(), o.log_bytes()[: g.cfg.log_cap]), f"{what}: log differs"


def _delta_pair():
    """source: 5000 keys in 16384 buckets, INLINE, 37 keys raised by INV + VAL launches run while INLINE; target:
    the same keys in 4096 buckets, LOG"""
    from hermes_amd import kvs
    src, so, _ = make_pair(N_KEYS, 16384, 1 << 20)
    dst, do, _ = make_pair(N_KEYS, 4096, 1 << 19, machine_id=1)
    assert src.evictions == 0 and dst.evictions == 0
    ids = np.random.default_rng(11).permutation(N_KEYS)[:37]
    assert src.prefer_layout(INLINE)
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE     # (the single-workgroup kernel has no inline instance)
    try:
        _raise(both(src, so), ids, (4, 2), 9, 0)
    finally:
        kvs.HermesKV.default_flags = 0
    assert src.layout()["state"] == INLINE and dst.layout()["state"] == LOG
    return src, so, dst, do, ids


def test_delta_resync_loopback():
    from hermes_amd.replica_group import delta_resync
    src, so, dst, do, ids = _delta_pair()
    lay = src.layout()
    parts = np.unique(gen_keys(N_KEYS)[ids] & np.uint64((1 << PART_BITS) - 1)).astype(np.int64)
    mask = np.zeros(1 << PART_BITS, np.uint8)
    mask[parts] = 1
    image = CM.oracle_image(so, L.DEFAULT)
    rec = DM.extract_parts_model(image, PART_BITS, mask)
    want = RM.install_counts(do, rec)
    assert want == {"raised": 37, "equal": len(rec) - 37, "older": 0, "missed": 0}
    out = delta_resync(dst, src, part_bits=PART_BITS)
    RM.apply_records(do, rec, L.DEFAULT, L.membership(3, 1))
    assert {k: out[k] for k in RM.COUNTS} == want
    assert out["differing_before"] == len(parts) and out["partitions"] == 1 << PART_BITS
    assert out["records"] == out["scanned_keys"] == len(rec)
    assert out["records"] * 10 <= N_KEYS          # a tenth of a full repair's records at the most
    assert out["differing_after"] == 0 and out["unresolved"] == []
    assert src.layout() == lay, "the delta repair moved the source's layout or its counters"
    h0, h1 = src.census().host(), dst.census().host()
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert h0[f] == h1[f], f"{f}: source {h0[f]} != target {h1[f]}"
    assert_tables_equal(dst, do, "the target after the delta repair")
    # again: nothing differs, nothing is shipped; and in three bucket chunks after another round of writes
    again = delta_resync(dst, src, part_bits=PART_BITS)
    assert again["differing_before"] == 0 and again["records"] == 0 and again["scanned_keys"] == 0
    assert all(again[k] == 0 for k in RM.COUNTS) and again["differing_after"] == 0
    ids2 = np.arange(1000, 1020)
    _raise(both(src, so), ids2, (6, 2), 4, 0)
    out3 = delta_resync(dst, src, chunk_buckets=16384 // 3 + 1)      # the default part_bits: min(20, log2(4096))
    assert out3["partitions"] == 4096 and out3["raised"] == 20 and out3["differing_after"] == 0
    assert out3["differing_before"] == len(np.unique(gen_keys(N_KEYS)[ids2] & np.uint64(4095)))
    assert src.census().digest_sum == dst.census().digest_sum
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


def test_delta_resync_reports_a_newer_target():
    """one key newer on the target than on the source: its record counts as older, its partition stays in
    `unresolved`, and every other differing partition is resolved"""
    from hermes_amd.replica_group import delta_resync
    src, so, dst, do, ids = _delta_pair()
    keys = gen_keys(N_KEYS)
    P = 1 << PART_BITS
    parts = set((keys[ids] & np.uint64(P - 1)).astype(np.int64).tolist())
    newer = next(i for i in range(N_KEYS) if int(keys[i]) & (P - 1) not in parts)
    # (an INV alone: the reference's VAL loop does not return from a batch of one element, on the oracle twin)
    _raise(both(dst, do), [newer], (9, 2), 13, 1, vals=False)
    out = delta_resync(dst, src, part_bits=PART_BITS)
    own = int(keys[newer]) & (P - 1)
    assert out["differing_before"] == len(parts) + 1
    assert out["older"] == 1 and out["raised"] == 37 and out["missed"] == 0
    assert out["equal"] == out["records"] - 38
    assert out["differing_after"] == 1 and out["unresolved"] == [own]
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


# ------------------------------------------------------------------ 8. group_delta_resync over gloo
G_KEYS, G_BITS = 4000, 10
G_WRITES = {1: np.arange(100, 160), 2: np.arange(2000, 2045)}      # what stale rank 1, and stale rank 2, missed


def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import group_census, group_delta_resync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        g = HermesKV(G_KEYS, (8192, 4096, 16384)[rank], 1 << 20, machine_id=rank)     # three geometries
        keys = gen_keys(G_KEYS)
        mb = L.membership(4, rank)
        for missed_by, ids in G_WRITES.items():      # the source saw both rounds of writes (a fourth machine's), a
            if rank != missed_by:                    # stale rank only the other's
                g.batch_host(L.BatchType.invs, RC.invs(keys, ids, 3, (4, 3), L.DEFAULT, 6), mb)
                g.batch_host(L.BatchType.vals, RC.vals(keys, ids, 3, (4, 3)), mb)
        before = group_census(g, None)
        res = group_delta_resync(g, None, 0, [1, 2], G_BITS, chunk_buckets=8192 // 3 + 1)
        after = group_census(g, None)
        again = group_delta_resync(g, None, 0, [1, 2], None, None)
        q.put((rank, before, res, after, again, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, None, None, 0, repr(e)))


def test_group_delta_resync_over_gloo():
    """three ranks as fresh child processes sharing the GPU over gloo: ranks 1 and 2 each missed other writes of
    rank 0's; the source extracts with the union of their masks, so each stale rank's `equal` covers the other's
    partitions; afterwards the group census agrees"""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_child, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
    part = (gen_keys(G_KEYS) & np.uint64((1 << G_BITS) - 1)).astype(np.int64)
    own = {r: np.unique(part[ids]) for r, ids in G_WRITES.items()}
    union = np.union1d(own[1], own[2])
    n_union = int(np.isin(part, union).sum())
    for rank, before, out, after, again, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert not before["live_ranks_agree"] and before["rows"][0][2] == before["rows"][rank][2] == G_KEYS
        assert after["live_ranks_agree"] and after["not_valid"] == [0, 0, 0], after
        assert out["partitions"] == 1 << G_BITS and out["selected"] == len(union)
        assert out["records"] == out["scanned_keys"] == n_union
        assert out["differing_after"] == 0 and out["unresolved"] == []
        assert again["selected"] == 0 and again["records"] == 0 and again["partitions"] == 4096
        if rank:
            assert out["differing_before"] == len(own[rank])
            assert out["raised"] == len(G_WRITES[rank]) and out["missed"] == 0 and out["older"] == 0
            assert out["equal"] == n_union - len(G_WRITES[rank])
            assert out["equal"] > int(np.isin(part, own[rank]).sum()) - len(G_WRITES[rank]), "the union mask was used"
        else:
            assert all(out[k] == 0 for k in RM.COUNTS) and out["differing_before"] == 0
    assert res[0][1] == res[1][1] == res[2][1] and res[0][3] == res[1][3] == res[2][3]
