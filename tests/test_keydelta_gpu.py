"""The key-level delta repair on the device (hkv_table_summaries_async, hkv_table_need_async, hkv_table_fetch_async;
k_table_summaries, k_table_need, k_table_fetch) against tests/keydelta_model.py and the oracle.

Summaries: the device's 16-byte rows equal the model's as sets -- fresh populates of the extract's geometries under
bucket chunks, min_ts, masks of no, every and about 1 % of the partitions, a NULL mask, a short buffer over a canary;
mid-protocol states in 64-B and 320-B entries; an INLINE table whose log copies have gone stale. Need: the six counts
and the key set equal the model's on tests/repair_cases.py's target, at the counts around the block sizes and past
one grid step, and the table is not written. Fetch: positional, byte for byte. Then key_delta_resync beside
delta_resync on identical pairs, on a loopback group with a failed replica, and group_key_delta_resync over gloo.
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
from tests import keydelta_model as KM  # noqa: E402
from tests import repair_cases as RC  # noqa: E402
from tests import repair_model as RM  # noqa: E402
from tests.gen import bytecopy  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0xA5
CANARY64 = int(np.array([CANARY] * 8, np.uint8).view(np.int64)[0])
NS = [0, 1, 3, 63, 64, 65, 4096, 4097, 140000]     # 140000: past the 131072 a grid of 2048 blocks takes in one step


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


def assert_tables_equal(g, o, what):
    assert np.array_equal(g.index_bytes(), o.index_bytes()), f"{what}: index differs"
    assert np.array_equal(g.log_bytes(), o.log_bytes()[: g.cfg.log_cap]), f"{what}: log differs"


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


def _stale_image(image, T):
    """what a reader of index and log would see of an INLINE table: the inline keys' entries as they were when the
    table was converted, every other entry current"""
    idx, log_now, head, cap, sizes = image
    _, _, _, phys, ikeys, _ = C.census(idx, T.log, cap)
    assert np.array_equal(ikeys, T.inline_keys)
    stale = log_now.copy()
    at = phys[:, None] + np.arange(64)[None, :]
    stale[at] = T.log[at]
    return idx, stale, head, cap, sizes


# ------------------------------------------------------------------ 1. summaries
def check_summaries(g, image, what, part_bits=0, mask=None, rng=None, min_ts=0, short=False):
    """one call against the model, over a canary: counts, the rows as a set, nothing past them"""
    want = KM.sort_summaries(KM.summaries_model(image, part_bits, mask, rng, min_ts))
    lo, hi = (None, None) if rng is None else rng
    scanned = RM.scanned_model(image, lo, hi) if mask is None else DM.scanned_parts_model(image, part_bits, mask, lo, hi)
    R = len(want)
    cap = max(R - 3, 0) if short else R
    buf = torch.full((R * 16 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dmask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    x = g.summaries(rng, min_ts, part_bits if mask is not None or part_bits else None, dmask, out=buf, cap=cap)
    assert x.host() == {"records": R, "scanned_keys": scanned}, f"{what}: {x.host()} != ({R}, {scanned})"
    assert x.written == cap
    got = KM.sort_summaries(x.records_host())
    if short:
        have = {r.tobytes() for r in want}
        assert len({r.tobytes() for r in got}) == cap and all(r.tobytes() in have for r in got), f"{what}: short buffer"
    else:
        assert got.shape == want.shape and np.array_equal(got, want), f"{what}: summaries differ from the model"
    assert (buf[cap * 16:].cpu().numpy() == CANARY).all(), f"{what}: written at or past min(records, cap) * 16"
    if dmask is not None:
        assert np.array_equal(dmask.cpu().numpy(), mask), f"{what}: the call wrote its mask"
    return x


def masks_of(part_bits, seed):
    P = 1 << part_bits
    rng = np.random.default_rng(seed)
    few = np.zeros(P, np.uint8)
    few[rng.permutation(P)[:max(P // 100, 1)]] = 0x80      # about 1 % (any non-zero byte selects)
    return {"none": np.zeros(P, np.uint8), "every": np.ones(P, np.uint8), "1 %": few}


@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big", [
    (5000, 16384, 1 << 20, False),     # default-shaped: under one key per bucket
    (20000, 2048, 1 << 21, False),     # full buckets: lanes take a bucket's fifth to eighth record
    (3000, 4096, 1 << 17, False),      # the log wraps: dead slots leave no summary
    (1500, 256, 1 << 20, True),        # 320-byte entries: still 32 B read per key
    (0, 64, 1 << 16, False),           # no key
    (1, 64, 1 << 16, False),           # one key
    (40, 16, 1 << 16, False),          # 16 buckets: a quarter of one block's step
    (100, 32, 1 << 16, False),         # 32 buckets
])
def test_summaries_fresh_populate(n_keys, num_bkts, log_cap, big):
    g, o, sizes = make_pair(n_keys, num_bkts, log_cap, big=big)
    image = device_image(g, sizes)
    before = g.layout()
    x = check_summaries(g, image, "whole")
    R = x.records
    assert R == CM.census_model(*image)["keys"]
    # twice into one buffer: overwritten, not accumulated
    first, counts = KM.sort_summaries(x.records_host()), x.host()
    x.tensor.fill_(CANARY)
    y = g.summaries(out=x.tensor)
    assert y.host() == counts and np.array_equal(KM.sort_summaries(y.records_host()), first)
    cuts = [0, num_bkts // 3 + 1, num_bkts - 5, num_bkts]
    assert sum(check_summaries(g, image, f"[{lo}, {hi})", rng=(lo, hi)).records for lo, hi in zip(cuts, cuts[1:])) == R
    assert g.summaries((7, 7)).host() == {"records": 0, "scanned_keys": 0}
    if R >= 4:
        check_summaries(g, image, "short buffer", short=True)
    top = num_bkts.bit_length() - 1
    for part_bits in sorted({0, 4, top}):
        for name, mask in masks_of(part_bits, 21 + part_bits).items():
            check_summaries(g, image, f"part_bits {part_bits}, {name}", part_bits, mask)
        check_summaries(g, image, f"part_bits {part_bits}, NULL mask", part_bits)
    if R >= 4:
        check_summaries(g, image, "masked, chunk, short", 4, masks_of(4, 3)["every"], (cuts[1], cuts[2]), short=True)
    # a write round over half the keys, then min_ts above the other half
    if n_keys >= 2:
        half = n_keys // 2
        nb = max(half // 500, 1)
        stride = half // nb
        inv = RC.invs(gen_keys(n_keys), np.arange(nb * stride), 1, (4, 1), sizes, 3)
        g.batch_host(L.BatchType.invs, inv, L.membership(3, 0), n_batches=nb, stride=stride)
        image = device_image(g, sizes)
        t = (4 << 8) | 1
        newer = check_summaries(g, image, "min_ts", min_ts=t).records
        assert newer < R and (n_keys < 1000 or 0 < newer)
        check_summaries(g, image, "min_ts above every key", min_ts=t + 1)
        check_summaries(g, image, "min_ts, mask, chunk", 4, masks_of(4, 5)["every"], (cuts[1], cuts[2]), t)
    lay = g.layout()
    assert lay == before and lay["state"] == LOG and lay["conversions"] == 0 and lay["inline_launches"] == 0
    assert g.take_error_flags() == 0


def test_summaries_grid_stride():
    """2^21 buckets: 4096 block steps of 512 buckets for a grid of at most 2048 blocks"""
    g, o, sizes = make_pair(30000, 1 << 21, 1 << 22)
    image = device_image(g, sizes)
    assert check_summaries(g, image, "whole").records == CM.census_model(*image)["keys"]
    check_summaries(g, image, "1 % of 2^21 partitions, a chunk", 21, masks_of(21, 9)["1 %"], (700001, (1 << 21) - 5))
    assert g.take_error_flags() == 0


@pytest.mark.parametrize("big", [False, True])
def test_summaries_mid_protocol_states(big):
    """tests/repair_cases.source_script on the device and its oracle twin: VALID, INVALID, WRITE and INVALID_WRITE
    keys at mixed timestamps, in 64-B and 320-B entries"""
    g, o, sizes = make_pair(1000, 4096, 1 << 22, big=big)
    RC.source_script(both(g, o), gen_keys(1000), sizes)
    image = CM.oracle_image(o, sizes)
    x = check_summaries(g, image, "scripted")
    states = set(x.summaries_host()["state"].tolist())
    assert {int(L.State.VALID), int(L.State.INVALID), int(L.State.WRITE), int(L.State.INVALID_WRITE)} <= states
    mask = (np.random.default_rng(5).random(8) < 0.5).astype(np.uint8)
    mask[3] = 1
    check_summaries(g, image, "scripted, masked, min_ts", 3, mask, (1000, 4000), (4 << 8) | 1)
    check_summaries(g, image, "scripted, 1 %", 12, masks_of(12, 2)["1 %"])
    assert g.layout()["conversions"] == 0 and g.take_error_flags() == 0


def test_summaries_inline_with_stale_logs():
    """the summaries are read from the lines: they equal the model on the twin's image, and not the summaries a
    reader of index and log would give"""
    g, o, T, m = _inline_twelve("summaries inline")
    before = g.layout()
    image = CM.oracle_image(o, L.DEFAULT)
    x = check_summaries(g, image, "INLINE")
    assert x.records == int(T.present.sum())
    for lo, hi in ((0, 100), (100, 101), (101, T.bkts)):
        check_summaries(g, image, f"INLINE [{lo}, {hi})", rng=(lo, hi))
    t = (CM.census_model(*image)["max_ts"] >> 8) << 8
    check_summaries(g, image, "INLINE, masked, min_ts", 7, masks_of(7, 4)["every"], min_ts=t)
    check_summaries(g, image, "INLINE, 1 %", 7, masks_of(7, 4)["1 %"])
    stale = KM.sort_summaries(KM.summaries_model(_stale_image(image, T)))
    assert not np.array_equal(stale, KM.sort_summaries(x.records_host()))
    assert g.layout() == before, "the summaries moved the layout or its counters"
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 2. need
GEOM = {False: dict(src=(5000, 16384, 1 << 20), dst=(4700, 2048, 1 << 19)),
        True: dict(src=(2000, 1024, 1 << 20), dst=(1800, 512, 1 << 20))}
_cache = {}


def source(big):
    """the scripted source on the device and its oracle twin, made once per entry size (the calls under test are
    read-only): (g, o, sizes, image, records by key)"""
    if ("src", big) not in _cache:
        n_keys, bkts, cap = GEOM[big]["src"]
        g, o, sizes = make_pair(n_keys, bkts, cap, big=big, machine_id=RC.SRC_ID)
        RC.source_script(both(g, o), gen_keys(n_keys), sizes)
        image = CM.oracle_image(o, sizes)
        _cache["src", big] = (g, o, sizes, image, RM.extract_model(image))
    return _cache["src", big]


def target():
    """tests/repair_cases.py's target on the device and its oracle twin, made once, with the source's summaries
    shuffled and their classes by the model: (g, o, summaries, classes)"""
    if "dst" not in _cache:
        n_keys, bkts, cap = GEOM[False]["dst"]
        g, o, sizes = make_pair(n_keys, bkts, cap, machine_id=RC.DST_ID)
        RC.target_script(both(g, o), gen_keys(n_keys), sizes)
        summ = KM.summaries_of_records(source(False)[4], sizes)
        summ = summ[np.random.default_rng(7).permutation(len(summ))]
        counts, _, cls = KM.need_model(o, summ, sizes)
        # the pair produces every one of the six classes
        assert all(counts[c] > 0 for c in KM.CLASSES), counts
        _cache["dst"] = (g, o, summ, cls)
    return _cache["dst"]


def need_want(cls, summ):
    counts = {c: int((cls == c).sum()) for c in KM.CLASSES}
    need = np.isin(cls, KM.NEEDED) if len(cls) else np.zeros(0, bool)
    counts["needed"] = int(need.sum())
    return counts, np.sort(summ["key"][need].astype(np.uint64))


@pytest.mark.parametrize("n", NS)
def test_need_against_model(n):
    g, o, summ, cls = target()
    idx = np.resize(np.arange(len(summ)), n) if n > len(summ) else np.arange(n)      # 140000: every summary 28 times
    s, c = summ[idx], cls[idx]
    want, want_keys = need_want(c, s)
    if n == NS[-1]:
        assert all(want[k] > 0 for k in KM.CLASSES), want
    table = (g.index_bytes(), g.log_bytes())
    dev = torch.from_numpy(s.view(np.uint8).reshape(-1).copy() if n else np.zeros(16, np.uint8)).cuda()
    keys = torch.full((n + 8,), CANARY64, dtype=torch.int64, device="cuda")
    nd = g.need(dev, n=n, out=keys[:max(n, 1)])
    assert nd.host() == want, f"n = {n}: {nd.host()} != {want}"
    host = keys.cpu().numpy()
    assert np.array_equal(np.sort(host[:want["needed"]].view(np.uint64)), want_keys), f"n = {n}: the key set differs"
    assert (host[want["needed"]:] == CANARY64).all(), f"n = {n}: written at or past needed * 8"
    if n:
        assert np.array_equal(dev.cpu().numpy(), s.view(np.uint8).reshape(-1)), "need wrote its summaries"
    assert np.array_equal(g.index_bytes(), table[0]) and np.array_equal(g.log_bytes(), table[1]), "need wrote the table"
    assert g.layout()["conversions"] == 0 and g.take_error_flags() == 0


def test_need_short_list_and_defaults():
    """need_cap below needed, over a canary; the result is overwritten; need(Summaries) takes its count"""
    g, o, summ, cls = target()
    want, want_keys = need_want(cls, summ)
    K = want["needed"]
    assert K > 10
    dev = torch.from_numpy(summ.view(np.uint8).reshape(-1).copy()).cuda()
    keys = torch.full((K + 8,), CANARY64, dtype=torch.int64, device="cuda")
    nd = g.need(dev, out=keys[:K - 6])
    assert nd.host() == want and nd.written == K - 6
    host = keys.cpu().numpy()
    got = host[:K - 6].view(np.uint64)
    have = want_keys.tolist()
    assert len(set(got.tolist())) == K - 6 and set(got.tolist()) <= set(have)
    assert (host[K - 6:] == CANARY64).all(), "written at or past need_cap * 8"
    # straight from the source's summaries (an int64 view of them is taken too), n read from the Summaries
    sg = source(False)[0]
    sm = sg.summaries()
    nd2 = g.need(sm)
    assert nd2.host() == want and np.array_equal(np.sort(nd2.keys_host()), want_keys)
    nd3 = g.need(sm.tensor.view(torch.int64)[:2 * sm.records])
    assert nd3.host() == want
    assert g.take_error_flags() == 0 and sg.take_error_flags() == 0


def test_need_inline_target_with_stale_logs():
    """summaries made from the twin's image and moved: every fourth newer, older, of another state, the rest equal,
    and absent keys; on an INLINE target after twelve launches and no export"""
    g, o, T, m = _inline_twelve("need inline")
    before = g.layout()
    image = CM.oracle_image(o, L.DEFAULT)
    summ = KM.summaries_model(image).copy()
    i = np.arange(len(summ)) % 4
    i[np.nonzero(summ["state"] != KM.VALID)[0][::2]] = 3      # (half of the keys that are not VALID: to VALID)
    summ["ts_ver"][i == 0] += 10
    summ["ts_ver"][i == 2], summ["ts_cid"][i == 2] = 0, 0
    flip = i == 3
    summ["state"][flip] = np.where(summ["state"][flip] == KM.VALID, int(L.State.INVALID), KM.VALID)
    absent = np.zeros(40, KM.SUMMARY)
    absent["key"] = np.setdiff1d(gen_keys(T.n_keys + 40), T.keys)[:40]
    absent["ts_ver"], absent["state"] = 3, KM.VALID
    summ = np.concatenate([summ, absent])[np.random.default_rng(2).permutation(len(summ) + 40)]
    want, want_keys, cls = KM.need_model(o, summ)
    assert all(want[c] > 0 for c in KM.CLASSES), want
    inl = T.is_inline(summ["key"])
    assert len({c for c in cls[inl]}) >= 5 and 0 < inl.sum() < len(summ)      # inline keys and keys read from the log
    # a reader of the stale log copies would class the inline keys otherwise
    stale = _stale_image(image, T)
    moved = 0
    for s, c in zip(summ[inl][:400], cls[inl][:400]):
        off = KM.lookup_image(stale, int(s["key"]))
        e = stale[1][off:off + 64].copy().view(L.entry_dtype(L.DEFAULT))[0]
        moved += KM.classify((int(s["ts_ver"]) << 8) | int(s["ts_cid"]), int(s["state"]),
                             (int(e["ts_ver"]) << 8) | int(e["ts_cid"]), int(e["state"])) != c
    assert moved > 0
    nd = g.need(torch.from_numpy(summ.view(np.uint8).reshape(-1).copy()).cuda())
    assert nd.host() == want and np.array_equal(np.sort(nd.keys_host()), want_keys)
    assert g.layout() == before, "need moved the layout or its counters"
    m.check_table("after need")
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 3. fetch
def fetch_keys(big, n, seed):
    """n keys of the source's, of keys it does not hold, repeated and in shuffled order, with the model's records"""
    g, o, sizes, image, records = source(big)
    held = records[:, 8:16].copy().view("<u8").reshape(-1)
    n_src = GEOM[big]["src"][0]
    absent = np.setdiff1d(gen_keys(n_src + 64), gen_keys(n_src))[:50]
    pool = np.concatenate([held, absent]).astype(np.uint64)
    if ("pool", big) not in _cache:
        _cache["pool", big] = KM.fetch_model(image, pool)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(pool), n)
    if n >= 3:
        pick[0], pick[1], pick[2] = len(held), 5, 5          # an absent key first, then one key twice
    return pool[pick], _cache["pool", big][pick], int((pick >= len(held)).sum())


@pytest.mark.parametrize("big,n", [(False, n) for n in NS] + [(True, n) for n in (1, 3, 65, 4097)])
def test_fetch_against_model(big, n):
    g, o, sizes, image, records = source(big)
    E = sizes.entry
    keys, want, n_absent = fetch_keys(big, n, 11 + n)
    if 3 <= n <= 65:
        assert np.array_equal(want, KM.fetch_model(image, keys))     # (the pool's rows are the model's)
    dk = torch.from_numpy(keys.view(np.int64).copy() if n else np.zeros(2, np.int64)).cuda()
    buf = torch.full((n * E + 64,), CANARY, dtype=torch.uint8, device="cuda")
    f = g.fetch(dk, n=n, out=buf)
    assert f.host() == {"found": n - n_absent, "absent": n_absent}
    got = f.records_host()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f"n = {n}: records {bad[:8]} differ"
    assert (buf[n * E:].cpu().numpy() == CANARY).all(), "written past n * E"
    if n >= 3:
        assert n_absent > 0 and not got[0, :8].any() and not got[0, 16:].any() and np.array_equal(got[1], got[2])
        # two calls into one buffer: the second's keys, nothing of the first's
        keys2, want2, absent2 = fetch_keys(big, n, 99 + n)
        f2 = g.fetch(torch.from_numpy(keys2.view(np.int64).copy()).cuda(), out=buf)
        assert f2.host() == {"found": n - absent2, "absent": absent2} and np.array_equal(f2.records_host(), want2)
    assert g.layout()["conversions"] == 0 and g.take_error_flags() == 0


def test_fetch_inline_source_with_stale_logs():
    g, o, T, m = _inline_twelve("fetch inline")
    before = g.layout()
    image = CM.oracle_image(o, L.DEFAULT)
    present = T.keys[T.present]
    absent = np.setdiff1d(gen_keys(T.n_keys + 40), T.keys)[:10]
    keys = np.concatenate([present, absent, present[:7]]).astype(np.uint64)
    keys = keys[np.random.default_rng(3).permutation(len(keys))]
    want = KM.fetch_model(image, keys)
    f = g.fetch(torch.from_numpy(keys.view(np.int64).copy()).cuda())
    assert f.host() == {"found": len(present) + 7, "absent": 10}
    assert np.array_equal(f.records_host(), want)
    assert not np.array_equal(KM.fetch_model(_stale_image(image, T), keys), want)
    assert 0 < T.is_inline(keys).sum() < len(keys)
    assert g.layout() == before, "the fetch moved the layout or its counters"
    m.check_table("after fetch")
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 4. refusals
def test_refusals():
    from hermes_amd import lib
    from hermes_amd.kvs import HermesKV
    r = lib.raw()

    def refused(rc, *words):
        msg = r.hkv_last_error()
        assert rc < 0 and msg and all(w in msg for w in words), (rc, msg)

    def P(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)

    buf = torch.full((64 * 64 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    keys = torch.full((64,), CANARY64, dtype=torch.int64, device="cuda")
    sel = torch.ones(2048, dtype=torch.uint8, device="cuda")
    g = HermesKV(1000, 1024, 1 << 17, rmw=True)
    refused(r.hkv_table_summaries_async(g.h, 4, P(sel), 0, 1024, 0, P(buf), 64, P(res), None), b"summaries", b"RMW")
    refused(r.hkv_table_need_async(g.h, P(buf), 4, P(keys), 4, P(res), None), b"need", b"RMW")
    refused(r.hkv_table_fetch_async(g.h, P(keys), 4, P(buf), P(res), None), b"fetch", b"RMW")
    for call in (lambda: g.summaries(), lambda: g.need(buf, n=4), lambda: g.fetch(keys, n=4)):
        with pytest.raises(lib.HkvError):
            call()
    g2 = HermesKV(1000, 1024, 1 << 17)
    img = (g2.index_bytes(), g2.log_bytes())
    refused(r.hkv_table_summaries_async(g2.h, 11, P(sel), 0, 1024, 0, P(buf), 64, P(res), None), b"summaries", b"part_bits")
    refused(r.hkv_table_summaries_async(g2.h, 11, None, 0, 1024, 0, P(buf), 64, P(res), None), b"summaries", b"part_bits")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 0, 1025, 0, P(buf), 64, P(res), None), b"summaries", b"bucket range")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 9, 8, 0, P(buf), 64, P(res), None), b"summaries", b"bucket range")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 0, 1024, 0, P(buf, 8), 64, P(res), None), b"summaries", b"aligned")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 0, 1024, 0, P(buf), 64, P(res, 8), None), b"summaries", b"aligned")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 0, 1024, 0, None, 64, P(res), None), b"summaries")
    refused(r.hkv_table_summaries_async(g2.h, 4, P(sel), 0, 1024, 0, P(buf), 64, None, None), b"summaries")
    refused(r.hkv_table_need_async(g2.h, P(buf, 8), 4, P(keys), 4, P(res), None), b"need", b"aligned")
    refused(r.hkv_table_need_async(g2.h, P(buf), 4, P(keys, 8), 4, P(res), None), b"need", b"aligned")
    refused(r.hkv_table_need_async(g2.h, P(buf), 4, P(keys), 4, P(res, 8), None), b"need", b"aligned")
    refused(r.hkv_table_need_async(g2.h, None, 4, P(keys), 4, P(res), None), b"need")
    refused(r.hkv_table_need_async(g2.h, P(buf), 4, None, 4, P(res), None), b"need")
    refused(r.hkv_table_need_async(g2.h, P(buf), 4, P(keys), 4, None, None), b"need")
    refused(r.hkv_table_fetch_async(g2.h, P(keys, 8), 4, P(buf), P(res), None), b"fetch", b"aligned")
    refused(r.hkv_table_fetch_async(g2.h, P(keys), 4, P(buf, 8), P(res), None), b"fetch", b"aligned")
    refused(r.hkv_table_fetch_async(g2.h, P(keys), 4, P(buf), P(res, 8), None), b"fetch", b"aligned")
    refused(r.hkv_table_fetch_async(g2.h, None, 4, P(buf), P(res), None), b"fetch")
    refused(r.hkv_table_fetch_async(g2.h, P(keys), 4, None, P(res), None), b"fetch")
    with pytest.raises(lib.HkvError, match="summaries.*part_bits"):
        g2.summaries(part_bits=11, part_mask=sel)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all() and (res.cpu().numpy() == -1).all() and (keys.cpu().numpy() == CANARY64).all()
    assert (sel.cpu().numpy() == 1).all(), "a refused call wrote"
    assert np.array_equal(g2.index_bytes(), img[0]) and np.array_equal(g2.log_bytes(), img[1])
    assert g.take_error_flags() == 0 and g2.take_error_flags() == 0


# ------------------------------------------------------------------ 5. key_delta_resync, loopback
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


def _raised_pair(n_raised=1000):
    """source: 5000 keys in 16384 buckets with n_raised keys raised to (4, 2), the last tenth of them left INVALID;
    target: the same keys in 4096 buckets"""
    src, so, _ = make_pair(N_KEYS, 16384, 1 << 20)
    dst, do, _ = make_pair(N_KEYS, 4096, 1 << 19, machine_id=1)
    ids = np.random.default_rng(11).permutation(N_KEYS)[:n_raised]
    cut = n_raised - n_raised // 10
    _raise(both(src, so), ids[:cut], (4, 2), 9, 0)
    _raise(both(src, so), ids[cut:], (4, 2), 9, 0, vals=False)
    return src, so, dst, do, ids


def model_repair(so, do, part_bits, mb):
    """the key-level repair on the oracle twins by its definition: the rows' diff, the source's summaries of the
    differing partitions, the target's need list, the source's records of it applied to the target's twin"""
    S = L.DEFAULT
    image = CM.oracle_image(so, S)
    rows_s = DM.part_rows_model(image, part_bits)
    mask, differing = DM.diff_model(rows_s, DM.part_rows_model(CM.oracle_image(do, S), part_bits))
    summ = KM.summaries_model(image, part_bits, mask)
    counts, need_keys, _ = KM.need_model(do, summ, S)
    rec = KM.fetch_model(image, need_keys)
    install = RM.install_counts(do, rec, S)
    RM.apply_records(do, rec, S, mb)
    return differing, len(summ), counts, install


def test_key_delta_resync_beside_delta_resync():
    from hermes_amd.replica_group import delta_resync, key_delta_resync
    E = 64
    src, so, dst, do, ids = _raised_pair()
    src2, _, dst2, _, _ = _raised_pair()
    lay = src.layout()
    ref = delta_resync(dst2, src2, part_bits=PART_BITS)
    out = key_delta_resync(dst, src, part_bits=PART_BITS)
    differing, n_summ, counts, install = model_repair(so, do, PART_BITS, L.membership(3, 1))
    assert counts["newer"] == 1000 and counts["missed"] == 0 and counts["needed"] == 1000
    assert out["classes"] == {c: counts[c] for c in KM.CLASSES} and out["needed"] == 1000 == out["records"]
    assert out["summaries"] == n_summ == ref["records"] == out["scanned_keys"]
    assert {k: out[k] for k in RM.COUNTS} == install == {"raised": 1000, "equal": 0, "older": 0, "missed": 0}
    assert out["differing_before"] == differing == ref["differing_before"] and out["partitions"] == 1 << PART_BITS
    assert out["differing_after"] == ref["differing_after"] == 0 and out["unresolved"] == ref["unresolved"] == []
    assert np.array_equal(dst.census_parts(PART_BITS).host(), dst2.census_parts(PART_BITS).host())
    assert np.array_equal(dst.census_parts(PART_BITS).host(), src.census_parts(PART_BITS).host())
    assert_tables_equal(dst, do, "the target after the key-level repair")
    assert out["bytes_summaries"] == 16 * n_summ and out["bytes_keys"] == 8 * 1000 and out["bytes_records"] == E * 1000
    assert out["bytes_partition_delta"] == E * n_summ == E * ref["records"]
    assert out["bytes_summaries"] + out["bytes_keys"] + out["bytes_records"] < out["bytes_partition_delta"]
    assert src.layout() == lay
    # nothing differs: nothing is shipped
    again = key_delta_resync(dst, src, part_bits=PART_BITS)
    assert again["differing_before"] == 0 and again["summaries"] == again["needed"] == again["records"] == 0
    assert all(again[k] == 0 for k in RM.COUNTS) and not any(again["classes"].values())
    assert again["bytes_summaries"] == again["bytes_keys"] == again["bytes_records"] == again["bytes_partition_delta"] == 0
    # in three bucket chunks after another round of writes, at the default part_bits
    _raise(both(src, so), np.arange(1000, 1020), (6, 2), 4, 0)
    out3 = key_delta_resync(dst, src, chunk_buckets=16384 // 3 + 1)
    assert out3["partitions"] == 4096 and out3["raised"] == out3["needed"] == 20 and out3["differing_after"] == 0
    assert out3["classes"]["same"] == out3["summaries"] - 20
    assert src.census().digest_sum == dst.census().digest_sum
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


def test_key_delta_resync_reports_what_it_cannot_repair():
    """a key newer on the target (class older) and a key the target lacks (missed, fetched and missed by the install,
    as in delta_resync): both partitions stay in unresolved"""
    from hermes_amd.replica_group import key_delta_resync
    src, so, _ = make_pair(N_KEYS, 16384, 1 << 20)
    dst, do, _ = make_pair(N_KEYS - 1, 4096, 1 << 19, machine_id=1)      # the target lacks the last id
    keys = gen_keys(N_KEYS)
    _raise(both(src, so), np.arange(100, 137), (4, 2), 9, 0)
    _raise(both(dst, do), [4000], (9, 2), 13, 1, vals=False)
    out = key_delta_resync(dst, src, part_bits=PART_BITS)
    differing, n_summ, counts, install = model_repair(so, do, PART_BITS, L.membership(3, 1))
    assert counts["older"] == 1 and counts["missed"] == 1 and counts["newer"] == 37
    assert out["classes"] == {c: counts[c] for c in KM.CLASSES} and out["needed"] == 38
    assert {k: out[k] for k in RM.COUNTS} == install == {"raised": 37, "equal": 0, "older": 0, "missed": 1}
    P = 1 << PART_BITS
    left = sorted({int(keys[4000]) & (P - 1), int(keys[N_KEYS - 1]) & (P - 1)})
    assert out["differing_after"] == len(left) and sorted(out["unresolved"]) == left
    assert_tables_equal(dst, do, "the target")
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


def test_key_delta_resync_insert_rebuilds_an_empty_target():
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import key_delta_resync
    n_keys, bkts, cap = 4000, 8192, 1 << 20
    src, so, sizes = make_pair(n_keys, bkts, cap)
    _raise(both(src, so), np.arange(100, 700), (4, 2), 6, 0, n_keys=n_keys)
    dst = HermesKV(n_keys, bkts // 2, cap, machine_id=1, populate=False)
    out = key_delta_resync(dst, src, chunk_buckets=bkts // 3 + 1, insert=True)
    held = src.census().keys
    assert out["summaries"] == out["needed"] == out["inserted"] == out["classes"]["missed"] == held
    assert out["missed"] == 0 and out["raised"] == out["equal"] == 0
    assert out["replaced"] + out["evictions"] == 0
    a, b = src.census().host(), dst.census().host()
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert a[f] == b[f], f
    assert out["differing_after"] == 0 and out["unresolved"] == []
    again = key_delta_resync(dst, src, insert=True)
    assert again["summaries"] == 0 and again["inserted"] == 0
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0


def test_key_delta_resync_loopback_group():
    """Three replicas; replica 2 fails between rounds and the others run three more: key_delta_resync from replica
    0 brings replica 2's partition rows and digest to replica 0's and its image to its oracle twin's after the
    model's needed records."""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import LoopbackGroup, ReplicaRound, key_delta_resync
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
    src, dst = mirrors[0].g, mirrors[2].g
    assert src.census().digest_sum != dst.census().digest_sum
    differing, n_summ, counts, install = model_repair(mirrors[0].o, mirrors[2].o, 8, L.membership(n_rep, 2))
    out = key_delta_resync(dst, src, part_bits=8, chunk_buckets=bkts // 3 + 1)
    assert out["differing_before"] == differing > 0 and out["summaries"] == n_summ
    assert out["classes"] == {c: counts[c] for c in KM.CLASSES} and counts["newer"] > 0 and counts["missed"] == 0
    assert {k: out[k] for k in RM.COUNTS} == install and out["needed"] == counts["needed"] < n_summ
    assert out["differing_after"] == 0 and out["unresolved"] == []
    h0, h2 = src.census().host(), dst.census().host()
    for f in ("digest_sum", "digest_xor", "keys", "by_state"):
        assert h0[f] == h2[f], f"{f}: replica 0 {h0[f]} != replica 2 {h2[f]}"
    mirrors[2].check_table("replica 2 after the key-level repair")
    assert key_delta_resync(dst, src, part_bits=8)["summaries"] == 0
    assert all(m.g.take_error_flags() == 0 for m in mirrors)


# ------------------------------------------------------------------ 6. group_key_delta_resync over gloo
G_KEYS, G_BITS = 4000, 10
G_WRITES = np.arange(100, 700)      # what the stale rank missed


def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import group_census, group_key_delta_resync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        g = HermesKV(G_KEYS, (8192, 4096)[rank], 1 << 20, machine_id=rank)     # the stale rank has another geometry
        keys = gen_keys(G_KEYS)
        if rank == 0:
            mb = L.membership(3, 0)
            for lo in range(0, len(G_WRITES), 200):
                ids = G_WRITES[lo:lo + 200]
                g.batch_host(L.BatchType.invs, RC.invs(keys, ids, 2, (4, 2), L.DEFAULT, 6), mb)
                g.batch_host(L.BatchType.vals, RC.vals(keys, ids, 2, (4, 2)), mb)
        before = group_census(g, None)
        res = group_key_delta_resync(g, None, 0, [1], G_BITS, chunk_buckets=8192 // 3 + 1)
        after = group_census(g, None)
        again = group_key_delta_resync(g, None, 0, [1], None, None)
        q.put((rank, before, res, after, again, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, None, None, 0, repr(e)))


def test_group_key_delta_resync_over_gloo():
    """two ranks as fresh child processes sharing the GPU over gloo: rank 1 missed INVs and VALs that rank 0
    applied; the source ships summaries, takes rank 1's need list and ships those 600 records; afterwards the group
    census agrees"""
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
    part = (gen_keys(G_KEYS) & np.uint64((1 << G_BITS) - 1)).astype(np.int64)
    own = np.unique(part[G_WRITES])
    n_sel = int(np.isin(part, own).sum())
    for rank, before, out, after, again, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert not before["live_ranks_agree"] and before["rows"][0][2] == before["rows"][1][2] == G_KEYS
        assert after["live_ranks_agree"] and after["not_valid"] == [0, 0], after
        assert out["partitions"] == 1 << G_BITS and out["selected"] == len(own)
        assert out["summaries"] == out["scanned_keys"] == n_sel and out["records"] == 600
        assert out["bytes_summaries"] == 16 * n_sel and out["bytes_records"] == 64 * 600
        assert out["bytes_partition_delta"] == 64 * n_sel
        assert out["differing_after"] == 0 and out["unresolved"] == []
        assert again["selected"] == 0 and again["summaries"] == 0 and again["records"] == 0
        if rank == 1:
            assert out["differing_before"] == len(own) and out["needed"] == 600
            assert out["classes"] == {"missed": 0, "newer": 600, "validate": 0, "same": n_sel - 600, "state_only": 0, "older": 0}
            assert {k: out[k] for k in RM.COUNTS} == {"raised": 600, "equal": 0, "older": 0, "missed": 0}
        else:
            assert all(out[k] == 0 for k in RM.COUNTS) and out["needed"] == 0 and not any(out["classes"].values())
    assert res[0][1] == res[1][1] and res[0][3] == res[1][3]
