"""The invertible sketch on the device (hkv_summaries_sketch_async, hkv_sketch_decode_async; k_sketch_fold,
k_sketch_subtract, k_sketch_pass, k_sketch_close) against tests/sketch_model.py: the cells byte for byte at the
counts around the block size and the subtable sizes from one cell to several blocks; every decode case's lists as
sets, remainder cells, pass count, undecoded and exhausted; short lists over a canary; the refusals. Then
sketch_delta_resync beside key_delta_resync on identically built pairs and the oracle twin, its fallback, its insert,
and group_sketch_delta_resync over gloo.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import gen_keys  # noqa: E402
from tests import census_model as CM  # noqa: E402
from tests import delta_model as DM  # noqa: E402
from tests import keydelta_model as KM  # noqa: E402
from tests import repair_cases as RC  # noqa: E402
from tests import repair_model as RM  # noqa: E402
from tests import sketch_model as SM  # noqa: E402
from tests.test_keydelta_gpu import _raise, assert_tables_equal, both, make_pair  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0xA5
CANARY64 = int(np.array([CANARY] * 8, np.uint8).view(np.int64)[0])
NS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4099]      # around a wave, around a block, past sixteen blocks
SUBS = [1, 2, 32, 1000, 4096]                         # one cell; not a power of two; sixteen blocks of a pass


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev_bytes(summ):
    """a list of summaries on the device (never an empty tensor)"""
    raw = np.ascontiguousarray(summ).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if len(raw) else np.zeros(16, np.uint8)).cuda()


def dev_sketch(summ, sub, **kw):
    from hermes_amd.kvs import sketch
    return sketch(dev_bytes(summ), sub, n=len(summ), **kw)


_elems = {}


def elements(n, seed=5):
    if (n, seed) not in _elems:
        _elems[n, seed] = SM.random_elements(np.random.default_rng(seed), n)
    return _elems[n, seed]


# ------------------------------------------------------------------ 1. the fold
@pytest.mark.parametrize("sub", SUBS)
def test_cells_against_model(sub):
    for n in NS:
        e = elements(4099)[:n]
        got = dev_sketch(e, sub)
        assert got.sub_cells == sub and got.nbytes == 96 * sub
        assert np.array_equal(got.host(), SM.sketch_model(e, sub)), f"n = {n}, S = {sub}: cells differ from the model"


def test_duplicate_accumulate_and_overwrite():
    from hermes_amd.kvs import sketch
    e = elements(4099)
    sub = 100
    # a duplicated element counts twice and cancels in the xor words
    twice = np.concatenate([e[:40], e[7:8]])
    got = dev_sketch(twice, sub)
    assert np.array_equal(got.host(), SM.sketch_model(twice, sub))
    assert not np.array_equal(got.host(), SM.sketch_model(e[:40], sub))
    # accumulate equals concatenation, into a Sketch and into a bare tensor of dirty cells
    whole = SM.sketch_model(e[:700], sub)
    sk = dev_sketch(e[:300], sub)
    assert dev_sketch(e[300:700], sub, out=sk, accumulate=True).cells.data_ptr() == sk.cells.data_ptr()
    assert np.array_equal(sk.host(), whole)
    # a second call into the same buffer gives the same bytes: overwritten, not accumulated
    raw = torch.full((3 * sub * 4,), CANARY64, dtype=torch.int64, device="cuda")
    for _ in range(2):
        assert np.array_equal(dev_sketch(e[:700], sub, out=raw).host(), whole)
    # a shuffled list, and a list passed as int64 words with its count taken from its length
    shuffled = e[:700][np.random.default_rng(1).permutation(700)]
    assert np.array_equal(sketch(dev_bytes(shuffled).view(torch.int64), sub).host(), whole)
    # no element: all-zero cells over dirty ones
    assert not dev_sketch(e[:0], sub, out=raw).host().any()


# ------------------------------------------------------------------ 2. the decode
def check_decode(list_a, list_b, sub, what):
    """one decode against the model: counts, lists as sets, the remainder, the reserved words; A's buffer holds the
    remainder and B's is not written"""
    from hermes_amd.kvs import sketch_decode
    A, B = SM.sketch_model(list_a, sub), SM.sketch_model(list_b, sub)
    want = SM.decode_model(A, B, sub)
    a, b = dev_sketch(list_a, sub), dev_sketch(list_b, sub)
    d = sketch_decode(a, b)
    got = d.host()
    counts = {"only_a": len(want["only_a"]), "only_b": len(want["only_b"]), "undecoded": want["undecoded"],
              "passes": want["passes"], "exhausted": want["exhausted"]}
    assert got == counts, f"{what}: {got} != {counts}"
    assert not d.result[5:].cpu().numpy().any(), f"{what}: reserved words"
    assert d.remainder is a and np.array_equal(a.host(), want["cells"]), f"{what}: the remainder differs from the model"
    assert np.array_equal(b.host(), B), f"{what}: the decode wrote B"
    la, lb = d.only_a_host(), d.only_b_host()
    assert len(la) == counts["only_a"] and SM.as_set(la) == SM.as_set(want["only_a"]), f"{what}: only_a"
    assert len(lb) == counts["only_b"] and SM.as_set(lb) == SM.as_set(want["only_b"]), f"{what}: only_b"
    return want


def test_decode_identical_and_disjoint_lists():
    e = elements(4099)
    w = check_decode(e[:500], e[:500][::-1], 100, "identical lists")
    assert w["passes"] == 0 and w["undecoded"] == 0 and not w["cells"].any()
    w = check_decode(e[:0], e[:0], 1, "empty lists, one cell")
    assert w["passes"] == 0
    w = check_decode(e[:40], e[40:100], 80, "disjoint lists")
    assert w["undecoded"] == 0 and len(w["only_a"]) == 40 and len(w["only_b"]) == 60
    w = check_decode(e[:1], e[:0], 1, "one element, one cell")
    assert w["undecoded"] == 0 and w["passes"] == 1
    w = check_decode(e[:0], e[:1], 1, "one element on the other side")
    assert w["undecoded"] == 0 and len(w["only_b"]) == 1


@pytest.mark.parametrize("n,seed", [(1, 1), (10, 1), (100, 1), (100, 3), (1000, 1)])
def test_decode_random_differences(n, seed):
    """tests/test_sketch_cpu.py's cases at 2.0 cells per element, (100, 3) being the one that keeps a 2-core"""
    list_a, list_b, only_a, only_b = SM.difference_case(n, seed)
    w = check_decode(list_a, list_b, max(32, -(-2 * n // 3)), f"n = {n}, seed {seed}")
    assert (w["undecoded"] == 0) == ((n, seed) != (100, 3))
    if not w["undecoded"]:
        assert SM.as_set(w["only_a"]) == SM.as_set(only_a) and SM.as_set(w["only_b"]) == SM.as_set(only_b)


def test_decode_many_passes_and_many_blocks():
    e = elements(4099)
    w = check_decode(e[:1000], e[:0], 434, "1000 elements in 1.3 cells each")
    assert w["undecoded"] == 0 and w["passes"] > 12
    w = check_decode(e[:3000], e[3000:4099], 2800, "4099 elements over eleven blocks a pass")
    assert w["undecoded"] == 0 and len(w["only_a"]) == 3000 and len(w["only_b"]) == 1099


def test_decode_undecodable_and_partial():
    e = elements(4099)
    w = check_decode(e[:2], e[:0], 1, "S = 1, two elements on one side")
    assert w["undecoded"] == 3 and w["passes"] == 0
    w = check_decode(e[:2], e[2:3], 1, "S = 1 with +1, +1, -1")
    assert w["undecoded"] == 3 and w["passes"] == 0 and w["cells"][:, 0].tolist() == [1, 1, 1]
    w = check_decode(np.concatenate([e[:1], e[:1], e[1:2]]), e[:0], 50, "a duplicate stays")
    assert w["undecoded"] == 3 and len(w["only_a"]) == 1
    w = check_decode(SM.random_elements(np.random.default_rng(11), 60), e[:0], 16, "60 elements in 48 cells")
    assert w["undecoded"] > 0 and 0 < len(w["only_a"]) < 60


def test_decode_short_lists_over_a_canary():
    """cap_a and cap_b below the counts: the counts exceed the caps, the elements past them still leave the cells,
    and nothing is written at or past cap * 16 bytes"""
    from hermes_amd import lib
    r = lib.raw()
    e = elements(4099)
    sub = 200
    list_a, list_b = e[:130], e[100:300]      # 100 only in A, 170 only in B
    want = SM.decode_model(SM.sketch_model(list_a, sub), SM.sketch_model(list_b, sub), sub)
    assert want["undecoded"] == 0 and len(want["only_a"]) == 100 and len(want["only_b"]) == 170
    for cap_a, cap_b in ((7, 64), (0, 0)):
        a, b = dev_sketch(list_a, sub), dev_sketch(list_b, sub)
        la = torch.full((100 * 16 + 64,), CANARY, dtype=torch.uint8, device="cuda")
        lb = torch.full((170 * 16 + 64,), CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        rc = r.hkv_sketch_decode_async(ctypes.c_void_p(a.cells.data_ptr()), ctypes.c_void_p(b.cells.data_ptr()), sub,
                                       ctypes.c_void_p(la.data_ptr()) if cap_a else None, cap_a,
                                       ctypes.c_void_p(lb.data_ptr()) if cap_b else None, cap_b,
                                       ctypes.c_void_p(res.data_ptr()), None)
        assert rc == 0, r.hkv_last_error()
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [100, 170, 0, want["passes"], 0, 0, 0, 0]
        assert not a.host().any()
        ha, hb = la.cpu().numpy(), lb.cpu().numpy()
        assert (ha[cap_a * 16:] == CANARY).all() and (hb[cap_b * 16:] == CANARY).all(), "written at or past a cap"
        got_a, got_b = SM.as_set(ha[:cap_a * 16]), SM.as_set(hb[:cap_b * 16])
        assert len(got_a) == cap_a and got_a <= SM.as_set(want["only_a"])
        assert len(got_b) == cap_b and got_b <= SM.as_set(want["only_b"])


def test_refusals():
    from hermes_amd import lib
    r = lib.raw()
    cells = torch.full((2, 3 * 4 * 4 + 2), CANARY64, dtype=torch.int64, device="cuda")
    lists = torch.full((2, 64 + 16), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((10,), -1, dtype=torch.int64, device="cuda")
    summ = dev_bytes(elements(4099)[:4])
    before = summ.cpu().numpy().copy()

    def P(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)

    def refused(rc, name):
        msg = r.hkv_last_error()
        assert rc < 0 and msg and msg.startswith(name + b":"), (rc, msg)

    a, b, la, lb = cells[0], cells[1], lists[0], lists[1]
    fold, dec = r.hkv_summaries_sketch_async, r.hkv_sketch_decode_async
    for args in ((P(summ), 4, None, 4), (None, 4, P(a), 4), (P(summ, 8), 3, P(a), 4), (P(summ), 4, P(a, 8), 4),
                 (P(summ), 4, P(a), 0), (P(summ), 4, P(a), 1 << 32), (P(summ), 4, P(a), (1 << 64) - 1)):
        for accumulate in (0, 1):
            refused(fold(*args, accumulate, None), b"sketch")
    for args in ((None, P(b), 4, P(la), 4, P(lb), 4, P(res)), (P(a), None, 4, P(la), 4, P(lb), 4, P(res)),
                 (P(a), P(b), 4, P(la), 4, P(lb), 4, None), (P(a), P(b), 4, None, 4, P(lb), 4, P(res)),
                 (P(a), P(b), 4, P(la), 4, None, 4, P(res)), (P(a, 8), P(b), 4, P(la), 4, P(lb), 4, P(res)),
                 (P(a), P(b, 8), 4, P(la), 4, P(lb), 4, P(res)), (P(a), P(b), 4, P(la, 8), 4, P(lb), 4, P(res)),
                 (P(a), P(b), 4, P(la), 4, P(lb, 8), 4, P(res)), (P(a), P(b), 4, P(la), 4, P(lb), 4, P(res, 8)),
                 (P(a), P(b), 0, P(la), 4, P(lb), 4, P(res)), (P(a), P(b), 1 << 32, P(la), 4, P(lb), 4, P(res))):
        refused(dec(*args, None), b"sketch_decode")
    torch.cuda.synchronize()
    assert (cells.cpu().numpy() == CANARY64).all() and (lists.cpu().numpy() == CANARY).all(), "a refused call wrote"
    assert (res.cpu().numpy() == -1).all() and np.array_equal(summ.cpu().numpy(), before)


# ------------------------------------------------------------------ 3. sketch_delta_resync, loopback
PART_BITS = 6
GEOM = {False: (4000, 8192, 4096, 1 << 20), True: (1500, 2048, 1024, 1 << 20)}     # keys, source and target buckets, log


def _distinct_partitions(n_keys, count, part_bits, skip=0):
    """the lowest ids whose keys lie in `count` different partitions (after the first `skip` such ids)"""
    part = (gen_keys(n_keys) & np.uint64((1 << part_bits) - 1)).astype(np.int64)
    _, first = np.unique(part, return_index=True)
    return np.sort(first)[skip:skip + count]


def _scripted_pair(big, inline_dst, lacks=3):
    """source: every key, twelve raised to (4, 2) VALID and two more left INVALID, one key a partition; target, in a
    half of the buckets: all but the last `lacks` ids, one key raised to (8, 2) -- newer than the source's --;
    INLINE when asked (37 more keys are then written alike on both tables, the target's while INLINE). With their
    oracle twins. Timestamp versions are even: the oracle reads an odd one as a held seqlock."""
    from hermes_amd import kvs
    n_keys, src_bkts, dst_bkts, cap = GEOM[big]
    src, so, sizes = make_pair(n_keys, src_bkts, cap, big=big)
    dst, do, _ = make_pair(n_keys - lacks, dst_bkts, cap, big=big, machine_id=0 if inline_dst else 1)
    ids = _distinct_partitions(n_keys - lacks, 15, PART_BITS)
    _raise(both(src, so), ids[:12], (4, 2), 9, 0, sizes, n_keys)
    _raise(both(src, so), ids[12:14], (4, 2), 9, 0, sizes, n_keys, vals=False)
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE if inline_dst else 0
    try:
        _raise(both(dst, do), ids[14:15], (8, 2), 13, 0 if inline_dst else 1, sizes, n_keys, vals=False)
    finally:
        kvs.HermesKV.default_flags = 0
    if inline_dst:      # the same 37 writes on both tables, the target's run while INLINE: they convert it
        assert dst.prefer_layout(INLINE)
        _raise(both(src, so), np.arange(200, 237), (2, 2), 5, 0, sizes, n_keys)
        kvs.HermesKV.default_flags = kvs.BATCH_ENGINE     # (the single-workgroup kernel has no inline instance)
        try:
            _raise(both(dst, do), np.arange(200, 237), (2, 2), 5, 0, sizes, n_keys)
        finally:
            kvs.HermesKV.default_flags = 0
    assert dst.layout()["state"] == (INLINE if inline_dst else LOG)
    return src, so, dst, do, sizes


def _model_repair(so, do, sizes, part_bits, mb, sub=None):
    """the sketch-level repair on the oracle twins by its definition: the rows' diff, both tables' summaries of the
    differing partitions, the decode of their sketches, the target's need list of only_a, the source's records of
    it applied to the target's twin. Returns what the device must report."""
    image_s, image_d = CM.oracle_image(so, sizes), CM.oracle_image(do, sizes)
    mask, differing = DM.diff_model(DM.part_rows_model(image_s, part_bits), DM.part_rows_model(image_d, part_bits))
    s_src, s_dst = KM.summaries_model(image_s, part_bits, mask), KM.summaries_model(image_d, part_bits, mask)
    sub = max(32, -(-4 * int(differing) // 3)) if sub is None else sub
    d = SM.decode_model(SM.sketch_model(s_src, sub), SM.sketch_model(s_dst, sub), sub)
    ok = d["undecoded"] == 0
    only_src = np.ascontiguousarray(d["only_a"]).view(np.uint8).reshape(-1, 16).copy().view(KM.SUMMARY).reshape(-1)
    counts, need_keys, _ = KM.need_model(do, only_src if ok else s_src, sizes)
    rec = KM.fetch_model(image_s, need_keys)
    install = RM.install_counts(do, rec, sizes)
    RM.apply_records(do, rec, sizes, mb)
    return {"differing": int(differing), "summaries": len(s_src), "sub_cells": sub, "only_src": len(d["only_a"]),
            "only_dst": len(d["only_b"]), "undecoded": d["undecoded"], "passes": d["passes"], "fallback": not ok,
            "classes": {c: counts[c] for c in KM.CLASSES}, "needed": counts["needed"], "install": install}


@pytest.mark.parametrize("big,inline_dst", [(False, False), (False, True), (True, False)])
def test_sketch_delta_resync_beside_key_delta_resync(big, inline_dst):
    from hermes_amd.replica_group import key_delta_resync, sketch_delta_resync
    src, so, dst, do, sizes = _scripted_pair(big, inline_dst)
    src2, _, dst2, _, _ = _scripted_pair(big, inline_dst)      # the twin pair, for the key-level repair
    src3, _, dst3, _, _ = _scripted_pair(big, inline_dst)      # and for the fallback
    E = sizes.entry
    lay_s, lay_d = src.layout(), dst.layout()
    ref = key_delta_resync(dst2, src2, part_bits=PART_BITS)
    out = sketch_delta_resync(dst, src, part_bits=PART_BITS)
    low = sketch_delta_resync(dst3, src3, part_bits=PART_BITS, sub_cells=1)
    want = _model_repair(so, do, sizes, PART_BITS, L.membership(3, 0 if inline_dst else 1))
    assert not want["fallback"] and want["only_src"] == 18 and want["only_dst"] == 15, want
    for k in ("sub_cells", "only_src", "only_dst", "undecoded", "passes", "fallback", "classes", "needed", "summaries"):
        assert out[k] == want[k], (k, out[k], want[k])
    assert out["classes"] == {"missed": 3, "newer": 14, "validate": 0, "same": 0, "state_only": 0, "older": 1}
    assert out["differing_before"] == want["differing"] == ref["differing_before"] and out["partitions"] == 1 << PART_BITS
    # the same records as the key-level repair: its counts, its need count, and the target byte for byte
    assert {k: out[k] for k in RM.COUNTS} == {k: ref[k] for k in RM.COUNTS} == want["install"]
    assert want["install"] == {"raised": 14, "equal": 0, "older": 0, "missed": 3}
    assert out["needed"] == ref["needed"] == out["records"] == 17 and out["summaries"] == ref["summaries"]
    assert out["differing_after"] == ref["differing_after"] and sorted(out["unresolved"]) == sorted(ref["unresolved"])
    assert 0 < out["differing_after"] <= 4      # the key newer at the target and the three it lacks are reported
    # the bytes: the sketch for the summaries
    assert out["bytes_sketch"] == 96 * out["sub_cells"] < out["bytes_summaries"] == 16 * out["summaries"] == ref["bytes_summaries"]
    assert out["bytes_keys"] == 8 * 17 and out["bytes_records"] == E * 17
    # layout counters do not move (the exports below send an INLINE table to LOG)
    assert src.layout() == lay_s
    now = dst.layout()
    assert now["state"] == lay_d["state"] and now["conversions"] == lay_d["conversions"]
    # the fallback: one cell per subtable cannot decode; the key-level exchange runs and ends in the same tables
    assert low["fallback"] and low["undecoded"] == 3 and low["sub_cells"] == 1 and low["bytes_sketch"] == 96
    assert low["needed"] == 17 and low["classes"] == ref["classes"] and low["classes"]["older"] == 1 and low["bytes_summaries"] == ref["bytes_summaries"]
    assert {k: low[k] for k in RM.COUNTS} == want["install"] and low["differing_after"] == out["differing_after"]
    for name, g in (("key-level", dst2), ("fallback", dst3)):
        assert np.array_equal(dst.census_parts(PART_BITS).host(), g.census_parts(PART_BITS).host()), name
    idx, log = dst.index_bytes(), dst.log_bytes()
    for name, g in (("key-level", dst2), ("fallback", dst3)):
        assert np.array_equal(idx, g.index_bytes()) and np.array_equal(log, g.log_bytes()), f"{name}: the targets differ"
    assert_tables_equal(dst, do, "the target after the sketch-level repair")
    # nothing the repair can still change: the same partitions differ, nothing is needed but the three missed keys
    again = sketch_delta_resync(dst, src, part_bits=PART_BITS)
    assert again["raised"] == 0 and again["needed"] == 3 == again["missed"] and not again["fallback"]
    for g in (src, dst, src2, dst2, src3, dst3):
        assert g.take_error_flags() == 0


def test_sketch_delta_resync_nothing_differs_and_chunks():
    from hermes_amd.replica_group import sketch_delta_resync
    src, so, dst, do, sizes = _scripted_pair(False, False, lacks=0)
    want = _model_repair(so, do, sizes, PART_BITS, L.membership(3, 1))
    out = sketch_delta_resync(dst, src, part_bits=PART_BITS, chunk_buckets=8192 // 3 + 1)      # both tables in chunks
    for k in ("sub_cells", "only_src", "only_dst", "undecoded", "passes", "fallback", "classes", "needed", "summaries"):
        assert out[k] == want[k], (k, out[k], want[k])
    assert out["raised"] == 14 and out["missed"] == 0 and out["differing_after"] == 1      # the key newer at the target
    assert_tables_equal(dst, do, "the target after the repair in chunks")
    src2, _, dst2, _, _ = _scripted_pair(False, False, lacks=0)
    assert sketch_delta_resync(dst2, src2, part_bits=PART_BITS, chunk_buckets=700, sub_cells=1)["fallback"]
    assert np.array_equal(dst.index_bytes(), dst2.index_bytes()) and np.array_equal(dst.log_bytes(), dst2.log_bytes())
    # two tables that agree: nothing is folded, shipped or decoded
    a, _, _ = make_pair(1000, 1024, 1 << 18)
    b, _, _ = make_pair(1000, 2048, 1 << 18, machine_id=1)
    none = sketch_delta_resync(b, a)
    assert none["differing_before"] == 0 and none["summaries"] == none["needed"] == none["only_src"] == 0
    assert none["sub_cells"] == 32 and not none["fallback"] and none["passes"] == 0 and none["differing_after"] == 0
    for g in (src, dst, src2, dst2, a, b):
        assert g.take_error_flags() == 0


def test_sketch_delta_resync_insert():
    """insert=True into a target that lacks forty keys, beside the key-level repair of a twin; and into an empty
    target, once with a sketch sized for it and once with the default, which falls back"""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import key_delta_resync, sketch_delta_resync
    n_keys, bkts, cap = 4000, 8192, 1 << 20
    fields = ("digest_sum", "digest_xor", "keys", "by_state")
    src, so, sizes = make_pair(n_keys, bkts, cap)
    _raise(both(src, so), np.arange(100, 130), (4, 2), 6, 0, n_keys=n_keys)
    want = src.census().host()
    dst, _, _ = make_pair(n_keys - 40, bkts // 2, cap, machine_id=1)
    dst2, _, _ = make_pair(n_keys - 40, bkts // 2, cap, machine_id=1)
    ref = key_delta_resync(dst2, src, part_bits=8, insert=True)
    out = sketch_delta_resync(dst, src, part_bits=8, insert=True)
    assert not out["fallback"] and out["undecoded"] == 0 and out["only_src"] == 70 and out["only_dst"] == 30
    assert out["inserted"] == ref["inserted"] == 40 and out["raised"] == ref["raised"] == 30 and out["missed"] == 0
    assert out["needed"] == ref["needed"] == 70 and out["replaced"] + out["evictions"] == 0
    assert out["bytes_sketch"] < out["bytes_summaries"] == ref["bytes_summaries"]
    assert out["differing_after"] == 0 and out["unresolved"] == []
    for g in (dst, dst2):
        got = g.census().host()
        assert all(got[f] == want[f] for f in fields)
    for sub, fallback in ((2 * n_keys // 3 + 1, False), (None, True)):
        empty = HermesKV(n_keys, bkts // 2, cap, machine_id=1, populate=False)
        out = sketch_delta_resync(empty, src, part_bits=8, chunk_buckets=bkts // 3 + 1, insert=True, sub_cells=sub)
        assert out["fallback"] == fallback and out["inserted"] == out["needed"] == out["summaries"] == want["keys"]
        assert (out["only_src"] == want["keys"] and out["only_dst"] == 0) or fallback
        got = empty.census().host()
        assert all(got[f] == want[f] for f in fields) and out["differing_after"] == 0
        assert empty.take_error_flags() == 0
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0 and dst2.take_error_flags() == 0


# ------------------------------------------------------------------ 4. group_sketch_delta_resync over gloo
G_KEYS, G_BITS = 4000, 8
G_FIRST = _distinct_partitions(G_KEYS, 40, G_BITS)               # what the stale rank missed, one key a partition
G_SECOND = _distinct_partitions(G_KEYS, 30, G_BITS, skip=60)     # ... and what it missed after the first repair


def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import group_census, group_sketch_delta_resync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        g = HermesKV(G_KEYS, (8192, 4096)[rank], 1 << 20, machine_id=rank)     # the stale rank has another geometry
        keys = gen_keys(G_KEYS)
        mb = L.membership(3, 0)

        def write(ids, ts):
            if rank == 0:
                g.batch_host(L.BatchType.invs, RC.invs(keys, ids, 2, ts, L.DEFAULT, 6), mb)
                g.batch_host(L.BatchType.vals, RC.vals(keys, ids, 2, ts), mb)

        write(G_FIRST, (4, 2))
        before = group_census(g, None)
        low = group_sketch_delta_resync(g, None, 0, [1], G_BITS, chunk_buckets=8192 // 3 + 1, sub_cells=1)
        mid = group_census(g, None)
        write(G_SECOND, (6, 2))
        res = group_sketch_delta_resync(g, None, 0, [1], G_BITS, chunk_buckets=8192 // 3 + 1)
        after = group_census(g, None)
        again = group_sketch_delta_resync(g, None, 0, [1], None, None)
        q.put((rank, before, low, mid, res, after, again, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, None, None, None, None, 0, repr(e)))


def test_group_sketch_delta_resync_over_gloo():
    """two ranks as fresh child processes sharing the GPU over gloo: rank 1 missed forty writes that rank 0 applied;
    with one cell per subtable both ranks fall back to the key-level exchange; after thirty more writes the source
    ships its sketch, rank 1 decodes it against its own and asks for those thirty records; the group census agrees
    after each"""
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
    n1, n2 = (int(np.isin(part, part[ids]).sum()) for ids in (G_FIRST, G_SECOND))
    for rank, before, low, mid, out, after, again, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert not before["live_ranks_agree"] and mid["live_ranks_agree"] and after["live_ranks_agree"]
        assert after["not_valid"] == [0, 0], after
        # the fallback, decided for every rank alike
        assert low["fallback"] and low["sub_cells"] == 1 and low["bytes_sketch"] == 96 and low["selected"] == 40
        assert low["summaries"] == n1 and low["records"] == 40 and low["bytes_summaries"] == 16 * n1
        assert low["differing_after"] == 0 and low["unresolved"] == []
        # the sketch-level exchange
        assert not out["fallback"] and out["selected"] == 30 and out["sub_cells"] == 40 and out["bytes_sketch"] == 96 * 40
        assert out["summaries"] == out["scanned_keys"] == n2 and out["records"] == 30
        assert out["bytes_sketch"] < out["bytes_summaries"] == 16 * n2 and out["bytes_records"] == 64 * 30
        assert out["differing_after"] == 0 and out["unresolved"] == []
        assert again["selected"] == 0 and again["summaries"] == 0 and again["records"] == 0 and not again["fallback"]
        if rank == 1:
            assert low["undecoded"] == 3 and low["needed"] == 40 and low["classes"]["newer"] == 40
            assert {k: low[k] for k in RM.COUNTS} == {"raised": 40, "equal": 0, "older": 0, "missed": 0}
            assert out["differing_before"] == 30 and out["needed"] == 30 and out["undecoded"] == 0 and out["passes"] > 0
            assert out["only_src"] == 30 and out["only_dst"] == 30
            assert out["classes"] == {"missed": 0, "newer": 30, "validate": 0, "same": 0, "state_only": 0, "older": 0}
            assert {k: out[k] for k in RM.COUNTS} == {"raised": 30, "equal": 0, "older": 0, "missed": 0}
        else:
            assert all(out[k] == 0 for k in RM.COUNTS) and out["needed"] == 0 and not any(out["classes"].values())
            assert out["only_src"] == out["only_dst"] == out["undecoded"] == 0
    assert res[0][1] == res[1][1] and res[0][5] == res[1][5]
