"""The invertible sketch on the model alone (include/hermeskv.h, "Sketch-level delta repair"; tests/sketch_model.py):
the ABI of the two calls against the built library (no GPU needed: the refusals come before any device work), the
sketch as a function of the multiset, the decode of random differences at 2.0 cells per element, inputs that cannot
decode, and, on the oracle tables of tests/test_keydelta_cpu.py, that the summaries a decode returns make the target
need exactly the keys that all of the source's summaries make it need.
"""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from tests import census_model as CM
from tests import delta_model as DM
from tests import keydelta_model as KM
from tests import sketch_model as SM

S = L.DEFAULT
# Seeds at which the model decodes every case below. Of seeds 1..40, seed 3 at n = 100 leaves a 2-core of six
# elements (nine cells): at 2.0 cells per element a small difference fails now and then, which is what a repair's
# fallback is for. That case is kept as its own test.
SEEDS = (1, 2, 4, 5, 6)


_elements = SM.random_elements


def _sub_cells(n):
    return max(32, -(-2 * n // 3))   # 3 S >= ceil(2.0 n), floor 32


# ------------------------------------------------------------------ ABI (fails on a library without the two calls)
def test_abi_of_the_sketch_calls():
    from hermes_amd import lib
    r = lib.raw()
    assert r.hkv_abi_version() == 10 == lib.ABI_VERSION
    assert r.hkv_sketch_cell_bytes() == 32
    assert r.hkv_sketch_result_bytes() == 64
    buf = (ctypes.c_uint8 * 512)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 256), ctypes.c_void_p(base + 8)
    refusals = (
        ("sketch", lambda: r.hkv_summaries_sketch_async(p, 1, None, 1, 0, None)),           # NULL cells
        ("sketch", lambda: r.hkv_summaries_sketch_async(None, 1, p, 1, 0, None)),           # a count, no buffer
        ("sketch", lambda: r.hkv_summaries_sketch_async(odd, 1, p, 1, 0, None)),            # alignment
        ("sketch", lambda: r.hkv_summaries_sketch_async(p, 1, odd, 1, 0, None)),
        ("sketch", lambda: r.hkv_summaries_sketch_async(p, 1, q, 0, 0, None)),              # S == 0
        ("sketch", lambda: r.hkv_summaries_sketch_async(p, 1, q, 1 << 32, 0, None)),        # S >= 2^32
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(None, q, 1, None, 0, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, None, 1, None, 0, None, 0, q, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, None, 0, None, 0, None, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, None, 1, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, None, 0, None, 1, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(odd, q, 1, None, 0, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, odd, 1, None, 0, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, odd, 1, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, None, 0, odd, 1, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1, None, 0, None, 0, odd, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 0, None, 0, None, 0, p, None)),
        ("sketch_decode", lambda: r.hkv_sketch_decode_async(p, q, 1 << 32, None, 0, None, 0, p, None)),
    )
    for name, call in refusals:
        rc = call()
        msg = r.hkv_last_error()
        assert rc < 0 and msg and msg.startswith(name.encode() + b":"), (name, rc, msg)
    assert not any(buf)


def test_python_bindings_exist():
    from hermes_amd import kvs, replica_group
    assert callable(kvs.sketch) and callable(kvs.sketch_decode)
    assert callable(replica_group.sketch_delta_resync) and callable(replica_group.group_sketch_delta_resync)
    assert kvs.SKETCH_MAX_PASSES == SM.MAX_PASSES == 192 and kvs.SKETCH_CELL_BYTES == 32
    with open(__file__.rsplit("/tests/", 1)[0] + "/include/hermeskv.h") as f:
        assert "#define HKV_SKETCH_MAX_PASSES 192\n" in f.read()


# ------------------------------------------------------------------ the sketch is a function of the multiset
def test_shuffled_list_gives_equal_cells():
    rng = np.random.default_rng(7)
    e = _elements(rng, 500)
    for sub in (1, 7, 32, 333):
        a = SM.sketch_model(e, sub)
        assert np.array_equal(a, SM.sketch_model(e[rng.permutation(len(e))], sub))
        assert int(a[:, 0].sum()) == 3 * len(e)
        for j in range(3):   # every element once per subtable
            assert int(a[j * sub:(j + 1) * sub, 0].sum()) == len(e)


def test_accumulate_equals_concatenation():
    rng = np.random.default_rng(8)
    e = _elements(rng, 300)
    whole = SM.sketch_model(e, 50)
    parts = SM.sketch_model(e[:120], 50)
    assert SM.sketch_model(e[120:], 50, cells=parts) is parts
    assert np.array_equal(whole, parts)
    # a duplicated element counts twice and cancels in the xor words
    twice = SM.sketch_model(np.concatenate([e[:1], e[:1]]), 5)
    assert sorted(twice[:, 0].tolist())[-3:] == [2, 2, 2] and not twice[:, 1:].any()


def test_slots_depend_on_the_version():
    """two versions of one key fall into unrelated cells: over many keys the slots agree about once in S"""
    rng = np.random.default_rng(9)
    e = _elements(rng, 2000)
    f = e.copy()
    f["ts_ver"] += 1
    wa, wb = SM.words(e), SM.words(f)
    same = SM.slot(SM.check(wa[:, 0], wa[:, 1]), 0, 1000) == SM.slot(SM.check(wb[:, 0], wb[:, 1]), 0, 1000)
    assert same.sum() < 20


# ------------------------------------------------------------------ the decode
@pytest.mark.parametrize("n", [1, 10, 100, 1000])
def test_random_differences_decode_at_two_cells_per_element(n):
    sub = _sub_cells(n)
    for seed in SEEDS:
        list_a, list_b, only_a, only_b = SM.difference_case(n, seed)
        A, B = SM.sketch_model(list_a, sub), SM.sketch_model(list_b, sub)
        d = SM.decode_model(A, B, sub)
        assert d["undecoded"] == 0 and not d["cells"].any(), (n, seed, d["undecoded"])
        assert d["exhausted"] == 0 and d["passes"] <= SM.MAX_PASSES // 4, (n, seed, d["passes"])
        assert SM.as_set(d["only_a"]) == SM.as_set(only_a) and len(d["only_a"]) == len(only_a)
        assert SM.as_set(d["only_b"]) == SM.as_set(only_b) and len(d["only_b"]) == len(only_b)


def test_a_small_two_core_at_two_cells_per_element():
    """n = 100, seed 3: six elements share nine cells so that none is pure; the other 94 are returned"""
    list_a, list_b, only_a, only_b = SM.difference_case(100, 3)
    sub = _sub_cells(100)
    d = SM.decode_model(SM.sketch_model(list_a, sub), SM.sketch_model(list_b, sub), sub)
    assert d["undecoded"] == 9 and d["exhausted"] == 0 and len(d["only_a"]) + len(d["only_b"]) == 94
    assert SM.as_set(d["only_a"]) <= SM.as_set(only_a) and SM.as_set(d["only_b"]) <= SM.as_set(only_b)


def test_identical_lists_decode_to_nothing():
    e = _elements(np.random.default_rng(3), 100)
    A = SM.sketch_model(e, 40)
    d = SM.decode_model(A, A.copy(), 40)
    assert d["passes"] == 0 and d["undecoded"] == 0 and d["exhausted"] == 0
    assert len(d["only_a"]) == 0 and len(d["only_b"]) == 0 and not d["cells"].any()


def test_undecodable_inputs_leave_a_two_core():
    e = _elements(np.random.default_rng(4), 3)
    zero = np.zeros((3, 4), np.uint64)
    # S = 1, two elements on one side: every cell holds both, none is pure
    d = SM.decode_model(SM.sketch_model(e[:2], 1), zero, 1)
    assert d["undecoded"] == 3 and d["passes"] == 0 and len(d["only_a"]) == 0 and len(d["only_b"]) == 0
    assert d["cells"][:, 0].tolist() == [2, 2, 2]
    # S = 1 with +1, +1, -1: the counts say 1, the xor of three elements passes no check
    d = SM.decode_model(SM.sketch_model(e[:2], 1), SM.sketch_model(e[2:], 1), 1)
    assert d["undecoded"] == 3 and d["passes"] == 0 and d["cells"][:, 0].tolist() == [1, 1, 1]
    assert len(d["only_a"]) == 0 and len(d["only_b"]) == 0


def test_partial_decode_and_the_pass_cap():
    """far too few cells: some elements peel, a 2-core stays; and a cap below the passes needed reports exhausted"""
    rng = np.random.default_rng(11)
    e = _elements(rng, 60)
    sub = 16
    A = SM.sketch_model(e, sub)
    d = SM.decode_model(A, np.zeros_like(A), sub)
    assert d["undecoded"] > 0 and 0 < len(d["only_a"]) < 60 and d["exhausted"] == 0
    assert SM.as_set(d["only_a"]) <= SM.as_set(e)
    rest = [x for x in SM.words(e).tolist() if tuple(x) not in SM.as_set(d["only_a"])]
    assert np.array_equal(d["cells"], SM.sketch_model(np.array(rest, np.uint64), sub))   # the remainder is their sketch
    e = _elements(rng, 1000)
    A = SM.sketch_model(e, 434)   # 1.3 cells per element: many passes
    full = SM.decode_model(A, np.zeros_like(A), 434)
    assert full["undecoded"] == 0 and 12 < full["passes"] <= SM.MAX_PASSES - 3 and full["exhausted"] == 0
    cut = SM.decode_model(A, np.zeros_like(A), 434, max_passes=full["passes"] - 1)
    assert cut["exhausted"] == 1 and cut["undecoded"] > 0 and cut["passes"] == full["passes"] - 1


# ------------------------------------------------------------------ on the oracle's tables
def test_decoded_summaries_need_the_keys_all_summaries_need():
    from tests.test_keydelta_cpu import N_KEYS, _Done, _table
    from oracle.oracle import gen_keys
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
    dst = _table(16384, 1 << 20)   # the same ids, freshly populated: it differs in the keys the launches wrote
    image_src, image_dst = CM.oracle_image(src, S), CM.oracle_image(dst, S)
    part_bits = 10
    mask, count = DM.diff_model(DM.part_rows_model(image_src, part_bits), DM.part_rows_model(image_dst, part_bits))
    assert 0 < count
    s_src = KM.summaries_model(image_src, part_bits, mask)
    s_dst = KM.summaries_model(image_dst, part_bits, mask)   # the same mask on both
    differing = len(SM.as_set(s_src) ^ SM.as_set(s_dst))
    assert 0 < differing < len(s_src)
    sub = _sub_cells(differing)
    d = SM.decode_model(SM.sketch_model(s_src, sub), SM.sketch_model(s_dst, sub), sub)
    assert d["undecoded"] == 0, (d["undecoded"], differing, sub)
    assert SM.as_set(d["only_a"]) == SM.as_set(s_src) - SM.as_set(s_dst)
    assert SM.as_set(d["only_b"]) == SM.as_set(s_dst) - SM.as_set(s_src)
    only_src = np.ascontiguousarray(d["only_a"]).view(np.uint8).reshape(-1, 16).copy().view(KM.SUMMARY).reshape(-1)
    c_all, keys_all, _ = KM.need_model(dst, s_src, S)
    c_dec, keys_dec, _ = KM.need_model(dst, only_src, S)
    assert c_all["needed"] > 0 and np.array_equal(keys_all, keys_dec)
