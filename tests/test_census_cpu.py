"""The census definition (include/hermeskv.h, "Table census and digest") on the oracle and the numpy model alone:
what the digest must and must not depend on, the wrapped geometry's live / dead slots, that the scripted scenario
the GPU tests walk through is not vacuous, and the size of the ctypes binding. No GPU."""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import census_model as CM

CONFIGS = [dict(rmw=False, big=False), dict(rmw=True, big=False), dict(rmw=True, big=True)]


def image(o, sizes=L.DEFAULT):
    return CM.oracle_image(o, sizes)


def populated(n, bkts, cap, big=False, rmw=False, runs=None, ecl=None):
    """ecl: big objects of that many extra cache lines (default: 4 with big, the default geometry without)"""
    ecl = (4 if big else 0) if ecl is None else ecl
    sizes = L.Sizes(True, ecl) if ecl else L.DEFAULT
    o = OracleKVS(bkts, cap, 0, rmw, ecl > 0, ecl)
    for k in runs or (n,):
        o.populate(k, sizes.kvs_value)
    return o, sizes


def test_digest_is_keyed_by_key_not_by_position():
    """The same 1000 keys in 1024 and in 4096 buckets (the same log order, another bucket order), and in a table
    populated twice (600 keys, then all 1000: ids 0..599 get new entries behind the first run's, so the log order
    differs and 600 old entries lie unreferenced): one digest, one census."""
    n = 1000
    a, _ = populated(n, 1024, 1 << 17)
    b, _ = populated(n, 4096, 1 << 17)
    c, _ = populated(n, 4096, 1 << 18, runs=(600, n))
    ca, cb, cc = (CM.census_model(*image(o)) for o in (a, b, c))
    assert ca["keys"] == n and ca["by_state"][int(L.State.VALID)] == n and ca["offenders"] == 0
    assert not np.array_equal(a.index_bytes(), b.index_bytes()[:len(a.index_bytes())])
    assert not np.array_equal(b.log_bytes()[:n * 64], c.log_bytes()[:n * 64])
    assert ca == cb == cc
    assert ca["digest_sum"] and ca["digest_xor"]


def _one_key(o, sizes, i=123):
    key = int(gen_keys(i + 1)[i])
    off = o.lookup(key)
    assert off is not None
    return off


# the five big-object sizes of tests/test_value_sizes_gpu.py, each in a log that wraps (capacity below n * entry)
SIZED_WRAPPED = [pytest.param(600, 1024, 1 << 16, False, 1, id="ecl1"), pytest.param(600, 1024, 1 << 16, False, 2, id="ecl2"),
                 pytest.param(600, 1024, 1 << 17, False, 5, id="ecl5"), pytest.param(600, 1024, 1 << 18, False, 8, id="ecl8"),
                 pytest.param(600, 1024, 1 << 19, False, 16, id="ecl16")]


@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big,ecl", [
    pytest.param(500, 1024, 1 << 18, False, None, id="False"), pytest.param(500, 1024, 1 << 18, True, None, id="True"),
    *SIZED_WRAPPED])
def test_digest_sensitivity_and_insensitivity(n_keys, num_bkts, log_cap, big, ecl):
    o, sizes = populated(n_keys, num_bkts, log_cap, big=big, rmw=big, ecl=ecl)
    idx, log, head, cap, _ = image(o, sizes)
    base = CM.census_model(idx, log, head, cap, sizes)
    assert (ecl is None) == (head <= cap)                # (a wrapped log still holds the lowest ids)
    off = _one_key(o, sizes)
    dt = L.entry_dtype(sizes)

    def flipped(byte, bit=0x04):
        l2 = log.copy()
        l2[off + byte] ^= bit
        return CM.census_model(idx, l2, head, cap, sizes)

    # replicated bytes: every one of them moves both digest words
    sens = {"state": 18, "ts_cid": 23, "ts_ver byte 0": 24, "ts_ver byte 3": 27, "value first": 33,
            "value last": 33 + sizes.st_value - 1, "key": 9}
    assert sens["value last"] == sizes.entry - 1
    for what, byte in sens.items():
        c = flipped(byte)
        assert c["digest_sum"] != base["digest_sum"] and c["digest_xor"] != base["digest_xor"], what
    # replica-local bytes: none of them moves the digest
    local = {"key_first": 3, "opcode": 16, "val_len": 17, "ack_bv": 19, "rmw_lwid": 20, "obi": 21, "lock": 22,
             "llw_cid": 28, "llw_ver byte 0": 29, "llw_ver byte 3": 32}
    for name in ("opcode", "val_len", "ack_bv", "rmw_lwid", "obi", "lock", "llw_cid"):
        assert dt.fields[name][1] == local[name]
    assert dt.fields["llw_ver"][1] == 29
    for what, byte in local.items():
        assert CM.digest(flipped(byte)) == CM.digest(base), what
    assert flipped(21)["obi_set"] == base["obi_set"] + 1          # (the counts do see obi)
    # two keys swapping their values is seen too (the sum is over keys, each hashed with its key)
    off2 = _one_key(o, sizes, 124)
    l2 = log.copy()
    assert log[off + 33] != log[off2 + 33]
    l2[off + 33], l2[off2 + 33] = log[off2 + 33], log[off + 33]
    assert CM.digest(CM.census_model(idx, l2, head, cap, sizes)) != CM.digest(base)


@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big,ecl", [
    pytest.param(3000, 4096, 1 << 17, False, None, id="3000-4096-131072-False"),
    pytest.param(2000, 1024, 1 << 18, True, None, id="2000-1024-262144-True"), *SIZED_WRAPPED])
def test_wrapped_geometry_live_and_dead_slots(n_keys, num_bkts, log_cap, big, ecl):
    """test_populate_bit_exact's wrapping geometries, and one per big-object size: the log has overwritten the
    oldest entries, their slots are still in use; the census counts exactly the ids the lookup finds"""
    o, sizes = populated(n_keys, num_bkts, log_cap, big=big, rmw=big, ecl=ecl)
    assert log_cap < n_keys * sizes.entry
    c = CM.census_model(*image(o, sizes))
    found = sum(o.lookup(int(k)) is not None for k in gen_keys(n_keys))
    assert c["dead_slots"] > 0
    assert 0 < c["keys"] == found < n_keys
    assert c["by_state"][int(L.State.VALID)] == c["keys"]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_scripted_states_are_not_vacuous(cfg):
    """tests/scripted.py on the oracle alone, a census after every launch: the sequence the GPU test compares
    launch by launch shows three states or more, two writers of keys that are not VALID, and op buffer indices"""
    from tests.scripted import run_scripted
    rmw, big = cfg["rmw"], cfg["big"]
    o, sizes = populated(1000, 4096, 1 << 22, big=big, rmw=rmw)
    seen = []

    def runner(btype, elems, mb, rw=None, node_suspected=None):
        o.batch_multi(btype, elems, 1, len(elems), None, mb, rw=rw, node_suspected=node_suspected)
        seen.append(CM.census_model(*image(o, sizes)))

    run_scripted(runner, gen_keys(1000), sizes, rmw)
    assert len(seen) == 8
    CM.assert_not_vacuous(seen)
    assert all(c["keys"] == 1000 for c in seen)
    assert len({CM.digest(c) for c in seen}) >= 5


def test_binding_size():
    """ctypes' hkv_census is the library's (loads libhermeskv.so, as test_capi does)"""
    from tests.test_capi import _ensure_built
    _ensure_built()
    from hermes_amd import lib
    from hermes_amd.kvs import CENSUS_FIELDS, CENSUS_WORDS
    assert ctypes.sizeof(lib.HkvCensus) == lib.raw().hkv_census_bytes() == 8 * CENSUS_WORDS
    assert tuple(CENSUS_FIELDS) == CM.FIELDS
    assert CENSUS_FIELDS["by_state"] == (2, 8) and CENSUS_FIELDS["not_valid_by_cid"] == (11, 9)
    assert CENSUS_FIELDS["offenders"] == (24, 1)
