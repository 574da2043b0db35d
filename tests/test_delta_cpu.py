"""The partitioned census and the delta repair on the oracle alone (include/hermeskv.h, "Partitioned census and
delta repair"): the rows of tests/delta_model.py fold to the census at every part_bits, do not depend on the bucket
count or the log order, and differ exactly in the partitions of the keys that were written; the masked extract of
those partitions, installed by the repair's definition, makes the rows equal. Then the ABI of the three calls (no
GPU needed: the refusals come before any device work).
"""
import ctypes

import numpy as np
import pytest

from hermes_amd import layout as L
from oracle.oracle import OracleKVS, gen_keys
from tests import census_model as CM
from tests import delta_model as DM
from tests import repair_cases as RC
from tests import repair_model as RM

S = L.DEFAULT
N_KEYS = 5000


def _table(bkts, cap, runs=(N_KEYS,), machine_id=0):
    o = OracleKVS(bkts, cap, machine_id)
    for k in runs:
        o.populate(k, S.kvs_value)
    return o


def _raise(o, ids, ts=(4, 1), salt=9, machine_id=0):
    """INV + VAL launches from machine ts[1] that move the keys `ids` to timestamp ts, VALID"""
    keys = gen_keys(N_KEYS)
    mb = L.membership(3, machine_id)
    for lo in range(0, len(ids), RC.BATCH):
        part = np.asarray(ids[lo:lo + RC.BATCH])
        o.batch(L.BatchType.invs, RC.invs(keys, part, ts[1], ts, S, salt), mb)
        o.batch(L.BatchType.vals, RC.vals(keys, part, ts[1], ts), mb)


@pytest.fixture(scope="module")
def scripted():
    """5000 keys in 16384 buckets after tests/repair_cases.source_script: keys that are not VALID"""
    o = _table(16384, 1 << 20)
    RC.source_script(lambda bt, e, mb: o.batch_multi(bt, e, 1, len(e), None, mb), gen_keys(N_KEYS), S)
    image = CM.oracle_image(o, S)
    census = CM.census_model(*image)
    assert census["offenders"] > 0 and census["keys"] == N_KEYS
    return image, census


@pytest.mark.parametrize("part_bits", [0, 3, 10, 14])
def test_rows_fold_to_the_census(scripted, part_bits):
    image, census = scripted
    assert part_bits <= 14 == (DM.num_buckets(image)).bit_length() - 1
    rows = DM.part_rows_model(image, part_bits)
    assert rows.shape == (1 << part_bits, 4)
    assert DM.fold(rows) == DM.census_fold(census)
    if part_bits == 0:
        assert rows[0].tolist() == [census[k] for k in ("digest_sum", "digest_xor", "keys", "offenders")]
    else:
        assert (rows[:, 3] > 0).sum() >= 2, "not_valid in two partitions or more"
    if part_bits == 14:   # one bucket per partition: a row's keys are its bucket's live slots
        _, bkt, _, _ = CM.live_entries(*image)
        assert np.array_equal(rows[:, 2], np.bincount(bkt, minlength=16384).astype(np.uint64))


def test_rows_do_not_depend_on_geometry():
    """the same keys in 16384 buckets and, populated in two runs (another log order, 3000 unreferenced entries), in
    4096: identical rows at every part_bits both tables admit"""
    a = _table(16384, 1 << 20)
    b = _table(4096, 1 << 20, runs=(3000, N_KEYS))
    for o in (a, b):
        _raise(o, np.arange(100, 400))
    ia, ib = CM.oracle_image(a, S), CM.oracle_image(b, S)
    assert CM.census_model(*ia)["keys"] == CM.census_model(*ib)["keys"] == N_KEYS
    assert not np.array_equal(ia[1][:N_KEYS * 64], ib[1][:N_KEYS * 64])
    for part_bits in (0, 5, 12):
        ra, rb = DM.part_rows_model(ia, part_bits), DM.part_rows_model(ib, part_bits)
        assert np.array_equal(ra, rb), part_bits
        assert ra[:, 2].sum() == N_KEYS
    with pytest.raises(AssertionError):
        DM.part_rows_model(ib, 13)       # more partitions than the table has buckets


def test_differing_partitions_are_the_written_keys():
    """37 keys raised on one of two equal tables: the rows differ exactly in {key & (P - 1)}; the model's masked
    extract of those partitions, applied by the repair's definition, makes all rows equal"""
    part_bits, P = 10, 1024
    src = _table(16384, 1 << 20)
    dst = _table(4096, 1 << 19, machine_id=1)
    ids = np.random.default_rng(11).permutation(N_KEYS)[:37]
    _raise(src, ids)
    isrc, idst = CM.oracle_image(src, S), CM.oracle_image(dst, S)
    rs, rd = DM.part_rows_model(isrc, part_bits), DM.part_rows_model(idst, part_bits)
    mask, count = DM.diff_model(rs, rd)
    want = np.unique(gen_keys(N_KEYS)[ids] & np.uint64(P - 1)).astype(np.int64)
    assert np.array_equal(np.nonzero(mask)[0], want) and count == len(want)
    rec = DM.extract_parts_model(isrc, part_bits, mask)
    assert len(rec) == int(rs[mask != 0, 2].sum()) == DM.scanned_parts_model(isrc, part_bits, mask)
    assert 37 <= len(rec) and len(rec) * 10 <= N_KEYS, len(rec)      # a tenth of a full repair's records at most
    have = {r.tobytes() for r in RM.extract_model(isrc)}
    assert all(r.tobytes() in have for r in rec)
    counts = RM.install_counts(dst, rec)
    assert counts == {"raised": 37, "equal": len(rec) - 37, "older": 0, "missed": 0}
    RM.apply_records(dst, rec, S, L.membership(3, 1))
    after = DM.part_rows_model(CM.oracle_image(dst, S), part_bits)
    assert np.array_equal(after, rs)
    left, n_left = DM.diff_model(rs, after)
    assert n_left == 0 and not left.any()
    # a bucket sub-range and min_ts filter the same records further
    sub = DM.extract_parts_model(isrc, part_bits, mask, 1000, 9000)
    assert 0 < len(sub) < len(rec)
    assert len(DM.extract_parts_model(isrc, part_bits, mask, min_ts=(4 << 8) | 1)) == 37
    # accumulate: a second peer's differences are or-ed in
    both, n = DM.diff_model(rs, rs, mask=mask.copy())
    assert np.array_equal(both, mask) and n == count


# ------------------------------------------------------------------ ABI (fails on a library without the three calls)
def test_abi_of_the_partition_calls():
    from hermes_amd import lib
    from hermes_amd.lib import HkvPartRow
    r = lib.raw()
    assert r.hkv_abi_version() == 10 == lib.ABI_VERSION
    assert r.hkv_part_row_bytes() == ctypes.sizeof(HkvPartRow) == 32
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    seen = []
    for name, call in (("census_parts", lambda: r.hkv_table_census_parts_async(None, 0, p, None)),
                       ("extract_parts", lambda: r.hkv_table_extract_parts_async(None, 0, p, 0, 0, 0, p, 1, p, None)),
                       ("part_rows_diff", lambda: r.hkv_part_rows_diff_async(None, p, 0, p, p, 0, None))):
        rc = call()
        msg = r.hkv_last_error()
        assert rc < 0 and msg and name.encode() in msg, (name, rc, msg)
        seen.append(msg)
    assert len(set(seen)) == 3
    assert not any(buf)
