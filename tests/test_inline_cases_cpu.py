"""The inputs of tests/test_inline_parity_gpu.py are not vacuous: every case of tests/inline_cases.py on the oracle
alone. The geometries hold what the cases draw from (full buckets, evicted keys, a fair share of inline keys), and
every case produces the outcome codes it promises both on inline keys and on the others -- so a kernel that reads
an inline key's entry from the wrong place has results to get wrong. The promised sets are what the oracle gives
with the committed seeds."""
import numpy as np
import pytest

from hermes_amd import layout as L
from tests import inline_cases as C

R, B = L.Resp, L.Bucket
GET_COMPLETE, PUT_SUCCESS, GET_STALL, PUT_STALL, MISS = (int(R.GET_COMPLETE), int(R.PUT_SUCCESS), int(R.GET_STALL),
                                                         int(R.PUT_STALL), int(R.MISS))
INV_SUCCESS, OUT_OF_GROUP, INV_ABORT = int(R.INV_SUCCESS), L.INV_OUT_OF_GROUP, int(R.OP_INV_ABORT)
ACK_SUCCESS, LAST_ACK = int(R.ACK_SUCCESS), int(R.LAST_ACK_SUCCESS)
PUT_COMPLETE, RMW_COMPLETE = int(R.PUT_COMPLETE), int(R.RMW_COMPLETE)

LOCAL = {GET_COMPLETE, PUT_SUCCESS, GET_STALL, PUT_STALL}     # and MISS, on keys that are no inline keys
LOCAL_RMW = LOCAL | {int(R.RMW_SUCCESS), int(R.RMW_STALL), int(R.RMW_ABORT)}
INV = {INV_SUCCESS, OUT_OF_GROUP}                             # OUT_OF_GROUP: an equal timestamp, nothing raised
ACK = {ACK_SUCCESS, LAST_ACK}
VAL = {0, C.MOVED_TO_VALID}


def promised(rec, kind, want, absent=None):
    for inline in (True, False):
        missing = want - rec.codes(kind, inline)
        assert not missing, f"{kind} on {'inline' if inline else 'other'} keys: not produced {sorted(missing)}"
    assert not rec.codes(kind, True) & {MISS}, "an inline key is present"
    if absent is not None:
        assert (MISS in rec.codes(kind, False)) == absent, f"{kind}: MISS on absent keys"


@pytest.mark.parametrize("name,present,absent,inline,full,partly", [
    ("A", 2864, 136, 511, 123, 388), ("D", 15358, 4642, 2048, 1574, 474), ("S", 1000, 0, 656, 0, 656)])
def test_census(name, present, absent, inline, full, partly):
    o = C.make_oracle(name)
    T = C.describe(o, name)
    n_full = int((T.n_used == 8).sum())
    got = (int(T.present.sum()), int((~T.present).sum()), len(T.inline_keys), n_full,
           int(((T.n_used > 0) & (T.n_used < 8)).sum()))
    print(name, got)
    # the floors the cases need ...
    if name in "AD":
        assert n_full >= 100 and got[1] >= 100
    else:
        assert got[1] == 0 and o.evictions() == 0
    assert 0.10 <= len(T.inline_keys) / got[0] <= 0.70
    # ... and the image itself (populate is deterministic)
    assert got == (present, absent, inline, full, partly)
    # every inline key is found, is its bucket's lowest in-use slot's key, and in a full bucket that is slot 0
    assert all(o.lookup(int(k)) is not None for k in T.inline_keys)
    assert np.array_equal(T.bucket(T.inline_keys), T.inline_buckets)
    assert (T.first[T.n_used == 8] == 0).all() and (T.first[T.inline_buckets] == 8 - T.n_used[T.inline_buckets]).all()


@pytest.mark.parametrize("skew", [0, 3])
def test_rounds_case(skew):
    o = C.make_oracle("A", skew=skew)
    T = C.describe(o, "A")
    rec = C.Rec(T.inline_keys)
    C.case_rounds(C.OracleEngine(o), T, rec, skew=skew)
    promised(rec, "local", LOCAL | ({PUT_COMPLETE} if skew else set()), absent=True)
    promised(rec, "inv", INV, absent=True)
    promised(rec, "ack", ACK)
    promised(rec, "rw", {PUT_COMPLETE})
    promised(rec, "val", VAL)


def test_rmw_rounds_case():
    o = C.make_oracle("A", rmw=True)
    T = C.describe(o, "A")
    rec = C.Rec(T.inline_keys)
    C.case_rounds(C.OracleEngine(o), T, rec, rmw=True, rounds=4, big=(1,), check_after=(0, 1, 2, 3), memb_from=2)
    promised(rec, "local", LOCAL_RMW, absent=True)
    promised(rec, "inv", INV | {INV_ABORT}, absent=True)
    promised(rec, "ack", ACK)
    promised(rec, "rw", {PUT_COMPLETE, RMW_COMPLETE})
    promised(rec, "val", VAL)
    promised(rec, "memb", {PUT_COMPLETE, RMW_COMPLETE}, absent=True)


def test_collisions_case():
    o = C.make_oracle("S")
    T = C.describe(o, "S")
    K, M, fakes = C.collision_keys(T)
    assert T.is_inline([K])[0] and not T.is_inline([M])[0] and T.bucket([K])[0] == T.bucket([M])[0]
    for k, f in zip((K, M), fakes):   # same bucket, same tag, absent
        assert T.bucket([f])[0] == T.bucket([k])[0] and int(f) >> 48 == int(k) >> 48 and o.lookup(int(f)) is None
    rec = C.Rec(T.inline_keys)
    C.case_collisions(C.OracleEngine(o), T, rec)
    promised(rec, "local", LOCAL, absent=True)    # (the fakes: asserted MISS by the case itself)
    promised(rec, "inv", INV, absent=True)
    promised(rec, "ack", ACK)
    promised(rec, "rw", {PUT_COMPLETE})
    promised(rec, "val", VAL)


def test_dense_case():
    o = C.make_oracle("D")
    T = C.describe(o, "D")
    strata = C.dense_strata(T)
    assert all(len(v) >= 200 for v in strata.values())
    assert not T.present[np.isin(T.keys, strata["evicted"])].any()
    assert T.is_inline(strata["inline_full"]).all() and T.is_inline(strata["inline_part"]).all()
    assert not T.is_inline(strata["slot7_full"]).any()
    assert all(o.lookup(int(k)) is not None for k in strata["slot7_full"][:200])
    rec = C.Rec(T.inline_keys)
    C.case_dense(C.OracleEngine(o), T, rec)
    promised(rec, "local", LOCAL, absent=True)
    promised(rec, "inv", INV, absent=True)
    promised(rec, "val", VAL)


@pytest.mark.parametrize("n_rows,skip", [(2, -1), (2, 1), (8, -1), (8, 3)])
def test_ack_rows_case(n_rows, skip):
    _, me, _ = C.rows_setup(n_rows, skip)
    o = C.make_oracle("S", machine_id=me)
    T = C.describe(o, "S")
    rec = C.Rec(T.inline_keys)
    C.case_ack_rows(C.OracleEngine(o, me), T, rec, n_rows, skip, inline=True)
    promised(rec, "local", LOCAL)
    promised(rec, "rw", {PUT_COMPLETE})


def test_inv_rows_case():
    o = C.make_oracle("S")
    T = C.describe(o, "S")
    rec = C.Rec(T.inline_keys)
    C.case_inv_rows(C.OracleEngine(o), T, rec)
    promised(rec, "inv", {INV_SUCCESS})
    states = C.key_states(o, T.inline_keys)
    assert (states != int(L.State.VALID)).sum() > 20, "the INV rows invalidated inline keys"
