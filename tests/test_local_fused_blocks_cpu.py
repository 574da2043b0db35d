"""The cases of tests/local_block_cases.py on the oracle alone: each produces the outcome it is meant to -- the first
writer at the stated position, the stated number of first writers, elements on INVALID keys that replay, stall and
write, misses and skipped elements where they were put -- so a green run of tests/test_local_fused_blocks_gpu.py is
known to have exercised them. Needs no GPU."""
import numpy as np
import pytest

from hermes_amd import layout as L
from tests import inline_cases as C
from tests import local_block_cases as B


def setup(skew):
    o = C.make_oracle("S", skew=skew)
    return B.OracleBlockEngine(o), C.describe(o, "S")


@pytest.mark.parametrize("skew", [0, 3])
def test_block_edges(skew):
    eng, T = setup(skew)
    facts = B.case_block_edges(eng, T, skew=skew)
    assert [(f[0], f[1], f[2]) for f in facts] == [(n, r, p) for n, _, _ in B.SIZES for r in (False, True)
                                                   for p in (False, True)]
    codes = set()
    for n, ragged, patched, after, live, pos, before in facts:
        a8, b8 = after.view(np.uint8).reshape(n, -1), before.view(np.uint8).reshape(n, -1)
        assert len(live) == n and (not ragged or not live.all()), "ragged launches leave elements out"
        ran = live & ~np.isin(before["state"], C.SKIPPED_LOCAL)
        assert (after["state"][ran] != B.NEW).all() or (before["state"][ran] != B.NEW).all()
        assert np.array_equal(a8[~ran], b8[~ran]), "elements outside the counts and skipped ones stay as patched"
        if patched:   # positions 0, 31, 32 and 63 of every block hold a patched op, and those inside the counts ran
            edge = [i for i in range(n) if i % B.BLOCK in B.EDGE]
            assert set(edge) <= set(pos.tolist())
            assert (before["state"][pos] == B.NEW).all() and (after["state"][pos[live[pos]]] != B.NEW).all()
        codes |= set(after["state"][ran].tolist())
    assert {B.MISS, B.PUT_SUCCESS, B.GET_COMPLETE, B.GET_STALL, B.PUT_STALL} <= codes, codes
    # a count that ends inside wave 0's half, and a batch with count 0
    assert (B.ragged_counts(1, 64) < 32).all() and 0 in B.ragged_counts(3, 43) and 0 in B.ragged_counts(1, 1)
    assert 0 < B.ragged_counts(3, 43)[0] < 32 and B.ragged_counts(2, 100)[1] < 32


@pytest.mark.parametrize("skew", [0, 3])
def test_first_writer_position(skew):
    eng, T = setup(skew)
    facts = B.case_first_writer_position(eng, T, skew=skew)
    assert sorted((p, il) for p, il, *_ in facts) == sorted((p, il) for p in B.EDGE for il in (False, True))
    for p, il, oc, before, after in facts:
        i = np.arange(B.BLOCK)
        assert np.nonzero(after == B.PUT_SUCCESS)[0].tolist() == [p], "the first PUT is the key's first writer"
        assert (after[(i < p) & (oc == B.GET)] == B.GET_COMPLETE).all()
        assert (after[(i < p) & (oc == B.PUT)] == int(L.Bucket.IN_PROGRESS_PUT)).all()
        assert (after[(i > p) & (oc == B.GET)] == B.GET_STALL).all()
        assert np.isin(after[(i > p) & (oc == B.PUT)], [B.PUT_STALL, int(L.Resp.PUT_COMPLETE)]).all()
        if p < B.BLOCK - 1:
            assert ((i > p) & (oc == B.GET)).any() and ((i > p) & (oc == B.PUT)).any()
        if p > 0:
            assert ((i < p) & (oc == B.GET)).any()


@pytest.mark.parametrize("skew", [0, 3])
def test_first_writers_per_block(skew):
    eng, T = setup(skew)
    facts = B.case_first_writers_per_block(eng, T, skew=skew)
    assert tuple(k for k, _, _ in facts) == B.FIRST_WRITERS
    for k, pos, after in facts:
        assert np.nonzero(after == B.PUT_SUCCESS)[0].tolist() == pos.tolist() and len(pos) == k
        assert (np.delete(after, pos) == B.GET_COMPLETE).all()
        if k >= 2:
            assert (pos < 32).any() and (pos >= 32).any()


@pytest.mark.parametrize("skew", [0, 3])
def test_deferred(skew):
    eng, T = setup(skew)
    facts = B.case_deferred(eng, T, skew=skew)
    assert tuple(d for d, *_ in facts) == B.DEFERRED
    for d, st0, oc, after in facts:
        inv = st0 == int(L.State.INVALID)
        assert inv.sum() == d and (st0[~inv] == int(L.State.VALID)).all()
        assert (after[~inv] == B.GET_COMPLETE).all()
        assert B.REPLAY_SUCCESS in after[inv], "a GET replays"
        if d >= 2:
            assert B.GET_STALL in after[inv], "a GET on a key whose last writer is alive stalls"
            half = np.nonzero(inv)[0] % B.BLOCK < 32
            assert half.any() and (~half).any()
        if d == B.BLOCK:
            assert B.PUT_SUCCESS in after[inv] and B.PUT_STALL in after[inv]
            assert (after[inv & (oc == B.GET)] == B.GET_STALL).sum() > (d - 40) // 2, "later elements of replayed keys"


@pytest.mark.parametrize("skew", [0, 3])
def test_misses_and_skipped(skew):
    eng, T = setup(skew)
    miss, skipped, before, after = B.case_misses_and_skipped(eng, T, skew=skew)
    assert (after["state"][miss] == B.MISS).all() and (np.delete(after["state"], miss) != B.MISS).all()
    assert {B.GET, B.PUT} <= set(before["opcode"][miss].tolist())
    a8, b8 = after.view(np.uint8).reshape(len(after), -1), before.view(np.uint8).reshape(len(before), -1)
    assert np.array_equal(a8[skipped], b8[skipped])
    for pos in (miss, skipped):
        assert (pos % B.BLOCK < 32).any() and (pos % B.BLOCK >= 32).any() and (pos >= 2 * B.BLOCK).any()
    assert B.PUT_SUCCESS in after["state"] and B.GET_COMPLETE in after["state"]
