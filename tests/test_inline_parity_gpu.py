"""The inline-layout kernels against the oracle without reconverting.

A Mirror that exports the table after every launch sends it back to LOG each time, and the conversion in front of
the next launch copies every inline key's entry from the log into its line: log and line are then byte-equal when
each checked launch starts, and a kernel that reads an inline key's key, meta, value or lock byte from the log
gives right answers all the same. Here the Mirror checks the table only where a test says so
(table_check="deferred"), so launch after launch runs on lines that only kernels have written while the log copies
of the inline keys go stale; elements, read_write_ops, node_suspected, the ACK / VAL callbacks' output and the
error flags are still compared per launch. Every launch states the layout it must run in (from the launch kind,
tests/inline_cases.py), and the Mirror asserts it from the layout counters: no test passes by running in LOG.

The cases and their inputs are tests/inline_cases.py; tests/test_inline_cases_cpu.py shows on the oracle alone
that they produce their outcomes on inline keys and on the others.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def engine_path():
    """The multi-kernel engine for every launch: left to itself a launch of at most 4096 elements takes the
    single-workgroup kernel, which has no inline instance."""
    from hermes_amd import kvs
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    yield
    kvs.HermesKV.default_flags = 0


def make_pair(name, what, rmw=False, skew=0, machine_id=0):
    """device table and oracle twin of geometry `name`, INLINE preferred, behind a deferred Mirror"""
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO[name]
    g = HermesKV(n_keys, bkts, cap, machine_id=machine_id, rmw=rmw, skew=skew)
    o = C.make_oracle(name, rmw=rmw, skew=skew, machine_id=machine_id)
    T = C.describe(o, name)
    assert g.prefer_layout(INLINE)
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == 0 and lay["inline_launches"] == 0
    m = Mirror(g, o, what, table_check="deferred")
    return g, m, GpuEngine(m), T, C.Rec(T.inline_keys)


def both(rec, kind, codes):
    for inline in (True, False):
        assert codes <= rec.codes(kind, inline), (kind, inline, rec.seen)


@pytest.mark.parametrize("skew", [0, 3])
def test_protocol_rounds_without_reconversion(skew):
    """3a: six rounds of local / two unique INV launches / two unique ACK launches / VALs on geometry A, all INLINE,
    the table exported after rounds 2 and 5 only, and once more when all is over (round 6 wrote too): 12 launches run
    before the first export and 18 between the first two, on lines that only kernels have written. Each export costs
    two conversions (back to LOG, and INLINE again in front of the next launch); the last leaves the table in LOG."""
    g, m, eng, T, rec = make_pair("A", f"rounds skew {skew}", skew=skew)
    C.case_rounds(eng, T, rec, skew=skew)
    lay = g.layout()
    assert m.launches == 36 and lay["inline_launches"] == 36, lay
    assert lay["conversions"] == 5 and lay["state"] == INLINE, lay
    m.check_table("the end")
    lay = g.layout()
    assert lay["conversions"] == 6 and lay["state"] == LOG, lay
    both(rec, "local", {int(L.Resp.GET_COMPLETE), int(L.Resp.PUT_SUCCESS), int(L.Resp.GET_STALL)})
    both(rec, "rw", {int(L.Resp.PUT_COMPLETE)})
    both(rec, "val", {C.MOVED_TO_VALID})
    assert g.take_error_flags() == 0


def test_collisions_and_hot_inline_keys():
    """3b: an inline key, a bucket-mate that is not inline, and absent keys of the same bucket and tag, alone (hot
    segments) and among 300 others; the table exported once per pool."""
    g, m, eng, T, rec = make_pair("S", "collisions")
    C.case_collisions(eng, T, rec)
    lay = g.layout()
    assert m.launches == 3 * 5 and lay["inline_launches"] == 15 and lay["conversions"] == 6, lay
    both(rec, "rw", {int(L.Resp.PUT_COMPLETE)})
    assert g.take_error_flags() == 0


def test_dense_table():
    """3c: geometry D, where most buckets are full (the inline key in slot 0, seven more slots to probe) and a
    quarter of the keys were evicted: evicted keys, slot-0 and slot-7 keys of full buckets, inline keys of other
    buckets; one export at the end."""
    g, m, eng, T, rec = make_pair("D", "dense")
    C.case_dense(eng, T, rec)
    lay = g.layout()
    assert m.launches == 6 and lay["inline_launches"] == 6 and lay["conversions"] == 2, lay
    both(rec, "local", {int(L.Resp.GET_COMPLETE), int(L.Resp.PUT_SUCCESS)})
    assert g.take_error_flags() == 0


def test_rmw_table_mixed_layouts():
    """3d: an RMW-enabled table with 64-B entries is eligible, its unique INV and 56-B ACK launches and its VALs
    have inline kernels, its local and after-membership-change launches do not. Per round: local in LOG, then
    INVs (one conversion), ACKs and VALs INLINE; in the last two rounds the after-membership-change launch takes
    the table back (one conversion); the table is exported after every round (one conversion where the round ended
    INLINE). Two conversions per round either way."""
    g, m, eng, T, rec = make_pair("A", "rmw", rmw=True)
    seen = []
    real = m.check_table

    def counted(what):
        seen.append(g.layout())
        real(what)
    m.check_table = counted
    C.case_rounds(eng, T, rec, rmw=True, rounds=4, big=(1,), check_after=(0, 1, 2, 3), memb_from=2)
    lay = g.layout()
    assert m.launches == 4 * 6 + 2 and lay["inline_launches"] == 4 * 5, lay
    # before each round's export: INLINE in the first two rounds, LOG after the membership launch of the last two
    assert [s["state"] for s in seen] == [INLINE, INLINE, LOG, LOG], seen
    assert [s["conversions"] for s in seen] == [1, 3, 6, 8], seen
    assert lay["conversions"] == 8 and lay["state"] == LOG, lay
    assert int(L.Resp.OP_INV_ABORT) in rec.codes("inv", True), rec.seen
    both(rec, "rw", {int(L.Resp.PUT_COMPLETE), int(L.Resp.RMW_COMPLETE)})
    assert g.take_error_flags() == 0


@pytest.mark.parametrize("n_rows,skip", [(2, -1), (2, 1), (8, -1), (8, 3)])
def test_ack_rows(n_rows, skip):
    """3e: ACK rows launches with the VAL callbacks (k_unique_rows, the 2-row and the 8-row instance), with and
    without a skip row, twice in a row, INLINE; one export after the second."""
    _, me, _ = C.rows_setup(n_rows, skip)
    g, m, eng, T, rec = make_pair("S", f"rows {n_rows} {skip}", machine_id=me)
    C.case_ack_rows(eng, T, rec, n_rows, skip, inline=True)
    lay = g.layout()
    assert m.launches == 4 and lay["inline_launches"] == 4 and lay["conversions"] == 2, lay
    both(rec, "rw", {int(L.Resp.PUT_COMPLETE)})
    assert m.codes[(int(L.BatchType.acks), "vals_sent", 0)] > 0, m.codes
    assert g.take_error_flags() == 0


def test_nine_rows_are_refused():
    """Nine rows: the library takes at most HKV_MAX_ROWS = 8 and refuses the descriptor before it touches the
    layout, so there is no launch that could run in LOG; the table stays as the local launch left it."""
    from hermes_amd.lib import HkvError
    g, m, eng, T, rec = make_pair("S", "rows 9")
    with pytest.raises(HkvError, match="HKV_BATCH_ROWS"):
        C.case_ack_rows(eng, T, rec, 9, -1, inline=False, reps=1)
    lay = g.layout()
    assert lay["state"] == INLINE and lay["inline_launches"] == 1 and lay["conversions"] == 1, lay
    assert m.launches == 1 and g.take_error_flags() == 0


def test_inv_rows():
    """3e: the library accepts INV rows (without d_ack_out and node_suspected): three rows of 56-B INVs, INLINE."""
    g, m, eng, T, rec = make_pair("S", "inv rows")
    C.case_inv_rows(eng, T, rec)
    lay = g.layout()
    assert m.launches == 2 and lay["inline_launches"] == 2 and lay["conversions"] == 2, lay
    assert int(L.Resp.INV_SUCCESS) in rec.codes("inv", True)
    assert g.take_error_flags() == 0


@pytest.mark.parametrize("machines", [3, 8])
def test_whole_round_checked_once_per_step(machines):
    """3f: the bench round of test_retry_round_mirrored (skew 3, retry; 60,000 keys, 40 workers) with 2 and with 7
    virtual peers (the 2-row and the 8-row ACK rows instance), every launch INLINE and compared per launch, the
    table exported once per step -- not after each of its launches."""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.workload import Round, zipf_params
    n_keys, bkts, cap = 60_000, 1 << 16, 1 << 23
    g = HermesKV(n_keys, bkts, cap, machine_id=0, skew=3)
    o = OracleKVS(bkts, cap, 0, skew=3)
    o.populate(n_keys, g.sizes.kvs_value)
    m = Mirror(g, o, f"round of {machines}", table_check="deferred", expect_inline=True)
    r = Round(g, 40, L.membership(machines, 0), list(range(1, machines)), zipf_params(n_keys, 0.99), 200, seed=0x5EED,
              max_steps=8, trace_len=1024, retry_stalled=True)
    assert r.inline and r.fused
    steps = 3
    for step in range(steps):
        r.step()
        torch.cuda.synchronize()
        assert g.layout()["state"] == INLINE
        m.check_table(f"step {step}")
    # local, one INV launch per peer, their ACKs as one rows launch, VAL
    assert m.launches == steps * (machines + 2)
    lay = g.layout()
    assert lay["conversions"] == 2 * steps and lay["inline_launches"] >= 5 * steps, lay
    st = r.stats()
    assert st["committed"] > 0 and st["dropped"] == 0, st
    assert (m.codes[(int(L.BatchType.acks), "vals_sent", 0)] > 0) == r.fused_vals, m.codes
    assert m.codes[(int(L.BatchType.invs), "out8", int(L.Resp.INV_SUCCESS))] > 0
    assert m.codes[(int(L.BatchType.local_ops), "out9", int(L.Resp.PUT_COMPLETE))] > 0, m.codes
    assert g.take_error_flags() == 0
