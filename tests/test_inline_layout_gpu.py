"""The table's two layouts (include/hermeskv.h, "Table layouts"): LOG -- index and log, the reference's image --
and INLINE, the private residency of one 128-B line per bucket holding the bucket and the whole entry of the key
in its lowest in-use slot. Conversions round-trip; the same rounds give the same bytes in either layout; a launch
without inline kernels sends the table back to LOG first; ineligible tables stay LOG; every export is the
reference's image whatever the layout.

Base geometry: 4096 keys in 4096 buckets of 64-B entries, a Poisson load of 1: about 63 % of the keys are inline
keys and about 8 % of the buckets hold three or more keys, so both kinds of hit are exercised (asserted from the
exported index by the tests themselves).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS  # noqa: E402
from tests import gen  # noqa: E402
from tests.helpers import Mirror  # noqa: E402
from tests.inline_cases import census  # noqa: E402

N_KEYS, BKTS, CAP = 4096, 4096, 1 << 19
LOG, INLINE = 0, 1
FLAG = np.uint64(1 << 63)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def assert_census(n_keys, nz, n_used):
    assert int(n_used.sum()) == n_keys, "no evictions at this load"
    frac = len(nz) / n_keys
    assert 0.50 <= frac <= 0.75, f"inline keys are {frac:.2%} of the keys"
    assert int((n_used >= 3).sum()) >= 100, "buckets with three or more keys"


def make_table(skew=0, **kw):
    from hermes_amd.kvs import HermesKV
    return HermesKV(N_KEYS, BKTS, CAP, machine_id=0, skew=skew, **kw)


def make_round(g, n_keys=N_KEYS, write_permille=200, rmw_permille=0, **kw):
    from hermes_amd.workload import Round, zipf_params
    return Round(g, 40, L.membership(3, 0), [1, 2], zipf_params(n_keys, 0.99), write_permille, rmw_permille,
                 seed=0x5EED, max_steps=8, trace_len=1024, **kw)


def test_round_trip_and_line_format():
    g = make_table()
    idx0, log0 = g.index_bytes(), g.log_bytes()
    slots, first, nz, phys, _, n_used = census(idx0, log0, CAP)
    assert_census(N_KEYS, nz, n_used)
    lay = g.layout()
    assert lay["state"] == LOG and lay["preferred"] == LOG and lay["conversions"] == 0
    assert g.prefer_layout(INLINE)
    g.apply_layout()
    lay = g.layout()
    assert lay["state"] == INLINE and lay["conversions"] == 1 and lay["line_bytes"] == BKTS * 128
    lines = g.line_bytes()                     # (does not convert)
    assert g.layout()["state"] == INLINE
    lw = lines.view("<u8").reshape(BKTS, 16)
    flags = (lw[:, :8] & FLAG) != 0
    # the bucket half is the bucket, with the flag on the lowest in-use slot and on no other
    assert np.array_equal(lw[:, :8] & ~FLAG, slots)
    want = np.zeros_like(flags)
    want[nz, first[nz]] = True
    assert np.array_equal(flags, want)
    assert not flags[first < 0].any(), "an empty bucket carries no flag"
    # the entry half is that key's whole log entry
    ent = lines.reshape(BKTS, 128)[nz, 64:]
    assert np.array_equal(ent, log0[phys[:, None] + np.arange(64)[None, :]])
    # both exports convert back and are byte-equal to the ones before
    idx1, log1 = g.index_bytes(), g.log_bytes()
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == 2
    assert np.array_equal(idx0, idx1) and np.array_equal(log0, log1)


def test_same_rounds_in_both_layouts(monkeypatch):
    """Two tables from the same seed, one INLINE and one held in LOG by the switch, four configs[1]-shaped
    rounds (retry, skew 3, 40 workers, 2 virtual peers): byte-equal after every round."""
    tables = []
    for inline in (True, False):
        monkeypatch.setenv("HKV_INLINE", "1" if inline else "0")
        g = make_table(skew=3)
        calls = [0]
        real = g.batch

        def counted(*a, _real=real, _calls=calls, **k):
            _calls[0] += 1
            _real(*a, **k)
        g.batch = counted
        r = make_round(g, retry_stalled=True)
        assert r.inline == inline and r.fused
        tables.append((g, r, calls))
    (ga, a, calls), (gb, b, _) = tables
    _, _, nz, _, _, n_used = census(gb.index_bytes(), gb.log_bytes(), CAP)
    assert_census(N_KEYS, nz, n_used)
    for step in range(4):
        k = a.clock % len(a.remote_packed)
        for _, r, _ in tables:
            r.step()
        torch.cuda.synchronize()
        assert ga.layout()["state"] == INLINE and gb.layout()["state"] == LOG
        for name in ("ops", "states", "opcodes", "patch", "cursor", "inv_out", "inv_count", "ack_out", "acks",
                     "val_out"):
            assert torch.equal(getattr(a, name), getattr(b, name)), f"round {step}: {name} differs"
        for j, (x, y) in enumerate(zip(a.remote_packed[k], b.remote_packed[k])):   # the peers' INV and VAL slabs
            if isinstance(x, torch.Tensor):
                assert torch.equal(x, y), f"round {step}: remote slab {k}.{j} differs"
        assert torch.equal(a.fold_counters(), b.fold_counters()), f"round {step}: counters differ"
        assert np.array_equal(ga.index_bytes(), gb.index_bytes()), f"round {step}: index differs"
        assert np.array_equal(ga.log_bytes(), gb.log_bytes()), f"round {step}: log differs"
    # every batch launch of the rounds has inline kernels, and each ran while INLINE (the exports above send
    # the table back to LOG after every round; the next round's first table reader converts it again)
    la, lb = ga.layout(), gb.layout()
    assert calls[0] == 4 * 5 and la["inline_launches"] >= calls[0], (calls, la)
    assert la["conversions"] == 8 and lb["conversions"] == 0 and lb["inline_launches"] == 0, (la, lb)
    assert a.stats() == b.stats() and a.stats()["committed"] > 0 and a.stats()["writes_completed"] > 0
    assert ga.take_error_flags() == 0 and gb.take_error_flags() == 0


def test_launch_without_inline_kernels_converts_first():
    """On an INLINE table, a small launch forced down the single-workgroup path and a non-unique INV launch, both
    on inline keys: the table goes to LOG for them (the Mirror agrees byte for byte after each), the next capable
    launch takes it back, and the conversion counter moves by two."""
    from hermes_amd.kvs import BATCH_SMALL
    g = make_table()
    o = OracleKVS(BKTS, CAP, 0)
    o.populate(N_KEYS, g.sizes.kvs_value)
    _, _, nz, _, inline_keys, n_used = census(g.index_bytes(), g.log_bytes(), CAP)
    assert_census(N_KEYS, nz, n_used)
    assert g.prefer_layout(INLINE)
    seen = []                      # the layout right after each launch, before the Mirror's exports
    real = g.batch

    def spy(*a, **k):
        real(*a, **k)
        seen.append(g.layout())
    g.batch = spy
    m = Mirror(g, o, "layout flips")
    rng = np.random.default_rng(77)
    tsp = gen.TsPool(rng)
    mb = L.membership(3, 0)
    sz = g.sizes

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def local(n_batches, stride):
        pool = gen.key_pool(rng, inline_keys, hot=300)
        ops = gen.local_ops(rng, pool, n_batches * stride, sz, False, tsp)
        m.batch(L.BatchType.local_ops, dev(ops), n_batches, stride, sz.op, mb)

    for what in ("small", "invs"):
        g.apply_layout()
        before = g.layout()
        assert before["state"] == INLINE
        if what == "small":
            g.default_flags = BATCH_SMALL
            local(4, 64)
            g.default_flags = 0
        else:   # keys repeat within the launch: the engine's INV path, which has no inline instance
            pool = gen.key_pool(rng, inline_keys, hot=300)
            invs = gen.invs(rng, pool, 40 * 125, sz, False, tsp, machine_num=3)
            m.batch(L.BatchType.invs, dev(invs), 40, 125, sz.op, mb)
        assert seen[-1]["state"] == LOG and seen[-1]["conversions"] == before["conversions"] + 1, (what, seen[-1])
        assert seen[-1]["inline_launches"] == before["inline_launches"]
        local(40, 250)            # the local direct path: capable
        assert seen[-1]["state"] == INLINE and seen[-1]["conversions"] == before["conversions"] + 2, (what, seen[-1])
        assert seen[-1]["inline_launches"] == before["inline_launches"] + 1
    assert m.launches == 4


@pytest.mark.parametrize("kind", ["big_objects", "wrapped_log"])
def test_ineligible_tables_stay_log(kind):
    from hermes_amd.kvs import HermesKV
    if kind == "big_objects":
        n_keys, bkts, cap, kw = 4096, 4096, 1 << 21, dict(rmw=True, big_objects=True, extra_cache_lines=4)
        o = OracleKVS(bkts, cap, 0, True, True, 4)
    else:
        n_keys, bkts, cap, kw = 3000, 4096, 1 << 17, {}     # 3000 x 64 B > 128 KiB: the log wraps at populate
        o = OracleKVS(bkts, cap, 0)
    g = HermesKV(n_keys, bkts, cap, machine_id=0, **kw)
    o.populate(n_keys, g.sizes.kvs_value)
    assert kind != "wrapped_log" or g.log_head > cap
    assert not g.prefer_layout(INLINE)
    lay = g.layout()
    assert not lay["eligible"] and lay["state"] == LOG
    m = Mirror(g, o, kind)
    r = make_round(g, n_keys, **(dict(write_permille=500, rmw_permille=500) if kind == "big_objects" else {}))
    assert not r.inline
    for _ in range(2):
        r.step()
    torch.cuda.synchronize()
    assert m.launches >= 2 * 5 and r.stats()["committed"] > 0
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == 0 and lay["inline_launches"] == 0
    assert g.take_error_flags() == 0


class _DeviceBytes:
    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 3}


def test_device_log_of_an_inline_table(monkeypatch):
    """hkv_device_log after a round on an INLINE table: the pointer's bytes are hkv_copy_log's, and those of a
    twin table that ran the same round in LOG."""
    logs = []
    for inline in (True, False):
        monkeypatch.setenv("HKV_INLINE", "1" if inline else "0")
        g = make_table(skew=3)
        r = make_round(g, retry_stalled=True)
        r.step()
        torch.cuda.synchronize()
        assert g.layout()["state"] == (INLINE if inline else LOG)
        dev = torch.as_tensor(_DeviceBytes(g.device_log(), CAP), device="cuda").cpu().numpy().copy()
        assert g.layout()["state"] == LOG
        assert np.array_equal(dev, g.log_bytes())
        logs.append(dev)
    assert np.array_equal(logs[0], logs[1])
    populated = make_table(skew=3).log_bytes()
    assert not np.array_equal(logs[0], populated), "the round wrote entries"


def test_full_size_inline_round_invariants():
    """configs[1] at full size (100M keys, 16384 virtual workers: the bench's round) on an INLINE table. A log
    pointer held across rounds is stale for the inline keys there, so the log is taken again after every round
    (hkv_device_log converts): every key is VALID again -- every local write ACKed by both peers and completed,
    every INV's VAL applied -- no INV was held back, writes completed, no consistency flag; and each round's
    launches ran while INLINE, with the two conversions per round that taking the log costs."""
    from hermes_amd.kvs import HermesKV, sized_geometry
    from hermes_amd.workload import Round, zipf_params
    n_keys = 100_000_000
    bkts, cap = sized_geometry(n_keys, L.DEFAULT)
    g = HermesKV(n_keys, bkts, cap, machine_id=0)
    r = Round(g, 16384, L.membership(3, 0), [1, 2], zipf_params(n_keys, 0.99), 200, 0, seed=0x5EED, max_steps=4)
    assert r.inline and r.fused
    entry = g.sizes.entry
    assert g.log_head == n_keys * entry

    def not_valid():
        log = torch.as_tensor(_DeviceBytes(g.device_log(), n_keys * entry), device="cuda")
        return int((log.view(n_keys, entry)[:, 18] != int(L.State.VALID)).sum())
    assert not_valid() == 0
    for step in range(3):
        r.step()
        torch.cuda.synchronize()
        lay = g.layout()
        assert lay["state"] == INLINE and lay["inline_launches"] >= 5 * (step + 1), lay
        bad = not_valid()
        assert g.layout()["state"] == LOG and g.layout()["conversions"] == 2 * (step + 1)
        assert bad == 0, f"round {step}: {bad} keys not VALID"
    # the inline keys' entries did change under the rounds: timestamps moved on in most written keys
    log = torch.as_tensor(_DeviceBytes(g.device_log(), n_keys * entry), device="cuda").view(n_keys, entry)
    assert int((log[:, 24:28].contiguous().view(torch.int32) != 0).sum()) > 300_000
    st = r.stats()
    assert st["invs_held"] == 0 and st["committed"] > 4_000_000 and st["writes_completed"] > 600_000, st
    assert g.take_error_flags() == 0
