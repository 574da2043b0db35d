"""HermesKV.census() (hkv_table_census_async, k_table_census) on the device against tests/census_model.py.

Every field of the census must equal the numpy model: on the table's own exported image after a fresh populate
(every geometry of test_populate_bit_exact and the edge tables), on the oracle twin's image after every launch of
the scripted protocol scenario, and -- the case the census exists for -- on the twin's image of an INLINE table
whose log copies have gone stale under twelve launches with no export in between, where a census read from the
log is shown (on the CPU) to give another digest. Then the offender list, and replica groups: equal digests after
a round, a different one after an INV that only one replica saw, and group_census over gloo.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import OracleKVS, gen_keys  # noqa: E402
from tests import census_model as CM  # noqa: E402
from tests import gen  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

LOG, INLINE = 0, 1
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_pair(n_keys, num_bkts, log_cap, rmw=False, big=False, machine_id=0, ecl=None):
    """ecl: big objects of that many extra cache lines (default: 4 with big, the default geometry without)"""
    from hermes_amd.kvs import HermesKV
    ecl = (4 if big else 0) if ecl is None else ecl
    sizes = L.Sizes(True, ecl) if ecl else L.DEFAULT
    g = HermesKV(n_keys, num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl, populate=n_keys > 0)
    o = OracleKVS(num_bkts, log_cap, machine_id, rmw, ecl > 0, ecl)
    if n_keys:
        o.populate(n_keys, sizes.kvs_value)
    return g, o, sizes


def twin_image(o, sizes):
    return CM.oracle_image(o, sizes)


def assert_census(got: dict, want: dict, what: str):
    assert tuple(got) == CM.FIELDS
    for f in CM.FIELDS:
        assert got[f] == want[f], f"{what}: {f}: device {got[f]} != model {want[f]}"


# ------------------------------------------------------------------ 1. LOG, fresh populate
@pytest.mark.parametrize("n_keys,num_bkts,log_cap,big", [
    (5000, 16384, 1 << 20, False),     # default-shaped: under one key per bucket, nothing evicted
    (20000, 2048, 1 << 21, False),     # ~10 keys per bucket: full buckets, evictions
    (3000, 4096, 1 << 17, False),      # the log wraps: dead slots
    (1500, 256, 1 << 20, True),        # big objects, 320-byte entries
    (2000, 1024, 1 << 18, True),       # big objects whose log wraps
    (0, 64, 1 << 16, False),           # no key
    (1, 64, 1 << 16, False),           # one key
    (40, 16, 1 << 16, False),          # 16 buckets: a quarter of one block's step
    (100, 32, 1 << 16, False),         # 32 buckets: not a multiple of the 64 buckets a block takes per step
    (60000, 1 << 18, 1 << 23, False),  # 4096 steps for a grid of at most 2048 blocks: the grid-stride loop
])
def test_census_log_fresh_populate(n_keys, num_bkts, log_cap, big):
    g, o, sizes = make_pair(n_keys, num_bkts, log_cap, big=big, rmw=big)
    a = g.census()
    sync = g.census_host()
    b = g.census(out=a.tensor)                       # again, into the same buffer: overwritten, not accumulated
    first = a.tensor.cpu().numpy().tobytes()         # (stream order: reads the second result)
    c = g.census(out=torch.full((32,), -1, dtype=torch.int64, device="cuda"))   # into a dirty buffer
    assert c.tensor.cpu().numpy().tobytes() == first == b.tensor.cpu().numpy().tobytes()
    lay = g.layout()
    assert lay["state"] == LOG and lay["conversions"] == 0 and lay["inline_launches"] == 0
    want = CM.census_model(g.index_bytes(), g.log_bytes(0, log_cap + sizes.entry), g.log_head, log_cap, sizes)
    assert_census(a.host(), want, "async")
    assert_census(sync, want, "sync")
    assert want == CM.census_model(*twin_image(o, sizes)), "the device image is the oracle's"
    assert a.keys == want["keys"] and a.by_state == want["by_state"]     # the lazy attributes
    if n_keys >= 1000:
        assert want["keys"] > 0 and want["by_state"][int(L.State.VALID)] == want["keys"]
        assert (want["dead_slots"] > 0) == (g.log_head > log_cap)
    else:
        assert want["keys"] == n_keys
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 2. mid-protocol states, LOG
@pytest.mark.parametrize("cfg", [dict(rmw=False, big=False), dict(rmw=True, big=False), dict(rmw=True, big=True)])
def test_census_mid_protocol_states(cfg):
    """tests/scripted.py on the device and the oracle twin: local launch, INVs from peers, ACKs, membership
    changes, replays, VALs; after every launch the census equals the model on the twin's image"""
    from tests.scripted import run_scripted
    rmw, big = cfg["rmw"], cfg["big"]
    g, o, sizes = make_pair(1000, 4096, 1 << 22, rmw=rmw, big=big)
    seen = []

    def runner(btype, elems, mb, rw=None, node_suspected=None):
        eo = gen.bytecopy(elems)
        rwo = gen.bytecopy(rw) if rw is not None else None
        ns_o = node_suspected.copy() if node_suspected is not None else None
        g.batch_host(btype, elems, mb, rw=rw, node_suspected=node_suspected)
        o.batch_multi(btype, eo, 1, len(eo), None, mb, rw=rwo, node_suspected=ns_o)
        want = CM.census_model(*twin_image(o, sizes))
        assert_census(g.census().host(), want, f"launch {len(seen)} type {int(btype)}")
        seen.append(want)

    run_scripted(runner, gen_keys(1000), sizes, rmw)
    assert len(seen) == 8
    CM.assert_not_vacuous(seen)          # (on the oracle's side)
    assert g.layout()["conversions"] == 0
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 3. INLINE with stale logs
def test_census_inline_with_stale_logs():
    """Two protocol rounds of tests/inline_cases.py on geometry A, INLINE, twelve launches and no export: the
    inline keys' log entries still hold their populate-time bytes. The census reads the lines."""
    from hermes_amd import kvs
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO["A"]
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE     # (the single-workgroup kernel has no inline instance)
    try:
        g = HermesKV(n_keys, bkts, cap)
        o = C.make_oracle("A")
        T = C.describe(o, "A")
        assert g.prefer_layout(INLINE)
        m = Mirror(g, o, "census inline", table_check="deferred")
        C.case_rounds(GpuEngine(m), T, C.Rec(T.inline_keys), rounds=2, big=(1,), check_after=())
    finally:
        kvs.HermesKV.default_flags = 0
    before = g.layout()
    assert m.launches == 12 and before["state"] == INLINE and before["inline_launches"] == 12, before
    assert before["conversions"] == 1, before
    want = CM.census_model(*twin_image(o, L.DEFAULT), inline=True)
    k = want["offenders"]
    assert k >= 8 and want["keys"] == int(T.present.sum())
    buf = torch.full((k + 4,), CANARY, dtype=torch.int64, device="cuda")
    c = g.census(offender_cap=k + 4, offender_keys=buf)
    got = c.host()
    assert g.layout() == before, "the census moved the layout or its counters"
    assert got["from_lines"] == len(T.inline_keys) > 0
    assert_census(got, want, "INLINE")
    assert np.array_equal(np.sort(c.offenders_host()), CM.offender_keys(*twin_image(o, L.DEFAULT)))
    assert (buf[k:].cpu().numpy() == CANARY).all()
    # what a reader of index and log would have seen: the inline keys' entries as they were when the table was
    # converted (the populate image), every other entry current -- another digest, so no census read from the
    # log passes this test
    idx, log_now, head, _, _ = twin_image(o, L.DEFAULT)
    _, _, _, phys, ikeys, _ = C.census(idx, T.log, cap)
    assert np.array_equal(ikeys, T.inline_keys)
    stale = log_now.copy()
    rows = phys[:, None] + np.arange(64)[None, :]
    stale[rows] = T.log[rows]
    assert not np.array_equal(stale, log_now)
    stale_c = CM.census_model(idx, stale, head, cap, L.DEFAULT)
    assert stale_c["digest_sum"] != want["digest_sum"] and stale_c["digest_xor"] != want["digest_xor"]
    # the export sends the table to LOG: the same census, read from index and log
    image = CM.census_model(g.index_bytes(), g.log_bytes(0, cap + 64), g.log_head, cap, L.DEFAULT)
    after = g.layout()
    assert after["state"] == LOG and after["conversions"] == 2, after
    got_log = g.census().host()
    assert g.layout() == after
    assert got_log["from_lines"] == 0
    assert_census(got_log, image, "LOG after export")
    assert_census({**got_log, "from_lines": got["from_lines"]}, got, "LOG against INLINE")
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 4. offender list
def _inv_elems(keys, sender, ts_ver, ts_cid, sizes=L.DEFAULT):
    a = np.zeros(len(keys), dtype=L.op_dtype(sizes))
    a["key"] = keys
    a["opcode"] = int(L.Op.INV)
    a["state"] = sender
    a["ts_ver"], a["ts_cid"] = ts_ver, ts_cid
    a["val_len"] = sizes.st_value >> sizes.shift
    a["value"][:] = ord("I")
    return a


def test_census_offender_list():
    g, o, sizes = make_pair(3000, 512, 1 << 18)
    keys = gen_keys(3000)
    pick = np.array([k for k in keys[100:160] if o.lookup(int(k)) is not None][:40], dtype=np.uint64)
    mb = L.membership(3, 0)
    for sender, part in ((1, pick[:25]), (2, pick[25:])):
        inv = _inv_elems(part, sender, 2, sender)
        inv_o = gen.bytecopy(inv)
        g.batch_host(L.BatchType.invs, inv, mb)
        o.batch_multi(L.BatchType.invs, inv_o, 1, len(inv_o), None, mb)
        assert (inv_o["opcode"] == int(L.Resp.INV_SUCCESS)).all()
    want = CM.census_model(*twin_image(o, sizes))
    want_keys = CM.offender_keys(*twin_image(o, sizes))
    k = len(want_keys)
    assert k == len(pick) == 40 and want["offenders"] == k
    assert want["not_valid_by_cid"][1] == 25 and want["not_valid_by_cid"][2] == 15
    # room for all
    buf = torch.full((k + 6,), CANARY, dtype=torch.int64, device="cuda")
    c = g.census(offender_cap=k + 6, offender_keys=buf)
    assert_census(c.host(), want, "cap >= k")
    assert np.array_equal(np.sort(buf[:k].cpu().numpy().view(np.uint64)), want_keys)
    assert (buf[k:].cpu().numpy() == CANARY).all()
    # room for three
    buf = torch.full((8,), CANARY, dtype=torch.int64, device="cuda")
    c = g.census(offender_cap=3, offender_keys=buf)
    assert_census(c.host(), want, "cap 3")
    got = buf.cpu().numpy().view(np.uint64)
    assert len(set(got[:3].tolist())) == 3 and np.isin(got[:3], want_keys).all()
    assert (got[3:] == CANARY).all()
    assert len(c.offenders_host()) == 3
    # no list
    c = g.census()
    assert c.offender_keys is None and c.offenders == k
    assert g.census_host()["offenders"] == k
    assert g.take_error_flags() == 0


# ------------------------------------------------------------------ 5. replica groups
@pytest.mark.parametrize("n_rep", [2, 3])
def test_census_loopback_group(n_rep):
    """After a full round every replica's digest is the same and every key VALID; an INV that only replica 0
    applied shows in its digest and under its sender's cid."""
    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import LoopbackGroup, ReplicaRound, census_row, census_rows_agree
    from hermes_amd.workload import zipf_params
    n_keys, bkts, cap = 4000, 8192, 1 << 20
    z = zipf_params(n_keys, 0.99)
    reps, mirrors = [], []
    for r in range(n_rep):
        g = HermesKV(n_keys, bkts, cap, machine_id=r)
        o = OracleKVS(bkts, cap, r)
        o.populate(n_keys, L.DEFAULT.kvs_value)
        mirrors.append(Mirror(g, o, f"replica {r}"))
        reps.append(ReplicaRound(g, 16, n_rep, r, z, 400, seed=77 + r, trace_len=512))
    grp = LoopbackGroup(reps)
    fresh = mirrors[0].g.census().host()
    for _ in range(2):
        grp.step()
    torch.cuda.synchronize()
    cs = [m.g.census() for m in mirrors]
    hosts = [c.host() for c in cs]
    for r, (m, h) in enumerate(zip(mirrors, hosts)):
        assert_census(h, CM.census_model(*twin_image(m.o, L.DEFAULT)), f"replica {r}")
        assert h["by_state"][int(L.State.VALID)] == h["keys"] > 0 and h["offenders"] == 0
        assert CM.digest(h) == CM.digest(hosts[0]), f"replica {r} against replica 0"
    assert CM.digest(hosts[0]) != CM.digest(fresh) and hosts[0]["max_ts"] > fresh["max_ts"]   # writes happened
    # (the replicas' logs are not equal byte for byte: last-local-write timestamps are each replica's own)
    rows = [[int(x) & CM.M64 for x in census_row(c).cpu().tolist()] for c in cs]
    assert census_rows_agree(rows, range(n_rep)) and [r[3] for r in rows] == [0] * n_rep
    # one more INV launch, from replica 1, that only replica 0 applies
    keys = gen_keys(n_keys)
    pick = np.array([k for k in keys[200:240] if mirrors[0].o.lookup(int(k)) is not None], dtype=np.uint64)
    inv = _inv_elems(pick, 1, (hosts[0]["max_ts"] >> 8) + 2, 1)
    mirrors[0].g.batch_host(L.BatchType.invs, inv, L.membership(n_rep, 0))
    assert (inv["opcode"] == int(L.Resp.INV_SUCCESS)).all()
    c0 = mirrors[0].g.census()
    h0 = c0.host()
    assert_census(h0, CM.census_model(*twin_image(mirrors[0].o, L.DEFAULT)), "replica 0 after the INV")
    assert CM.digest(h0) != CM.digest(hosts[1])
    assert h0["not_valid_by_cid"][1] == len(pick) > 0 and h0["offenders"] == len(pick)
    rows[0] = [int(x) & CM.M64 for x in census_row(c0).cpu().tolist()]
    assert not census_rows_agree(rows, range(n_rep)) and census_rows_agree(rows, range(1, n_rep))
    assert all(m.g.take_error_flags() == 0 for m in mirrors)


def _gloo_child(rank, world, port, q):
    import os

    import torch.distributed as dist

    from hermes_amd.kvs import HermesKV
    from hermes_amd.replica_group import ReplicaGroupRound, group_census
    from hermes_amd.workload import zipf_params
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        n_keys = 4000
        g = HermesKV(n_keys, 8192, 1 << 20, machine_id=rank)
        drv = ReplicaGroupRound(g, 16, zipf_params(n_keys, 0.99), 400, seed=99, world=world, rank=rank, trace_len=512)
        for _ in range(2):
            drv.step()
        res = group_census(g, None, live_ranks=range(world))
        own = g.census().host()
        q.put((rank, res, own, int(g.take_error_flags()), None))
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 -- reported by the parent
        q.put((rank, None, None, 0, repr(e)))


def test_group_census_over_gloo():
    """group_census with two ranks as fresh child processes sharing the GPU over gloo: one all_gather of CUDA
    tensors, the same rows on both ranks, the live ranks agree"""
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
    for rank, out, own, flags, err in res:
        assert err is None, f"rank {rank}: {err}"
        assert flags == 0
        assert out["live_ranks_agree"] and out["live_ranks"] == [0, 1] and out["not_valid"] == [0, 0], out
        assert out["rows"][rank] == [own["digest_sum"], own["digest_xor"], own["keys"], 0]
        assert own["keys"] > 0
    assert res[0][1] == res[1][1]
