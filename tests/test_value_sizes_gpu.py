"""Big-object value sizes other than 287 bytes on the device, bit for bit against the oracle.

hkv_table_create accepts big objects of 1 to 16 extra cache lines (ECL); every other GPU test runs the default
geometry or ECL 4. Every other size runs the kernels' general value class (BatchPlan::sv == 0), and within it
values above 320 bytes take other branches than values below (per-lane value copies, k_apply_patch, an LDS slab
above 64 KiB). Five sizes, each the smallest witness of a branch:

  ECL  st_value / entry / op
   1     95 /  128 /  120   power-of-two entry (no entry straddles the log's wrap), wave value copies, 2 chunks
   2    159 /  192 /  184   an entry that straddles the wrap, 3 chunks (the install's tail of two runs)
   5    351 /  384 /  376   first size past 320 B: per-lane value copies, k_apply_patch, 6 chunks
   8    543 /  576 /  568   first k_resolve0 slab past 64 KiB (72,704 B), value past 496 B, 9 chunks
  16   1055 / 1088 / 1080   the largest: 138,240-B slab, val_len 131, 17 chunks, an entry of more than 1024 B

The bodies are those of tests/test_gpu_parity.py (which compares elements, read_write_ops, node_suspected and
the whole index and log after every launch), tests/test_census_gpu.py and tests/test_repair_gpu.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from oracle.oracle import gen_keys  # noqa: E402
from tests import census_model as CM  # noqa: E402
from tests import gen  # noqa: E402
from tests import repair_cases as RC  # noqa: E402
from tests import repair_model as RM  # noqa: E402
from tests import test_gpu_parity as P  # noqa: E402
from tests.test_repair_gpu import assert_extract  # noqa: E402

ECLS = [1, 2, 5, 8, 16]
LOG, INLINE = 0, 1


def _ecl_id(e):
    return f"ecl{e:02d}"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(params=["engine", "small"])
def engine_path(request):
    """as tests/test_gpu_parity.py: the multi-kernel engine, and the single-workgroup kernel that launches of at
    most 4096 elements then take"""
    from hermes_amd import kvs
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE if request.param == "engine" else kvs.BATCH_SMALL
    yield request.param
    kvs.HermesKV.default_flags = 0


# ------------------------------------------------------------------ populate
@pytest.mark.parametrize("ecl", ECLS, ids=_ecl_id)
def test_populate_bit_exact(ecl):
    """2560 keys in 256 buckets (10 per bucket: evictions) and a log of between a third and a half of their entries,
    so it wraps twice: the first lap ends with the reference's skip to the capacity, the second runs on across it"""
    sizes = L.Sizes(True, ecl)
    n, bkts = 2560, 256
    cap = 1 << ((n * sizes.entry).bit_length() - 2)
    assert 2 * cap <= n * sizes.entry < 4 * cap
    g, o, _ = P.make_pair(n, bkts, cap, rmw=True, ecl=ecl)
    P.assert_tables_equal(g, o, "populate")
    assert g.evictions == o.evictions() > 0
    assert g.log_head == o.log_head() > 2 * cap
    offs = [o.lookup(int(k)) for k in gen_keys(n)]
    live = [x for x in offs if x is not None]
    assert 0 < len(live) < n
    straddles = sum(x + sizes.entry > cap for x in live)
    if cap % sizes.entry:
        assert straddles >= 1, "no live entry runs across the capacity"
        x = max(live)
        assert np.array_equal(g.log_bytes(0, cap + sizes.entry)[x:x + sizes.entry], CM.oracle_image(o, sizes)[1][x:x + sizes.entry])
    else:
        assert straddles == 0 and sizes.entry == 128


# ------------------------------------------------------------------ randomized protocol rounds
class _Outcomes:
    """what makes a run of random_protocol_rounds non-vacuous at a value size: values that travelled"""

    def __init__(self, sizes):
        self.sizes = sizes
        self.written = set()       # values of PUTs that succeeded and of INVs that raised (random bytes)
        self.read_back = 0         # GET_COMPLETEs that returned one of them
        self.raised = 0            # INV_SUCCESSes whose value and timestamp the entry now holds
        self.codes = set()

    def __call__(self, kind, elems, o):
        if kind == "local":
            st = elems["state"]
            self.codes |= {("local", int(x)) for x in np.unique(st)}
            for v in elems["value"][st == int(L.Resp.GET_COMPLETE)]:
                self.read_back += v.tobytes() in self.written
            for v in elems["value"][np.isin(st, [int(L.Resp.PUT_SUCCESS), int(L.Resp.RMW_SUCCESS)])]:
                self.written.add(v.tobytes())
        elif kind == "invs":
            self.codes |= {("invs", int(x)) for x in np.unique(elems["opcode"])}
            log = o.log_bytes()
            ok = (elems["opcode"] == int(L.Resp.INV_SUCCESS)) & (elems["state"] != int(L.Resp.MISS))
            for e in elems[ok]:
                off = o.lookup(int(e["key"]))
                if off is None or off + self.sizes.entry > len(log):
                    continue
                ent = log[off:off + self.sizes.entry].view(L.entry_dtype(self.sizes))[0]
                if (int(ent["ts_ver"]), int(ent["ts_cid"])) == (int(e["ts_ver"]), int(e["ts_cid"])) and \
                        np.array_equal(ent["value"], e["value"]):
                    self.raised += 1
                    self.written.add(e["value"].tobytes())
        else:
            self.codes |= {("acks", int(x)) for x in np.unique(elems["opcode"])}


@pytest.mark.parametrize("rmw", [False, True], ids=["plain", "rmw"])
@pytest.mark.parametrize("ecl", ECLS, ids=_ecl_id)
def test_random_protocol_rounds(engine_path, ecl, rmw):
    """test_gpu_parity.test_random_protocol_rounds' body: local ops, INVs with node_suspected, ACKs with
    read_write_ops, VALs and the after-membership batch, packed and ragged launches alternating, elements and the
    whole table compared after every launch. Without RMWs INV launches take k_inv_resolve / k_inv_commit<0> and ACK
    launches k_ack_resolve; with them INV launches take k_resolve0<kInvs, 0, 128> (the LDS slab) and local and ACK
    launches k_resolve0_direct<*, 0>."""
    seen = _Outcomes(L.Sizes(True, ecl))
    P.random_protocol_rounds(rmw, True, ecl=ecl, observe=seen)
    assert seen.read_back > 0, "no GET returned a value an earlier PUT or INV of this run wrote"
    assert seen.raised > 0, "no INV raised its key"
    assert ("local", int(L.Resp.PUT_SUCCESS)) in seen.codes and ("local", int(L.Resp.GET_COMPLETE)) in seen.codes
    if rmw:
        assert ("local", int(L.Resp.RMW_SUCCESS)) in seen.codes
        assert ("local", int(L.Resp.RMW_ABORT)) in seen.codes or ("invs", int(L.Resp.OP_INV_ABORT)) in seen.codes


@pytest.mark.parametrize("rmw", [False, True], ids=["plain", "rmw"])
@pytest.mark.parametrize("ecl", [1, 16], ids=_ecl_id)
def test_max_size_batches_single_hot_key(engine_path, ecl, rmw):
    """maximum batch sizes on one or two keys: the rounds after round 0 (k_cand, k_resolve<*, 0>), k_commit<0> and
    the fallback k_fb_exec<*, 0>"""
    P.max_size_batches_single_hot_key(rmw, True, ecl=ecl)


@pytest.mark.parametrize("ecl", [1, 5, 16], ids=_ecl_id)
def test_scripted_rare_outcomes(engine_path, ecl):
    """tests/scripted.py with RMWs: every outcome code of the build (required_outcomes) produced at the size"""
    P.scripted_rare_outcomes(True, True, ecl=ecl)


# ------------------------------------------------------------------ unique launches
@pytest.mark.parametrize("rmw", [False, True], ids=["plain", "rmw"])
@pytest.mark.parametrize("ecl", [1, 8], ids=_ecl_id)
def test_unique_inv_launch_matches_oracle(engine_path, ecl, rmw):
    """HKV_BATCH_UNIQUE INV launches in place (k_unique<kInvs, 0, 1>: the LDS-staged passes are for 64-B and 320-B
    entries), and the duplicate-key check (error flag bit 4) on the engine path"""
    P.unique_inv_launch_matches_oracle(engine_path, rmw, True, ecl=ecl)


@pytest.mark.parametrize("rmw", [False, True], ids=["plain", "rmw"])
@pytest.mark.parametrize("ecl", [1, 8], ids=_ecl_id)
def test_unique_ack_launch_matches_oracle(engine_path, ecl, rmw):
    """HKV_BATCH_UNIQUE ACK launches (k_unique<kAcks, 0, 1>): two machines, so the one peer's ACK is a write's last.
    Each worker's ACK batch holds one ACK per key -- for the writes its own local batch just issued (matching:
    LAST_ACK_SUCCESS, the read_write_ops slot completes) and for other keys at a timestamp nobody wrote (not
    matching) -- no key twice in the launch, ragged counts, read_write_ops = the local buffers."""
    rng = np.random.default_rng(99 + ecl)
    sizes = L.Sizes(True, ecl)
    n_keys = 2000
    g, o, _ = P.make_pair(n_keys, 1024, 1 << (n_keys * sizes.entry + 1024).bit_length(), rmw=rmw, ecl=ecl)
    keys = gen_keys(n_keys)
    tsp = gen.TsPool(rng)
    mb = L.membership(2, 0)
    W, S = 8, 250
    completed = 0
    for rnd in range(3):
        loc = gen.local_ops(rng, gen.key_pool(rng, keys, hot=600), W * S, sizes, rmw, tsp)
        loc["state"] = int(L.Bucket.NEW)
        loc_o = gen.bytecopy(loc)
        P._run_both(g, o, L.BatchType.local_ops, loc, loc_o, mb, W, S, None)
        P.assert_elems_equal(loc, loc_o, f"round {rnd} local")
        ack = np.zeros(W * S, dtype=L.op_dtype(sizes) if rmw else L.msg_dtype())
        sender = "state" if rmw else "sender"
        counts = np.zeros(W, np.int32)
        used = set()
        wrote = np.isin(loc["state"], [int(L.Resp.PUT_SUCCESS), int(L.Resp.RMW_SUCCESS)])
        n_match = 0
        for w in range(W):
            j = w * S
            for i in range(w * S, (w + 1) * S):
                k = int(loc["key"][i])
                if k in used or not (wrote[i] or rng.random() < 0.3):
                    continue
                used.add(k)
                ack[j]["key"], ack[j]["opcode"], ack[j][sender] = k, int(L.Op.ACK), 1
                ack[j]["ts_cid"] = loc["ts_cid"][i] if wrote[i] else 1
                ack[j]["ts_ver"] = loc["ts_ver"][i] if wrote[i] else 1000 + 2 * rnd
                n_match += bool(wrote[i])
                j += 1
            counts[w] = j - w * S
        assert n_match > 50 and counts.sum() > n_match + 50
        if rmw:
            ack["value"] = rng.integers(0, 256, size=ack["value"].shape)
        ack_o = gen.bytecopy(ack)
        rw_g, rw_o = gen.bytecopy(loc), gen.bytecopy(loc)
        g.batch_host(L.BatchType.acks, ack, mb, rw=rw_g, n_batches=W, stride=S, counts=counts, rw_stride_elems=S,
                     unique=True)
        o.batch_multi(L.BatchType.acks, ack_o, W, S, counts, mb, rw=rw_o, rw_stride_elems=S)
        P.assert_elems_equal(ack, ack_o, f"round {rnd} unique acks")
        P.assert_elems_equal(rw_g, rw_o, f"round {rnd} unique acks rw")
        P.assert_tables_equal(g, o, f"round {rnd} unique acks")
        live = (np.arange(S)[None, :] < counts[:, None]).reshape(-1)
        assert (ack["opcode"][live] == int(L.Resp.LAST_ACK_SUCCESS)).sum() >= n_match // 2
        completed += int((rw_g["state"] != loc["state"]).sum())
        # the peer's VALs bring nothing here: the completed keys are VALID again for the next round
    assert completed > 100


# ------------------------------------------------------------------ the INV and ACK direct paths
@pytest.mark.parametrize("ecl", [2, 8], ids=_ecl_id)
def test_inv_direct_path_edge_cases(engine_path, ecl):
    """k_inv_resolve / k_inv_commit<0>: 10 batches of 900 (9000 elements, past the 8192-element lookup head)"""
    P.inv_direct_path_edge_cases(True, ecl=ecl, W=10, rounds=3)


@pytest.mark.parametrize("ecl", [2, 8], ids=_ecl_id)
def test_ack_direct_path_edge_cases(engine_path, ecl):
    P.ack_direct_path_edge_cases(True, ecl=ecl, W=6, rounds=4)


# ------------------------------------------------------------------ census, extract, install
@pytest.mark.parametrize("ecl", ECLS, ids=_ecl_id)
def test_census_extract_install(engine_path, ecl):
    """A LOG table of 1500 keys two random protocol rounds in (several states and writers), against
    tests/census_model.py and tests/repair_model.py: the census with its offender list, an extract of everything
    and of a bucket sub-range above a timestamp, and the install of its records into a table of another bucket
    count and capacity -- after INV launches moved some keys ahead on the source and others on the target, so
    records raise, equal and lose -- which then holds the model's digest."""
    n_keys = 1500
    g, o, sizes = P.random_protocol_rounds(False, True, ecl=ecl, rounds=2, n_keys=n_keys)
    keys = gen_keys(n_keys)
    ahead_src, ahead_dst = np.arange(700, 800), np.arange(900, 1000)
    mb = L.membership(5, 0)
    inv = RC.invs(keys, ahead_src, 1, (40, 1), sizes, 11)
    inv_o = gen.bytecopy(inv)
    g.batch_host(L.BatchType.invs, inv, mb)
    o.batch_multi(L.BatchType.invs, inv_o, 1, len(inv_o), None, mb)
    P.assert_elems_equal(inv, inv_o, "source INVs")
    image = CM.oracle_image(o, sizes)
    assert g.layout()["state"] == LOG
    # census
    want = CM.census_model(*image)
    CM.assert_not_vacuous([want])
    k = want["offenders"]
    assert k > 100
    buf = torch.full((k + 4,), -1, dtype=torch.int64, device="cuda")
    c = g.census(offender_cap=k + 4, offender_keys=buf)
    got = c.host()
    for f in CM.FIELDS:
        assert got[f] == want[f], f"census {f}: device {got[f]} != model {want[f]}"
    assert np.array_equal(np.sort(c.offenders_host()), CM.offender_keys(*image))
    assert (buf[k:].cpu().numpy() == -1).all()
    # extract: everything, and buckets [100, 357) from (2, 0) on
    x = g.extract()
    records = RM.extract_model(image)
    assert_extract(x, records, RM.scanned_model(image), sizes, "whole")
    assert len(records) == want["keys"] and records.shape[1] == sizes.entry
    t = (2 << 8) | 0
    part = RM.extract_model(image, 100, 357, min_ts=t)
    assert 0 < len(part) < RM.scanned_model(image, 100, 357)
    assert_extract(g.extract((100, 357), min_ts=t, cap=n_keys), part, RM.scanned_model(image, 100, 357), sizes, "sub-range")
    # install into another geometry
    cap2 = 1 << ((n_keys * sizes.entry).bit_length() + 1)
    assert cap2 != g.cfg.log_cap
    h, ho, _ = P.make_pair(n_keys, 256, cap2, machine_id=2, ecl=ecl)
    mb2 = L.membership(5, 2)
    inv = RC.invs(keys, ahead_dst, 3, (60, 3), sizes, 13)
    inv_o = gen.bytecopy(inv)
    h.batch_host(L.BatchType.invs, inv, mb2)
    ho.batch_multi(L.BatchType.invs, inv_o, 1, len(inv_o), None, mb2)
    P.assert_elems_equal(inv, inv_o, "target INVs")
    counts = RM.install_counts(ho, records, sizes)
    assert counts["raised"] >= 100 and counts["equal"] > 0 and counts["older"] > 50, counts
    res = h.install(x, n=len(records))
    RM.apply_records(ho, records, sizes, mb2)
    assert res.host() == counts
    P.assert_tables_equal(h, ho, "install")
    model = CM.census_model(*CM.oracle_image(ho, sizes))
    got = h.census().host()
    assert CM.digest(got) == CM.digest(model) and got == model
    assert g.take_error_flags() == 0 and h.take_error_flags() == 0


# ------------------------------------------------------------------ refusals
def test_refusals():
    """No kernel runs: big objects of 0 or 17 extra cache lines make no table; d_ack_out on a unique INV launch of a
    table of another size than 64-B or 320-B entries is an error that leaves elements and table as they were; the
    inline layout is as unavailable as it is to a 320-B table."""
    from hermes_amd import kvs, lib
    from hermes_amd.kvs import HermesKV
    r = lib.raw()
    for ecl in (0, 17):
        cfg = kvs.make_config(100, 256, 1 << 20, big_objects=True, extra_cache_lines=ecl)
        h = ctypes.c_void_p()
        rc = r.hkv_table_create(ctypes.byref(cfg), ctypes.byref(h))
        assert rc < 0 and not h.value and b"extra_cache_lines" in r.hkv_last_error()
        with pytest.raises(lib.HkvError):
            HermesKV(100, 256, 1 << 20, big_objects=True, extra_cache_lines=ecl)
    tables = {ecl: HermesKV(500, 256, 1 << 20, big_objects=True, extra_cache_lines=ecl) for ecl in (1, 4, 8)}
    g = tables[1]
    sizes = g.sizes
    before = (g.index_bytes(), g.log_bytes())
    inv = RC.invs(gen_keys(500), np.arange(64), 1, (4, 1), sizes, 3)
    elems = torch.from_numpy(inv.view(np.uint8).reshape(-1).copy()).cuda()
    ack_out = torch.full((64 * sizes.op,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.HkvError, match="d_ack_out"):
        g.batch(L.BatchType.invs, elems, 1, 64, sizes.op, L.membership(3, 0), unique=True, ack_out=ack_out,
                ack_out_size=sizes.op)
    torch.cuda.synchronize()
    assert np.array_equal(elems.cpu().numpy(), inv.view(np.uint8).reshape(-1)) and (ack_out.cpu().numpy() == 0x5A).all()
    assert np.array_equal(g.index_bytes(), before[0]) and np.array_equal(g.log_bytes(), before[1])
    # the inline layout: whatever a 320-B table answers, the other sizes answer
    answers = {}
    for ecl, t in tables.items():
        img = (t.index_bytes(), t.log_bytes())
        a = [t.prefer_layout(INLINE)]
        try:
            t.apply_layout()
            a.append("applied")
        except lib.HkvError:
            a.append("refused")
        lay = t.layout()
        a += [lay["state"], lay["eligible"], lay["conversions"]]
        answers[ecl] = a
        assert lay["state"] == LOG and lay["conversions"] == 0 and not lay["eligible"]
        assert np.array_equal(t.index_bytes(), img[0]) and np.array_equal(t.log_bytes(), img[1])
        t.prefer_layout(LOG)
    assert answers[1] == answers[4] == answers[8] and answers[4][0] is False
    assert all(t.take_error_flags() == 0 for t in tables.values())
