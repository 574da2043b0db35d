"""Packed ACK rows launches (k_unique_rows) where the kernel finds each position's batch from a window of the
offsets, every launch mirrored into the oracle (tests/helpers.py's Mirror: elements, read_write_ops, the state
and opcode mirrors, the VAL callbacks' output, index and log).

A case is one local launch whose PUTs all begin a write -- worker w writes `writes[w]` distinct keys at random
slots of its buffer -- and then the two peers' ACKs to those writes as one two-row launch: worker w's batch holds
its writes' positions in random order, some positions on keys nobody wrote or that the table lacks, some with a
timestamp that matches no write, holes (opcode 0) in either row, and `pad[w]` positions that are holes in both
rows. A completion goes to the wrong worker's buffer if the batch is wrong, and the Mirror's comparison of
read_write_ops shows it. The kernel's window is 128 offsets, so a run of empty workers overflows it from 128 on.

The four-position instance takes launches of kRowsWidePositions = 28 * 256 * 32 + 1 positions and more; the test
cannot see which instance ran, so the launches one position above and one below that count are there for both
instances to be mirrored at the sizes where the choice changes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hermes_amd import layout as L  # noqa: E402
from tests import gen  # noqa: E402
from tests import inline_cases as C  # noqa: E402
from tests.helpers import GpuEngine, Mirror  # noqa: E402

INLINE = 1
WIDE = 28 * 256 * 32 + 1   # kRowsWidePositions (hkv_batch.hip)
PUT_OK, PUT_DONE = int(L.Resp.PUT_SUCCESS), int(L.Resp.PUT_COMPLETE)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def engine_path():
    """the multi-kernel engine for every launch (a launch of at most 4096 elements would take k_small)"""
    from hermes_amd import kvs
    kvs.HermesKV.default_flags = kvs.BATCH_ENGINE
    yield
    kvs.HermesKV.default_flags = 0


class TailMirror(Mirror):
    """A Mirror whose device launch covers `tail` elements more than the batches hold (stride past the last
    offset); everything is compared as for the launch without them, the caller checks the tail itself."""
    tail = 0

    def _launch(self, btype, elems, n_batches, total, *a, **k):
        super()._launch(btype, elems, n_batches, total + self.tail, *a, **k)


def make_pair(what, inline, machine_id=0, name="A"):
    from hermes_amd.kvs import HermesKV
    n_keys, bkts, cap = C.GEO[name]
    g = HermesKV(n_keys, bkts, cap, machine_id=machine_id)
    o = C.make_oracle(name, machine_id=machine_id)
    T = C.describe(o, name)
    if inline:
        assert g.prefer_layout(INLINE)
    m = TailMirror(g, o, what, table_check="deferred")
    return g, m, GpuEngine(m, layout=None if inline else False), T


def dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def local_writes(eng, rng, T, W, S, writes):
    """The local launch: W x S ops, worker w's PUTs on writes[w] keys of its own at random slots, GETs on keys
    nobody writes elsewhere. Returns (the workers' buffers after it, the PUT slots, the keys left unused)."""
    sizes = eng.sizes
    writes = np.asarray(writes)
    assert len(writes) == W and writes.max() <= S
    keys = rng.permutation(T.keys[T.present])
    nw = int(writes.sum())
    assert nw + 400 <= len(keys)
    wkeys, gkeys, spare = keys[:nw], keys[nw:nw + 200], keys[nw + 200:]
    loc = np.zeros(W * S, dtype=L.op_dtype(sizes))
    loc["key"] = gkeys[rng.integers(0, len(gkeys), size=W * S)]
    loc["opcode"] = int(L.Op.GET)
    loc["state"] = int(L.Bucket.NEW)
    loc["val_len"] = sizes.st_value >> sizes.shift
    loc["value"] = rng.integers(0, 256, size=(W * S, sizes.st_value))
    slots = np.concatenate([w * S + np.sort(rng.choice(S, int(c), replace=False)) for w, c in enumerate(writes)] or
                           [np.zeros(0, np.int64)]).astype(np.int64)
    loc["key"][slots] = wkeys
    loc["opcode"][slots] = int(L.Op.PUT)
    eng.launch(L.BatchType.local_ops, loc, W, S, L.membership(*eng.memb), inline=True)
    assert (loc["state"][slots] == PUT_OK).all(), "every PUT must have begun a write"
    return loc, slots, spare


def ack_rows(rng, loc, slots, spare, W, S, senders, pad, tail, noise=0.1, holes=0.12, stale=0.08):
    """The two rows' ACKs (see the module's text). Returns (elems, offsets, total, row_stride, clean): clean marks
    the write slots whose position has both ACKs and the right timestamp."""
    pad = np.asarray(pad)
    parts, clean = [], np.zeros(len(loc), bool)
    spare = list(spare)
    for w in range(W):
        mine = slots[slots // S == w]
        mine = mine[rng.permutation(len(mine))]
        n_noise = int(rng.binomial(len(mine), noise)) if len(mine) else 0
        a = np.zeros((2, len(mine) + n_noise + int(pad[w])), dtype=L.msg_dtype())
        order = rng.permutation(a.shape[1])
        pw, pn = order[:len(mine)], order[len(mine):len(mine) + n_noise]
        for r in range(2):
            a[r]["key"][pw] = loc["key"][mine]
            a[r]["ts_ver"][pw] = loc["ts_ver"][mine]
            a[r]["ts_cid"][pw] = loc["ts_cid"][mine]
            a[r]["opcode"][pw] = int(L.Op.ACK)
            a[r]["sender"][pw] = senders[r]
        old = rng.random(len(mine)) < stale          # an ACK of an older write: no completion
        a[0]["ts_ver"][pw[old]] -= 2
        a[1]["ts_ver"][pw[old]] -= 2
        for j in pn:                                 # a key nobody wrote, or one the table lacks
            k = spare.pop() if rng.random() < 0.7 else np.uint64(rng.integers(1, 2**62))
            for r in range(2):
                a[r]["key"][j], a[r]["opcode"][j], a[r]["sender"][j] = k, int(L.Op.ACK), senders[r]
                a[r]["ts_ver"][j], a[r]["ts_cid"][j] = 2, rng.integers(0, 3)
        hole = rng.random((2, a.shape[1])) < holes
        hole[:, order[len(mine) + n_noise:]] = False
        for r in range(2):
            a[r]["opcode"][hole[r]] = 0
        ok = np.zeros(a.shape[1], bool)
        ok[pw] = ~old
        ok &= ~hole.any(axis=0)
        clean[mine] = ok[pw]
        parts.append(a)
    counts = np.array([p.shape[1] for p in parts], np.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(off[-1]) + tail
    row_stride = total + 5
    elems = np.zeros(row_stride + total, dtype=L.msg_dtype())
    for r in range(2):
        row = C.cat([p[r] for p in parts]) if parts else np.zeros(0, L.msg_dtype())
        elems[r * row_stride:r * row_stride + len(row)] = row
        # positions past the last offset hold what would be elements: they are in no batch
        elems[r * row_stride + len(row):r * row_stride + total] = row[:tail] if len(row) >= tail else 0
    return elems, off, total, row_stride, clean


def launch_rows(m, elems, W, total, mb, off, loc, S, rows, mirrors, inline):
    """GpuEngine.launch for an ACK rows launch, with or without the state and opcode mirrors"""
    t, rw = dev(elems), dev(loc)
    kw = {"offsets": torch.from_numpy(np.ascontiguousarray(off, np.int32)).cuda(), "rw": rw,
          "rw_stride_bytes": S * loc.dtype.itemsize,
          "ack_out": torch.zeros((rows[1] + total) * 16, dtype=torch.uint8, device="cuda")}
    if mirrors:
        kw["rw_state"] = torch.from_numpy(loc["state"].copy()).cuda()
        kw["rw_opcodes"] = torch.from_numpy(loc["opcode"].copy()).cuda()
    m.expect_inline = inline
    m.batch(L.BatchType.acks, t, W, total, 16, mb, unique=True, rows=rows, **kw)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    if rows[2] >= 0:
        lo, hi = rows[2] * rows[1] * 16, (rows[2] * rows[1] + total) * 16
        assert np.array_equal(got[lo:hi], elems.view(np.uint8).reshape(-1)[lo:hi]), "the skip row was written"
    elems.view(np.uint8).reshape(-1)[:] = got
    loc.view(np.uint8).reshape(-1)[:] = rw.cpu().numpy()


def shape(kind, rng):
    """(W, S, writes per worker, pad per worker, positions past the last offset)"""
    z = np.zeros
    if kind == "empty_run":        # 140 empty workers in the middle: the window of 128 offsets ends inside the run
        w = rng.integers(1, 7, size=400)
        w[130:270] = 0
        return 400, 8, w, z(400, int), 3
    if kind == "long_batch":       # 150 writes of one worker: blocks of 32 and of 64 positions strictly inside it
        return 8, 200, np.array([3, 0, 9, 150, 1, 0, 40, 2]), z(8, int), 3
    if kind == "edges_empty":      # first and last worker empty
        w = rng.integers(1, 30, size=70)
        w[0] = w[-1] = 0
        return 70, 32, w, z(70, int), 0
    if kind == "one_worker":
        return 1, 250, np.array([100]), z(1, int), 2
    if kind == "many_workers":     # two narrowing steps (more than 4096 batches), most workers empty
        w = (rng.random(5000) < 0.2) * rng.integers(1, 4, size=5000)
        return 5000, 4, w, z(5000, int), 1
    raise KeyError(kind)


def run_case(what, W, S, writes, pad, tail, skip=-1, mirrors=True, inline=True, seed=7, exact_total=None,
             noise=0.1, holes=0.12, stale=0.08):
    rng = np.random.default_rng(seed)
    machines, me, senders = C.rows_setup(2, skip)
    g, m, eng, T = make_pair(what, inline, machine_id=me)
    eng.memb = (machines, me)
    mb = L.membership(machines, me)
    loc, slots, spare = local_writes(eng, rng, T, W, S, writes)
    elems, off, total, row_stride, clean = ack_rows(rng, loc, slots, spare, W, S, senders, pad, tail, noise, holes, stale)
    if exact_total is not None:
        assert total == exact_total, (total, exact_total)
    before = loc["state"].copy()
    launch_rows(m, elems, W, total, mb, off, loc, S, (2, row_stride, skip), mirrors, inline)
    m.check_table(what)
    assert g.take_error_flags() == 0
    done = loc["state"] != before
    if skip < 0:   # both peers' ACKs complete a write; with a skip row the one row that runs is the only peer's
        assert np.array_equal(done, clean) and (loc["state"][done] == PUT_DONE).all()
    else:
        assert done.sum() > 0 or not clean.any()
    return loc, done


@pytest.mark.parametrize("inline", [True, False])
@pytest.mark.parametrize("mirrors", [True, False])
@pytest.mark.parametrize("kind", ["empty_run", "long_batch", "edges_empty", "one_worker", "many_workers"])
def test_ack_rows_shapes(kind, mirrors, inline):
    rng = np.random.default_rng(11)
    W, S, writes, pad, tail = shape(kind, rng)
    loc, done = run_case(f"{kind} {mirrors} {inline}", W, S, writes, pad, tail, mirrors=mirrors, inline=inline)
    assert done.sum() > 0
    if kind == "empty_run":   # completions on both sides of the run
        assert done[:130 * S].any() and done[270 * S:].any()


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("kind", ["empty_run", "long_batch"])
def test_ack_rows_skip_row(kind, skip):
    rng = np.random.default_rng(13)
    W, S, writes, pad, tail = shape(kind, rng)
    run_case(f"{kind} skip {skip}", W, S, writes, pad, tail, skip=skip, seed=17 + skip)


@pytest.mark.parametrize("total", [1, 63, 64, 65, 1003])
def test_ack_rows_totals(total):
    """exactly `total` positions, every one a write's (no noise), in 5 workers; holes and old timestamps stay"""
    rng = np.random.default_rng(total)
    writes = np.bincount(rng.integers(0, 5, size=total), minlength=5)
    run_case(f"total {total}", 5, 250, writes, np.zeros(5, int), 0, exact_total=total, noise=0.0, seed=total)


def test_ack_rows_no_completion():
    """every ACK carries an older timestamp: nothing completes, read_write_ops stay as they are"""
    rng = np.random.default_rng(19)
    W, S, writes, pad, tail = shape("edges_empty", rng)
    loc, done = run_case("stale", W, S, writes, pad, tail, stale=1.0)
    assert done.sum() == 0


@pytest.mark.parametrize("inline,mirrors", [(True, True), (False, False)])
@pytest.mark.parametrize("delta", [1, -1])
def test_ack_rows_around_the_wide_instance(delta, inline, mirrors):
    """kRowsWidePositions + 1 positions (the four-position instance) and kRowsWidePositions - 1 (the two-position
    one): 5000 workers of at most 4 writes, 200 of them empty in a row, the positions filled up with holes in both
    rows (the oracle replays the 1,700 or so real ACKs of each row), one batch of 3,000 positions among them."""
    rng = np.random.default_rng(23)
    W, S = 5000, 4
    writes = (rng.random(W) < 0.15) * rng.integers(1, 5, size=W)
    writes[2000:2200] = 0
    want = WIDE + delta - 2   # two positions past the last offset
    pad = np.zeros(W, int)
    busy = np.nonzero(writes)[0]
    pad[busy[7]] = 3000
    # the rest spread over the busy workers; the noise positions are fixed first, so no noise here
    rest = want - int(writes.sum()) - 3000
    pad[busy] += np.bincount(rng.integers(0, len(busy), size=rest), minlength=len(busy))
    loc, done = run_case(f"wide {delta} {inline}", W, S, writes, pad, 2, mirrors=mirrors, inline=inline,
                         exact_total=WIDE + delta, noise=0.0)
    assert done[:2000 * S].any() and done[2200 * S:].any()


@pytest.mark.parametrize("inline", [True, False])
def test_packed_invs_end_before_the_stride(inline):
    """k_unique_lds: packed offsets whose total is 37 below the launch's stride. The elements past the last offset
    are INVs with newer timestamps on keys of their own: applied, they would change the table and themselves, and
    their ACKs would be written."""
    rng = np.random.default_rng(29)
    g, m, eng, T = make_pair(f"inv tail {inline}", inline)
    tsp = gen.TsPool(rng)
    n, tail, W = 1000, 37, 8
    keys = rng.permutation(T.keys[T.present])[:n + tail]
    a = gen.invs(rng, keys, n + tail, eng.sizes, False, tsp, machine_num=3)
    a["key"] = keys
    a["opcode"] = int(L.Op.INV)
    a["state"] = 1
    a["ts_ver"][n:] = 1000
    esz = a.dtype.itemsize
    off = np.concatenate([[0], np.cumsum(C.split_counts(rng, n, W))]).astype(np.int32)
    t = dev(a)
    acks = torch.full(((n + tail) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    m.tail = tail
    m.expect_inline = inline
    m.batch(L.BatchType.invs, t, W, n, esz, L.membership(3, 0), unique=True, ack_out=acks,
            offsets=torch.from_numpy(off).cuda())
    m.tail = 0
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy()[n * esz:], a.view(np.uint8).reshape(-1)[n * esz:]), "the tail was written"
    assert (acks.cpu().numpy()[n * 16:] == 0xEE).all(), "ACKs were written for the tail"
    m.check_table("inv tail")
    assert g.take_error_flags() == 0
