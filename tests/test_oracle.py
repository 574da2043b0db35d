"""Pins the CPU restatement (oracle/) before it is trusted as the parity checker.

1. CityHash128 against vectors produced by the reference's own city.c (tests/golden/cityhash_ref.json,
   made by tools/make_golden.py from oracle/_ref), and live against oracle/_ref when it is built.
2. hermes_batch_ops_to_KVS semantics against the reference outputs recorded in SURVEY.md section 4
   (tests/golden/known_answers.json).
"""
import numpy as np
import pytest

from hermes_amd import layout as L
from oracle import oracle as O
from tests.helpers import load_golden, run_known_answers


def test_cityhash_matches_reference_vectors():
    g = load_golden("cityhash_ref.json")
    for v in g["key_ids_le32"]:
        f, s = O.cityhash128(int(v["id"]).to_bytes(4, "little"))
        assert (f, s) == (int(v["first"]), int(v["second"])), v["id"]
    for v in g["short_strings"]:
        f, s = O.cityhash128(bytes.fromhex(v["hex"]))
        assert (f, s) == (int(v["first"]), int(v["second"])), v["hex"]


def test_cityhash_live_reference_when_built():
    r = O.reference_cityhash128(b"\x05\x00\x00\x00")
    if r is None:
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    rng = np.random.default_rng(1)
    for i in rng.integers(0, 2**31, size=2000):
        b = int(i).to_bytes(4, "little")
        assert O.cityhash128(b) == O.reference_cityhash128(b)


def test_gen_keys_matches_scalar():
    keys = O.gen_keys(1000)
    for i in (0, 1, 5, 999):
        assert keys[i] == O.cityhash128(i.to_bytes(4, "little"))[1]


class _OracleEngine:
    def __init__(self, kv):
        self.kv = kv

    def batch(self, btype, elems, mb, rw=None):
        self.kv.batch(btype, elems, mb, rw=rw)

    def entry(self, key):
        off = self.kv.lookup(int(key))
        assert off is not None
        return self.kv.log_bytes()[off:off + L.DEFAULT.entry].view(L.entry_dtype())[0]


@pytest.fixture(scope="module")
def table_1m():
    ka = load_golden("known_answers.json")["config"]
    kv = O.OracleKVS(ka["num_bkts"], ka["log_cap"], machine_id=ka["machine_id"])
    kv.populate(ka["num_keys"], ka["val_len"])
    return kv, O.gen_keys(ka["num_keys"])


def test_known_answers(table_1m):
    kv, keys = table_1m
    run_known_answers(_OracleEngine(kv), keys)


def test_exactly_three_misses_at_1m():
    ka = load_golden("known_answers.json")
    c = ka["config"]
    kv = O.OracleKVS(c["num_bkts"], c["log_cap"])
    kv.populate(c["num_keys"], c["val_len"])
    keys = O.gen_keys(c["num_keys"])
    ops = np.zeros(c["num_keys"], dtype=L.op_dtype())
    ops["key"] = keys
    ops["opcode"] = int(L.Op.GET)
    ops["state"] = int(L.Bucket.NEW)
    for b in range(0, len(ops), 250):
        kv.batch(L.BatchType.local_ops, ops[b:b + 250], L.membership(3, 0))
    miss = np.nonzero(ops["state"] == int(L.Resp.MISS))[0].tolist()
    assert miss == ka["always_miss_ids"]
    assert (ops["state"][ops["state"] != int(L.Resp.MISS)] == int(L.Resp.GET_COMPLETE)).all()
    # value = 'a' + id % 20 (spacetime.c:58), val_len 30 after populate
    ok = ops["state"] == int(L.Resp.GET_COMPLETE)
    ids = np.arange(c["num_keys"])
    assert (ops["value"][ok, 0] == (ord("a") + ids[ok] % 20)).all()
    assert (ops["val_len"][ok] == 30).all()


def test_big_object_val_len_quirks():
    """SURVEY 7 bit-exact quirks: uint8 val_len arithmetic with SHIFT_BITS 3 (spacetime.h:263-273)."""
    kv = O.OracleKVS(1 << 12, 1 << 24, big_objects=True, extra_cache_lines=4, rmw=True)
    sz = L.BIG
    kv.populate(1000, sz.kvs_value)
    keys = O.gen_keys(1000)
    ops = np.zeros(2, dtype=L.op_dtype(sz))
    ops["key"] = keys[[3, 4]]
    ops["opcode"] = int(L.Op.GET)
    ops["state"] = int(L.Bucket.NEW)
    kv.batch(L.BatchType.local_ops, ops, L.membership(3, 0))
    assert (ops["state"] == int(L.Resp.GET_COMPLETE)).all()
    assert (ops["val_len"] == 244).all()


# KVS_VALUE_SIZE = EXTRA_CACHE_LINES * 64 + 46 (hrd.h:36-47), ST_VALUE_SIZE = KVS_VALUE_SIZE - 15 (spacetime.h:29,
# the 15-byte spacetime_object_meta), sizeof(struct mica_op) = 16 + 1 + 1 + KVS_VALUE_SIZE and sizeof(spacetime_op_t)
# = 16 + 2 + ST_VALUE_SIZE (spacetime.h:170-185), both rounded up to their 8-byte alignment; worked out by hand
VALUE_SIZES = {  # ecl: (kvs_value, st_value, entry, op)
    1: (110, 95, 128, 120),
    2: (174, 159, 192, 184),
    5: (366, 351, 384, 376),
    8: (558, 543, 576, 568),
    16: (1070, 1055, 1088, 1080),
}
# The val_len bytes, all uint8 arithmetic with SHIFT_BITS 3, by hand per size:
#   carried   what an op or INV carries and a replay writes into the op: ST_VALUE_SIZE >> 3 (hermesKV.c:20, 151)
#   populated entry byte 17 after spacetime_populate_fixed_len(KVS_VALUE_SIZE): KVS_VALUE_SIZE >> 3 (spacetime.c:48)
#   get_pop   op byte 10 after a GET of a populated key: (populated >> 3) - 16 (get_val_len, spacetime.h:263-267)
#   put       entry byte 17 after a PUT: (carried >> 3) + 16 (set_val_len, spacetime.h:269-273; hermesKV.c:113)
#   get_put   op byte 10 after a GET of that key: (put >> 3) - 16
#   inv       entry byte 17 after a raising INV: (uint8_t) KVS_VALUE_SIZE (hermesKV.c:548)
#   get_inv   op byte 10 after a GET of that key, validated: (inv >> 3) - 16
VAL_LEN = {  # ecl: (carried, populated, get_pop, put, get_put, inv, get_inv)
    1: (11, 13, 241, 17, 242, 110, 253),        # 95>>3; 110>>3; 1-16; 1+16; 2-16; 110; 13-16
    2: (19, 21, 242, 18, 242, 174, 5),          # 159>>3; 174>>3; 2-16; 2+16; 2-16; 174; 21-16
    5: (43, 45, 245, 21, 242, 110, 253),        # 351>>3; 366>>3; 5-16; 5+16; 2-16; 366-256; 13-16
    8: (67, 69, 248, 24, 243, 46, 245),         # 543>>3; 558>>3; 8-16; 8+16; 3-16; 558-512; 5-16
    16: (131, 133, 0, 32, 244, 46, 245),        # 1055>>3; 1070>>3; 16-16; 16+16; 4-16; 1070-1024; 5-16
}


@pytest.mark.parametrize("ecl", sorted(VALUE_SIZES))
def test_value_size_derived_sizes(ecl):
    """Sizes and the oracle's hko_*_size at the five big-object sizes the GPU suite runs, against literals"""
    import ctypes
    kvs_value, st_value, entry, op = VALUE_SIZES[ecl]
    sz = L.Sizes(True, ecl)
    assert (sz.kvs_value, sz.st_value, sz.entry, sz.op, sz.shift) == (kvs_value, st_value, entry, op, 3)
    assert L.op_dtype(sz).itemsize == op and L.entry_dtype(sz).itemsize == entry
    assert L.entry_dtype(sz).fields["value"][1] + st_value == 18 + kvs_value
    cfg = O.Config(1, ecl, 0, 0, 1 << 8, 1 << 16, 0, 0)
    got = []
    for name in ("hko_kvs_value_size", "hko_st_value_size", "hko_entry_size", "hko_op_size"):
        f = getattr(O.lib(), name)
        f.restype, f.argtypes = ctypes.c_uint32, [ctypes.POINTER(O.Config)]
        got.append(f(ctypes.byref(cfg)))
    assert tuple(got) == VALUE_SIZES[ecl]


@pytest.mark.parametrize("ecl", sorted(VAL_LEN))
def test_value_size_val_len_bytes(ecl):
    """entry byte 17 and op byte 10 after populate, a GET, a PUT, a raising INV and a write replay, per size"""
    carried, populated, get_pop, put, get_put, inv_len, get_inv = VAL_LEN[ecl]
    sz = L.Sizes(True, ecl)
    kv = O.OracleKVS(1 << 10, 1 << 21, big_objects=True, extra_cache_lines=ecl)
    kv.populate(1000, sz.kvs_value)
    keys = O.gen_keys(1000)
    mb = L.membership(3, 0)
    k_put, k_inv, k_rep = (int(keys[i]) for i in (3, 4, 5))
    assert carried == (sz.st_value >> sz.shift) & 0xFF

    def byte17(key):
        return int(kv.log_bytes()[kv.lookup(key) + 17])

    def get(key, membership=mb):
        op = np.zeros(1, dtype=L.op_dtype(sz))
        op["key"], op["opcode"], op["state"] = key, int(L.Op.GET), int(L.Bucket.NEW)
        kv.batch(L.BatchType.local_ops, op, membership)
        return op[0]

    assert byte17(k_put) == byte17(k_inv) == populated
    g = get(k_put)
    assert int(g["state"]) == int(L.Resp.GET_COMPLETE) and int(g["val_len"]) == get_pop
    # a PUT: the entry takes set_val_len of what the op carries, the op's byte stays
    p = np.zeros(1, dtype=L.op_dtype(sz))
    p["key"], p["opcode"], p["state"], p["val_len"] = k_put, int(L.Op.PUT), int(L.Bucket.NEW), carried
    p["value"] = 7
    kv.batch(L.BatchType.local_ops, p, mb)
    assert int(p["state"][0]) == int(L.Resp.PUT_SUCCESS) and int(p["val_len"][0]) == carried
    assert byte17(k_put) == put
    # ACKs from both peers validate it: the GET then reads get_val_len of the PUT's byte
    ack = np.zeros(2, dtype=L.msg_dtype())
    ack["key"], ack["opcode"], ack["sender"] = k_put, int(L.Op.ACK), [1, 2]
    ack["ts_ver"], ack["ts_cid"] = p["ts_ver"][0], p["ts_cid"][0]
    kv.batch(L.BatchType.acks, ack, mb, rw=p)
    g = get(k_put)
    assert int(g["state"]) == int(L.Resp.GET_COMPLETE) and int(g["val_len"]) == get_put and int(g["value"][-1]) == 7
    # a raising INV: (uint8_t) KVS_VALUE_SIZE; its own byte stays; validated, a GET reads get_val_len of it
    for key in (k_inv, k_rep):
        inv = np.zeros(1, dtype=L.op_dtype(sz))
        inv["key"], inv["opcode"], inv["state"], inv["val_len"] = key, int(L.Op.INV), 2, carried
        inv["ts_ver"], inv["ts_cid"] = 2, 2
        inv["value"] = 9
        kv.batch(L.BatchType.invs, inv, mb)
        assert int(inv["opcode"][0]) == int(L.Resp.INV_SUCCESS) and int(inv["val_len"][0]) == carried
        assert byte17(key) == inv_len
    val = np.zeros(1, dtype=L.msg_dtype())
    val["key"], val["opcode"], val["sender"], val["ts_ver"], val["ts_cid"] = k_inv, int(L.Op.VAL), 2, 2, 2
    kv.batch(L.BatchType.vals, val, mb)
    g = get(k_inv)
    assert int(g["state"]) == int(L.Resp.GET_COMPLETE) and int(g["val_len"]) == get_inv and int(g["value"][0]) == 9
    # a GET of the key node 2 left INVALID, after node 2 was dropped: the write replay fills the op
    r = get(k_rep, L.membership(3, 0, alive=0b011))
    assert int(r["state"]) == int(L.Resp.REPLAY_SUCCESS) and int(r["val_len"]) == carried
    assert (r["value"] == 9).all() and byte17(k_rep) == inv_len


@pytest.mark.parametrize("rmw,big", [(False, False), (True, False), (True, True)])
def test_scripted_rare_outcomes_oracle(rmw, big):
    """tests/scripted.py on the oracle alone: every branch outcome it expects (written out from
    hermesKV.c) happens, and together they cover every code the batch function can emit."""
    from tests.scripted import required_outcomes, run_scripted
    sz = L.BIG if big else L.DEFAULT
    kv = O.OracleKVS(1 << 12, 1 << 22, machine_id=0, rmw=rmw, big_objects=big, extra_cache_lines=4 if big else 0)
    kv.populate(1000, sz.kvs_value)

    def runner(btype, elems, mb, rw=None, node_suspected=None):
        if node_suspected is not None:
            node_suspected[0] = kv.batch(btype, elems, mb, rw=rw)
        else:
            kv.batch(btype, elems, mb, rw=rw)

    seen = run_scripted(runner, O.gen_keys(1000), sz, rmw)
    missing = required_outcomes(rmw) - seen
    assert not missing, f"not produced: {sorted(missing, key=str)}"


@pytest.mark.parametrize("big", [False, True])
def test_scripted_skew_optimisations_oracle(big):
    """tests/scripted.py's skew scenario on the oracle (skew_flags 3): read completion and write
    coalescing outcomes written out from hermesKV.c:196-356, incl. the 16-bit version of the
    write path and the REPLAY exception."""
    from tests.scripted import run_scripted_skew
    sz = L.BIG if big else L.DEFAULT
    kv = O.OracleKVS(1 << 12, 1 << 22, machine_id=0, big_objects=big, extra_cache_lines=4 if big else 0, skew=3)
    kv.populate(1000, sz.kvs_value)
    seen = run_scripted_skew(lambda bt, e, mb, rw=None, node_suspected=None: kv.batch(bt, e, mb, rw=rw),
                             O.gen_keys(1000), sz)
    assert (0, int(L.Resp.PUT_COMPLETE)) in seen and (0, int(L.Resp.GET_COMPLETE)) in seen


def test_skew_flags_off_keep_stalls_oracle():
    """The same first batch without the flags: every op behind the write stalls (the default build)."""
    from tests.scripted import SK, _sk_ops
    kv = O.OracleKVS(1 << 12, 1 << 22, machine_id=0)
    kv.populate(1000, L.DEFAULT.kvs_value)
    keys = O.gen_keys(1000)
    l1 = _sk_ops(L.DEFAULT, [("hot", L.Op.PUT, (0, 0)), ("hot", L.Op.GET, (0, 0)), ("hot", L.Op.PUT, (0, 0)),
                             ("hot", L.Op.GET, (0, 7))], keys)
    kv.batch(L.BatchType.local_ops, l1, L.membership(3, 0))
    assert [int(x) for x in l1["state"]] == [int(L.Resp.PUT_SUCCESS), int(L.Resp.GET_STALL), int(L.Resp.PUT_STALL),
                                             int(L.Resp.GET_STALL)]
    assert [int(x) for x in l1["ts_ver"]] == [2, 0, 0, 0]
    assert SK["hot"] < 1000
