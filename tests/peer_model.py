"""A plain numpy / Python restatement of the workload generators and the virtual peers
(include/hermeskv_workload.h), for tests/test_peer_model_cpu.py and tests/test_virtual_peers_gpu.py.

Written from the header and the reference lines it cites, with no call into the kernels it models: integers
are Python ints or uint64 arrays (wrapping), everything else is float64. The table is read through
OracleKVS.lookup, the reference's lookup (hermesKV.c:952-993: first tag match, window check, key compare).

  splitmix64, unit_double, zipf_params, zipf_draw   the seeded streams and the Gray / YCSB Zipfian
  gen_trace                                         hkv_wl_gen_trace (create_uni_trace / parse_trace)
  peer_draws, gen_peer_round                        hkv_wl_gen_peer_round
  peer_versions, stamp, peer_ts_words               hkv_wl_peer_ts / _peer_ts_at / _refill_plan_peer_ts
                                                    (update_actions_n_unlock, hermesKV.c:100-141)
  peer_answer, peer_acks_rows / _packed / _pm / _queue
                                                    hkv_wl_peer_acks*, (ack_copy_and_modify_elem,
                                                    hermes_worker.c:100-118; the INV-abort of hermesKV.c:566-576)
  ack_offsets                                       hkv_wl_ack_offsets
"""
from __future__ import annotations

import collections

import numpy as np

OP_INV, OP_ACK, OP_VAL, OP_INV_ABORT = 114, 115, 116, 139   # spacetime.h:51-89
OP_GET, OP_PUT, OP_RMW = 111, 112, 113
M64 = (1 << 64) - 1

Zipf = collections.namedtuple("Zipf", "theta zetan alpha eta half_pow n")


def splitmix64(x):
    """Steele / Lea / Flood's splitmix64 finaliser over uint64 (an int or an array), wrapping"""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def unit_double(r):
    """the top 53 bits as a double in [0, 1)"""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def zipf_params(n: int, theta: float) -> Zipf:
    """Gray et al., "Quickly generating billion-record synthetic databases" (the YCSB generator) over ids [0, n)"""
    if theta <= 0:
        return Zipf(0.0, 0.0, 0.0, 0.0, 0.0, n)
    zetan = float(np.sum(np.arange(1, n + 1, dtype=np.float64) ** -theta))
    zeta2 = 1.0 + 2.0 ** -theta
    eta = (1.0 - (2.0 / n) ** (1.0 - theta)) / (1.0 - zeta2 / zetan)
    return Zipf(theta, zetan, 1.0 / (1.0 - theta), eta, 1.0 + 0.5 ** theta, n)


def zipf_power(z, u):
    """n * (eta*u - eta + 1)^alpha, the power-law branch before it is truncated"""
    u = np.asarray(u, dtype=np.float64)
    return float(z.n) * np.power(z.eta * u - z.eta + 1.0, z.alpha)


def zipf_branch(z, u):
    """which branch a draw takes: 0 uniform, 1 `uz < 1`, 2 `uz < half_pow`, 3 the power law"""
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    if z.theta <= 0:
        return np.zeros(len(u), np.int64)
    uz = u * z.zetan
    return np.where(uz < 1.0, 1, np.where(uz < z.half_pow, 2, 3))


def zipf_draw(z, u):
    """rank == id: id 0 is the hottest key (parse_trace, util.c:337-343)"""
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    n = int(z.n)
    if z.theta <= 0:
        ids = np.floor(u * float(n)).astype(np.uint64)
        return np.minimum(ids, np.uint64(n - 1))
    br = zipf_branch(z, u)
    with np.errstate(invalid="ignore"):
        p = np.floor(zipf_power(z, np.where(br == 3, u, 1.0)))
    ids = np.minimum(p, float(n - 1)).astype(np.uint64)     # the clamp to n - 1
    return np.where(br == 1, np.uint64(0), np.where(br == 2, np.uint64(1), ids))


def trace_randoms(n_workers, length, seed):
    g = np.arange(n_workers * length, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r1 = splitmix64(np.uint64(seed & M64) ^ (np.uint64(0x1000003) * g))
    return r1, splitmix64(r1 ^ np.uint64(0x5EED))


def gen_trace(n_workers, length, zipf, write_pm, rmw_pm, seed, keys):
    """(key, op, id) of trace[w * length + j]; keys = gen_keys(n): CityHash128(&id, 4).second per id"""
    r1, r2 = trace_randoms(n_workers, length, seed)
    ids = zipf_draw(zipf, unit_double(r1)).astype(np.uint32)
    coin = (r2 % np.uint64(1000)).astype(np.int64)
    rcoin = ((r2 >> np.uint64(32)) % np.uint64(1000)).astype(np.int64)
    op = np.full(len(ids), OP_GET, np.uint8)
    put = coin < write_pm                                   # create_uni_trace, util.c:236-240
    op[put] = OP_PUT
    if rmw_pm:
        op[put & (rcoin < rmw_pm)] = OP_RMW
    return np.asarray(keys, np.uint64)[ids], op, ids


def peer_draws(n_workers, per_peer, n_peers, zipf, rmw_pm, rnd, seed):
    """Every draw (w, r, j) of a peer round: ids and RMW flags [W][R][per_peer], and keep: the draw is its
    peer's first of that id in the peer's own op order w * per_peer + j"""
    W, R, P = n_workers, n_peers, per_peer
    g = np.arange(W * R * P, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r1 = splitmix64(np.uint64(seed & M64) ^ np.uint64((rnd << 40) & M64) ^ (np.uint64(0x9E37) * g))
    ids = zipf_draw(zipf, unit_double(r1)).astype(np.uint32).reshape(W, R, P)
    flags = (((r1 >> np.uint64(3)) % np.uint64(1000)).astype(np.int64) < rmw_pm).reshape(W, R, P) & bool(rmw_pm)
    keep = np.zeros((W, R, P), bool)
    for r in range(R):
        first = {}
        for w in range(W):
            for j in range(P):
                first.setdefault(int(ids[w, r, j]), (w, j))    # (w, j) ascending = the order index ascending
        for w, j in first.values():
            keep[w, r, j] = True
    return ids, flags, keep


def gen_peer_round(n_workers, per_peer, peer_ids, op_size, st_value, shift, zipf, rmw_pm, rnd, seed, keys, fill=0):
    """(invs [W][R * per_peer][op_size], vals [..][16], peer_counts [W][R]): the kept draws compacted per worker
    in peer order, then in j order; every other slot holds `fill` bytes, as the caller left it"""
    W, R = n_workers, len(peer_ids)
    ids, flags, keep = peer_draws(W, per_peer, R, zipf, rmw_pm, rnd, seed)
    keys = np.asarray(keys, np.uint64)
    invs = np.full((W, R * per_peer, op_size), fill, np.uint8)
    vals = np.full((W, R * per_peer, 16), fill, np.uint8)
    counts = np.zeros((W, R), np.int32)
    for w in range(W):
        o = 0
        for r, peer in enumerate(peer_ids):
            for j in np.nonzero(keep[w, r])[0]:
                x = invs[w, o]
                x[0:8] = np.frombuffer(int(keys[ids[w, r, j]]).to_bytes(8, "little"), np.uint8)
                x[8], x[9], x[10], x[11] = OP_INV, peer, (st_value >> shift) & 0xFF, peer
                x[12:16] = 0                     # the version: filled in per round
                x[16], x[17] = int(flags[w, r, j]), 0
                x[18:] = (ord("a") + peer) & 0xFF
                vals[w, o] = x[:16]
                vals[w, o, 8] = OP_VAL
                o += 1
            counts[w, r] = int(keep[w, r].sum())
    return invs, vals, counts


def key_of(elem) -> int:
    return int.from_bytes(bytes(elem[:8]), "little")


def peer_versions(oracle, invs, rmw_build=None):
    """(ver, phys) per INV [n][op_size]: the version the peer's write takes from the key's entry in the oracle's
    table as it stands (u32 at entry byte 24; + 2 without RMWs or for an RMW, + 4 for a plain write in an RMW
    build; 2 for an absent key), and the entry's log offset (-1: absent)"""
    rmw_build = bool(oracle.cfg.rmw_enabled) if rmw_build is None else rmw_build
    log = oracle.log_bytes()
    ver, phys = np.zeros(len(invs), np.uint32), np.full(len(invs), -1, np.int64)
    for i, x in enumerate(invs):
        off = oracle.lookup(key_of(x))
        if off is None:
            ver[i] = 2
            continue
        cur = int.from_bytes(bytes(log[off + 24:off + 28]), "little")
        ver[i] = (cur + (2 if (not rmw_build or (x[16] & 1)) else 4)) & 0xFFFFFFFF
        phys[i] = off
    return ver, phys


def stamp(elems, opcode, ver):
    """a copy with the opcode and bytes 12..15 = ver, every other byte unchanged"""
    out = np.array(elems, np.uint8, copy=True)
    out[:, 8] = opcode
    out[:, 12:16] = np.asarray(ver, "<u4").view(np.uint8).reshape(-1, 4)
    return out


def round_tag(rnd: int) -> int:
    return (rnd + 1) & 0x7FFFFF


def peer_ts_words(words, invs, ver, phys, entry_size, rnd):
    """d_peer_ts after the stamping launch: for a present key of a peer below 8, word [phys / entry_size][peer] =
    tag(round + 1) << 41 | rmw << 40 | ver << 8 | peer (the largest when several name one word); the rest of
    `words` (uint64 [slots * 8]) as it was"""
    out = np.array(words, np.uint64, copy=True)
    for x, v, p in zip(invs, ver, phys):
        peer = int(x[9])
        if p < 0 or peer >= 8:
            continue
        w = (round_tag(rnd) << 41) | (int(x[16] & 1) << 40) | (int(v) << 8) | peer
        i = (int(p) // entry_size) * 8 + peer
        out[i] = max(int(out[i]), w)
    return out


def peer_answer(inv, peer, ack_size, oracle=None, words=None, entry_size=64, rnd=0, slot=None):
    """Peer `peer`'s answer to one INV into `slot` (ack_size bytes as the caller left them; default zeros):
    the ACK -- the INV's first 16 bytes, opcode ACK, sender = peer -- or, with `words` (an RMW build), for an
    RMW INV whose (version, cid) is below the peer's word of this round, the peer's INV-abort: its own
    timestamp and RMW flag, sender = peer, val_len and no_coales of the INV, value 'a' + peer"""
    y = np.zeros(ack_size, np.uint8) if slot is None else slot
    op_size = len(inv)
    if words is not None and (inv[16] & 1) and peer < 8 and ack_size >= op_size:
        off = oracle.lookup(key_of(inv))
        if off is not None:
            pw = int(words[(off // entry_size) * 8 + peer])
            ours = (int.from_bytes(bytes(inv[12:16]), "little") << 8) | int(inv[11])
            pts = pw & 0xFFFFFFFFFF
            if (pw >> 41) == round_tag(rnd) and pts > ours:
                y[0:8] = inv[0:8]
                y[8], y[9], y[10], y[11] = OP_INV_ABORT, peer, inv[10], pts & 0xFF
                y[12:16] = np.frombuffer((pts >> 8).to_bytes(4, "little"), np.uint8)
                y[16], y[17] = (pw >> 40) & 1, inv[17]
                y[18:op_size] = (ord("a") + peer) & 0xFF
                return y
    y[:16] = inv[:16]
    y[8], y[9] = OP_ACK, peer
    return y


def _answers(invs, inv_count, peer_ids, ack_size, place, out, **kw):
    W = len(inv_count)
    for w in range(W):
        for j in range(int(inv_count[w])):
            for r, peer in enumerate(peer_ids):
                peer_answer(invs[w, j], peer, ack_size, slot=out[place(w, j, r)], **kw)
    return out


def peer_acks_rows(invs, inv_count, peer_ids, ack_size, out_stride, out, **kw):
    """hkv_wl_peer_acks, rows: invs [W][inv_stride][op_size]; out [W * out_stride][ack_size] (prefilled);
    element w * out_stride + j * R + r. Returns (out, ack_count = R * inv_count)"""
    R = len(peer_ids)
    _answers(invs, inv_count, peer_ids, ack_size, lambda w, j, r: w * out_stride + j * R + r, out, **kw)
    return out, (np.asarray(inv_count) * R).astype(np.int32)


def peer_acks_packed(invs, inv_count, peer_ids, ack_size, out_off, out, **kw):
    """hkv_wl_peer_acks with d_out_off: worker w's answers from element out_off[w]"""
    R = len(peer_ids)
    _answers(invs, inv_count, peer_ids, ack_size, lambda w, j, r: int(out_off[w]) + j * R + r, out, **kw)
    return out, (np.asarray(inv_count) * R).astype(np.int32)


def peer_acks_pm(invs, inv_count, peer_ids, ack_size, inv_off, out, **kw):
    """hkv_wl_peer_acks_pm: peer r's answers are block r of T = inv_off[W] elements, worker w's at inv_off[w]"""
    R, T = len(peer_ids), int(inv_off[len(inv_count)])
    _answers(invs, inv_count, peer_ids, ack_size, lambda w, j, r: r * T + int(inv_off[w]) + j, out, **kw)
    return out, (np.asarray(inv_count) * R).astype(np.int32)


def peer_acks_queue(invs, inv_count, peer_ids, ack_size, q_stride, aq_n, vq_n, out, **kw):
    """hkv_wl_peer_acks_queue: the answers appended to worker w's queue row at aq_n[w]; the new aq_n, and
    ack_count = the whole queue, or 0 while the worker has VALs outstanding (hermes_worker.c:479)"""
    R = len(peer_ids)
    _answers(invs, inv_count, peer_ids, ack_size, lambda w, j, r: w * q_stride + int(aq_n[w]) + j * R + r, out, **kw)
    q = (np.asarray(aq_n) + np.asarray(inv_count) * R).astype(np.int32)
    return out, q, np.where(np.asarray(vq_n) > 0, 0, q).astype(np.int32)


def ack_offsets(counts, n_peers):
    """(offsets [n + 1], total, max): offsets[w] = n_peers * (counts before w)"""
    c = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(c * n_peers)]).astype(np.int32)
    return off, int(off[-1]), int(c.max()) if len(c) else 0
