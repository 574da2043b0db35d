"""The shapes tests/test_virtual_peers_gpu.py runs the generators at, in one place so that
tests/test_peer_model_cpu.py can show on a machine without a GPU that the exact comparison is safe at them (no
power-law draw within rounding of an integer) and that the Round check has inline keys whose version moves."""
from __future__ import annotations

import numpy as np

from hermes_amd import layout as L
from tests import peer_model as PM

SEED = 0x5EED

# hkv_wl_gen_trace: (W, len, n, theta, write permille, rmw permille, with d_trace_id)
TRACE_CASES = [
    (40, 1024, 60000, 0.99, 200, 0, True),
    (40, 1024, 60000, 0.99, 200, 500, False),
    (3, 100, 3, 0.99, 200, 0, True),
    (8, 256, 3000, 0.0, 200, 0, True),
]

# hkv_wl_gen_peer_round on n = 3000, theta 0.99 (hot ids repeat across workers):
# (W, per_peer, peer ids, big ops, rmw permille, round indices)
PEER_ROUND_CASES = [
    (40, 50, [1, 2], False, 0, (0, 5)),
    (3, 300, [1, 2, 3, 4, 5, 6, 7], False, 0, (0,)),      # the second pass of the 256-wide loop, peer id 7
    (8, 50, [1, 2], True, 500, (1,)),
]
PEER_ROUND_KEYS = 3000

# the Round check: the bench round of test_whole_round_checked_once_per_step
ROUND = dict(n_keys=60_000, bkts=1 << 16, cap=1 << 23, W=40, peers=[1, 2], per_peer=50, theta=0.99, write_pm=200,
             max_steps=8, trace_len=1024, steps=6)


def round_peer_seed(seed=SEED, machine_id=0):
    """the seed Round gives its virtual peers (hermes_amd/workload.py, _gen_remote)"""
    return seed * 7919 + machine_id


def power_law_margin(z, u):
    """the smallest relative distance of n * pow(...) from an integer over the draws that take the power law
    (inf when none does)"""
    u = np.asarray(u, np.float64)
    u = u[PM.zipf_branch(z, u) == 3]
    if not len(u):
        return np.inf
    x = PM.zipf_power(z, u)
    return float(np.min(np.abs(x - np.rint(x)) / x))


def all_draws():
    """(zipf, u) of every draw the GPU module compares exactly"""
    out = []
    for W, ln, n, theta, _, _, _ in TRACE_CASES:
        r1, _ = PM.trace_randoms(W, ln, SEED)
        out.append((f"trace {W}x{ln} n={n}", PM.zipf_params(n, theta), PM.unit_double(r1)))
    for W, pp, peers, _, _, rounds in PEER_ROUND_CASES:
        for rnd in rounds:
            out.append((f"peer round {W}x{pp}x{len(peers)} round {rnd}", PM.zipf_params(PEER_ROUND_KEYS, 0.99),
                        peer_units(W, pp, len(peers), rnd, SEED)))
    return out


def peer_units(W, per_peer, n_peers, rnd, seed):
    g = np.arange(W * n_peers * per_peer, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r1 = PM.splitmix64(np.uint64(seed & PM.M64) ^ np.uint64((rnd << 40) & PM.M64) ^ (np.uint64(0x9E37) * g))
    return PM.unit_double(r1)


def round_slabs(keys):
    """the model's peer slabs of the Round check, one per round index: INVs [n][56] back to back in the packed
    (peer-major) order Round keeps them"""
    c = ROUND
    z = PM.zipf_params(c["n_keys"], c["theta"])
    out = []
    for k in range(c["max_steps"]):
        invs, _, counts = PM.gen_peer_round(c["W"], c["per_peer"], c["peers"], L.DEFAULT.op, L.DEFAULT.st_value,
                                            L.DEFAULT.shift, z, 0, k, round_peer_seed(), keys)
        out.append(pack_peer_major(invs, counts))
    return out


def pack_peer_major(rows, counts):
    """rows [W][R * per_peer][size] with counts [W][R] -> the elements back to back, batch (r, w) peer-major"""
    W, R = counts.shape
    start = np.cumsum(counts, axis=1) - counts
    parts = [rows[w, start[w, r]:start[w, r] + counts[w, r]] for r in range(R) for w in range(W)]
    return np.concatenate(parts) if parts else rows.reshape(-1, rows.shape[-1])[:0]
