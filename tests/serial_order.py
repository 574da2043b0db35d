"""Is there a serial order of concurrent callers' calls that explains what every call returned?

TEST INFRASTRUCTURE ONLY (CPU, oracle only). `calls[k]` is thread k's recorded calls to
hermes_batch_ops_to_KVS in program order: the batch type, the elements and read_write_ops as
passed in and as returned, and the CLOCK_MONOTONIC times just before the call and just after it
returned. find_serial_order looks for a total order of all calls such that

* each thread's calls appear in program order,
* a call that ended before another started precedes it (real-time order),
* applying the calls in that order on the oracle reproduces every call's output elements and
  read_write_ops byte for byte, and
* the oracle's log over len(final_log) then equals final_log.

INV, VAL and ACK outputs do not reveal the state they met, so a wrong choice between two blind writes
shows only calls later and a plain depth-first search does not stay bounded. The search here keeps a
running hash of the table state and a set of dead (positions, state hash) pairs: most orders of
overlapping calls commute and reach the same pair, which is then explored once.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from tests import gen

ENTRY = 64   # bytes of one log entry of the default build (layout.DEFAULT.entry)


class Call(NamedTuple):
    type: int
    n: int
    esz: int
    ein: np.ndarray              # uint8, n * esz
    eout: np.ndarray
    rin: Optional[np.ndarray]    # uint8, read_write_ops as passed in (ACK batches), else None
    rout: Optional[np.ndarray]
    start: int
    end: int


class NoSerialOrder(AssertionError):
    """The search failed. `exhausted`: every order was ruled out (else the cap on applications was
    hit); `prefix`: the longest prefix reached, as (thread, call) pairs; `diffs`: for each call
    that was eligible after that prefix, why it could not come next."""

    def __init__(self, exhausted, applications, prefix, diffs, n_calls):
        self.exhausted, self.applications, self.prefix, self.diffs = exhausted, applications, prefix, diffs
        why = "no serial order exists (search exhausted)" if exhausted else "the cap on applications was hit"
        lines = [f"{why}: {applications} applications, longest prefix {len(prefix)} of {n_calls} calls"]
        lines += [f"  after {prefix[-1] if prefix else 'the start'}: {d}" for d in diffs]
        super().__init__("\n".join(lines))


class _Frame:
    __slots__ = ("cands", "i", "undo", "diffs")

    def __init__(self, cands, undo):
        self.cands, self.i, self.undo, self.diffs = cands, 0, undo, []


def _first_diff(k, c, call, got, want, what):
    esz = call.esz if what == "element" else 56
    i = int(np.flatnonzero(got != want)[0]) // esz
    key = int(np.frombuffer(want[i * esz:i * esz + 8].tobytes(), "<u8")[0])
    return (f"thread {k} call {c} (type {call.type}) {what} {i} key {key:#018x}: got "
            f"{got[i * esz:(i + 1) * esz].tobytes().hex()} wanted {want[i * esz:(i + 1) * esz].tobytes().hex()}")


def find_serial_order(calls, oracle, mb, final_log=None, max_applications=None):
    """Returns (order, applications): the order as (thread, call index) pairs, found by applying
    calls to `oracle` (left in the final state), and the number of oracle.batch applications the
    search made. Raises NoSerialOrder."""
    T = len(calls)
    N = sum(len(c) for c in calls)
    if max_applications is None:
        max_applications = 4 * T * N
    log = oracle.log_bytes()
    lane = np.arange(ENTRY, dtype=np.int64)

    # every call's distinct keys as log offsets (batches never change the index), its inputs as the oracle takes them
    off_of = {}

    def offsets(raw, esz):
        keys = np.unique(np.ascontiguousarray(raw.reshape(-1, esz)[:, :8]).view("<u8"))
        out = []
        for key in keys.tolist():
            if key not in off_of:
                off_of[key] = oracle.lookup(key)
            if off_of[key] is not None:
                out.append(off_of[key])
        return out

    prep = []
    remaining = {}   # log offset -> calls not yet applied that touch it
    for k in range(T):
        row = []
        for call in calls[k]:
            offs = set(offsets(call.ein, call.esz))
            if call.rin is not None:
                offs |= set(offsets(call.rin, 56))
            offs = np.array(sorted(offs), dtype=np.int64)
            for o in offs.tolist():
                remaining[o] = remaining.get(o, 0) + 1
            row.append((offs, offs[:, None] + lane[None, :],
                        call.ein.view(np.dtype((np.void, call.esz))),
                        call.rin.view(np.dtype((np.void, 56))) if call.rin is not None else None))
        prep.append(row)

    if final_log is not None:
        # bytes no call touches never change: a difference there rules out every order at once
        final_log = np.asarray(final_log, dtype=np.uint8)
        stray = log[:len(final_log)] != final_log
        for o in remaining:
            stray[o:o + ENTRY] = False
        if stray.any():
            at = int(np.flatnonzero(stray)[0])
            raise NoSerialOrder(True, 0, [], [f"final log differs at byte {at}, in an entry no call touches: got "
                                              f"{int(final_log[at]):#04x} wanted {int(log[at]):#04x}"], N)
    n_final = len(final_log) if final_log is not None else 0

    pos = [0] * T
    state_hash = 0
    applications = 0
    dead = set()
    memo = {}
    best = (-1, [], [])

    def eligible():
        front = [(calls[k][pos[k]].start, k) for k in range(T) if pos[k] < len(calls[k])]
        if not front:
            return []
        min_end = min(calls[k][pos[k]].end for _, k in front)
        return [k for s, k in sorted(front) if s <= min_end]

    def put_back(undo):
        nonlocal state_hash
        k, offs, idx, before, delta = undo
        log[idx] = before
        pos[k] -= 1
        state_hash ^= delta
        for o in offs.tolist():
            remaining[o] += 1

    frames = [_Frame(eligible(), None)]
    while frames:
        f = frames[-1]
        depth = len(frames) - 1
        if f.i == len(f.cands):   # left without success: this (positions, state) leads nowhere
            if depth > best[0]:
                best = (depth, [(fr.undo[0], pos_k) for fr, pos_k in _walk(frames)], f.diffs)
            dead.add((tuple(pos), state_hash))
            frames.pop()
            if f.undo is not None:
                put_back(f.undo)
            continue
        k = f.cands[f.i]
        f.i += 1
        c = pos[k]
        call = calls[k][c]
        offs, idx, ein_v, rin_v = prep[k][c]
        before = log[idx]
        # what a call does is a function of its inputs and its keys' entries alone: met again in the same
        # local state (on another path of the search), its outcome is taken from the memo, not the oracle
        mkey = (k, c, hash(before.tobytes()))
        outcome = memo.get(mkey)
        if outcome is None:
            if applications >= max_applications:
                if depth >= best[0]:
                    best = (depth, [(fr.undo[0], pos_k) for fr, pos_k in _walk(frames)], f.diffs)
                raise NoSerialOrder(False, applications, best[1], best[2], N)
            e = gen.bytecopy(ein_v)
            rw = gen.bytecopy(rin_v) if rin_v is not None else None
            oracle.batch(call.type, e, mb, rw=rw)
            applications += 1
            got = e.view(np.uint8).reshape(-1)
            if not np.array_equal(got, call.eout):
                outcome = _first_diff(k, c, call, got, call.eout, "element")
            elif rw is not None and not np.array_equal(rw.view(np.uint8).reshape(-1), call.rout):
                outcome = _first_diff(k, c, call, rw.view(np.uint8).reshape(-1), call.rout, "read_write_op")
            else:
                after = log[idx]
                rows = np.flatnonzero((before != after).any(axis=1))
                delta = 0
                for r in rows.tolist():
                    o = int(offs[r])
                    delta ^= hash((o, before[r].tobytes())) ^ hash((o, after[r].tobytes()))
                outcome = (rows, after[rows], delta)
            memo[mkey] = outcome
            if isinstance(outcome, str):
                log[idx] = before
        elif not isinstance(outcome, str):
            log[idx[outcome[0]]] = outcome[1]
        if isinstance(outcome, str):
            f.diffs.append(outcome)
            continue
        delta = outcome[2]
        after = log[idx]
        pos[k] += 1
        state_hash ^= delta
        lost = None
        for r, o in enumerate(offs.tolist()):
            remaining[o] -= 1
            if remaining[o] == 0 and o + ENTRY <= n_final and lost is None and \
                    not np.array_equal(after[r], final_log[o:o + ENTRY]):
                lost = (f"thread {k} call {c} (type {call.type}) is the last to touch log offset {o}: final log has "
                        f"{final_log[o:o + ENTRY].tobytes().hex()} wanted {after[r].tobytes().hex()}")
        undo = (k, offs, idx, before, delta)
        if lost is not None:
            f.diffs.append(lost)
            put_back(undo)
            continue
        if (tuple(pos), state_hash) in dead:
            f.diffs.append(f"thread {k} call {c} (type {call.type}) matches, but leads to a state already ruled out")
            put_back(undo)
            continue
        frames.append(_Frame(eligible(), undo))
        if depth + 1 == N:
            return [(fr.undo[0], pos_k) for fr, pos_k in _walk(frames)], applications
    raise NoSerialOrder(True, applications, best[1], best[2], N)


def call_keys(call):
    keys = set(np.ascontiguousarray(call.ein.reshape(-1, call.esz)[:, :8]).view("<u8").reshape(-1).tolist())
    if call.rin is not None:
        keys |= set(np.ascontiguousarray(call.rin.reshape(-1, 56)[:, :8]).view("<u8").reshape(-1).tolist())
    return keys


def contention(calls):
    """What makes a history worth checking: the share of calls that overlap in time with a call of
    another thread sharing a key, and the set of (batch type, response code) pairs returned."""
    flat = [(k, call, call_keys(call)) for k in range(len(calls)) for call in calls[k]]
    contended = 0
    for k, a, ka in flat:
        contended += any(j != k and b.start <= a.end and a.start <= b.end and not ka.isdisjoint(kb)
                         for j, b, kb in flat)
    seen = set()
    for _, call, _ in flat:
        out = call.eout.reshape(call.n, call.esz)
        seen.update((call.type, int(code)) for code in np.unique(out[:, 9 if call.type == 0 else 8]))
    return contended / max(1, len(flat)), seen


def _walk(frames):
    """(frame, call index) of every applied call along the current path."""
    seen = {}
    for fr in frames[1:]:
        k = fr.undo[0]
        seen[k] = seen.get(k, -1) + 1
        yield fr, seen[k]
