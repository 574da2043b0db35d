"""The invertible sketch of include/hermeskv.h ("Sketch-level delta repair") restated in numpy. Written from the
header's text, not from the kernels: an element is a 16-byte summary read as two little-endian words (a, b); its
check word is c = mix64(mix64(a + G) + b); its cell in subtable j is j S + (((mix64(c + (j + 1) G) >> 32) S) >> 32);
a cell is (count, key_xor, meta_xor, check_xor); the decode runs pass p over subtable p mod 3 on the cells as they
are when the pass begins.

Cells are uint64 [3 S, 4]; lists of elements are uint64 [n, 2] (a, b).
"""
from __future__ import annotations

import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
MAX_PASSES = 192   # HKV_SKETCH_MAX_PASSES
M64 = (1 << 64) - 1


def mix64(x):
    """the splitmix64 finaliser (the census's), on uint64 arrays"""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def words(summaries) -> np.ndarray:
    """summaries (any array of whole 16-byte summaries) as uint64 [n, 2]: a = bytes 0..7, b = bytes 8..15"""
    return np.ascontiguousarray(summaries).view(np.uint8).reshape(-1, 16).copy().view("<u8").astype(np.uint64).reshape(-1, 2)


def check(a, b):
    with np.errstate(over="ignore"):
        return mix64(mix64(np.asarray(a, np.uint64) + G) + np.asarray(b, np.uint64))


def slot(c, j: int, S: int):
    """the element's cell within subtable j (add j S for the cell's index)"""
    with np.errstate(over="ignore"):
        h = mix64(np.asarray(c, np.uint64) + np.uint64(j + 1) * G) >> np.uint64(32)
        return (h * np.uint64(S)) >> np.uint64(32)   # (below 2^32 times below 2^32: no overflow)


def _apply(cells, idx, sign, a, b, c):
    """cells[idx] += sign * element, for arrays of cell indices (repeats allowed)"""
    with np.errstate(over="ignore"):
        np.add.at(cells[:, 0], idx, sign)
    np.bitwise_xor.at(cells[:, 1], idx, a)
    np.bitwise_xor.at(cells[:, 2], idx, b)
    np.bitwise_xor.at(cells[:, 3], idx, c)


def sketch_model(summaries, S: int, cells: np.ndarray | None = None) -> np.ndarray:
    """the sketch of the list: uint64 [3 S, 4]; `cells`: a sketch to add the list to (returned, modified)"""
    assert 1 <= S < 1 << 32
    w = words(summaries)
    if cells is None:
        cells = np.zeros((3 * S, 4), np.uint64)
    a, b = w[:, 0], w[:, 1]
    c = check(a, b)
    one = np.ones(len(w), np.uint64)
    for j in range(3):
        _apply(cells, (np.uint64(j * S) + slot(c, j, S)).astype(np.int64), one, a, b, c)
    return cells


def subtract_model(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    D = np.empty_like(A)
    with np.errstate(over="ignore"):
        D[:, 0] = A[:, 0] - B[:, 0]
    D[:, 1:] = A[:, 1:] ^ B[:, 1:]
    return D


def decode_model(A: np.ndarray, B: np.ndarray, S: int, max_passes: int = MAX_PASSES) -> dict:
    """the decode of A - B: only_a, only_b (uint64 [n, 2], in pass order), cells (the remainder), passes, undecoded,
    exhausted"""
    D = subtract_model(np.asarray(A, np.uint64), np.asarray(B, np.uint64))
    lists = {1: [], M64: []}
    passes, idle, p = 0, 0, 0
    while p < max_passes and idle < 3:
        j = p % 3
        sub = D[j * S:(j + 1) * S]
        cnt, a, b, c = sub[:, 0].copy(), sub[:, 1].copy(), sub[:, 2].copy(), sub[:, 3].copy()
        pure = ((cnt == np.uint64(1)) | (cnt == np.uint64(M64))) & (check(a, b) == c) & \
            (slot(c, j, S) == np.arange(S, dtype=np.uint64))
        i = np.nonzero(pure)[0]
        if len(i):
            cnt, a, b, c = cnt[i], a[i], b[i], c[i]
            with np.errstate(over="ignore"):
                sign = np.uint64(0) - cnt   # the cells lose the pure cell's count
            for jj in range(3):
                _apply(D, (np.uint64(jj * S) + slot(c, jj, S)).astype(np.int64), sign, a, b, c)
            assert not D[j * S + i].any()
            for s in (1, M64):
                m = cnt == np.uint64(s)
                lists[s].append(np.stack([a[m], b[m]], axis=1))
            passes, idle = p + 1, 0
        else:
            idle += 1
        p += 1
    cat = lambda l: np.concatenate(l) if l else np.zeros((0, 2), np.uint64)
    return {"only_a": cat(lists[1]), "only_b": cat(lists[M64]), "cells": D, "passes": passes,
            "undecoded": int(D.any(axis=1).sum()), "exhausted": int(idle < 3)}


def as_set(elements) -> set:
    """a list of elements (uint64 [n, 2], or summaries) as a set of (a, b)"""
    e = np.asarray(elements)
    if e.dtype != np.uint64 or e.ndim != 2:
        e = words(e)
    return {(int(x), int(y)) for x, y in e.tolist()}


def random_elements(rng, n: int) -> np.ndarray:
    """n distinct summaries (16-byte rows as a structured array: key, ts version, ts cid, state, two zero bytes)
    with scattered keys and plausible metadata, for the tests"""
    s = np.zeros(n, np.dtype([("key", "<u8"), ("ts_ver", "<u4"), ("ts_cid", "u1"), ("state", "u1"), ("zero", "u1", (2,))]))
    with np.errstate(over="ignore"):
        s["key"] = rng.permutation(np.arange(1, 4 * n + 1, dtype=np.uint64))[:n] * G
    s["ts_ver"] = rng.integers(1, 1 << 20, n)
    s["ts_cid"] = rng.integers(0, 5, n)
    s["state"] = rng.integers(0, 5, n)
    return s


def difference_case(n: int, seed: int):
    """(list_a, list_b, only_a, only_b): two lists that share 2 n elements and differ in n, each of which is on one
    side by a coin"""
    rng = np.random.default_rng(1000 * n + seed)
    e = random_elements(rng, 3 * n)
    common, diff = e[:2 * n], e[2 * n:]
    side = rng.random(n) < 0.5
    return np.concatenate([common, diff[side]]), np.concatenate([diff[~side], common]), diff[side], diff[~side]
