"""Times the table census (HermesKV.census) on the benchmark's table -- BASELINE configs[1]: 100M keys, 2^27
buckets -- in LOG state, in INLINE state after a few rounds, and against the way to the same answer without it:
bench.py's table_digest on the INLINE table, with the conversion to LOG it forces and the conversion back that the
next round would pay. HIP events around each repetition, 10 repetitions after 2 warm-ups, median and spread.

    python tools/census_bench.py [--keys N] [--out FILE]

Asserts that the census in INLINE state converts nothing (the layout counters), and that the LOG and INLINE
censuses of the same table agree.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s


def timed(torch, fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def line(name, ms, floor_bytes=None):
    s = sorted(ms)
    med = statistics.median(s)
    out = f"{name:<44} median {med:9.3f} ms   min {s[0]:9.3f}   max {s[-1]:9.3f}   ({len(s)} reps)"
    if floor_bytes:
        fl = floor_bytes / HBM_PEAK * 1e3
        out += f"\n{'':<44} must fetch {floor_bytes / 2**30:6.2f} GiB = {fl:.3f} ms at 8 TB/s; " \
               f"median = {floor_bytes / (med * 1e-3) / 1e12:.2f} TB/s, {med / fl:.2f}x the floor"
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=100_000_000)
    p.add_argument("--workers", type=int, default=16384)
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    import bench
    from hermes_amd import layout as L
    from hermes_amd.kvs import LAYOUT_INLINE, LAYOUT_LOG, HermesKV, sized_geometry
    from hermes_amd.workload import Round, zipf_params

    bkts, cap = sized_geometry(a.keys)
    kvs = HermesKV(a.keys, bkts, cap, skew=3)
    torch.cuda.synchronize()
    out = torch.empty(32, dtype=torch.int64, device="cuda")
    rows = [f"table census, {a.keys} keys, {bkts} buckets, log capacity {cap} B, {torch.cuda.get_device_name(0)}",
            "HIP events around each repetition; one device, one run", ""]

    # LOG, fresh populate
    ms = timed(torch, lambda: kvs.census(out=out))
    c_log = kvs.census(out=out).host()
    assert kvs.layout()["state"] == LAYOUT_LOG and kvs.layout()["conversions"] == 0
    rows.append(line("census, LOG", ms, bkts * 64 + c_log["keys"] * 128))
    rows.append(f"    keys {c_log['keys']}  dead_slots {c_log['dead_slots']}  VALID {c_log['by_state'][1]}")

    # a few rounds of the benchmark's workload: the table goes INLINE and stays there
    rnd = Round(kvs, a.workers, L.membership(3, 0), [1, 2], zipf_params(a.keys, 0.99), 200, 0, seed=0x5EED,
                max_steps=a.rounds + 8, retry_stalled=True)
    assert rnd.inline, "the round does not run on the inline residency"
    for _ in range(a.rounds):
        rnd.step()
    torch.cuda.synchronize()
    before = kvs.layout()
    assert before["state"] == LAYOUT_INLINE, before
    ms = timed(torch, lambda: kvs.census(out=out))
    c_inl = kvs.census(out=out).host()
    after = kvs.layout()
    assert after == before, f"the census moved the layout: {before} -> {after}"
    rows.append(line("census, INLINE (after %d rounds)" % a.rounds, ms,
                     bkts * 128 + (c_inl["keys"] - c_inl["from_lines"]) * 128))
    rows.append(f"    keys {c_inl['keys']}  from_lines {c_inl['from_lines']}  not VALID {c_inl['offenders']}  "
                f"conversions {after['conversions']} before and after (13 census calls)")

    # without it: bench.py's digest of the exported log, and back to INLINE as the next round would go
    def old_way():
        bench.table_digest(kvs, a.keys)
        kvs.apply_layout()
    conv0 = kvs.layout()["conversions"]
    ms = timed(torch, old_way)
    lay = kvs.layout()
    assert lay["state"] == LAYOUT_INLINE and lay["conversions"] == conv0 + 2 * 12, lay
    rows.append(line("bench.table_digest + both conversions", ms))
    ms = timed(torch, lambda: bench.table_digest(kvs, a.keys))     # (the table stays LOG: no conversion)
    rows.append(line("bench.table_digest alone (table LOG)", ms))
    assert kvs.layout()["state"] == LAYOUT_LOG
    c_back = kvs.census(out=out).host()
    same = {k: v for k, v in c_back.items() if k != "from_lines"} == {k: v for k, v in c_inl.items() if k != "from_lines"}
    assert same and c_back["from_lines"] == 0, (c_back, c_inl)
    rows.append("    census of the same table after the export (LOG): every field equal to the INLINE census")
    assert kvs.take_error_flags() == 0
    text = "\n".join(rows) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
