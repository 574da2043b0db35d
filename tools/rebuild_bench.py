"""Times the rebuild of a replica from a live one (HermesKV.upsert) on the benchmark's table -- BASELINE configs[1]:
100M keys, source 2^27 buckets: an upsert of the source's full extract into an empty table of 2^27 and of 2^26
buckets; an upsert whose every record is present, beside an install of the same records; and, in the same session,
what the library offered for the job before: hkv_table_populate of the same number of keys followed by an install of
every record (every entry written twice). HIP events around each repetition, 2 warm-ups, 7 repetitions, median
[min, max]; the upsert's phases (install pass, scan and pairs, sort, bucket replay, log writes) from the events the
library records between them (HKV_UPSERT_PHASES).

    python tools/rebuild_bench.py [--keys N] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["HKV_UPSERT_PHASES"] = "1"   # read when the library is loaded

HBM_PEAK = 8.0e12   # bytes / s
PHASES = ("install pass", "scan + pairs", "sort", "bucket replay", "log writes")


def line(name, ms, floor_bytes=None, note=""):
    s = sorted(ms)
    med = statistics.median(s)
    out = f"{name:<52} median {med:9.3f} ms   min {s[0]:9.3f}   max {s[-1]:9.3f}   ({len(s)} reps)"
    if floor_bytes:
        fl = floor_bytes / HBM_PEAK * 1e3
        out += f"\n{'':<52} must move {floor_bytes / 2**30:6.2f} GiB = {fl:.3f} ms at 8 TB/s; {med / fl:.2f}x the floor{note}"
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=100_000_000)
    p.add_argument("--out", default=None)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    import torch

    from hermes_amd import lib
    from hermes_amd.kvs import HermesKV, sized_geometry

    E = 64
    keys = a.keys
    bkts, cap = sized_geometry(keys)
    src = HermesKV(keys, bkts, cap, machine_id=0)
    x = src.extract()
    n = x.records
    rec = x.tensor
    c = src.census().host()
    rows = [f"replica rebuild, {keys} keys ({n} live), source {bkts} buckets, log capacity {cap} B, "
            f"{torch.cuda.get_device_name(0)}",
            f"HIP events around each repetition, {a.warm} warm-ups, {a.reps} repetitions; one device, one run", ""]

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def phases(t):
        ms = (ctypes.c_float * 5)()
        lib.check(lib.raw().hkv_debug_upsert_phases(t.h, ms), "hkv_debug_upsert_phases")
        return list(ms)

    # 1. upsert into an empty table, per target geometry; a fresh table per repetition (created outside the timing)
    for tb in (bkts, bkts // 2):
        ms, ph, last = [], [], None
        for i in range(a.warm + a.reps):
            dst = HermesKV(keys, tb, cap, machine_id=1, populate=False)
            torch.cuda.synchronize()
            t, out = event_ms(lambda: dst.upsert(rec, n=n))
            if i >= a.warm:
                ms.append(t)
                ph.append(phases(dst))
            last = (out, dst.census().host())
            dst.close()
        out, cd = last
        assert out["inserted"] == n and out["raised"] == out["equal"] == out["older"] == 0, out
        # bytes: install pass reads records + buckets (n x 128) and writes a flag byte; scan reads n flags, writes 4 n;
        # pairs read 5 n + 8 n of keys' lines, write 20 n; sort 3 passes x 16 n; replay reads 8 n + 8 n + buckets
        # 64 n, writes 64 n; log reads 4 n + 64 n, writes 64 n
        floor = n * (128 + 1) + n * 5 + n * (5 + 64 + 20) + 3 * 16 * n + n * (16 + 128) + n * (4 + 128)
        rows.append(line(f"upsert into an empty table of {tb} buckets", ms, floor, " (sum of the phases' floors)"))
        for k, name in enumerate(PHASES):
            rows.append(line(f"    phase: {name}", [p_[k] for p_ in ph]))
        rows.append(f"    result {out}")
        rows.append(f"    target keys {cd['keys']} of {n}; digests equal: "
                    f"{(cd['digest_sum'], cd['digest_xor']) == (c['digest_sum'], c['digest_xor'])}")
        rows.append("")

    # 2. the parent's way: populate the same keys, then install every record
    ms_pop, ms_ins, ms_both = [], [], []
    ires = torch.empty(4, dtype=torch.int64, device="cuda")
    for i in range(a.warm + a.reps):
        dst = HermesKV(keys, bkts // 2, cap, machine_id=1, populate=False)
        torch.cuda.synchronize()
        tp, _ = event_ms(lambda: dst.populate(keys, dst.sizes.kvs_value))
        ti, _ = event_ms(lambda: dst.install(rec, n=n, result=ires))
        if i >= a.warm:
            ms_pop.append(tp)
            ms_ins.append(ti)
            ms_both.append(tp + ti)
        if i < a.warm + a.reps - 1:
            dst.close()
    rows.append(line(f"populate({keys}) into {bkts // 2} buckets", ms_pop))
    rows.append(line("install of every record into it (all equal)", ms_ins))
    rows.append(line("populate + install: the job before the upsert", ms_both))
    rows.append("")

    # 3. nothing missed: upsert beside install, the source's own records into the source (the populated target of
    # half the buckets lacks the keys it evicted at populate, so an upsert there would insert)
    ms_u, ms_i, ms_k = [], [], []
    for i in range(a.warm + a.reps):
        tu, out = event_ms(lambda: src.upsert(rec, n=n))
        if i >= a.warm:
            ms_k.append(phases(src)[0])
        ti, _ = event_ms(lambda: src.install(rec, n=n, result=ires))
        assert out["inserted"] == 0
        if i >= a.warm:
            ms_u.append(tu)
            ms_i.append(ti)
    rows.append(line("upsert, every record present (nothing inserted)", ms_u, n * (E + 128 + 1)))
    rows.append(line("    its install pass alone (events inside the call)", ms_k))
    rows.append(line("install of the same records", ms_i, n * (E + 128)))
    assert src.take_error_flags() == 0 and dst.take_error_flags() == 0
    text = "\n".join(rows) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
