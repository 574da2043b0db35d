"""Times the replica repair (HermesKV.extract / HermesKV.install) on the benchmark's table -- BASELINE configs[1]:
100M keys, 2^27 buckets -- for a LOG and for an INLINE pair of tables: a full extract of the source, a full install
into a second table with half the buckets, and, for comparison, the same records applied the way the library
already could: unique INV launches plus VAL launches through HermesKV.batch (the INV and VAL arrays are built on the
device beforehand, outside the timing). HIP events around each repetition, warm-ups first, median [min, max].

    python tools/repair_bench.py [--keys N] [--out FILE]

Every timed install raises every key: the records' versions are bumped (untimed) before each repetition, for both
paths alike, so both write the meta and the value of every record. An install of records the target already
holds (every record "equal": the lookup and the compare, nothing written) is timed as well. Asserts that the digests
of source and target agree after an install of the unmodified records, that neither call converts a table, and
that the install's counts add up.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s
CHUNK = 1 << 22     # elements per launch of the two-launch path


def timed(torch, fn, prep=None, warm=2, reps=7):
    ms = []
    for i in range(warm + reps):
        if prep:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return ms


def line(name, ms, floor_bytes=None, note=""):
    s = sorted(ms)
    med = statistics.median(s)
    out = f"{name:<46} median {med:9.3f} ms   min {s[0]:9.3f}   max {s[-1]:9.3f}   ({len(s)} reps)"
    if floor_bytes:
        fl = floor_bytes / HBM_PEAK * 1e3
        out += f"\n{'':<46} must move {floor_bytes / 2**30:6.2f} GiB = {fl:.3f} ms at 8 TB/s; " \
               f"median = {floor_bytes / (med * 1e-3) / 1e12:.2f} TB/s, {med / fl:.2f}x the floor{note}"
    return out


def marshal(torch, L, rec, n, E):
    """the records as the INV and VAL arrays of the header's definition, on the device (64-B records)"""
    r = rec[:n * E].view(n, E)
    inv = torch.zeros((n, 56), dtype=torch.uint8, device=rec.device)
    val = torch.zeros((n, 16), dtype=torch.uint8, device=rec.device)
    for lo in range(0, n, 1 << 24):
        s = slice(lo, min(lo + (1 << 24), n))
        for a, oc in ((inv, int(L.Op.INV)), (val, int(L.Op.VAL))):
            a[s, 0:8] = r[s, 8:16]
            a[s, 8] = oc
            a[s, 9] = r[s, 23]
            a[s, 11] = r[s, 23]
            a[s, 12:16] = r[s, 24:28]
        inv[s, 10] = 31
        inv[s, 18:49] = r[s, 33:64]
    return inv, val


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=100_000_000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from hermes_amd import layout as L
    from hermes_amd.kvs import LAYOUT_INLINE, HermesKV, sized_geometry

    E = 64
    bkts, cap = sized_geometry(a.keys)
    free0 = torch.cuda.mem_get_info()[0]
    need = 2 * (bkts * 64 + cap) + bkts * 128 + bkts * 64 + a.keys * (E + 56 + 16 + 24) + (8 << 30)
    keys = a.keys
    rows = []
    if need > free0:
        keys //= 2
        bkts, cap = sized_geometry(keys)
        rows.append(f"(two {a.keys}-key tables plus records do not fit in {free0 / 2**30:.0f} GiB free: halved to {keys})")
    mb = L.membership(3, 1)
    rows[:0] = [f"replica repair, {keys} keys, source {bkts} buckets, target {bkts // 2} buckets, log capacity {cap} B, "
                f"{torch.cuda.get_device_name(0)}",
                "HIP events around each repetition, 2 warm-ups; one device, one run", ""]
    rec = torch.empty(keys * E, dtype=torch.uint8, device="cuda")
    res = torch.empty(2, dtype=torch.int64, device="cuda")
    ires = torch.empty(4, dtype=torch.int64, device="cuda")

    def bump(t, col):   # every record / element one version step newer (the version's low byte)
        t[:, col] += 2

    for name in ("LOG", "INLINE"):   # a fresh pair of tables each: the timed installs leave the target ahead
        src = HermesKV(keys, bkts, cap, machine_id=0)
        dst = HermesKV(keys, bkts // 2, cap, machine_id=1)
        if name == "INLINE":
            for t in (src, dst):
                assert t.prefer_layout(LAYOUT_INLINE), "the table is not eligible for the inline residency"
                t.apply_layout()
        torch.cuda.synchronize()
        lay0 = (src.layout(), dst.layout())
        ms = timed(torch, lambda: src.extract(out=rec, result=res))
        x = src.extract(out=rec, result=res)
        n = x.records
        assert n == x.scanned_keys <= keys
        c = src.census().host()
        assert c["keys"] == n
        fetch = bkts * (64 if name == "LOG" else 128) + (n - c["from_lines"]) * 128
        rows.append(line(f"extract, {name}", ms, fetch + n * E, " (the census's fetch + the records written)"))
        rows.append(f"    records {n}  from_lines {c['from_lines']}")
        # the unmodified records: the target ends with the source's digest
        first = dst.install(x, n=n, result=ires).host()
        assert sum(first.values()) == n, first
        cd = dst.census().host()
        held = n - first["missed"]
        rows.append(f"    install of the extract: {first}; target keys {cd['keys']}")
        if first["missed"] == 0 and cd["keys"] == n:
            assert (cd["digest_sum"], cd["digest_xor"]) == (c["digest_sum"], c["digest_xor"]), "digests differ"
            rows.append("    source and target digests equal")
        ms = timed(torch, lambda: dst.install(rec, n=n, result=ires))
        assert dst.install(rec, n=n, result=ires).host()["raised"] == 0
        il = cd["from_lines"]
        reads = n * E + (n * 128 if name == "LOG" else il * 128 + (n - il) * 192)
        rows.append(line(f"install, {name}, every record equal", ms, reads, " (records + bucket + entry, read)"))
        r2 = rec[:n * E].view(n, E)
        ms = timed(torch, lambda: dst.install(rec, n=n, result=ires), prep=lambda: bump(r2, 24))
        got = ires.cpu().tolist()
        assert got[0] == held and got[1] == got[2] == 0, got
        rows.append(line(f"install, {name}, every record raised", ms, reads + held * 64,
                         " (the same + a 64-B line written back)"))
        # the way the parent already has: unique INV launches + VAL launches of the same records
        inv, val = marshal(torch, L, rec, n, E)
        torch.cuda.synchronize()

        def two_launches():
            for lo in range(0, n, CHUNK):
                m = min(CHUNK, n - lo)
                dst.batch(L.BatchType.invs, inv[lo:lo + m].view(-1), 1, m, 56, mb, unique=True)
            for lo in range(0, n, CHUNK):
                m = min(CHUNK, n - lo)
                dst.batch(L.BatchType.vals, val[lo:lo + m].view(-1), 1, m, 16, mb)

        def prep2():
            bump(inv, 12)
            bump(val, 12)
            inv[:, 8] = int(L.Op.INV)      # the launches leave their result codes in the elements
            val[:, 8] = int(L.Op.VAL)
        ms = timed(torch, two_launches, prep=prep2)
        rows.append(line(f"unique INV + VAL launches, {name} ({-(-n // CHUNK)} of each)", ms))
        del inv, val
        l1 = (src.layout(), dst.layout())
        assert all(u["state"] == v["state"] and u["conversions"] == v["conversions"] for u, v in zip(lay0, l1)), \
            f"a table was converted: {lay0} -> {l1}"
        assert src.take_error_flags() == 0 and dst.take_error_flags() == 0
        src.close()
        dst.close()
        rows.append("")
    text = "\n".join(rows) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
