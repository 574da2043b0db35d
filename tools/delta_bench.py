"""Times the partitioned census and the delta repair (HermesKV.census_parts, the masked HermesKV.extract,
replica_group.delta_resync) beside the calls they stand next to (HermesKV.census, the plain extract, the install,
replica_group.resync) on the benchmark's table -- BASELINE configs[1]: a source of 100M keys in 2^27 buckets, a
target with half the buckets -- for a LOG and for an INLINE pair. HIP events around each repetition, 2 warm-ups,
7 repetitions, median [min, max]; everything in one session.

    python tools/delta_bench.py [--keys N] [--out FILE]

Per pair: census() of both tables; census_parts at part_bits 12, 16 and 20 with both mappings of its kernel
(HKV_CENSUS_PARTS_MAPPING, read by the library at every call), whose rows must be equal and fold to census(); the
plain extract; the masked extract at part_bits 20 with no partition, about 1 % of them and all of them selected;
the install of records the target holds; then, after INV + VAL launches that raise 10,000 of the source's keys
(again, one version higher, before every repetition, untimed), a delta_resync and a full resync of the same pair,
with the records and bytes either ships.

Run from a checkout that has no partition calls, it times the census, the extract and the install only, under the
same row names: that is how the numbers of two commits are compared in one session.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from repair_bench import line, marshal, timed  # noqa: E402

RAISED = 10_000
PART_BITS = (12, 16, 20)
MAPPING = "HKV_CENSUS_PARTS_MAPPING"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=100_000_000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch

    from hermes_amd import kvs as K
    from hermes_amd import layout as L
    from hermes_amd import replica_group as G
    from hermes_amd.kvs import LAYOUT_INLINE, HermesKV, sized_geometry

    parts = hasattr(HermesKV, "census_parts")
    E = 64
    keys = a.keys
    bkts, cap = sized_geometry(keys)
    out_f = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out_f = open(a.out, "w")

    def row(text=""):   # (written as it comes: a run that ends early leaves what it measured)
        print(text, flush=True)
        if out_f:
            out_f.write(text + "\n")
            out_f.flush()

    row(f"partitioned census and delta repair, {keys} keys, source {bkts} buckets, target {bkts // 2} buckets, "
        f"log capacity {cap} B, {torch.cuda.get_device_name(0)}")
    row("HIP events around each repetition, 2 warm-ups; one device, one run" +
        ("" if parts else "; this checkout has no partition calls"))
    row()
    rec = torch.empty(keys * E, dtype=torch.uint8, device="cuda")
    res = torch.empty(2, dtype=torch.int64, device="cuda")
    ires = torch.empty(4, dtype=torch.int64, device="cuda")
    cen = torch.empty(32, dtype=torch.int64, device="cuda")
    prow = torch.empty(4 << max(PART_BITS), dtype=torch.int64, device="cuda")

    for name in ("LOG", "INLINE"):
        src = HermesKV(keys, bkts, cap, machine_id=0)
        dst = HermesKV(keys, bkts // 2, cap, machine_id=1)
        if name == "INLINE":
            for t in (src, dst):
                assert t.prefer_layout(LAYOUT_INLINE), "the table is not eligible for the inline residency"
                t.apply_layout()
        torch.cuda.synchronize()
        lay0 = (src.layout(), dst.layout())
        for t, who in ((src, "source"), (dst, "target")):
            row(line(f"census, {name}, {who}", timed(torch, lambda: t.census(out=cen))))
        c = src.census(out=cen).host()

        if parts:
            for pb in PART_BITS:
                got = {}
                for m in ("A", "B"):
                    os.environ[MAPPING] = m
                    ms = timed(torch, lambda: src.census_parts(pb, out=prow))
                    row(line(f"census_parts, {name}, source, part_bits {pb}, mapping {m}", ms))
                    got[m] = src.census_parts(pb, out=prow).host().copy()
                os.environ.pop(MAPPING)
                r = got["A"]
                assert np.array_equal(r, got["B"]), "the two mappings' rows differ"
                assert int(r[:, 0].sum(dtype=np.uint64)) == c["digest_sum"] and int(r[:, 2].sum()) == c["keys"]
                assert int(np.bitwise_xor.reduce(r[:, 1])) == c["digest_xor"] and int(r[:, 3].sum()) == c["offenders"]
            row("    both mappings' rows equal at every part_bits, and fold to the census")

        ms = timed(torch, lambda: src.extract(out=rec, result=res))
        x = src.extract(out=rec, result=res)
        n = x.records
        assert n == x.scanned_keys == c["keys"]
        row(line(f"extract, {name}", ms))
        row(f"    records {n}  from_lines {c['from_lines']}")

        if parts:
            pb = max(PART_BITS)
            P = 1 << pb
            some = (torch.rand(P, device="cuda", generator=torch.Generator("cuda").manual_seed(7)) < 0.01).to(torch.uint8)
            for what, mask in (("none", torch.zeros(P, dtype=torch.uint8, device="cuda")), ("about 1 %", some),
                               ("all", torch.full((P,), 0x80, dtype=torch.uint8, device="cuda"))):
                ms = timed(torch, lambda: src.extract(out=rec, result=res, part_bits=pb, part_mask=mask))
                h = src.extract(out=rec, result=res, part_bits=pb, part_mask=mask).host()
                row(line(f"masked extract, {name}, part_bits {pb}, {what} selected", ms))
                row(f"    partitions selected {int((mask != 0).sum())} of {P}  records {h['records']}  "
                    f"scanned_keys {h['scanned_keys']}")
                assert h["records"] == h["scanned_keys"] == {"none": 0, "all": n}.get(what, h["records"])
            x = src.extract(out=rec, result=res)   # (the last masked extract wrote the same records: all selected)

        first = dst.install(x, n=n, result=ires).host()
        assert sum(first.values()) == n, first
        row(f"    install of the extract: {first}")
        ms = timed(torch, lambda: dst.install(rec, n=n, result=ires))
        assert dst.install(rec, n=n, result=ires).host()["raised"] == 0
        row(line(f"install, {name}, every record equal", ms))

        if parts:
            # RAISED of the source's keys, spread over the table, as INVs and VALs of another machine
            r2 = rec[:n * E].view(n, E)
            # (whole numbers: a float32 ramp up to n - 1 rounds its end past n at 100M records)
            pick = torch.arange(min(RAISED, n), dtype=torch.int64, device="cuda") * max(n // RAISED, 1)
            assert int(pick.max()) < n
            sub = r2[pick].contiguous()
            m = sub.shape[0]
            inv, val = marshal(torch, L, sub.view(-1), m, E)
            for arr in (inv, val):
                arr[:, 9] = 2    # sender
                arr[:, 11] = 2   # ts_cid
            mb = L.membership(3, 0)

            def raise_keys():
                for arr, oc in ((inv, L.Op.INV), (val, L.Op.VAL)):
                    arr[:, 12] += 2          # one version step (the version's low byte)
                    arr[:, 8] = int(oc)      # the launches leave their result codes in the elements
                flags, HermesKV.default_flags = HermesKV.default_flags, K.BATCH_ENGINE
                try:
                    src.batch(L.BatchType.invs, inv.view(-1), 1, m, 56, mb, unique=True)
                    src.batch(L.BatchType.vals, val.view(-1), 1, m, 16, mb)
                finally:
                    HermesKV.default_flags = flags

            last = {}

            def run(fn):
                def go():
                    last.clear()
                    last.update(fn(dst, src))
                return go
            for what, fn in (("delta_resync", G.delta_resync), ("resync (every key)", G.resync)):
                ms = timed(torch, run(fn), prep=raise_keys)
                row(line(f"{what}, {name}, {m} keys raised", ms))
                row(f"    {last}")
                row(f"    shipped {last['records']} records = {last['records'] * E} B")
                # (a raised key that the target evicted at populate counts as missed, not raised)
                assert m - first["missed"] <= last["raised"] <= m and last["older"] == 0, last
            d = G.delta_resync(dst, src)
            row(f"    delta_resync once more, nothing raised: {d}")
            del inv, val, sub

        l1 = (src.layout(), dst.layout())
        row(f"    layout state, conversions: source {lay0[0]['state']}, {lay0[0]['conversions']} -> {l1[0]['state']}, "
            f"{l1[0]['conversions']}; target {lay0[1]['state']}, {lay0[1]['conversions']} -> {l1[1]['state']}, "
            f"{l1[1]['conversions']}")
        assert all(u["state"] == v["state"] for u, v in zip(lay0, l1)), f"a table changed residency: {lay0} -> {l1}"
        assert src.take_error_flags() == 0 and dst.take_error_flags() == 0
        src.close()
        dst.close()
        row()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
