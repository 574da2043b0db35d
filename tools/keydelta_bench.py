"""Times the key-level delta repair (HermesKV.summaries / need / fetch, replica_group.key_delta_resync) beside the
calls it stands next to (the masked HermesKV.extract, replica_group.delta_resync and resync) on the benchmark's
table -- BASELINE configs[1]: a source of 100M keys in 2^27 buckets, a target with half the buckets -- for a LOG
and for an INLINE pair. HIP events around each repetition, 2 warm-ups, 7 repetitions, median [min, max]; everything
in one session.

    python tools/keydelta_bench.py [--keys N] [--out FILE]

Per pair, at part_bits 20: summaries with no partition, about 1 % of them and all of them selected, each beside the
masked extract of the same selection; need of the 1 % and of all summaries against the target (which holds every
key at the same timestamp: the lookup and the compare, class `same`); fetch of the 1 % selection's keys; then, after
INV + VAL launches that raise 10,000 of the source's keys (again, one version higher, before every repetition,
untimed), key_delta_resync, delta_resync and a full resync of the same pair, with the bytes each ships, and fetch of
the 10,000 needed keys alone. Beside each pass the bytes it must move and that floor at 8 TB/s.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from repair_bench import line, marshal, timed  # noqa: E402

RAISED = 10_000
PART_BITS = 20


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=100_000_000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from hermes_amd import kvs as K
    from hermes_amd import layout as L
    from hermes_amd import replica_group as G
    from hermes_amd.kvs import LAYOUT_INLINE, HermesKV, sized_geometry

    E = 64
    keys = a.keys
    bkts, cap = sized_geometry(keys)
    pb = min(PART_BITS, (bkts // 2).bit_length() - 1)
    P = 1 << pb
    out_f = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out_f = open(a.out, "w")

    def row(text=""):   # (written as it comes: a run that ends early leaves what it measured)
        print(text, flush=True)
        if out_f:
            out_f.write(text + "\n")
            out_f.flush()

    row(f"key-level delta repair, {keys} keys, source {bkts} buckets, target {bkts // 2} buckets, "
        f"log capacity {cap} B, part_bits {pb}, {torch.cuda.get_device_name(0)}")
    row("HIP events around each repetition, 2 warm-ups; one device, one run")
    row()
    rec = torch.empty(keys * E, dtype=torch.uint8, device="cuda")
    res = torch.empty(2, dtype=torch.int64, device="cuda")
    sbuf = torch.empty(keys * 16, dtype=torch.uint8, device="cuda")
    kbuf = torch.empty(keys, dtype=torch.int64, device="cuda")
    some = (torch.rand(P, device="cuda", generator=torch.Generator("cuda").manual_seed(7)) < 0.01).to(torch.uint8)
    masks = (("none", torch.zeros(P, dtype=torch.uint8, device="cuda")), ("about 1 %", some),
             ("all", torch.full((P,), 0x80, dtype=torch.uint8, device="cuda")))

    for name in ("LOG", "INLINE"):
        src = HermesKV(keys, bkts, cap, machine_id=0)
        dst = HermesKV(keys, bkts // 2, cap, machine_id=1)
        if name == "INLINE":
            for t in (src, dst):
                assert t.prefer_layout(LAYOUT_INLINE), "the table is not eligible for the inline residency"
                t.apply_layout()
        torch.cuda.synchronize()
        lay0 = (src.layout(), dst.layout())
        unit = 128 if name == "INLINE" else 64      # bytes read per bucket
        counts = {}
        for what, mask in masks:
            sel = int((mask != 0).sum())
            ms_x = timed(torch, lambda: src.extract(out=rec, result=res, part_bits=pb, part_mask=mask))
            ms_s = timed(torch, lambda: src.summaries(part_bits=pb, part_mask=mask, out=sbuf))
            h = src.summaries(part_bits=pb, part_mask=mask, out=sbuf).host()
            n = counts[what] = h["records"]
            assert n == h["scanned_keys"] == src.extract(out=rec, result=res, part_bits=pb, part_mask=mask).records
            # buckets of the selected partitions, then per key: the entry's sector (an inline key's is in its line)
            # and the summary, or the entry and the record
            b_sel = bkts * sel // P * unit + P
            row(line(f"masked extract, {name}, {what} selected", ms_x, b_sel + n * (64 + E)))
            row(line(f"summaries, {name}, {what} selected", ms_s, b_sel + n * (32 + 16)))
            row(f"    partitions selected {sel} of {P}  keys {n}  summaries {16 * n} B  records {E * n} B")
        n_all = counts["all"]

        # the target holds every key the source holds, but for the ones its fuller buckets evicted at populate
        for what, mask in masks[1:]:
            n = counts[what]
            sm = src.summaries(part_bits=pb, part_mask=mask, out=sbuf)
            ms = timed(torch, lambda: dst.need(sm, n=n, out=kbuf))
            nd = dst.need(sm, n=n, out=kbuf).host()
            row(line(f"need, {name}, {what} selected", ms, n * (16 + unit // 2 + 32)))
            row(f"    {nd}")
            assert nd["same"] + nd["missed"] == n and nd["needed"] == nd["missed"], nd
        n1 = counts["about 1 %"]
        sm = src.summaries(part_bits=pb, part_mask=masks[1][1], out=sbuf)
        k1 = sbuf[:n1 * 16].view(torch.int64).view(n1, 2)[:, 0].contiguous()
        ms = timed(torch, lambda: src.fetch(k1, out=rec))
        f = src.fetch(k1, out=rec).host()
        assert f == {"found": n1, "absent": 0}, f
        row(line(f"fetch, {name}, the 1 % selection's {n1} keys", ms, n1 * (8 + unit + 64 + E)))

        # RAISED of the source's keys, spread over the table, as INVs and VALs of another machine
        x = src.extract(out=rec, result=res)
        assert x.records == n_all
        r2 = rec[:n_all * E].view(n_all, E)
        pick = torch.arange(min(RAISED, n_all), dtype=torch.int64, device="cuda") * max(n_all // RAISED, 1)
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
        for what, fn in (("key_delta_resync", G.key_delta_resync), ("delta_resync", G.delta_resync),
                         ("resync (every key)", G.resync)):
            ms = timed(torch, run(fn), prep=raise_keys)
            row(line(f"{what}, {name}, {m} keys raised", ms))
            row(f"    {last}")
            if "bytes_summaries" in last:
                shipped = last["bytes_summaries"] + last["bytes_keys"] + last["bytes_records"]
                row(f"    shipped {last['bytes_summaries']} B of summaries + {last['bytes_keys']} B of keys + "
                    f"{last['bytes_records']} B of records = {shipped} B; the partitioned delta of the same "
                    f"partitions: {last['bytes_partition_delta']} B ({last['bytes_partition_delta'] / max(shipped, 1):.2f}x); "
                    f"with 320-B entries: {shipped - last['bytes_records'] + 320 * last['needed']} B against "
                    f"{320 * last['summaries']} B "
                    f"({320 * last['summaries'] / max(shipped - last['bytes_records'] + 320 * last['needed'], 1):.2f}x)")
                assert last["needed"] == last["records"] and last["classes"]["older"] == 0, last
            else:
                row(f"    shipped {last['records']} records = {last['records'] * E} B")
            assert last["raised"] <= m and last["older"] == 0, last
        raise_keys()
        sm = src.summaries(part_bits=pb, part_mask=masks[2][1], out=sbuf)
        nk = dst.need(sm, n=n_all, out=kbuf).needed
        ms = timed(torch, lambda: src.fetch(kbuf, n=nk, out=rec))
        row(line(f"fetch, {name}, the {nk} needed keys", ms, nk * (8 + unit + 64 + E)))
        row(f"    key_delta_resync once more: {G.key_delta_resync(dst, src)}")
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
