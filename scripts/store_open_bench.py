#!/usr/bin/env python3
"""Reopening and scrubbing a chunk store on one MI355X (include/sdfs_store.h).

Per workload — --gib GiB of engine chunks at the default parameters (256 KiB buffers), written by
HipBufferWriter with LZ4 ("plain") or LZ4 + AES-256 with version-1 archives ("aes"):
    scan        sdfs_cdc_store_scan, HIP events, one stream
    map_copy    device-to-device copy of the maps' bytes: what the scan must at least read
    directory   sdfs_cdc_store_directory, HIP events
    open        open_store() end to end (scan -> [decrypt -> chain_lens -> raw_lens] -> index get ->
                directory), host clock around a device synchronise
    lookup      sdfs_cdc_store_lookup of every stored key plus as many absent ones, HIP events
    scrub       scrub() end to end at the default 65 536 records per slice, host clock; its stages
                from HIP events recorded as each is enqueued (the slices' sums, host reads included)
    scrub_one_slice   the same with every record in one slice
    read        HipBufferReader.read(verify=True) over all buffers, host clock: the same decrypt,
                decode and hash kernels plus a gather the scrub does not need
After a warm-up of every timed shape, REPS (>= 20) repetitions with the timed calls alternating
inside each repetition; every time is reported as median / min / max.  One JSON line, printed and
appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from sdfs_amd import HipVariableSha256HashEngine  # noqa: E402
from sdfs_amd import store as ST  # noqa: E402
from sdfs_amd.archive import HipBufferWriter, map_bytes  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import HipBufferReader  # noqa: E402

L = 262144
PB = 1 << 33
HL = 32
KEY = bytes(range(7, 39))


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def bench_workload(name, e, nbuf, reps):
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    aes = name == "aes"
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    batch.run(buffer_id_base=0)
    nrec = int(batch.total.item())
    ix = HipHashesMap(max(1 << 12, 1 << (nrec * 2).bit_length()))
    wr = HipBufferWriter(ix, hash_len=HL, aes=KEY if aes else None, version=1 if aes else 0)
    m, arcs = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    n, na = arcs.n_rec, arcs.n_arc
    lens = [map_bytes(arcs.map_stride, HL, arcs.version)] * na
    mc = int(e._params.max_len)
    images = (arcs.store, arcs.arc_base, arcs.arc_bytes, arcs.maps, lens)
    open_ = lambda: ST.open_store(*images, ix, PB, n, hash_len=HL, version=arcs.version,  # noqa: E731
                                  aes=wr.aes, max_chunk=mc)
    op = open_()
    torch.cuda.synchronize()
    for got, want in zip(op.directory(), arcs.directory()):
        assert torch.equal(got, want)
    assert op.n_rec == n and not op.extra["open"]["flags"].any()
    sc = op.extra["open"]["scan"]
    hashloc = op.extra["open"]["hashloc"]
    raw = op.raw_len.contiguous()  # a never-compacted store: directory entry k is record k
    keys = torch.cat([sc.key[:n], torch.randint(1, 255, (n, 32), dtype=torch.uint8, device="cuda")])
    q_arc = torch.cat([sc.arc[:n], sc.arc[:n]]).contiguous()
    hit = ST.lookup(op, q_arc, keys)
    torch.cuda.synchronize()
    assert int((hit.slot >= 0).sum()) == n and torch.equal(hit.store_off[:n], sc.store_off[:n])
    rd = HipBufferReader(L, HL, aes=KEY if aes else None, record_ivs=aes, engine=e)
    sl = slot_bytes(HL, L, 4095)
    out = torch.empty((nbuf, L), dtype=torch.uint8, device="cuda")
    read = lambda: rd.read(m, nbuf, sl, arcs.store, *arcs.directory(), PB, verify=True, out=out,  # noqa: E731
                           store_ivs=arcs.record_ivs())
    _, status, info = read()
    torch.cuda.synchronize()
    assert not status.any() and not info.bad_count.any() and torch.equal(out, batch.data.view(nbuf, L))
    flags, st = ST.scrub(op, e, aes=wr.aes)
    assert not flags.any() and not st.any()
    maps_copy = torch.empty_like(arcs.maps)
    # warm-up: every timed shape, >= 0.5 s
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.5:
        open_()
        ST.lookup(op, q_arc, keys)
        maps_copy.copy_(arcs.maps)
        torch.cuda.synchronize()
    ST.scrub(op, e, aes=wr.aes)
    ST.scrub(op, e, aes=wr.aes, batch_records=1 << 24)
    read()
    torch.cuda.synchronize()

    names = ("scan", "map_copy", "directory", "lookup")
    T = {s: [] for s in names + ("open", "scrub", "scrub_one_slice", "read")}
    S = {}
    for _ in range(reps):
        t = [ev() for _ in range(8)]
        maps_copy.copy_(arcs.maps)  # not timed: keeps the device busy while the host enqueues
        t[0].record()
        ST.scan_store(*images, HL, arcs.version, plain=not aes, max_chunk=mc)
        t[1].record()
        t[2].record()
        maps_copy.copy_(arcs.maps)
        t[3].record()
        t[4].record()
        ST.directory(sc.store_off[:n], sc.len[:n], raw, sc.flags[:n], hashloc, PB, n)
        t[5].record()
        t[6].record()
        ST.lookup(op, q_arc, keys)
        t[7].record()
        torch.cuda.synchronize()
        for i, s in enumerate(names):
            T[s].append(t[2 * i].elapsed_time(t[2 * i + 1]))
        t0 = time.perf_counter()
        open_()
        torch.cuda.synchronize()
        T["open"].append((time.perf_counter() - t0) * 1e3)
        marks = [("start", ev())]
        marks[0][1].record()

        def stage(nm):
            marks.append((nm, ev()))
            marks[-1][1].record()

        t0 = time.perf_counter()
        ST.scrub(op, e, aes=wr.aes, stages=stage)
        torch.cuda.synchronize()
        T["scrub"].append((time.perf_counter() - t0) * 1e3)
        acc = {}
        for (_, a), (nm, b) in zip(marks, marks[1:]):
            acc[nm] = acc.get(nm, 0.0) + a.elapsed_time(b)
        for nm, v in acc.items():
            S.setdefault(nm, []).append(v)
        t0 = time.perf_counter()
        ST.scrub(op, e, aes=wr.aes, batch_records=1 << 24)
        torch.cuda.synchronize()
        T["scrub_one_slice"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        read()
        torch.cuda.synchronize()
        T["read"].append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    res = {"buffers": nbuf, "bytes": nbuf * L, "records": n, "archives": na, "store_bytes": arcs.store_bytes,
           "map_bytes": sum(lens), "queries": 2 * n,
           **{s + "_ms": summary(v) for s, v in T.items()},
           "scrub_stage_ms": {s: summary(v) for s, v in S.items()},
           "scan_over_map_copy": round(med(T["scan"]) / med(T["map_copy"]), 2),
           "scrub_over_read": round(med(T["scrub"]) / med(T["read"]), 3),
           "scrub_one_slice_over_read": round(med(T["scrub_one_slice"]) / med(T["read"]), 3),
           "scrub_gb_s_stored": round(arcs.store_bytes / med(T["scrub"]) / 1e6, 1),
           "lookup_mqueries_s": round(2 * n / med(T["lookup"]) / 1e3, 1)}
    rd.destroy()
    wr.destroy()
    ix.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_open", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    res = {"bench": "store_open", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps}
    for name in ("plain", "aes"):
        res[name] = bench_workload(name, e, nbuf, a.reps)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    e.destroy()


if __name__ == "__main__":
    main()
