#!/usr/bin/env python3
"""Importing a map file from another volume on one MI355X (include/sdfs_import.h): the
import end to end and its stages, beside the route that existed before it — HipBufferReader.read
of the file from the source, then HipBufferWriter.write of those buffers into the destination —
in the same run.

The workload is §16/§17's: --gib GiB of engine chunks at the default parameters (256 KiB buffers),
written once into a source volume (LZ4 records).  Three destinations with the source's settings:
    none   an empty index
    half   the index holds the chunks of the file's first half (an earlier import of those slots)
    all    the index holds every chunk (an earlier import of the whole file)
Before each repetition the destination index is cleared and loaded from the exported state; that
is outside the timed region.
    import      HipFileImport.import_file into a fresh map (no verify)
    import_verify  the same with verify=True (none only)
    yardstick   read() of the whole file from the source into a batch's buffers, then write() of
                that batch (chunking, fingerprints, index, store, map images) into the destination
  host clock around a device synchronise, and
    pairs / index_get / plan / fetch / records / put_records / store / release / install
                HIP events around each stage of the import (its `stages` callback); copy_chunks /
                copy_map: a device-to-device copy of the fetched bytes / of the map's bytes
After a warm-up of every timed shape, REPS (>= 20) repetitions; every time is reported as median /
min / max.  One JSON line, printed and appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sdfs_amd import HipVariableSha256HashEngine  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import HipBufferReader  # noqa: E402
from sdfs_amd.replicate import HipFileImport, SourceVolume  # noqa: E402

L = 262144
PB = 1 << 33
HL = 32
STAGES = ("pairs", "index_get", "plan", "fetch", "records", "put_records", "store", "release", "install")


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    sl = slot_bytes(HL, L, 4095)
    # the source volume
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    batch.run(buffer_id_base=0)
    nrec = int(batch.total.item())
    cap = max(1 << 12, 1 << (nrec * 2).bit_length())
    ixs = HipHashesMap(cap)
    ws = HipBufferWriter(ixs, hash_len=HL)
    ms, arcs_s = ws.write(batch, PB, run=False)
    torch.cuda.synchronize()
    src = SourceVolume.from_archives(arcs_s, PB)
    k = arcs_s.n_rec
    # the destination, and the three states of its index
    ixd = HipHashesMap(cap)
    wd = HipBufferWriter(ixd, hash_len=HL)
    imp = HipFileImport(wd, L, engine=e)
    rd = HipBufferReader(L, HL, engine=e)
    back = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    fmap, res, arcs = imp.import_file(src, ms, nbuf, sl, nbuf * L, PB)  # none held: the store write() leaves
    torch.cuda.synchronize()
    sb = arcs_s.store_bytes
    assert not res.status.any() and torch.equal(fmap, ms) and arcs.n_rec == k and arcs.store_bytes == sb
    assert torch.equal(arcs.store[:sb], arcs_s.store[:sb]) and res.counts.tolist() == [nrec, 0, k, res.fetched_bytes,
                                                                                       nbuf, 0, 0, 0]
    rc = ixd.recount(fmap, nbuf, sl)
    assert rc.counts.tolist()[1:6] == [0, 0, 0, 0, 0]
    fetched_bytes = res.fetched_bytes
    state = {"none": None}
    dg, pos, ref, _ = ixd.export()
    state["all"] = (dg.clone(), pos.clone(), torch.zeros_like(ref))  # held, referenced by nothing yet
    ixd.clear()
    hmap = torch.zeros((nbuf // 2) * sl, dtype=torch.uint8, device="cuda")
    imp.import_slots(src, ms.view(nbuf, sl)[: nbuf // 2], list(range(nbuf // 2)), [L] * (nbuf // 2), hmap, sl, 0, PB)
    dg, pos, ref, _ = ixd.export()
    state["half"] = (dg.clone(), pos.clone(), torch.zeros_like(ref))
    held_half = int(dg.shape[0])
    del hmap, fmap, arcs
    torch.cuda.empty_cache()
    pb2 = PB + (1 << 30)  # new chunks go behind everything a state holds

    def reset(name):
        ixd.clear()
        if state[name] is not None:
            ixd.load(*state[name])
        torch.cuda.synchronize()

    def timed(name, f):
        reset(name)
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def do_import(verify=False, stages=None):
        return imp.import_file(src, ms, nbuf, sl, nbuf * L, pb2, verify=verify, stages=stages)

    def yardstick():
        rd.read(ms, nbuf, sl, src.store, src.store_off, src.store_len, src.store_raw_len, PB,
                out=back.data.view(nbuf, L))
        return wd.write(back, pb2)

    def staged(name):
        """One import with an event after every stage: {stage: ms}, the fetch's stages summed."""
        reset(name)
        marks = []

        def mark(stage):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((stage, ev))

        mark("start")
        out = do_import(stages=mark)
        torch.cuda.synchronize()
        t = {s: 0.0 for s in STAGES}
        for (_, e0), (stage, e1) in zip(marks, marks[1:]):
            t[stage if stage in t else "fetch"] += e0.elapsed_time(e1)
        return t, out

    # the yardstick leaves the same bytes in the buffers
    _, _ = timed("none", yardstick)
    assert torch.equal(back.data, batch.data)
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.5:  # warm-up of every timed shape, which also ramps the clock
        for name in state:
            timed(name, do_import)
            timed(name, yardstick)
        timed("none", lambda: do_import(verify=True))
    out = {"bench": "import", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps,
           "buffers": nbuf, "bytes": nbuf * L, "records": nrec, "source_records": k, "store_bytes": sb,
           "fetched_bytes": fetched_bytes, "map_bytes": nbuf * sl, "held_half": held_half}
    for name in state:
        T = {n: [] for n in ("import", "yardstick") + STAGES}
        counts = None
        for _ in range(a.reps):
            ms_i, (_, r, _) = timed(name, do_import)
            counts = r.counts.tolist()
            T["import"].append(ms_i)
            T["yardstick"].append(timed(name, yardstick)[0])
            st, _ = staged(name)
            for s in STAGES:
                T[s].append(st[s])
        med = statistics.median
        out[name] = {"counts": counts, **{n + "_ms": summary(v) for n, v in T.items()},
                     "import_over_yardstick": round(med(T["import"]) / med(T["yardstick"]), 3),
                     "import_faster": med(T["import"]) < med(T["yardstick"])}
    out["none"]["import_verify_ms"] = summary([timed("none", lambda: do_import(verify=True))[0]
                                               for _ in range(a.reps)])
    # the copies the stages are set beside
    chunks = torch.empty(fetched_bytes + 64, dtype=torch.uint8, device="cuda")
    dst_c, dst_m = torch.empty_like(chunks), torch.empty_like(ms)
    cc, cm = [], []
    for _ in range(a.reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        dst_c.copy_(chunks)
        ev[1].record()
        ev[2].record()
        dst_m.copy_(ms)
        ev[3].record()
        torch.cuda.synchronize()
        cc.append(ev[0].elapsed_time(ev[1]))
        cm.append(ev[2].elapsed_time(ev[3]))
    out["copy_chunks_ms"], out["copy_map_ms"] = summary(cc[3:]), summary(cm[3:])
    out["relation_all_held_faster"] = out["all"]["import_faster"]
    out["relation_none_held_faster"] = out["none"]["import_faster"]
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    imp.destroy()
    rd.destroy()
    for w in (ws, wd):
        w.destroy()
    ixs.destroy()
    ixd.destroy()
    e.destroy()


if __name__ == "__main__":
    main()
