#!/usr/bin/env python3
"""Client-side dedup on one MI355X (include/sdfs_ingest.h, sdfs_cdc_index_addref_slots):
the client route end to end and its stages, beside HipBufferWriter.write() on the same buffers in
the same run.

Per workload — --gib GiB of engine chunks at the default parameters (256 KiB buffers), all new
("new") or the upper half of the buffers copies of the lower half ("dup").  The client's side is
prepared once, outside the timed region: the buffers are chunked by the engine, the first
occurrence of each fingerprint is an entry of the writeChunks batch (raw payloads lying in the
buffers themselves, at whatever offset the cut left them; "lz4": the same chunks as LZ4 blocks), the
SparseDataChunk images and their `inserted` flags are those the answers give.
    write       HipBufferWriter.write(run=False): index -> LZ4 -> plan -> pack -> map images
                (the yardstick: the same code as the parent commit's write() behind the chunking)
    write_run   the same with the chunking (run=True)
    route       check_hashes + write_chunks + write_sparse_data_chunks into a zeroed map
    route_lz4   the same with LZ4 payloads
    write_chunks / write_chunks_lz4 / sparse    the two halves of the route on their own
  host clock around a device synchronise, the index cleared before each, and
    plan / copy / records / addref   HIP events around the call; (a) copy_d2d: a device-to-device
                copy of the staged bytes
After a warm-up of every timed shape, REPS (>= 20) repetitions; every time is reported as median /
min / max.  One JSON line, printed and appended to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sdfs_amd import HipVariableSha256HashEngine, _lib  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.ingest import ChunkBatch, HipChunkIngest  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import pair_cap  # noqa: E402

L = 262144
PB = 1 << 33
HL = 32


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def bench_workload(name, e, nbuf, reps):
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    if name == "dup":
        v = batch.data.view(nbuf, L)
        v[nbuf // 2:].copy_(v[: nbuf // 2])
    batch.run(buffer_id_base=0)
    nrec = int(batch.total.item())
    ix = HipHashesMap(max(1 << 12, 1 << (nrec * 2).bit_length()))
    wr = HipBufferWriter(ix, hash_len=HL)
    ing = HipChunkIngest(wr, L, engine=e)
    sl = slot_bytes(HL, L, 4095)
    stride = pair_cap(sl, HL)
    # route A once: the store and the map every client run must reproduce
    ma, arcs_a = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    k, sb = arcs_a.n_rec, arcs_a.store_bytes
    # the client's side, from A's answers: the first occurrences are the entries
    recs = batch.recs.view(-1, 48)[:nrec]
    dup = arcs_a.extra["dup"][:nrec]
    new = arcs_a.extra["new_list"].long()
    fields = recs[:, 32:].contiguous().view(torch.int64).view(nrec, 2)  # u64 buffer_id | u32 start, u32 len
    buf, start, ln = fields[:, 0], fields[:, 1] & 0xFFFFFFFF, fields[:, 1] >> 32
    digests = recs[:, :32].contiguous()
    ent_len = ln[new].to(torch.int32).contiguous()
    raw_total = int(ent_len.sum().item())
    raw_batch = ChunkBatch(digests[new].contiguous(), batch.data, (buf[new] * L + start[new]).contiguous(), ent_len,
                           ent_len, torch.zeros(k, dtype=torch.uint8, device="cuda"), raw_total)
    # the same chunks as LZ4 blocks, each where the compressor's plan put it (any alignment)
    z = wr._z
    src_off, src_len, dst_off, total = z.plan_records(recs, sel=arcs_a.extra["new_list"].contiguous(), uniform_len=L,
                                                      framed=False)
    area = torch.empty(int(total.item()) + 16, dtype=torch.uint8, device="cuda")
    blk_len = torch.zeros(k, dtype=torch.int32, device="cuda")
    z.compress_device(batch.data, src_off, src_len, area, dst_off, blk_len, framed=False)
    lz4_batch = ChunkBatch(raw_batch.hash, area, dst_off.contiguous(), blk_len, ent_len,
                           torch.ones(k, dtype=torch.uint8, device="cuda"), raw_total)
    # the images are A's own; pair i of buffer b is `inserted` iff its record was not a duplicate
    first = torch.cumsum(batch.counts.long(), 0) - batch.counts.long()
    which = torch.arange(nrec, device="cuda") - first[buf]
    flags = torch.zeros(nbuf, stride, dtype=torch.uint8, device="cuda")
    flags[buf, which] = 1 - dup
    images = ma.view(nbuf, sl).clone()
    dests, lens = list(range(nbuf)), [L] * nbuf
    fmap = torch.zeros(nbuf * sl, dtype=torch.uint8, device="cuda")

    def route(b):
        held = ing.check_hashes(digests)
        res = ing.write_chunks(b, PB)
        out = ing.write_sparse_data_chunks(fmap, sl, dests, images, lens, 0, inserted=flags)
        return held, res, out

    for b in (raw_batch, lz4_batch):  # the route leaves A's store, map and index
        ix.clear()
        fmap.zero_()
        held, res, out = route(b)
        torch.cuda.synchronize()
        arcs_b = res[4]
        assert bool((held == -1).all()) and not res[3].any() and not out.status.any()
        assert arcs_b.n_rec == k and arcs_b.store_bytes == sb and torch.equal(arcs_b.store[:sb], arcs_a.store[:sb])
        assert torch.equal(fmap, ma) and out.counts.tolist() == [nrec - k, 0, k, nbuf, 0, 0]
        rc = ix.recount(fmap, nbuf, sl)
        assert rc.counts.tolist()[1:5] == [0, 0, 0, 0]
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    # the stages alone run on the raw batch's plan
    ix.clear()
    res = ing.write_chunks(raw_batch, PB)
    cb, cp, pt = res[4].extra["plan"]
    B, P, stage = ctypes.byref(cb), ctypes.byref(cp), res[4].extra["stage"]
    recs_out = torch.zeros(k, 48, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(stage)
    torch.cuda.synchronize()

    def timed_host(f):
        ix.clear()
        fmap.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def sparse_after_chunks():
        return ing.write_sparse_data_chunks(fmap, sl, dests, images, lens, 0, inserted=flags)

    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.5:  # warm-up, which also ramps the clock
        lib.sdfs_cdc_ingest_chunks_copy(0, B, P, L, stage.data_ptr(), s)
        dst.copy_(stage)
        torch.cuda.synchronize()
    T = {n: [] for n in ("write", "write_run", "route", "route_lz4", "write_chunks", "write_chunks_lz4", "sparse",
                         "plan", "copy", "copy_d2d", "records", "addref")}
    for _ in range(reps):
        T["write"].append(timed_host(lambda: wr.write(batch, PB, run=False)))
        T["write_run"].append(timed_host(lambda: wr.write(batch, PB)))
        T["route"].append(timed_host(lambda: route(raw_batch)))
        T["route_lz4"].append(timed_host(lambda: route(lz4_batch)))
        T["write_chunks_lz4"].append(timed_host(lambda: ing.write_chunks(lz4_batch, PB)))
        T["write_chunks"].append(timed_host(lambda: ing.write_chunks(raw_batch, PB)))
        fmap.zero_()  # the index holds the chunks of the call above
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sparse_after_chunks()
        torch.cuda.synchronize()
        T["sparse"].append((time.perf_counter() - t0) * 1e3)
        t = [ev() for _ in range(10)]
        dst.copy_(stage)  # not timed: keeps the device busy while the host enqueues
        t[0].record()
        _lib.check(lib.sdfs_cdc_ingest_chunks_plan(0, B, L, raw_total, P, s))
        t[1].record()
        t[2].record()
        _lib.check(lib.sdfs_cdc_ingest_chunks_copy(0, B, P, L, stage.data_ptr(), s))
        t[3].record()
        t[4].record()
        dst[:raw_total].copy_(stage[:raw_total])
        t[5].record()
        t[6].record()
        _lib.check(lib.sdfs_cdc_ingest_chunks_records(0, B, P, recs_out.data_ptr(), cnt.data_ptr(), s))
        t[7].record()
        t[8].record()
        ing.addref_slots(images.view(-1), nbuf, sl, flags)
        t[9].record()
        torch.cuda.synchronize()
        for i, n in enumerate(("plan", "copy", "copy_d2d", "records", "addref")):
            T[n].append(t[2 * i].elapsed_time(t[2 * i + 1]))
    med = statistics.median
    out = {"buffers": nbuf, "bytes": nbuf * L, "records": nrec, "entries": k, "staged_bytes": raw_total,
           "lz4_payload_bytes": int(blk_len.sum().item()), "store_bytes": sb, "archives": arcs_a.n_arc,
           **{n + "_ms": summary(v) for n, v in T.items()},
           "route_over_write": round(med(T["route"]) / med(T["write"]), 3),
           "route_lz4_over_write": round(med(T["route_lz4"]) / med(T["write"]), 3),
           "copy_over_d2d": round(med(T["copy"]) / med(T["copy_d2d"]), 3),
           "copy_gb_s_read_plus_write": round(2 * raw_total / med(T["copy"]) / 1e6, 1)}
    wr.destroy()
    ix.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    res = {"bench": "ingest", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps}
    for name in ("new", "dup"):
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
