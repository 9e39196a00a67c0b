#!/usr/bin/env python3
"""Chunk store layer on one MI355X (include/sdfs_archive.h): device time of plan, pack
and map_emit, write() and compaction end to end, and the pack beside three reference times taken in
the same run.

Per workload — --gib GiB of engine chunks at the default parameters (256 KiB buffers), all new
("new") or the upper half of the buffers copies of the lower half ("dup"):
    plan / pack / map_emit   HIP events around each call, one stream
    write     HipBufferWriter.write() end to end (run -> index -> LZ4 -> plan -> pack -> map_emit
              -> map slots), host clock around a device synchronise, the index cleared before each
    compact   HipBlobArchiver.compact() with a seeded half of the records kept, host clock
    (a) copy  device-to-device copy of store_bytes: the ceiling
    (b) torch the same packing without the kernel: byte indices from repeat_interleave + arange,
              torch.take of the payload and index_copy_ into a zeroed store, the headers built
              from byte arithmetic and scattered the same way
    (c) gather  sdfs_cdc_read_assemble over the same buffers beside a copy of its own bytes
              (scripts/read_path_bench.py's write side), for its ratio to the copy
After a warm-up of every timed shape (>= 0.5 s of the pack, which also ramps the clock), REPS (>= 20)
repetitions with pack, (a), (b) and (c) alternating inside each repetition (an untimed copy runs
ahead, so that the events bracket device work, not the host's enqueueing); every time is reported
as median / min / max.  One JSON line, printed and appended to --out."""
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

import read_path_bench as RPB  # noqa: E402
from sdfs_amd import HipVariableSha256HashEngine  # noqa: E402
from sdfs_amd import read as RD  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.lz4 import HipLz4Compressor  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402

L = RPB.L
PB = RPB.PB
HL = 32


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def be32(v):
    """int64 [n] -> uint8 [n, 4], big-endian."""
    return torch.stack([(v >> s) & 255 for s in (24, 16, 8, 0)], 1).to(torch.uint8)


def torch_pack(arcs, src, src_off, src_len, digests, store_bytes):
    """(b): a zeroed store, the payload by one index pair per byte, the headers likewise."""
    n = int(src_len.shape[0])
    ln = src_len.long()
    excl = torch.cumsum(ln, 0) - ln
    ar = torch.arange(int(ln.sum().item()), device=src.device)
    s_idx = torch.repeat_interleave(src_off - excl, ln) + ar
    d_idx = torch.repeat_interleave(arcs.layout.store_off[:n] - excl, ln) + ar
    store = torch.zeros(store_bytes, dtype=torch.uint8, device=src.device)
    store.index_copy_(0, d_idx, torch.take(src, s_idx))
    hdr = torch.cat([be32(torch.full((n,), HL, dtype=torch.int64, device=src.device)), digests, be32(ln)], 1)
    h_idx = (arcs.layout.store_off[:n] - (8 + HL)).unsqueeze(1) + torch.arange(8 + HL, device=src.device)
    store.index_copy_(0, h_idx.reshape(-1), hdr.reshape(-1))
    return store


def bench_workload(name, e, z, nbuf, reps):
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
    A = wr.archiver
    m, arcs = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    k, sb = arcs.n_rec, arcs.store_bytes
    # the stages alone, over the records write() stored: the LZ4 output area again
    recs = batch.recs.view(-1, 48)
    new = arcs.extra["new_list"].contiguous()
    src_off, src_len, dst_off, total = z.plan_records(recs, sel=new, uniform_len=L)
    area = torch.empty((int(total.item()) + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    rec_len = torch.zeros(k, dtype=torch.int32, device="cuda")
    z.compress_device(batch.data, src_off, src_len, area, dst_off, rec_len, framed=True)
    digests = recs[new.long(), :HL].contiguous()
    lay = A.plan(rec_len, arc_cap=arcs.layout.arc_cap)
    store = torch.empty(sb + 16, dtype=torch.uint8, device="cuda")
    A.pack(lay, area, dst_off, rec_len, recs, new, store=store, store_bytes=sb)
    torch.cuda.synchronize()
    assert torch.equal(store[:sb], arcs.store[:sb])
    ref = torch_pack(arcs, area, dst_off, rec_len, digests, sb)
    assert torch.equal(ref, store[:sb])
    del ref
    # (c): the read gather over the same buffers
    w = RPB.write_side(e, z, nbuf, name == "dup")
    sl = slot_bytes(HL, L, 4095)
    pairs = RD.parse_map_slots(w["m"], nbuf, sl)
    plan = RD.plan_reads(pairs, w["store_off"], w["store_len"], w["raw"], PB)
    fk = int(plan["fetch_count"].item())
    chunks = torch.empty(int(plan["total_bytes"][0].item()) + 64, dtype=torch.uint8, device="cuda")
    fetch_len = torch.empty(fk, dtype=torch.int32, device="cuda")
    z.decompress_device(w["store"], plan["src_off"][:fk], plan["src_len"][:fk], chunks, plan["dst_off"][:fk],
                        plan["dst_cap"][:fk], fetch_len, framed=True)
    out = RD.assemble(pairs, L, plan["pair_fetch"], chunks, plan["dst_off"][:fk], fetch_len)
    assert torch.equal(out, w["data"])
    out2 = torch.empty_like(out)
    dst = torch.empty_like(store)
    g = torch.Generator(device="cuda").manual_seed(5)
    keep = (torch.rand(k, device="cuda", generator=g) < 0.5).to(torch.uint8)
    # warm-up: every timed shape, and >= 0.5 s of the pack for the clock
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.5:
        A.pack(lay, area, dst_off, rec_len, recs, new, store=store, store_bytes=sb)
        dst.copy_(store)
        torch.cuda.synchronize()
    torch_pack(arcs, area, dst_off, rec_len, digests, sb)
    A.map_emit(lay, rec_len, recs, new, n_arc=arcs.n_arc)
    A.compact(arcs, keep)
    RD.assemble(pairs, L, plan["pair_fetch"], chunks, plan["dst_off"][:fk], fetch_len, out=out)
    out2.copy_(out)
    torch.cuda.synchronize()

    T = {s: [] for s in ("plan", "pack", "map_emit", "copy", "torch", "gather", "gather_copy", "write", "compact")}
    for _ in range(reps):
        t = [ev() for _ in range(14)]
        dst.copy_(store)  # not timed: keeps the device busy while the host enqueues what is
        t[0].record()
        A.plan(rec_len, arc_cap=arcs.layout.arc_cap, lay=lay)
        t[1].record()
        t[2].record()
        A.pack(lay, area, dst_off, rec_len, recs, new, store=store, store_bytes=sb)
        t[3].record()
        t[4].record()
        dst[:sb].copy_(store[:sb])
        t[5].record()
        t[6].record()
        A.map_emit(lay, rec_len, recs, new, n_arc=arcs.n_arc)
        t[7].record()
        t[8].record()
        r = torch_pack(arcs, area, dst_off, rec_len, digests, sb)
        t[9].record()
        t[10].record()
        RD.assemble(pairs, L, plan["pair_fetch"], chunks, plan["dst_off"][:fk], fetch_len, out=out)
        t[11].record()
        t[12].record()
        out2.copy_(out)
        t[13].record()
        torch.cuda.synchronize()
        del r
        for i, s in enumerate(("plan", "pack", "copy", "map_emit", "torch", "gather", "gather_copy")):
            T[s].append(t[2 * i].elapsed_time(t[2 * i + 1]))
        ix.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wr.write(batch, PB)
        torch.cuda.synchronize()
        T["write"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        half = A.compact(arcs, keep)
        torch.cuda.synchronize()
        T["compact"].append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    spread = lambda v: max(v) - min(v)  # noqa: E731
    pack_ratio, gather_ratio = med(T["pack"]) / med(T["copy"]), med(T["gather"]) / med(T["gather_copy"])
    res = {"buffers": nbuf, "bytes": nbuf * L, "records": nrec, "stored_records": k, "archives": arcs.n_arc,
           "store_bytes": sb, "kept_records": half.n_rec, "kept_store_bytes": half.store_bytes,
           **{s + "_ms": summary(v) for s, v in T.items()},
           "pack_gb_s_read_plus_write": round(2 * sb / med(T["pack"]) / 1e6, 1),
           "copy_gb_s_read_plus_write": round(2 * sb / med(T["copy"]) / 1e6, 1),
           "write_gb_s": round(nbuf * L / med(T["write"]) / 1e6, 1),
           "pack_over_copy": round(pack_ratio, 3), "gather_over_copy": round(gather_ratio, 3),
           "torch_over_pack": round(med(T["torch"]) / med(T["pack"]), 2),
           "pack_ratio_above_gather_ratio_beyond_spread": (
               pack_ratio - gather_ratio
               > spread(T["pack"]) / med(T["copy"]) + spread(T["gather"]) / med(T["gather_copy"]))}
    wr.destroy()
    ix.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    z = HipLz4Compressor()
    res = {"bench": "archive", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps}
    for name in ("new", "dup"):
        res[name] = bench_workload(name, e, z, nbuf, a.reps)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    z.destroy()
    e.destroy()


if __name__ == "__main__":
    main()
