#!/usr/bin/env python3
"""Read path on one MI355X (include/sdfs_read.h): device time of read() and of each of
its stages, and the gather beside two reference times taken in the same run.

Write side, once per workload: --gib GiB of engine chunks at the default parameters (256 KiB
buffers), all new ("new") or the upper half of the buffers copies of the lower half ("dup"),
through the index, LZ4 framing (putChunk records) and the map images.  Then, per workload:
    stages    parse | plan (with the one host read of the scratch sizes) | decode | assemble,
              a HIP event between them, one stream
    read      HipBufferReader.read() end to end, host clock around a device synchronise
    assemble  sdfs_cdc_read_assemble alone (status kernel + gather kernel): the hot path
    (a) copy  device-to-device copy of the same nbuf x chunk_length bytes: the ceiling
    (b) torch the formulation without the kernel: a byte index from the pair arrays
              (repeat_interleave + arange), then torch.take into the buffers; the take alone is
              timed too
After a warm-up of every timed shape (>= 0.5 s of the gather, which also ramps the clock), REPS
(>= 20) repetitions with assemble, (a) and (b) alternating inside each repetition (an untimed copy
runs ahead of them, so that the events bracket device work, not the host's enqueueing); every time is
reported as median / min / max.  The one condition: the assemble median beats (b)'s median — and
that of (b)'s take alone — by more than the run-to-run spread (max - min) of the two together.
One JSON line, printed and appended to --out; exit status 1 when the condition fails."""
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
from sdfs_amd import read as RD  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.lz4 import HipLz4Compressor  # noqa: E402
from sdfs_amd.meta import emit_map_slots, slot_bytes  # noqa: E402

L = 262144
PB = 1 << 33


def write_side(e, z, nbuf, half_dup):
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    if half_dup:
        v = batch.data.view(nbuf, L)
        v[nbuf // 2:].copy_(v[: nbuf // 2])
    batch.run(buffer_id_base=0)
    recs = batch.record_table()
    ix = HipHashesMap(max(1 << 12, 1 << (int(recs.shape[0]) * 2).bit_length()))
    dup, loc, new, nc = ix.put_records(recs, batch.total, pos_base=PB)
    k = int(nc.item())
    src_off, src_len, dst_off, total = z.plan_records(recs, sel=new[: recs.shape[0]], count=nc.view(torch.int32),
                                                      uniform_len=L)
    src_off, src_len, dst_off = src_off[:k].contiguous(), src_len[:k].contiguous(), dst_off[:k].contiguous()
    store = torch.empty(int(total.item()) + 64, dtype=torch.uint8, device="cuda")
    store_len = torch.zeros(k, dtype=torch.int32, device="cuda")
    z.compress_device(batch.data, src_off, src_len, store, dst_off, store_len, framed=True)
    m, doop, ovf = emit_map_slots(batch, dup, loc)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    ix.destroy()
    return dict(data=batch.data.view(nbuf, L), m=m, store=store, store_off=dst_off, store_len=store_len, raw=src_len,
                k=k, records=int(recs.shape[0]), store_bytes=int(store_len.sum().item()))


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def torch_gather(pairs, pair_fetch, chunks, fetch_off, fetch_len, nbuf, take_only_ev=None):
    """(b): the images of the write path cover every buffer in order without gaps or overlaps, so
    the destination is the concatenation of the pairs' pieces and one source index per output byte
    is all it takes (anything more general needs a scatter on top)."""
    used = pair_fetch.view(-1) >= 0
    f = pair_fetch.view(-1)[used].long()
    ck = fetch_len[f].long()
    c = torch.minimum(pairs.nlen.view(-1)[used].long(), ck)
    src = fetch_off[f] + pairs.offset.view(-1)[used].long()
    excl = torch.cumsum(c, 0) - c
    idx = torch.repeat_interleave(src - excl, c) + torch.arange(int(nbuf) * L, device=chunks.device)
    if take_only_ev is not None:
        take_only_ev[0].record()
    out = torch.take(chunks, idx)
    if take_only_ev is not None:
        take_only_ev[1].record()
    return out.view(nbuf, L)


def bench_workload(name, e, z, nbuf, reps):
    w = write_side(e, z, nbuf, name == "dup")
    sl = slot_bytes(32, L, 4095)
    rd = RD.HipBufferReader(L, 32, engine=e)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def staged(times=None):
        t = [ev() for _ in range(5)]
        t[0].record()
        pairs = RD.parse_map_slots(w["m"], nbuf, sl)
        t[1].record()
        plan = RD.plan_reads(pairs, w["store_off"], w["store_len"], w["raw"], PB)
        chunk_bytes = int(plan["total_bytes"][0].item())
        k = int(plan["fetch_count"].item())
        t[2].record()
        chunks = torch.empty(chunk_bytes + 64, dtype=torch.uint8, device="cuda")
        fetch_len = torch.empty(k, dtype=torch.int32, device="cuda")
        z.decompress_device(w["store"], plan["src_off"][:k], plan["src_len"][:k], chunks, plan["dst_off"][:k],
                            plan["dst_cap"][:k], fetch_len, framed=True)
        t[3].record()
        out = RD.assemble(pairs, L, plan["pair_fetch"], chunks, plan["dst_off"][:k], fetch_len)
        t[4].record()
        torch.cuda.synchronize()
        if times is not None:
            for i, s in enumerate(("parse", "plan", "decode", "assemble")):
                times[s].append(t[i].elapsed_time(t[i + 1]))
        return pairs, plan, chunks, fetch_len, out, k

    pairs, plan, chunks, fetch_len, out, k = staged()
    assert k == w["k"] and not pairs.status.any() and torch.equal(out, w["data"])
    dst_off = plan["dst_off"][:k]
    ref = torch_gather(pairs, plan["pair_fetch"], chunks, dst_off, fetch_len, nbuf)
    assert torch.equal(ref, out)
    del ref
    got, status, info = rd.read(w["m"], nbuf, sl, w["store"], w["store_off"], w["store_len"], w["raw"], PB)
    assert torch.equal(got, w["data"]) and not status.any() and info.fetch_count == k
    del got
    # warm-up: every timed shape, and >= 0.5 s of the gather for the clock
    dst = torch.empty_like(out)
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.5:
        RD.assemble(pairs, L, plan["pair_fetch"], chunks, dst_off, fetch_len, out=out)
        dst.copy_(out)
        torch.cuda.synchronize()
    torch_gather(pairs, plan["pair_fetch"], chunks, dst_off, fetch_len, nbuf)
    staged()
    torch.cuda.synchronize()

    T = {s: [] for s in ("parse", "plan", "decode", "assemble")}
    asm, cpy, tb, tb_take, rd_ms = [], [], [], [], []
    for _ in range(reps):
        a0, a1, c0, c1, b0, b1, k0, k1 = (ev() for _ in range(8))
        dst.copy_(out)  # not timed: keeps the device busy while the host enqueues what is
        a0.record()
        RD.assemble(pairs, L, plan["pair_fetch"], chunks, dst_off, fetch_len, out=out)
        a1.record()
        c0.record()
        dst.copy_(out)
        c1.record()
        b0.record()
        r = torch_gather(pairs, plan["pair_fetch"], chunks, dst_off, fetch_len, nbuf, (k0, k1))
        b1.record()
        torch.cuda.synchronize()
        del r
        asm.append(a0.elapsed_time(a1))
        cpy.append(c0.elapsed_time(c1))
        tb.append(b0.elapsed_time(b1))
        tb_take.append(k0.elapsed_time(k1))
        staged(T)
        t0 = time.perf_counter()
        rd.read(w["m"], nbuf, sl, w["store"], w["store_off"], w["store_len"], w["raw"], PB)
        torch.cuda.synchronize()
        rd_ms.append((time.perf_counter() - t0) * 1e3)
    rd.destroy()
    nbytes = nbuf * L
    med = statistics.median
    spread = lambda v: max(v) - min(v)  # noqa: E731
    res = {"buffers": nbuf, "bytes": nbytes, "records": w["records"], "fetches": k, "store_bytes": w["store_bytes"],
           "stages_ms": {s: summary(v) for s, v in T.items()}, "read_ms": summary(rd_ms),
           "read_gb_s": round(nbytes / med(rd_ms) / 1e6, 1),
           "assemble_ms": summary(asm), "copy_ms": summary(cpy), "torch_ms": summary(tb),
           "torch_take_ms": summary(tb_take),
           "assemble_gb_s_read_plus_write": round(2 * nbytes / med(asm) / 1e6, 1),
           "copy_gb_s_read_plus_write": round(2 * nbytes / med(cpy) / 1e6, 1),
           "assemble_over_copy": round(med(asm) / med(cpy), 3),
           "torch_over_assemble": round(med(tb) / med(asm), 2),
           "torch_take_over_assemble": round(med(tb_take) / med(asm), 2),
           "beats_torch": med(tb) - med(asm) > spread(tb) + spread(asm),
           "beats_torch_take": med(tb_take) - med(asm) > spread(tb_take) + spread(asm)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_path", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    z = HipLz4Compressor()
    res = {"bench": "read_path", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps}
    for name in ("new", "dup"):
        res[name] = bench_workload(name, e, z, nbuf, a.reps)
        torch.cuda.empty_cache()
    res["condition_b_holds"] = all(res[n]["beats_torch"] and res[n]["beats_torch_take"] for n in ("new", "dup"))
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    z.destroy()
    e.destroy()
    sys.exit(0 if res["condition_b_holds"] else 1)


if __name__ == "__main__":
    main()
