#!/usr/bin/env python3
"""Ranged reads on one MI355X (include/sdfs_read.h): HipBufferReader.read_ranges beside
the whole-buffer route and a plain copy, in the same process.

Write side: scripts/read_path_bench.py's store — --gib GiB of engine chunks at the default
parameters (4 096 buffers of 256 KiB at 1 GiB), all new, through the index, LZ4 framing and the map
images; one file owns the whole image.  Cases:
    a  4 096 requests of 128 KiB at random 4 KiB-aligned positions
    b  4 096 requests of 4 KiB at random 4 KiB-aligned positions
    c  the whole file as one request
Per case, after a warm-up, REPS (>= 20) repetitions of
    ranges    read_ranges() end to end: HIP events around it and the host clock around a synchronise
    buffers   HipBufferReader.read() of exactly the touched buffers (their slots gathered with the
              same torch index read_ranges uses): what a caller had to do before ranged reads —
              slicing the requested bytes out of the buffers is not even counted
    copy      one device-to-device copy of as many bytes as the requests read
and, once, the fetched records and decoded bytes of both routes.  With --backup, one more line at
the backup profile's slot shape: chunk_length 40 MiB, max_len 128 KiB, --backup-buffers buffers,
--backup-requests requests of 128 KiB.  Every time is median / min / max in ms.  One JSON line per case, printed and
appended to --out.  Nothing is gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdfs_amd import HipVariableSha256HashEngine, SdfsConfig  # noqa: E402
from sdfs_amd import read as RD  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.lz4 import HipLz4Compressor  # noqa: E402
from sdfs_amd.meta import emit_map_slots, slot_bytes  # noqa: E402

PB = 1 << 33


def write_side(e, z, nbuf, buf_len):
    """read_path_bench.write_side ("new") for any buffer length."""
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=buf_len)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    batch.run(buffer_id_base=0)
    recs = batch.record_table()
    ix = HipHashesMap(max(1 << 12, 1 << (int(recs.shape[0]) * 2).bit_length()))
    dup, loc, new, nc = ix.put_records(recs, batch.total, pos_base=PB)
    k = int(nc.item())
    src_off, src_len, dst_off, total = z.plan_records(recs, sel=new[: recs.shape[0]], count=nc.view(torch.int32),
                                                      uniform_len=buf_len)
    src_off, src_len, dst_off = src_off[:k].contiguous(), src_len[:k].contiguous(), dst_off[:k].contiguous()
    store = torch.empty(int(total.item()) + 64, dtype=torch.uint8, device="cuda")
    store_len = torch.zeros(k, dtype=torch.int32, device="cuda")
    z.compress_device(batch.data, src_off, src_len, store, dst_off, store_len, framed=True)
    m, doop, ovf = emit_map_slots(batch, dup, loc)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    ix.destroy()
    return dict(data=batch.data.view(-1), m=m, store=store, store_off=dst_off, store_len=store_len, raw=src_len, k=k,
                records=int(recs.shape[0]))


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def decoded_bytes(w, pairs, pair_fetch):
    """Chunk bytes the route decoded: raw_len over the distinct directory entries its pairs name."""
    used = pair_fetch.view(-1) >= 0
    entries = torch.unique(pairs.hashloc.view(-1)[used] - PB)
    return int(w["raw"][entries].long().sum().item())


def bench_case(name, w, rd, cl, sl, nbuf, requests, reps):
    file_len = nbuf * cl
    files = np.array([(0, nbuf, file_len)], np.int64)
    args = (w["store"], w["store_off"], w["store_len"], w["raw"], PB)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    out, n_read, status, info = rd.read_ranges(w["m"], nbuf, sl, files, requests, *args)
    torch.cuda.synchronize()
    assert not status.any()
    total = int(n_read[n_read > 0].sum())
    host = out.cpu().numpy()
    data = w["data"].cpu().numpy()
    for (_, pos, siz, o), n in list(zip(requests.tolist(), n_read.tolist()))[:: max(1, len(requests) // 64)]:
        assert (host[o:o + n] == data[pos:pos + n]).all(), (name, pos, siz)
    del host, data
    rows = info.rows
    slots = w["m"].view(nbuf, sl)

    def buffers_route():
        return rd.read(slots[rows].contiguous(), int(rows.numel()), sl, *args)

    bufs, bstatus, binfo = buffers_route()
    torch.cuda.synchronize()
    assert not bstatus.any()
    counts = {"ranges_fetches": info.fetch_count, "buffers_fetches": binfo.fetch_count,
              "ranges_decoded_bytes": decoded_bytes(w, info.pairs, info.pair_fetch),
              "buffers_decoded_bytes": decoded_bytes(w, binfo.pairs, binfo.pair_fetch)}
    src = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    del bufs
    tw = time.perf_counter()  # warm-up: every timed shape, >= 0.5 s for the clock
    while time.perf_counter() - tw < 0.5:
        rd.read_ranges(w["m"], nbuf, sl, files, requests, *args, out=out)
        buffers_route()
        dst.copy_(src)
        torch.cuda.synchronize()
    r_ev, r_host, b_ev, b_host, c_ev = [], [], [], [], []
    for _ in range(reps):
        e0, e1 = ev(), ev()
        t0 = time.perf_counter()
        e0.record()
        rd.read_ranges(w["m"], nbuf, sl, files, requests, *args, out=out)
        e1.record()
        torch.cuda.synchronize()
        r_host.append((time.perf_counter() - t0) * 1e3)
        r_ev.append(e0.elapsed_time(e1))
        e0, e1 = ev(), ev()
        t0 = time.perf_counter()
        e0.record()
        b = buffers_route()
        e1.record()
        torch.cuda.synchronize()
        b_host.append((time.perf_counter() - t0) * 1e3)
        b_ev.append(e0.elapsed_time(e1))
        del b
        e0, e1 = ev(), ev()
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        c_ev.append(e0.elapsed_time(e1))
    # the stages of one more ranged read, a HIP event after each is enqueued
    marks = [("start", ev())]
    marks[0][1].record()

    def stage(s):
        marks.append((s, ev()))
        marks[-1][1].record()

    rd.read_ranges(w["m"], nbuf, sl, files, requests, *args, out=out, stages=stage)
    torch.cuda.synchronize()
    stages = {marks[i + 1][0]: round(marks[i][1].elapsed_time(marks[i + 1][1]), 4) for i in range(len(marks) - 1)}
    med = statistics.median
    return {"case": name, "chunk_length": cl, "buffers": nbuf, "requests": len(requests), "pieces": len(info.pieces.req),
            "touched_buffers": int(rows.numel()), "bytes_read": total, "touched_bytes": int(rows.numel()) * cl,
            "n_store": w["k"], **counts,
            "ranges_event_ms": summary(r_ev), "ranges_host_ms": summary(r_host),
            "buffers_event_ms": summary(b_ev), "buffers_host_ms": summary(b_host), "copy_event_ms": summary(c_ev),
            "ranges_stages_ms_one_run": stages,
            "buffers_over_ranges_host": round(med(b_host) / med(r_host), 2),
            "ranges_over_copy_event": round(med(r_ev) / max(med(c_ev), 1e-6), 2),
            "ranges_gb_s_of_bytes_read": round(total / med(r_host) / 1e6, 2)}


def aligned_requests(rng, n, siz, file_len):
    """n requests of siz bytes, as the int64 table [n, 4] of (file, file_pos, siz, out_off)."""
    q = np.zeros((n, 4), np.int64)
    q[:, 1] = rng.integers(0, (file_len - siz) // 4096 + 1, n) * 4096
    q[:, 2] = siz
    q[:, 3] = np.arange(n) * siz
    return q


def emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=4096)
    ap.add_argument("--backup", action="store_true", help="one more line at the backup profile's slot shape")
    ap.add_argument("--backup-buffers", type=int, default=4)
    ap.add_argument("--backup-requests", type=int, default=256)
    ap.add_argument("--no-default", action="store_true", help="skip cases a, b and c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_range", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    head = {"bench": "read_range", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    z = HipLz4Compressor()
    rng = np.random.default_rng(22)
    if not a.no_default:
        L = 262144
        nbuf = max(2, int(a.gib * (1 << 30)) // L)
        e = HipVariableSha256HashEngine()
        w = write_side(e, z, nbuf, L)
        rd = RD.HipBufferReader(L, 32, engine=e)
        sl = slot_bytes(32, L, 4095)
        for name, requests in [("a_128k", aligned_requests(rng, a.requests, 131072, nbuf * L)),
                               ("b_4k", aligned_requests(rng, a.requests, 4096, nbuf * L)),
                               ("c_whole_file", np.array([(0, 0, nbuf * L, 0)], np.int64))]:
            emit({**head, **bench_case(name, w, rd, L, sl, nbuf, requests, a.reps)}, a.out)
            torch.cuda.empty_cache()
        rd.destroy()
        e.destroy()
        del w
        torch.cuda.empty_cache()
    if a.backup:
        cfg = SdfsConfig.backup_volume()
        cl = cfg.chunk_length
        e = HipVariableSha256HashEngine(config=cfg)
        w = write_side(e, z, a.backup_buffers, cl)
        rd = RD.HipBufferReader(cl, 32, engine=e)
        sl = slot_bytes(32, cl, cfg.min_len)
        requests = aligned_requests(rng, a.backup_requests, 131072, a.backup_buffers * cl)
        line = bench_case("backup_128k", w, rd, cl, sl, a.backup_buffers, requests, a.reps)
        emit({**head, "max_len": cfg.max_len, "pair_cap": RD.pair_cap(sl, 32), **line}, a.out)
        rd.destroy()
        e.destroy()
    z.destroy()


if __name__ == "__main__":
    main()
