#!/usr/bin/env python3
"""Ranged writes on one MI355X (include/sdfs_write.h): HipFileWriter.write_ranges beside
the route a caller had to build before it existed, and the stage kernel beside a plain copy, in the
same process.

Write side: --gib GiB of engine chunks at the default parameters (4 096 buffers of 256 KiB at
1 GiB), all new, through HipBufferWriter.write; one file owns the whole image.  Cases:
    a  4 096 requests of 128 KiB at random 4 KiB-aligned positions
    b  4 096 requests of 4 KiB at random unaligned positions
    c  the whole file as one request
each with accel=True and accel=False.  Per case, after a warm-up, REPS (>= 20) repetitions of
    ranges    write_ranges() end to end: HIP events around it and the host clock around a synchronise
    buffers   the same requests by hand: read() of the touched buffers, the overlay built from
              torch ops (index tensors from the split's pieces), HipBufferWriter.write() of those
              buffers, claim_slots(-1) on the old images and the new images put in their place
    stage     sdfs_cdc_write_stage alone over the case's pieces
    copy      one device-to-device copy of as many bytes as the requests write
The blob is fresh random bytes for every repetition (outside the timed region), so every
repetition stores new chunks; the map image is put back before every repetition, the index is not
(its counts drift, nothing is read back).  With --backup, one more pair of lines at the backup
profile's slot shape: chunk_length 40 MiB, --backup-buffers buffers, --backup-requests requests of
128 KiB.  Every time is median / min / max in ms.  One JSON line per case, printed and appended to
--out.  Nothing is gated."""
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
from sdfs_amd import write as WR  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import HipBufferReader  # noqa: E402

PB = 1 << 33


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, reps, before=None):
    ev_ms, host_ms = [], []
    for _ in range(reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(e0.elapsed_time(e1))
    return ev_ms, host_ms


def bench_case(name, e, cfg, nbuf, requests, reps, accel):
    cl = cfg.chunk_length
    sl = slot_bytes(32, cl, cfg.min_len)
    base = DeviceBatch(e, nbuf=nbuf, buf_len=cl)
    base.fill_streams(first_stream=7000, bufs_per_stream=64)
    ix = HipHashesMap(1 << 25)
    wr = HipBufferWriter(ix, compress=True, min_len=cfg.min_len)
    m0, arcs = wr.write(base, PB)
    del base
    rd = HipBufferReader(cl, 32, engine=e)
    fw = WR.HipFileWriter(wr, rd, e, cl)
    pb2 = PB + int(arcs.store_off.shape[0])
    old = (arcs.store, arcs.store_off, arcs.store_len, arcs.raw_len, PB)
    files = np.array([(0, nbuf, nbuf * cl)], np.int64)
    total = int(requests[:, 2].sum())
    blob = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    m = m0.clone()

    def fresh():
        blob.random_(0, 256)
        m.copy_(m0)

    def ranges():
        return fw.write_ranges(m, nbuf, sl, files, requests, blob, pb2, *old, accel=accel)

    fresh()
    res = ranges()
    torch.cuda.synchronize()
    assert not res.status.any()
    pc = res.pieces
    rows = torch.from_numpy(pc.rows).cuda()
    nrows = len(pc.rows)
    # the route that exists without write_ranges, for the same requests
    hand = DeviceBatch(e, nbuf=nrows, buf_len=cl)
    p_len = torch.from_numpy(pc.len.astype(np.int64)).cuda()
    p_src = torch.from_numpy(pc.src_off).cuda()
    p_dst = torch.from_numpy(pc.row.astype(np.int64) * cl + pc.start).cuda()
    n_bytes = int(pc.len.astype(np.int64).sum())

    def buffers():
        slots = m.view(nbuf, sl)
        rd.read(slots[rows].contiguous(), nrows, sl, *old, out=hand.data.view(nrows, cl))
        first = torch.cumsum(p_len, 0) - p_len  # the overlay: one index per written byte
        within = torch.arange(n_bytes, device="cuda") - torch.repeat_interleave(first, p_len, output_size=n_bytes)
        hand.data[torch.repeat_interleave(p_dst, p_len, output_size=n_bytes) + within] = \
            blob[torch.repeat_interleave(p_src, p_len, output_size=n_bytes) + within]
        images, _ = wr.write(hand, pb2)
        sel = torch.zeros(nbuf, dtype=torch.uint8, device="cuda")
        sel[rows] = 1
        ix.claim_slots(m, nbuf, sl, -1, sel=sel)
        slots[rows] = images.view(nrows, sl)

    stage = torch.empty(nrows * cl + 64, dtype=torch.uint8, device="cuda")
    p_len32 = p_len.to(torch.int32)

    def stage_only():
        WR.stage_pieces(blob, p_src, p_dst, p_len32, cl, stage)

    src, dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    tw, warm = time.perf_counter(), 0  # warm-up: every timed shape, 0.5 s for the clock or three rounds
    while time.perf_counter() - tw < 0.5 and warm < 3:
        warm += 1
        fresh()
        ranges()
        fresh()
        buffers()
        stage_only()
        dst.copy_(src)
        torch.cuda.synchronize()
    r_ev, r_host = timed(ranges, reps, fresh)
    b_ev, b_host = timed(buffers, reps, fresh)
    s_ev, _ = timed(stage_only, reps)
    c_ev, _ = timed(lambda: dst.copy_(src), reps)
    # the stages of one more ranged write, a HIP event after each is enqueued
    fresh()
    marks = [("start", torch.cuda.Event(enable_timing=True))]
    marks[0][1].record()

    def stage_mark(s):
        marks.append((s, torch.cuda.Event(enable_timing=True)))
        marks[-1][1].record()

    res = fw.write_ranges(m, nbuf, sl, files, requests, blob, pb2, *old, accel=accel, stages=stage_mark)
    torch.cuda.synchronize()
    stages = {marks[i + 1][0]: round(marks[i][1].elapsed_time(marks[i + 1][1]), 4) for i in range(len(marks) - 1)}
    med = statistics.median
    routes = np.bincount(res.row_route, minlength=5).tolist()
    line = {"case": name, "accel": accel, "chunk_length": cl, "buffers": nbuf, "requests": len(requests),
            "pieces": res.n_pieces, "runs": res.n_runs, "touched_buffers": nrows, "bytes_written": n_bytes,
            "rows_fail_full_accel_materialise_overflow": routes, "archives": len(res.archives),
            "ranges_event_ms": summary(r_ev), "ranges_host_ms": summary(r_host),
            "buffers_event_ms": summary(b_ev), "buffers_host_ms": summary(b_host),
            "stage_event_ms": summary(s_ev), "copy_event_ms": summary(c_ev), "ranges_stages_ms_one_run": stages,
            "buffers_over_ranges_host": round(med(b_host) / med(r_host), 2),
            "stage_over_copy_event": round(med(s_ev) / max(med(c_ev), 1e-6), 2),
            "ranges_gb_s_of_bytes_written": round(n_bytes / med(r_host) / 1e6, 2)}
    rd.destroy()
    wr.destroy()
    ix.destroy()
    return line


def requests_of(rng, n, siz, file_len, align):
    """n requests of siz bytes, as the int64 table [n, 4] of (file, file_pos, len, src_off)."""
    q = np.zeros((n, 4), np.int64)
    q[:, 1] = rng.integers(0, (file_len - siz) // align + 1, n) * align
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
    ap.add_argument("--backup", action="store_true", help="two more lines at the backup profile's slot shape")
    ap.add_argument("--backup-buffers", type=int, default=4)
    ap.add_argument("--backup-requests", type=int, default=256)
    ap.add_argument("--no-default", action="store_true", help="skip cases a, b and c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_range", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    head = {"bench": "write_range", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    rng = np.random.default_rng(25)
    if not a.no_default:
        cfg = SdfsConfig()
        L = cfg.chunk_length
        nbuf = max(2, int(a.gib * (1 << 30)) // L)
        e = HipVariableSha256HashEngine()
        for name, requests in [("a_128k", requests_of(rng, a.requests, 131072, nbuf * L, 4096)),
                               ("b_4k_unaligned", requests_of(rng, a.requests, 4096, nbuf * L, 1)),
                               ("c_whole_file", np.array([(0, 0, nbuf * L, 0)], np.int64))]:
            for accel in (True, False):
                emit({**head, **bench_case(name, e, cfg, nbuf, requests, a.reps, accel)}, a.out)
                torch.cuda.empty_cache()
        e.destroy()
    if a.backup:
        cfg = SdfsConfig.backup_volume()
        e = HipVariableSha256HashEngine(config=cfg)
        requests = requests_of(rng, a.backup_requests, 131072, a.backup_buffers * cfg.chunk_length, 4096)
        for accel in (True, False):
            line = bench_case("backup_128k", e, cfg, a.backup_buffers, requests, a.reps, accel)
            emit({**head, "max_len": cfg.max_len, **line}, a.out)
            torch.cuda.empty_cache()
        e.destroy()


if __name__ == "__main__":
    main()
