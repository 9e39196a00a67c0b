#!/usr/bin/env python3
"""Extent copies and block rewrites on one MI355X (include/sdfs_extent.h).

The store of §16-§18: --gib GiB of engine chunks at the default parameters (256 KiB buffers) written
by HipBufferWriter with LZ4.  Timed, after a warm-up of every shape, REPS (>= 20) times, the shapes
alternating inside each repetition; every time is median / min / max:
    copy            copy_extents of the whole file into a fresh file, shifted by 12 345 bytes (host
                    clock around a device synchronise), its stages parse / extents / insert / emit /
                    claims from HIP events recorded as each is enqueued (the one host read falls
                    into "insert")
    rewrite         rewrite_blocks of one 64 KiB run of new data per buffer at offset 100 000, the
                    same way; its "write" stage is HipBufferWriter.write of the runs
    slots_copy      yardstick 1: a device-to-device copy of the destination slots' bytes
    copy_by_data    yardstick 2 for copy: what a caller had to do before — HipBufferReader.read of
    rewrite_by_data the touched buffers, the overlay as a device copy, HipBufferWriter.write of
                    them as whole buffers (code this feature does not change)
One JSON line, printed and appended to --out."""
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

from sdfs_amd import HipVariableSha256HashEngine, copy_extents, rewrite_blocks, split_extent  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import HipBufferReader  # noqa: E402

L = 262144
RL = 65536
PB = 1 << 33
SHIFT = 12345
RUN_POS = 100000


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


class Stages:
    """HIP events recorded as each stage is enqueued; ms per stage after a synchronise."""

    def __init__(self):
        self.marks = [("start", torch.cuda.Event(enable_timing=True))]
        self.marks[0][1].record()

    def __call__(self, name):
        self.marks.append((name, torch.cuda.Event(enable_timing=True)))
        self.marks[-1][1].record()

    def ms(self):
        return {nm: a.elapsed_time(b) for (_, a), (nm, b) in zip(self.marks, self.marks[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extent", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = max(2, int(a.gib * (1 << 30)) // L)
    e = HipVariableSha256HashEngine()
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    batch.run(buffer_id_base=0)
    nrec = int(batch.total.item())
    # room for the runs' new records of every repetition
    ix = HipHashesMap(1 << (4 * nrec + (a.reps + 4) * nbuf * 24).bit_length())
    wr = HipBufferWriter(ix)
    m, arcs = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    sl = slot_bytes(32, L, 4095)
    k1 = int(arcs.store_off.shape[0])
    rd = HipBufferReader(L, 32, engine=e)
    segs = np.asarray(split_extent(0, SHIFT, nbuf * L, L), dtype=np.uint32)  # prepared once, like the slots
    nd = nbuf + 1
    dst = torch.zeros(nd * sl, dtype=torch.uint8, device="cuda")
    dst_copy = torch.empty_like(dst)
    m_keep = m.clone()
    runs = DeviceBatch(e, nbuf=nbuf, buf_len=RL)
    whole = DeviceBatch(e, nbuf=nd, buf_len=L)   # yardstick 2's whole-buffer writes
    out = torch.empty((nbuf, L), dtype=torch.uint8, device="cuda")
    state = {"pb": PB + k1, "stream": 900000}
    run_buf, run_pos = np.arange(nbuf), np.full(nbuf, RUN_POS)

    def fresh_runs():
        runs.fill_streams(first_stream=state["stream"], bufs_per_stream=1)
        state["stream"] += nbuf

    def next_pb(n):
        pb = state["pb"]
        state["pb"] += n
        return pb

    def copy(stages=None):
        dst.zero_()
        return copy_extents(m_keep, dst, nbuf, nd, sl, segs, index=ix, chunk_length=L, stages=stages)

    def rewrite(timed=False):
        m.copy_(m_keep)
        fresh_runs()
        torch.cuda.synchronize()
        stages = Stages() if timed else None
        t0 = time.perf_counter()
        r = rewrite_blocks(wr, runs, next_pb(nbuf * runs.cap), m, nbuf, sl, run_buf, run_pos,
                           chunk_length=L, stages=stages)
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3, stages

    def read_all():
        got, status, _ = rd.read(m_keep, nbuf, sl, arcs.store, *arcs.directory(), PB, out=out)
        return got

    def copy_by_data():
        got = read_all()
        whole.data.zero_()
        whole.data[SHIFT: SHIFT + nbuf * L].copy_(got.view(-1))
        return wr.write(whole, next_pb(nd * whole.cap))

    def rewrite_by_data():
        got = read_all()
        got[:, RUN_POS: RUN_POS + RL].copy_(runs.data.view(nbuf, RL))
        batch.data.copy_(got.view(-1))
        return wr.write(batch, next_pb(nbuf * batch.cap))

    # correctness of what is timed, once
    _, status, seg_status, info = copy()
    torch.cuda.synchronize()
    assert info.written and not status.any() and not seg_status.any()
    (_, status, _, rinfo), _, _ = rewrite()
    assert not status.any()
    n_ins_copy, n_ins_rewrite = info.n_inserts, rinfo.n_inserts
    # warm-up: every timed shape
    for _ in range(2):
        copy()
        rewrite()
        copy_by_data()
        rewrite_by_data()
        dst_copy.copy_(dst)
        torch.cuda.synchronize()

    T = {s: [] for s in ("copy", "rewrite", "slots_copy", "copy_by_data", "rewrite_by_data")}
    S = {"copy": {}, "rewrite": {}}
    for _ in range(a.reps):
        dst.zero_()
        torch.cuda.synchronize()
        st = Stages()
        t0 = time.perf_counter()
        copy_extents(m_keep, dst, nbuf, nd, sl, segs, index=ix, chunk_length=L, stages=st)
        torch.cuda.synchronize()
        T["copy"].append((time.perf_counter() - t0) * 1e3)
        for nm, v in st.ms().items():
            S["copy"].setdefault(nm, []).append(v)
        _, ms, st = rewrite(timed=True)
        T["rewrite"].append(ms)
        for nm, v in st.ms().items():
            S["rewrite"].setdefault(nm, []).append(v)
        t = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t[0].record()
        dst_copy.copy_(dst)
        t[1].record()
        torch.cuda.synchronize()
        T["slots_copy"].append(t[0].elapsed_time(t[1]))
        for nm, fn in (("copy_by_data", copy_by_data), ("rewrite_by_data", rewrite_by_data)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            T[nm].append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    res = {"bench": "extent", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps,
           "buffers": nbuf, "bytes": nbuf * L, "records": nrec, "slot_bytes": sl, "segments": len(segs),
           "copy_inserts": n_ins_copy, "rewrite_inserts": n_ins_rewrite, "run_bytes": RL,
           **{s + "_ms": summary(v) for s, v in T.items()},
           "copy_stage_ms": {s: summary(v) for s, v in S["copy"].items()},
           "rewrite_stage_ms": {s: summary(v) for s, v in S["rewrite"].items()},
           "copy_over_slots_copy": round(med(T["copy"]) / med(T["slots_copy"]), 1),
           "copy_by_data_over_copy": round(med(T["copy_by_data"]) / med(T["copy"]), 2),
           "rewrite_by_data_over_rewrite": round(med(T["rewrite_by_data"]) / med(T["rewrite"]), 2)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    rd.destroy()
    wr.destroy()
    ix.destroy()
    e.destroy()


if __name__ == "__main__":
    main()
