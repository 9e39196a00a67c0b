#!/usr/bin/env python3
"""Map-file lifecycle on one MI355X (include/sdfs_index.h: claim_slots, recount, load, export;
DESIGN §20).

The store of §16-§19: --slots write buffers of 256 KiB of engine chunks at the default parameters
(4 096 = 1 GiB) written by HipBufferWriter, whose map is --slots slots of 7 181 bytes.  Timed, after
a warm-up of every shape, REPS (>= 20) times, the shapes alternating inside each repetition; every
shape twice over: "dev" = HIP events around what it enqueues, "host" = the host clock around the
call and a device synchronise.  Every time is median / min / max in ms:
    snapshot        mapfile.snapshot: the clone of the slots + claim_slots(+1)
    vanish          mapfile.vanish of that snapshot: claim_slots(-1) (the counts are back afterwards)
    recount         HipHashesMap.recount over the file's slots, cap 1024, no repair / repair
    recount_repair
    export          HipHashesMap.export of every entry (one host read for the count)
    load            HipHashesMap.load of that export into a cleared second index
    composed        yardstick 1, the route that existed before: parse_map_slots -> mask selection
                    -> claim_digests(-1, expect_pos = hashloc) for the same -1 per pair (its +1
                    twin, untimed, restores the counts)
    slots_copy      yardstick 2: a device-to-device copy of the slot bytes
    hot / distinct  32 slots x 128 pairs naming ONE digest, against 32 slots of 4 096 distinct
                    digests: what 4 096 atomics on one address cost (claim_slots, dev time)
One JSON line, printed and appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sdfs_amd import HipVariableSha256HashEngine, mapfile  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.extent import _live  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402
from sdfs_amd.read import parse_map_slots  # noqa: E402

L = 262144
PB = 1 << 33


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    """(dev ms, host ms, result) of fn(): events around what it enqueues, host clock to the end."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, r


def hot_images(ix, sl, dev):
    """32 slots whose 128 pairs all name one held digest, 32 slots of 4 096 distinct held digests."""
    import struct

    g = torch.Generator().manual_seed(9)
    dg = torch.randint(0, 256, (4097, 32), dtype=torch.uint8, generator=g)
    pos = torch.arange(4097, dtype=torch.int64) + (1 << 50)
    ix.load(dg.to(dev), pos.to(dev), torch.full((4097,), 1 << 30, dtype=torch.int64, device=dev))
    rows = dg.numpy()

    def image(keys):
        body = b"".join(rows[k].tobytes() + struct.pack(">qiiii", (1 << 50) + k, 2048, i * 2048, 0, 2048)
                        for i, k in enumerate(keys))
        return (struct.pack(">BIi", 0, 13 + len(body), len(keys)) + body + bytes(4)).ljust(sl, b"\0")

    hot = b"".join(image([4096] * 128) for _ in range(32))
    cold = b"".join(image(range(128 * s, 128 * s + 128)) for s in range(32))
    up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)  # noqa: E731
    return up(hot), up(cold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapfile", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    assert a.reps >= 20, "medians of at least 20 runs"
    nbuf = a.slots
    dev = torch.device("cuda:0")
    e = HipVariableSha256HashEngine()
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=7000, bufs_per_stream=64)
    batch.run(buffer_id_base=0)
    nrec = int(batch.total.item())
    ix = HipHashesMap(1 << (4 * nrec + 16384).bit_length())
    ix2 = HipHashesMap(1 << (4 * nrec + 16384).bit_length())
    wr = HipBufferWriter(ix)
    m, arcs = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    sl = slot_bytes(32, L, 4095)
    m = m[: nbuf * sl].contiguous()
    m_copy = torch.empty_like(m)
    every = torch.ones(nbuf, dtype=torch.bool, device=dev)
    state = {}

    def snapshot():
        state["snap"] = mapfile.snapshot(ix, m, nbuf, sl)

    def vanish():
        return ix.claim_slots(state["snap"], nbuf, sl, -1)

    def composed(delta=-1):
        p = parse_map_slots(m, nbuf, sl, 32)
        hashes, hashloc = _live(p, every)
        return ix.claim_digests(hashes.contiguous(), delta, expect_pos=hashloc)

    def export():
        state["export"] = ix.export()
        return state["export"][3]

    def load():
        dg, pos, ref, _ = state["export"]
        return ix2.load(dg, pos, ref)

    shapes = {"snapshot": snapshot, "vanish": vanish, "recount": lambda: ix.recount(m, nbuf, sl, cap=1024),
              "recount_repair": lambda: ix.recount(m, nbuf, sl, cap=1024, repair=True), "export": export, "load": load,
              "composed": composed, "slots_copy": lambda: m_copy.copy_(m)}

    # correctness of what is timed, once: the walk and the composed route agree, the audit is clean
    before = ix.export()
    snapshot()
    res = vanish()
    pairs, held = res.applied, before[3]
    assert res.missed == 0 and res.corrupt == 0 and res.nonempty == nbuf
    out = composed(-1)
    assert int((out != -1).sum().item()) == pairs == int(out.shape[0])
    composed(+1)
    rc = ix.recount(m, nbuf, sl, cap=1024)
    assert (rc.counted, rc.under, rc.over, rc.listed) == (pairs, 0, 0, 0)
    after = ix.export()
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2])
    ix3 = HipHashesMap(8192)  # its own index: these entries are named by no file
    hot, cold = hot_images(ix3, sl, dev)
    assert ix3.claim_slots(hot, 32, sl, -1).applied == 4096 and ix3.claim_slots(cold, 32, sl, -1).applied == 4096
    shapes["hot"] = lambda: ix3.claim_slots(hot, 32, sl, +1)
    shapes["distinct"] = lambda: ix3.claim_slots(cold, 32, sl, +1)

    def one_round(T=None):
        for nm, fn in shapes.items():
            if nm == "load":
                ix2.clear()
            d, h, _ = timed(fn)
            if T is not None:
                T[nm]["dev"].append(d)
                T[nm]["host"].append(h)
            if nm == "composed":
                composed(+1)

    for _ in range(3):
        one_round()
    T = {nm: {"dev": [], "host": []} for nm in shapes}
    for _ in range(a.reps):
        one_round(T)
    med = lambda nm, k="host": statistics.median(T[nm][k])  # noqa: E731
    res = {"bench": "mapfile", "device": torch.cuda.get_device_name(0), "chunk_length": L, "reps": a.reps,
           "slots": nbuf, "slot_bytes": sl, "map_bytes": nbuf * sl, "pairs": pairs, "fingerprints": held,
           **{nm + "_ms": {k: summary(v) for k, v in t.items()} for nm, t in T.items()},
           "composed_over_vanish": round(med("composed") / med("vanish"), 2),
           "vanish_over_slots_copy": round(med("vanish", "dev") / med("slots_copy", "dev"), 1),
           "hot_over_distinct": round(med("hot", "dev") / med("distinct", "dev"), 2)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    wr.destroy()
    ix.destroy()
    ix2.destroy()
    ix3.destroy()
    e.destroy()


if __name__ == "__main__":
    main()
