#!/usr/bin/env python3
"""Dedup index, the way back, on one MI355X: device time of
put_records, a claim of -1 on every record, the sweep of the then all-dead table, a rebuild, and
clear, at configs[2]'s record count (N, default 1.07 M records, half of them duplicates).

Per repetition, on one stream, with a HIP event between the steps:
    clear | put_records | rebuild (every fingerprint held) | claim -1 per record | sweep (all dead)
    | rebuild (tombstones only)
After a warm-up of the same sequence (>= 0.2 s), REPS repetitions; each time is reported as
median / min / max over the repetitions.  Two relations are reported beside them (same run):
claim <= put_records (the put does strictly more per record) and sweep <= 2 x clear (both stream
the table once; the factor allows for the scan and the scattered stores of the removed list).
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

from sdfs_amd.index import HipHashesMap  # noqa: E402

STEPS = ("clear", "put_records", "rebuild_live", "claim", "sweep", "rebuild_tombstones")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=int(os.environ.get("N", "1070000")))
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_gc", "bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs cuda:0 (no CPU fallback)"
    n = a.records
    g = torch.Generator(device="cuda").manual_seed(2)
    rec = torch.zeros(n, 48, dtype=torch.uint8, device="cuda")
    rec[:, :32] = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    fresh = n // 2  # the second half repeats fingerprints of the first (configs[2]: 50 % duplicates)
    src = torch.randint(0, fresh, (n - fresh,), device="cuda", generator=g)
    rec[fresh:, :32] = rec[src, :32]
    rec[:, 32:40] = (torch.arange(n, device="cuda") // 64).view(n, 1).contiguous().view(torch.uint8).view(n, 8)
    dg = rec[:, :32].contiguous()
    minus = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    distinct = int(torch.unique(dg, dim=0).shape[0])
    ix = HipHashesMap(a.capacity)
    st = ix.stats()
    s = torch.cuda.current_stream()

    def sequence(ev):
        ev[0].record(s)
        ix.clear()
        ev[1].record(s)
        _, _, _, nc = ix.put_records(rec, None, 0)
        ev[2].record(s)
        ix.compact()
        ev[3].record(s)
        ix.claim_digests(dg, minus)
        ev[4].record(s)
        _, _, counts = ix.sweep_device(n)
        ev[5].record(s)
        ix.compact()
        ev[6].record(s)
        return nc, counts

    def events():
        return [torch.cuda.Event(enable_timing=True) for _ in range(len(STEPS) + 1)]

    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.2:
        sequence(events())
        torch.cuda.synchronize()
    times = {k: [] for k in STEPS}
    for _ in range(a.reps):
        ev = events()
        nc, counts = sequence(ev)
        torch.cuda.synchronize()
        assert int(nc.item()) == distinct and counts.tolist() == [distinct, 0]
        for i, k in enumerate(STEPS):
            times[k].append(ev[i].elapsed_time(ev[i + 1]))
    after = ix.stats()
    assert (after.live, after.tombstones) == (0, 0)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"bench": "index_gc", "device": torch.cuda.get_device_name(0), "records": n, "distinct": distinct,
           "slots_usable": st.capacity, "table_mib": round((st.capacity * 8 // 7) * 64 / 2**20, 1), "reps": a.reps,
           "ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                  for k, v in times.items()},
           "claim_over_put": round(med["claim"] / med["put_records"], 3),
           "claim_le_put": med["claim"] <= med["put_records"],
           "sweep_over_clear": round(med["sweep"] / med["clear"], 3),
           "sweep_le_2x_clear": med["sweep"] <= 2 * med["clear"]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    ix.destroy()


if __name__ == "__main__":
    main()
