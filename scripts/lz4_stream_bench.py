#!/usr/bin/env python3
"""Map files at rest on one MI355X (include/sdfs_lz4_stream.h).

The store of §16-§20: --slots write buffers of 256 KiB of engine chunks at the default parameters
(4 096 = 1 GiB) written by HipBufferWriter, whose map is --slots slots of 7 181 bytes (29.4 MB = 449
blocks of 64 KiB at 4 096 slots).  Timed, after a warm-up of every shape, REPS (>= 20) times, the
shapes alternating inside each repetition; "dev" = HIP events around what a shape enqueues, "host" =
the host clock around the call and a device synchronise.  Every time is median / min / max in ms:
    close_map       mapfile.close_map: the .map.lz4 image of the map (one host read, of its length)
    open_map        mapfile.open_map of that image (two host reads: the sizes, the status)
    compress_dev    HipLz4BlockStream.compress_files alone: everything close_map enqueues
  the writer's stages, each its own entry point alone on the same blocks:
    lz4             yardstick and stage: the bare HipLz4Compressor.compress_device of the blocks
    xxh32_src       HipLz4BlockStream.xxh32 of the source blocks
    (scan + pack    = compress_dev - lz4 - xxh32_src, reported as pack_rest_ms)
  the reader's stages:
    walk            HipLz4BlockStream.scan: the header walk
    decode          yardstick and stage: the bare decompress_device of the same LZ4 blocks
    xxh32_out       xxh32 of the decoded blocks
    (list, RAW copy, verify = open_map dev - walk - decode - xxh32_out, reported as read_rest_ms)
  yardsticks:
    copy            a device-to-device copy of the map's bytes
    cpu_lz4 / cpu_unlz4   liblz4 on 16 host threads over the same blocks (oracle/lz4_sys.c)
    cpu_xxh32       the xxhash module over the same blocks, one host thread (when it imports)
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

from sdfs_amd import HipVariableSha256HashEngine, mapfile  # noqa: E402
from sdfs_amd.archive import HipBufferWriter  # noqa: E402
from sdfs_amd.device import DeviceBatch  # noqa: E402
from sdfs_amd.index import HipHashesMap  # noqa: E402
from sdfs_amd.lz4 import R123, HipLz4Compressor  # noqa: E402
from sdfs_amd.lz4_stream import BLOCK, SEED, HipLz4BlockStream  # noqa: E402
from sdfs_amd.meta import slot_bytes  # noqa: E402

L = 262144
PB = 1 << 33


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4_stream", "bench.jsonl"))
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
    wr = HipBufferWriter(ix)
    m, _ = wr.write(batch, PB, run=False)
    torch.cuda.synchronize()
    sl = slot_bytes(32, L, 4095)
    n = nbuf * sl
    m = torch.cat([m[:n], torch.zeros(64, dtype=torch.uint8, device=dev)])[:n]  # its own storage, room behind it
    z = HipLz4Compressor(R123)
    codec = HipLz4BlockStream(z)

    # the block list of the one file, for the stages timed alone
    nblk = -(-n // BLOCK)
    src_off = torch.arange(nblk, dtype=torch.int64, device=dev) * BLOCK
    src_len = torch.full((nblk,), BLOCK, dtype=torch.int32, device=dev)
    src_len[-1] = n - (nblk - 1) * BLOCK
    room = z.maxCompressedLength(BLOCK)
    lz_off = torch.arange(nblk, dtype=torch.int64, device=dev) * room
    lz_out = torch.empty(nblk * room + 64, dtype=torch.uint8, device=dev)
    lz_len = torch.zeros(nblk, dtype=torch.int32, device=dev)
    dec_out = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    dec_len = torch.zeros(nblk, dtype=torch.int32, device=dev)
    m_copy = torch.empty_like(m)
    state = {}

    def close_map():
        state["image"] = mapfile.close_map(codec, m, nbuf, sl)

    def open_map():
        state["back"] = mapfile.open_map(codec, state["image"], sl)

    shapes = {
        "close_map": close_map,
        "open_map": open_map,
        "compress_dev": lambda: codec.compress_files(m, [0], [n]),
        "lz4": lambda: z.compress_device(m, src_off, src_len, lz_out, lz_off, lz_len, framed=False),
        "xxh32_src": lambda: codec.xxh32(m, src_off, src_len, SEED),
        "walk": lambda: codec.scan(state["image"], [0], [int(state["image"].shape[0])]),
        "decode": lambda: z.decompress_device(lz_out, lz_off, lz_len, dec_out, src_off, src_len, dec_len, framed=False),
        "xxh32_out": lambda: codec.xxh32(dec_out, src_off, src_len, SEED),
        "copy": lambda: m_copy.copy_(m),
    }

    # correctness of what is timed, once
    close_map()
    open_map()
    back, k = state["back"]
    assert k == nbuf and torch.equal(back, m)
    status, n_blocks, decoded, consumed = codec.scan(state["image"], [0], [int(state["image"].shape[0])]).host()
    assert (int(status[0]), int(n_blocks[0]), int(decoded[0]), int(consumed[0])) == (0, nblk, n, int(state["image"].shape[0]))
    shapes["lz4"]()
    shapes["decode"]()
    torch.cuda.synchronize()
    assert torch.equal(dec_len, src_len) and torch.equal(dec_out[:n], m)
    raw_blocks = int((lz_len >= src_len).sum().item())

    def one_round(T=None):
        for nm, fn in shapes.items():
            d, h, _ = timed(fn)
            if T is not None:
                T[nm]["dev"].append(d)
                T[nm]["host"].append(h)

    for _ in range(3):
        one_round()
    T = {nm: {"dev": [], "host": []} for nm in shapes}
    for _ in range(a.reps):
        one_round(T)
    med = lambda nm, k="dev": statistics.median(T[nm][k])  # noqa: E731

    # CPU yardsticks: liblz4 on 16 threads over the same blocks, xxhash on one
    from oracle import lz4_oracle as Z  # the timed CPU baseline only

    host = m.cpu().numpy()
    offs = src_off.cpu().numpy().astype(np.uint64)
    lens = src_len.cpu().numpy().astype(np.uint32)
    cpu = {"cpu_lz4": [], "cpu_unlz4": [], "cpu_xxh32": []}
    try:
        import xxhash
    except ImportError:
        xxhash = None
    for _ in range(a.reps):
        out, oo, ol, secs = Z.system_batch(False, host, offs, lens, lens + lens // 255 + 16, 16)
        cpu["cpu_lz4"].append(secs * 1e3)
        _, _, bl, secs = Z.system_batch(True, out, oo, ol, lens, 16)
        assert (bl == lens).all()
        cpu["cpu_unlz4"].append(secs * 1e3)
        if xxhash is not None:
            t0 = time.perf_counter()
            for o, k in zip(offs, lens):
                xxhash.xxh32(host[int(o): int(o) + int(k)], seed=SEED).intdigest()
            cpu["cpu_xxh32"].append((time.perf_counter() - t0) * 1e3)

    res = {"bench": "lz4_stream", "device": torch.cuda.get_device_name(0), "reps": a.reps, "slots": nbuf,
           "slot_bytes": sl, "map_bytes": n, "blocks": nblk, "raw_blocks": raw_blocks,
           "image_bytes": int(state["image"].shape[0]),
           **{nm + "_ms": {k: summary(v) for k, v in t.items()} for nm, t in T.items()},
           **{nm + "_ms": summary(v) for nm, v in cpu.items() if v},
           "pack_rest_ms": round(med("compress_dev") - med("lz4") - med("xxh32_src"), 4),
           "read_rest_ms": round(med("open_map") - med("walk") - med("decode") - med("xxh32_out"), 4),
           "close_map_gbps": round(n / med("close_map", "host") / 1e6, 3),
           "open_map_gbps": round(n / med("open_map", "host") / 1e6, 3),
           "copy_gbps": round(n / med("copy") / 1e6, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    wr.destroy()
    ix.destroy()
    e.destroy()


if __name__ == "__main__":
    main()
