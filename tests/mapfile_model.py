"""Plain-Python model of the map-file walks over the dedup index — TEST INFRASTRUCTURE ONLY.

The index is a dict ``digest (32 bytes, zero-padded) -> [pos, ref]``; an entry whose count is <= 0
stays until ``sweep``.  Slot images are read with ``tests/read_model.py``'s ``parse`` (the TreeMap
rule, CORRUPT for an image that does not fit or holds a negative field).  Restated from the
reference:

* ``claim_slots``: ``claimKey(hash, hashloc, delta)`` per pair (RocksDBMap.java:388-509 through
  DedupFileStore.addRef / removeRef): held and pos == hashloc -> count += delta, else missed;
* ``vanish`` / ``index`` are claim_slots(-1 / +1) over every slot (LongByteArrayMap.java:817-882,
  884-890);
* ``trim`` (LongByteArrayMap.java:595-648): the slots ceil(pos / CL) .. floor((pos + len) / CL) release
  their pairs and become FREE (zeros);
* ``truncate`` (LongByteArrayMap.java:656-688, 536-539): the map keeps size // CL slots; the slots it
  loses release their pairs (the library's stated divergence: the reference's loop releases others);
* ``recount``: a shadow count per entry of the pairs that name it at its pos, compared with ref;
* ``load`` / ``export``: entries with explicit positions in and out.
"""
from __future__ import annotations

from tests import read_model as R


def pad32(h: bytes) -> bytes:
    return bytes(h).ljust(32, b"\0")


def trim_range(pos: int, length: int, cl: int):
    first = (pos + cl - 1) // cl
    end = (pos + length) // cl
    return (first, end) if end > first else (first, first)


def truncate_keep(size: int, cl: int) -> int:
    return size // cl


class IndexModel:
    def __init__(self):
        self.e = {}

    # ---- the way in and out
    def load(self, items):
        """items: [(digest, pos, ref)] -> [status]."""
        fresh = {}
        for d, p, _ in items:
            d = pad32(d)
            if d not in self.e:
                fresh[d] = min(fresh.get(d, p), p)
        for d, p in fresh.items():
            self.e[d] = [p, 0]
        out = []
        for d, p, r in items:
            ent = self.e[pad32(d)]
            if ent[0] == p:
                ent[1] += r
                out.append(0)
            else:
                out.append(1)
        return out

    def export(self):
        return sorted((d, p, r) for d, (p, r) in self.e.items())

    def sweep(self):
        dead = sorted((d, p) for d, (p, r) in self.e.items() if r <= 0)
        for d, _ in dead:
            del self.e[d]
        return dead

    def claim(self, digest, hashloc, delta) -> bool:
        ent = self.e.get(pad32(digest))
        if ent is None or ent[0] != hashloc:
            return False
        ent[1] += delta
        return True

    # ---- the walks
    def _walk(self, images, slot_bytes, hash_len, sel, apply):
        status, missed, counts = [], [], [0, 0, 0, 0]
        for s, img in enumerate(images):
            if sel is not None and not sel[s]:
                status.append(0)
                missed.append(0)
                continue
            st, pairs, _, _ = R.parse(img, slot_bytes, hash_len)
            miss = 0
            for p in pairs:
                if apply(p[0], p[1]):
                    counts[0] += 1
                else:
                    miss += 1
            counts[1] += miss
            counts[2] += st == R.CORRUPT
            counts[3] += bool(pairs)
            status.append(st)
            missed.append(miss)
        return counts, status, missed

    def claim_slots(self, images, slot_bytes, hash_len, delta, sel=None, free=False):
        """-> (counts[4], status[nslots], missed[nslots], the images afterwards)."""
        counts, status, missed = self._walk(images, slot_bytes, hash_len, sel,
                                            lambda h, loc: self.claim(h, loc, delta))
        out = []
        for s, img in enumerate(images):
            img = bytes(img).ljust(slot_bytes, b"\0")
            on = sel is None or sel[s]
            out.append(bytes(slot_bytes) if free and on and status[s] == 0 else img)
        return counts, status, missed, out

    def recount(self, images, slot_bytes, hash_len, sel=None, repair=False, cap=None, order=None):
        """-> (counts[8], status, missed, [(digest, pos, have, want)] of the first cap mismatches in
        ``order``, a list of digests — the table's slot order, which the model does not know)."""
        want = {d: 0 for d in self.e}

        def count(h, loc):
            ent = self.e.get(pad32(h))
            if ent is None or ent[0] != loc:
                return False
            want[pad32(h)] += 1
            return True

        c, status, missed = self._walk(images, slot_bytes, hash_len, sel, count)
        counts = c[:3] + [0, 0, 0, 0, 0]
        mis = []
        for d in (order if order is not None else sorted(self.e)):
            p, have = self.e[d]
            w = want[d]
            counts[3] += have < w
            counts[4] += have > w
            counts[5] += w == 0
            counts[6] += have == w
            if have != w:
                mis.append((d, p, have, w))
        if cap is not None:
            mis = mis[:cap]
        counts[7] = len(mis)
        if repair:
            for d in self.e:
                self.e[d][1] = want[d]
        return counts, status, missed, mis

    def trim(self, images, slot_bytes, hash_len, pos, length, cl):
        first, end = trim_range(pos, length, cl)
        first, end = min(first, len(images)), min(end, len(images))
        sel = [first <= s < end for s in range(len(images))]
        counts, status, missed, out = self.claim_slots(images, slot_bytes, hash_len, -1, sel, free=True)
        return (first, end), counts, out

    def truncate(self, images, slot_bytes, hash_len, size, cl):
        k = min(truncate_keep(size, cl), len(images))
        sel = [s >= k for s in range(len(images))]
        counts, _, _, _ = self.claim_slots(images, slot_bytes, hash_len, -1, sel)
        return k, counts, [bytes(i).ljust(slot_bytes, b"\0") for i in images[:k]]
