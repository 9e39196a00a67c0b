"""Plain-Python model of the map-file import — TEST INFRASTRUCTURE ONLY.

The rule of include/sdfs_import.h, restated over ``tests/mapfile_model.IndexModel`` (a dict
``digest -> [pos, ref]``) one request at a time:

1. an image is read by the rule of the map-file walks (``ingest_model.counting_pairs``): corrupt
   images, negative fields, the TreeMap rule for a repeated pos; every counting pair counts;
2. a counting pair whose fingerprint the destination index holds (before the batch) is held; any
   other is wanted and must name a live source directory entry (``k = hashloc - src_pos_base`` as an
   unsigned 64-bit value, ``k < n_src``, ``store_len != 0``, ``0 < raw_len <= max_chunk``) or its
   request gets EMISSING;
3. the entries wanted by the requests that are still clean are fetched, each once, in ascending k
   (fetch f lies at the prefix of ``raw_len`` rounded up to 16);
4. a fetch that fails or whose length is not ``raw_len`` gives EFETCH to every clean request that
   uses it; with verify, a wanted pair whose fetch succeeded and whose hash is not the chunk's
   digest gives EHASH;
5. the counting pairs of the accepted requests, in (request, image place) order, are fingerprint
   records ``(hash, f, 0, len)`` / ``(hash, 0, 0, 0)``, applied as ``put_records`` applies them;
6. every accepted request releases the pairs of the slot it replaces, then becomes that slot's
   bytes — image bytes first, the rest zero, the counting pairs' hashlocs rewritten to where their
   fingerprints live in the destination — and moves the file length.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

from tests import ingest_model as IM
from tests import mapfile_model as MM
from tests import read_model as R

CORRUPT, EMISSING, EFETCH, EHASH = R.CORRUPT, 32, 64, 128


@dataclass
class SourceModel:
    """entries[k] = (store_len, raw_len, chunk): what the source's record of hashloc pos_base + k
    decodes to (``None``: the fetch fails); store_len 0 = a dropped entry."""

    pos_base: int
    entries: list


@dataclass
class Imported:
    status: list
    req_missed: list
    pair_rec: list      # per request: {image place: record}
    counts: list        # records, held, fetches, raw bytes fetched, accepted, rejected, hashloc changed, missed
    records: list       # (hash32, buffer_id, start, len)
    fetches: list       # directory entries, ascending
    dst_off: list
    new_list: list      # records that inserted
    hashloc: list       # per record
    file_len: int
    chunks: dict = field(default_factory=dict)  # pos -> the chunk stored there by this call


def _r16(n: int) -> int:
    return (n + 15) // 16 * 16


class ImportModel:
    def __init__(self, index: MM.IndexModel, chunk_length: int, digest=None):
        self.ix, self.cl, self.digest = index, chunk_length, digest

    def import_slots(self, src: SourceModel, images, dests, lens, slots, slot_bytes: int, hash_len: int,
                     file_len: int, pos_base: int, verify: bool = False, max_chunk=None) -> Imported:
        """slots: the destination file's map as a list of slot images, edited in place."""
        max_chunk = self.cl if max_chunk is None else max_chunk
        bal = hash_len + 24
        nreq = len(images)
        status, missed, pairs_of = [], [], []
        total_missed = 0
        for img in images:
            st, pairs = IM.counting_pairs(img, slot_bytes, hash_len)
            want = []
            miss = 0
            for i, h, loc in pairs:
                if MM.pad32(h) in self.ix.e:
                    want.append(None)
                    continue
                k = (loc - src.pos_base) % (1 << 64)
                ok = k < len(src.entries) and src.entries[k][0] != 0 and 0 < src.entries[k][1] <= max_chunk
                miss += not ok
                want.append(k)
            if miss:
                st |= EMISSING
            total_missed += miss
            status.append(st)
            missed.append(miss)
            pairs_of.append(list(zip(pairs, want)))
        fetches = sorted({k for r in range(nreq) if not status[r] for _, k in pairs_of[r] if k is not None})
        f_of = {k: f for f, k in enumerate(fetches)}
        dst_off, at = [], 0
        for k in fetches:
            dst_off.append(at)
            at += _r16(src.entries[k][1])
        for r in range(nreq):
            if status[r]:
                continue
            for (i, h, loc), k in pairs_of[r]:
                if k is None:
                    continue
                _, raw, chunk = src.entries[k]
                if chunk is None or len(chunk) != raw:
                    status[r] |= EFETCH
                elif verify and MM.pad32(self.digest(chunk)[:hash_len]) != MM.pad32(h):
                    status[r] |= EHASH
        records, pair_rec, held = [], [], 0
        for r in range(nreq):
            mine = {}
            if not status[r]:
                for (i, h, loc), k in pairs_of[r]:
                    mine[i] = len(records)
                    if k is None:
                        records.append((MM.pad32(h), 0, 0, 0))
                        held += 1
                    else:
                        records.append((MM.pad32(h), f_of[k], 0, src.entries[k][1]))
            pair_rec.append(mine)
        new_list, hashloc, chunks = [], [], {}
        for n, (key, f, _, ln) in enumerate(records):
            if key in self.ix.e:
                self.ix.e[key][1] += 1
            else:
                pos = pos_base + len(new_list)
                self.ix.e[key] = [pos, 1]
                chunks[pos] = src.entries[fetches[f]][2]
                new_list.append(n)
            hashloc.append(self.ix.e[key][0])
        changed = accepted = 0
        for r in range(nreq):
            if status[r]:
                continue
            accepted += 1
            self.ix.claim_slots([slots[dests[r]]], slot_bytes, hash_len, -1)
            img = bytearray(bytes(images[r]).ljust(slot_bytes, b"\0"))
            n = max(struct.unpack(">i", img[5:9])[0], 0)
            img[13 + n * bal:] = bytes(slot_bytes - 13 - n * bal)
            for (i, h, loc), _ in pairs_of[r]:
                new = hashloc[pair_rec[r][i]]
                at = 9 + i * bal + hash_len
                changed += new != loc
                img[at: at + 8] = struct.pack(">q", new)
            slots[dests[r]] = bytes(img)
            file_len = max(file_len, dests[r] * self.cl + lens[r])
        counts = [len(records), held, len(fetches), sum(src.entries[k][1] for k in fetches), accepted,
                  nreq - accepted, changed, total_missed]
        return Imported(status, missed, pair_rec, counts, records, fetches, dst_off, new_list, hashloc, file_len, chunks)
