"""Plain-Python model of the client-side dedup front end — TEST INFRASTRUCTURE ONLY.

The three RPCs of StorageServiceImpl (StorageServiceImpl.java:175-382), restated over
``tests/mapfile_model.IndexModel`` (a dict ``digest -> [pos, ref]``) with the batch semantics of
include/sdfs_ingest.h and ``sdfs_cdc_index_addref_slots``:

* ``check_hashes``: ``HashesMap.get(hash)`` per hash, -1 where absent; an entry whose count is <= 0
  is still held;
* ``write_chunks``: per entry in order — empty -> (false, -1, 0); bad numbers -> EBOUNDS; an LZ4
  payload that does not decode to exactly raw_len bytes -> EDECODE; with verify, a chunk whose
  fingerprint is not the client's hash -> EHASH; every other entry is ``put(ChunkData(hash, chunk))``:
  absent -> inserted at ``pos_base + rank`` with count 1, present -> count + 1;
* ``addref_slots``: a request is accepted iff its image parses and every counting pair that is not
  ``inserted`` names a fingerprint held at its hashloc; an accepted request adds 1 per such pair, a
  rejected one moves nothing;
* ``write_sparse_data_chunks``: an accepted request releases the pairs of the slot it replaces,
  becomes that slot's bytes and moves the file length.
"""
from __future__ import annotations

import struct

from tests import lz4_block_model as Z
from tests import mapfile_model as MM
from tests import read_model as R

EMPTY, EBOUNDS, EDECODE, EHASH, EMISSED = 1, 2, 4, 8, 16
CORRUPT = R.CORRUPT


def counting_pairs(img: bytes, slot_bytes: int, hash_len: int):
    """-> (status, [(image index, hash, hashloc)]) of the pairs the TreeMap keeps: a pair that shares
    its pos with a later pair of the image does not count."""
    st, _, _, _ = R.parse(img, slot_bytes, hash_len)
    if st != R.OK:
        return st, []
    img = bytes(img).ljust(slot_bytes, b"\0")
    bal = hash_len + 24
    n = max(struct.unpack(">i", img[5:9])[0], 0)
    recs = []
    for i in range(n):
        rec = img[9 + i * bal: 9 + (i + 1) * bal]
        hashloc, _, pos, _, _ = struct.unpack(">qiiii", rec[hash_len:])
        recs.append((i, rec[:hash_len], hashloc, pos))
    last = {pos: i for i, _, _, pos in recs}
    return st, [(i, h, loc) for i, h, loc, pos in recs if last[pos] == i]


def plan_chunks(entries, blob_len: int, chunk_length: int, stage_cap=None):
    """What the plan decides from the client's numbers alone.  entries: [(hash, off, len, raw_len,
    compressed)] -> (status[], stage_off[], [(off, len, stage_off, raw_len, entry)] of the entries to
    decode, in entry order).  The places are the prefix of raw_len over every entry whose numbers
    are in bounds, whether or not it still fits the staging area."""
    status, stage_off, decode, staged = [], [], [], 0
    for i, (_, off, ln, raw, comp) in enumerate(entries):
        st, at = 0, 0
        if ln == 0:
            st = EMPTY
        elif raw == 0 or raw > chunk_length or off + ln > blob_len or (not comp and ln != raw):
            st = EBOUNDS
        else:
            at, staged = staged, staged + raw
            if stage_cap is not None and staged > stage_cap:
                st = EBOUNDS
        status.append(st)
        stage_off.append(0 if st else at)
        if not st and comp:
            decode.append((off, ln, at, raw, i))
    return status, stage_off, decode


class IngestModel:
    """index: an ``IndexModel``; digest(chunk) -> the fingerprint (for verify); stored_len(chunk) ->
    the length of the record the store keeps for it."""

    def __init__(self, index: MM.IndexModel, chunk_length: int, digest=None, stored_len=lambda c: len(c) + 4):
        self.ix, self.cl, self.digest, self.stored_len = index, chunk_length, digest, stored_len
        self.chunks = {}  # pos -> the chunk stored there

    def check_hashes(self, hashes):
        return [self.ix.e[MM.pad32(h)][0] if MM.pad32(h) in self.ix.e else -1 for h in hashes]

    def write_chunks(self, entries, blob: bytes, pos_base: int, verify: bool = False, stage_cap=None):
        """entries: [(hash, off, len, raw_len, compressed)] over ``blob`` ->
        (inserted[], pos[], stored_len[], status[])."""
        inserted, pos, stored, status = [], [], [], []
        rank = 0
        planned = plan_chunks(entries, len(blob), self.cl, stage_cap)[0]
        for (h, off, ln, raw, comp), st in zip(entries, planned):
            chunk = None
            if not st:
                payload = blob[off: off + ln]
                if comp:
                    r = Z.decode(payload, raw)
                    if isinstance(r, str) or len(r[0]) != raw:
                        st = EDECODE
                    else:
                        chunk = r[0]
                else:
                    chunk = payload
                if not st and verify and MM.pad32(self.digest(chunk)) != MM.pad32(h):
                    st = EHASH
            status.append(st)
            if st:
                inserted.append(0)
                pos.append(-1)
                stored.append(0)
                continue
            key = MM.pad32(h)
            if key in self.ix.e:
                self.ix.e[key][1] += 1
                inserted.append(0)
                stored.append(0)
            else:
                self.ix.e[key] = [pos_base + rank, 1]
                self.chunks[pos_base + rank] = chunk
                rank += 1
                inserted.append(1)
                stored.append(self.stored_len(chunk))
            pos.append(self.ix.e[key][0])
        return inserted, pos, stored, status

    def addref_slots(self, images, slot_bytes: int, hash_len: int, inserted=None):
        """inserted: per request a list of flags by image pair index (or None) ->
        (counts[6] with every miss listed, status[], missed[], sorted [(request, pair)])."""
        counts, status, missed, misses = [0] * 6, [], [], []
        for r, img in enumerate(images):
            st, pairs = counting_pairs(img, slot_bytes, hash_len)
            flags = inserted[r] if inserted is not None and inserted[r] is not None else []
            live = []
            for i, h, loc in pairs:
                if i < len(flags) and flags[i]:
                    counts[2] += 1
                else:
                    live.append((i, h, loc))
            miss = [i for i, h, loc in live if self.ix.e.get(MM.pad32(h), [None])[0] != loc]
            if st == R.OK and not miss:
                for _, h, _ in live:
                    self.ix.e[MM.pad32(h)][1] += 1
                counts[0] += len(live)
                counts[3] += 1
            else:
                st = st if st != R.OK else EMISSED
                counts[4] += 1
            counts[1] += len(miss)
            misses += [(r, i) for i in miss]
            status.append(st)
            missed.append(len(miss))
        counts[5] = len(misses)
        return counts, status, missed, sorted(misses)

    def write_sparse_data_chunks(self, slots, slot_bytes: int, hash_len: int, dests, images, lens, file_len: int,
                                 inserted=None):
        """slots: the file's map as a list of slot images, edited in place ->
        (addref_slots' results, the new file length)."""
        res = self.addref_slots(images, slot_bytes, hash_len, inserted)
        for r, st in enumerate(res[1]):
            if st:
                continue
            self.ix.claim_slots([slots[dests[r]]], slot_bytes, hash_len, -1)
            slots[dests[r]] = bytes(images[r]).ljust(slot_bytes, b"\0")
            file_len = max(file_len, dests[r] * self.cl + lens[r])
        return res, file_len
