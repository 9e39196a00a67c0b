"""Plain-Python model of reopening a chunk store from its images — TEST INFRASTRUCTURE ONLY.

A restatement of the reference's read side of the map and of the rules include/sdfs_store.h adds:

* ``geometry``: SimpleByteArrayLongMap.setUp on an existing file (SimpleByteArrayLongMap.java:198-261):
  version 0 = slots ``[key][BE32 value]`` from byte 0; version != 0: a file of <= 16 bytes is an empty
  map, a longer one with BE32 6442 at byte 0 is ``[16-byte header][key][BE32 pos][BE32 len]`` with
  the version from bytes 4..8, any other the version-0 layout; ``size = (len - offset) / EL``;
* ``slots``: next() (:136-175): every slot in slot order whose key is not all zero;
* ``index``: index() / indexRehashed() (:340-400) on the image as it lies;
* ``scan_archive`` / ``scan``: the records in (pos, slot) order, the RANGE / KEY / LEN / NZ flags, the
  nz rule of HashBlobArchive.getChunk (HashBlobArchive.java:1922-1934), the GAP status;
* ``directory``: directory entry ``hashloc - pos_base`` -> the lowest record ordinal that claims it.
"""
from __future__ import annotations

import struct

MAGIC = 6442
NONE = 0xFFFFFFFF
RANGE, KEY, LEN, NZ, FETCH, HASH = 1, 2, 4, 8, 16, 32
GAP, SLOTS = 1, 2


def be32(b, p=0) -> int:
    return struct.unpack(">I", bytes(b[p: p + 4]))[0]


def geometry(img: bytes, hash_len: int, version: int):
    """-> (offset, EL, version, size)."""
    off, el, ver = 0, hash_len + 4, 0
    if version != 0:
        if len(img) <= 16:
            return off, el, ver, 0
        if be32(img, 0) == MAGIC:
            off, el, ver = 16, hash_len + 8, be32(img, 4)
    return off, el, ver, (len(img) - off) // el


def slots(img: bytes, hash_len: int, version: int):
    """next(): [(slot, key, the slot's bytes after the key)] of the filled slots, in slot order."""
    off, el, _, size = geometry(img, hash_len, version)
    out = []
    for s in range(size):
        e = img[off + s * el: off + (s + 1) * el]
        if e[:hash_len] != bytes(hash_len):
            out.append((s, bytes(e[:hash_len]), bytes(e[hash_len:])))
    return out


def index(img: bytes, key: bytes, hash_len: int, version: int) -> int:
    """The slot that holds key, or -1: index() / indexRehashed(), an all-zero key absent."""
    off, el, _, size = geometry(img, hash_len, version)
    if size == 0 or key == bytes(hash_len):
        return -1
    at = lambda s: img[off + s * el: off + s * el + hash_len]  # noqa: E731
    h = struct.unpack(">i", key[8:12])[0] & 0x7FFFFFFF
    home = idx = h % size
    if at(idx) == key:
        return idx
    if at(idx) == bytes(hash_len) or size <= 2:  # FREE; size 2: the reference's % 0 throws, get returns -1
        return -1
    probe = 1 + h % (size - 2)
    while True:
        idx -= probe
        if idx < 0:
            idx += size
        if idx == home:
            return -1
        if at(idx) == key:
            return idx
        if at(idx) == bytes(hash_len):
            return -1


def check_record(arc: bytes, key: bytes, rest: bytes, ver: int, hash_len: int, header_bytes: int):
    """A filled slot against the archive image -> (pos, len, flags)."""
    pos = (be32(rest, 0) + 4) & 0xFFFFFFFF
    p = be32(rest, 0) + 4
    if p < header_bytes + 8 + hash_len or p > len(arc) or p > 0xFFFFFFFF:
        return pos, 0, RANGE
    img_len = be32(arc, p - 4)
    ln = be32(rest, 4) if ver != 0 else img_len
    if p + ln > len(arc):
        return pos, 0, RANGE
    flags = 0
    if ver != 0 and img_len != ln:
        flags |= LEN
        ln = 0
    if arc[p - 8 - hash_len: p - 4] != struct.pack(">I", hash_len) + key:
        flags |= KEY
    return pos, ln, flags


def nz_rule(rec: bytes, max_chunk: int):
    """-> (raw_len, flags) of a plain record [BE32 nz][payload]."""
    if len(rec) < 4:
        return 0, NZ
    nz = struct.unpack(">i", rec[:4])[0]
    raw = nz if nz > 0 else len(rec) - 4
    return (0, NZ) if raw > max_chunk else (raw, 0)


def scan_archive(arc: bytes, mp: bytes, hash_len: int, version: int, header_bytes: int, max_chunk: int, plain: bool):
    """-> (records [dict(slot, pos, len, key, raw_len, flags)] in (pos, slot) order, map version, size, status)."""
    _, _, ver, size = geometry(mp, hash_len, version)
    recs = []
    for s, key, rest in slots(mp, hash_len, version):
        pos, ln, flags = check_record(arc, key, rest, ver, hash_len, header_bytes)
        raw = 0
        if not flags & (RANGE | LEN):
            if plain:
                raw, f = nz_rule(arc[pos: pos + ln], max_chunk)
                flags |= f
            elif ln < 4:
                flags |= NZ
        recs.append(dict(slot=s, pos=pos, len=ln, key=key, raw_len=raw, flags=flags))
    recs.sort(key=lambda r: (r["pos"], r["slot"]))
    total = header_bytes + sum(8 + hash_len + r["len"] for r in recs if r["flags"] == 0)
    return recs, ver, size, (GAP if total != len(arc) else 0)


def scan(archives, maps, bases, hash_len: int, version: int, header_bytes: int, max_chunk: int, plain: bool):
    """Every archive in turn -> dict(records (with arc, store_off), arc_first, versions, sizes, status, ivs, slot_rec)."""
    out = dict(records=[], arc_first=[0], versions=[], sizes=[], status=[], ivs=[], slot_rec=[])
    for a, (arc, mp) in enumerate(zip(archives, maps)):
        recs, ver, size, st = scan_archive(arc, mp, hash_len, version, header_bytes, max_chunk, plain)
        row = [NONE] * size
        for r in recs:
            row[r["slot"]] = len(out["records"])
            out["records"].append(dict(r, arc=a, store_off=bases[a] + r["pos"]))
        out["arc_first"].append(len(out["records"]))
        out["versions"].append(ver)
        out["sizes"].append(size)
        out["status"].append(st)
        out["ivs"].append(bytes(arc[4:20]) if header_bytes and len(arc) >= 20 else bytes(16))
        out["slot_rec"].append(row)
    return out


def directory(records, hashloc, pos_base: int, n_store: int):
    """-> (store_off, store_len, raw_len, rec_of_k (-1 = none), [orphans, out of range, clashes])."""
    off, ln, raw, rec = [0] * n_store, [0] * n_store, [0] * n_store, [-1] * n_store
    info = [0, 0, 0]
    for i, (r, h) in enumerate(zip(records, hashloc)):
        if r["flags"] or h < 0:
            info[0] += 1
        elif not 0 <= h - pos_base < n_store:
            info[1] += 1
        elif rec[h - pos_base] >= 0:
            info[2] += 1
        else:
            k = h - pos_base
            off[k], ln[k], raw[k], rec[k] = r["store_off"], r["len"], r["raw_len"], i
    return off, ln, raw, rec, info


def scrub_flag(rec: bytes, key: bytes, max_chunk: int, digest, decode, decrypt=None) -> int:
    """What the scrub finds for one readable stored record: 0, FETCH or HASH.  decrypt(rec) and
    decode(block, n) raise ValueError on a record they cannot take; digest(chunk) -> bytes."""
    try:
        if decrypt is not None:
            rec = decrypt(rec)
        raw, f = nz_rule(rec, max_chunk)
        if f:
            return FETCH
        nz = struct.unpack(">i", rec[:4])[0]
        chunk = decode(rec[4:], nz) if nz > 0 else rec[4:]
    except ValueError:
        return FETCH
    return 0 if digest(chunk)[: len(key)] == key else HASH
