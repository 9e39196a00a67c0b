"""Plain-Python model of the map edits' rules — TEST INFRASTRUCTURE ONLY.

Restated from the reference on top of tests/read_model.py's ``parse`` / ``build_image``:

* ``insert``: ``SparseDataChunk.insertHashLocPair`` (SparseDataChunk.java:208-263) over a dict as the
  TreeMap.  The walk goes down from the floor entry of ``ep = p.pos + p.nlen``: an entry that starts
  at or after ``p.pos`` loses its first ``ep - pos`` bytes (and leaves the map when nothing is left);
  an entry that starts before ``p.pos`` and reaches it is cut at ``p.pos``, and when it also reaches
  past ``ep`` a clone with ``dup = true`` takes ``[ep, hep)``; the walk ends at the first entry that
  ends before ``p.pos``.  Then ``p`` is put at ``p.pos``.  ``ep > CHUNK_LENGTH`` raises.
  Line 248 puts the *old* object under the clone's key; ``literal=True`` does the same, the default
  puts the clone (the form this library implements, include/sdfs_extent.h).
* ``get_wl``: ``SparseDataChunk.getWL`` (:181-206).
* ``copy_extent_loop``: the while-loop of ``CopyExtents`` (mgmt/CopyExtents.java:96-155).
* ``paint``: later item wins, byte by byte; maximal runs of one item are the fragments.
* ``get_bytes``: ``SparseDataChunk.getBytes`` for versions >= 2 (:295-318) after the re-keying by
  each pair's own pos that persisting does (SparseDedupFile.java:621-666 builds a fresh chunk).

A pair is a list ``[hash, hashloc, len, pos, offset, nlen, dup]``; a map is ``{key: pair}``.
"""
from __future__ import annotations

from tests import read_model as R

HASH, HASHLOC, LEN, POS, OFFSET, NLEN, DUP = range(7)


class Overflow(IOError):
    pass


class NotFound(IOError):
    pass


class Runaway(RuntimeError):
    """The literal form's walk did not end within its step bound."""


def pair(h, hashloc, ln, pos, offset=0, nlen=None, dup=False):
    return [bytes(h), hashloc, ln, pos, offset, ln if nlen is None else nlen, dup]


def tree(pairs):
    """Pairs -> {pos: pair} (copies)."""
    return {p[POS]: list(p) + [False] * (7 - len(p)) for p in pairs}


def values(ar):
    """The map's values in key order, as tuples."""
    return [tuple(ar[k]) for k in sorted(ar)]


def _floor(ar, x):
    keys = [k for k in ar if k <= x]
    return max(keys) if keys else None


def insert(ar, p, chunk_length, literal=False, max_steps=10000):
    """Inserts p (a pair; the list object itself goes into the map).  Returns True when an entry was
    split."""
    ep = p[POS] + p[NLEN]
    if ep > chunk_length:
        raise Overflow(f"Overflow ep={ep} sp={p[POS]}")
    split = False
    x = ep
    for _ in range(max_steps):
        k = _floor(ar, x)
        if k is None:
            break
        h = ar[k]
        hpos, hep = h[POS], h[POS] + h[NLEN]
        if hep < p[POS]:
            break
        if h[POS] >= p[POS]:
            cut = ep - h[POS]
            h[POS] = ep
            h[OFFSET] += cut
            h[NLEN] -= cut
            ar.pop(hpos, None)
            if h[NLEN] > 0:
                ar[h[POS]] = h
        else:  # starts before p and reaches it
            if hep > ep:
                cut = ep - h[POS]
                t = list(h)
                t[OFFSET] += cut
                t[NLEN] -= cut
                t[POS] = ep
                t[DUP] = True
                ar[ep] = h if literal else t
                split = True
            h[NLEN] = p[POS] - h[POS]
            if h[NLEN] <= 0:
                ar.pop(h[POS], None)
        x = h[POS] - 1
    else:
        raise Runaway(f"{max_steps} steps")
    ar[p[POS]] = p
    return split


def get_wl(ar, x):
    k = _floor(ar, x)
    if k is not None:
        h = ar[k]
        if h[POS] <= x < h[POS] + h[NLEN]:
            c = list(h)
            c[OFFSET] += x - h[POS]
            c[NLEN] -= x - h[POS]
            c[POS] = x
            return c
    raise NotFound(f"Position not found {x}")


def copy_extent_loop(src, dst, sstart, dstart, length, chunk_length, literal=False):
    """src / dst: {buffer number: map}.  Copies [sstart, sstart + length) of the source file to
    dstart of the destination, inserting into dst's maps (made on demand).  Returns the steps walked,
    (src_buf, src_off, dst_buf, dst_off, nlen) each."""
    steps = []
    written = 0
    while written < length:
        sb, so = divmod(sstart + written, chunk_length)
        db, do = divmod(dstart + written, chunk_length)
        p = get_wl(src.get(sb, {}), so)
        p[NLEN] = min(p[NLEN], length - written)
        p[POS] = do
        if p[POS] + p[NLEN] > chunk_length:
            p[NLEN] = chunk_length - p[POS]
        p[DUP] = False
        insert(dst.setdefault(db, {}), p, chunk_length, literal=literal)
        steps.append((sb, so, db, do, p[NLEN]))
        written += p[NLEN]
    return steps


def segments_of(steps):
    """The steps of ``copy_extent_loop`` joined where they stay in one source and one destination
    buffer: what ``sdfs_amd.extent.split_extent`` must return."""
    out = []
    for sb, so, db, do, n in steps:
        if out and out[-1][0] == sb and out[-1][2] == db and out[-1][1] + out[-1][4] == so:
            out[-1] = (sb, out[-1][1], db, out[-1][3], out[-1][4] + n)
        else:
            out.append((sb, so, db, do, n))
    return out


def paint(base, inserts, chunk_length):
    """base: ascending, disjoint pairs; inserts: pairs with nlen >= 1 in application order.  A byte
    belongs to the last insert that covers it, else to its base pair.  Returns the fragments as
    (hash, hashloc, len, pos, offset, nlen) in pos order."""
    items = [p for p in base if p[NLEN] > 0] + list(inserts)
    owner = [-1] * chunk_length
    for i, p in enumerate(items):
        owner[p[POS]: p[POS] + p[NLEN]] = [i] * p[NLEN]
    out, x = [], 0
    while x < chunk_length:
        y = x
        while y < chunk_length and owner[y] == owner[x]:
            y += 1
        if owner[x] >= 0:
            p = items[owner[x]]
            out.append((p[HASH], p[HASHLOC], p[LEN], x, p[OFFSET] + x - p[POS], y - x))
        x = y
    return out


def persisted(ar):
    """The pair list a reopened image holds: values in key order, keyed again by their own pos."""
    again = {}
    for k in sorted(ar):
        again[ar[k][POS]] = ar[k]
    return [tuple(again[k]) for k in sorted(again)]


def get_bytes(ar, flags=0):
    ps = persisted(ar)
    doop = sum(p[NLEN] for p in ps if p[DUP])
    return R.build_image([p[:6] for p in ps], flags=flags, doop=doop)


def covered(ps, chunk_length):
    """(owner hashloc, offset in its chunk) per byte of the buffer, None where nothing covers it."""
    out = [None] * chunk_length
    for p in ps:
        for i in range(p[NLEN]):
            out[p[POS] + i] = (p[HASHLOC], p[OFFSET] + i)
    return out
