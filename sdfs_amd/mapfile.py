"""Map-file lifecycle on the MI355X: snapshot, delete, trim, truncate — the whole-file walks of
``org.opendedup.collections.LongByteArrayMap`` that move reference counts in the hash store.

Each is one call of :meth:`sdfs_amd.index.HipHashesMap.claim_slots` (``sdfs_cdc_index_claim_slots``,
include/sdfs_index.h): the HashLocPairs are read straight from the slot images on the device and
every one is applied as ``claimKey(hash, hashloc, +-1)``.  Nothing is parsed into a pair structure,
nothing waits on the host for a size.  ``m`` is a file's map on the device: uint8, ``nbuf`` slots of
``slot_len`` bytes, slot b = write buffer b.  The file's own bookkeeping (its length, the map file on
disk) stays with the caller.  No CPU fallback.

Two things the reference does are not mirrored (see the header): ``addRef`` / ``removeRef`` skip
hashloc 0 / 1 and the blank hash, here every pair counts as ``put_records`` counted it; and
``nextValue(true)`` can rewrite a pair's hashloc, here a claim matches only an equal pos.
"""
from __future__ import annotations


def trim_range(pos: int, length: int, chunk_length: int):
    """The slots ``trim`` frees: [ceil(pos / CL), floor((pos + length) / CL)) — the buffers wholly
    inside the byte range; empty when the end is not past the start
    (LongByteArrayMap.java:599-605)."""
    if min(pos, length) < 0 or chunk_length < 1:
        raise ValueError("negative range")
    first = -(-pos // chunk_length)
    end = (pos + length) // chunk_length
    return (first, end) if end > first else (first, first)


def truncate_keep(size: int, chunk_length: int) -> int:
    """Slots a map file keeps when the file is cut to ``size`` bytes: ``size // CL``
    (getMapFilePosition, LongByteArrayMap.java:536-539)."""
    if size < 0 or chunk_length < 1:
        raise ValueError("negative size")
    return size // chunk_length


def _range_mask(m, nbuf: int, first: int, end: int):
    import torch

    sel = torch.zeros(max(nbuf, 1), dtype=torch.uint8, device=m.device)
    sel[first:end] = 1
    return sel[:nbuf]


def index_map(index, m, nbuf: int, slot_len: int, hash_len: int = 32, stream=None):
    """``LongByteArrayMap.index()`` (LongByteArrayMap.java:884-890 -> nextValue(true), :310-356):
    ``addRef(p.hash, hashloc, 1)`` for every pair of every slot — what makes an imported or copied
    map count.  Returns the :class:`sdfs_amd.index.SlotClaims`."""
    return index.claim_slots(m, nbuf, slot_len, +1, hash_len=hash_len, stream=stream)


def snapshot(index, m, nbuf: int, slot_len: int, hash_len: int = 32, stream=None):
    """``copy(dest, index=true)`` (LongByteArrayMap.java:897-940): the slots are copied, then the
    copy is indexed.  Returns the cloned slot tensor, counted (no host wait)."""
    dest = m[: nbuf * slot_len].clone()
    index_map(index, dest, nbuf, slot_len, hash_len, stream)
    return dest


def vanish(index, m, nbuf: int, slot_len: int, hash_len: int = 32, stream=None) -> int:
    """File delete, ``vanish(index=true)`` (LongByteArrayMap.java:817-882, from
    SparseDedupFile.java:302-306): ``removeRef(p.hash, hashloc, 1)`` for every pair of every slot.
    Returns the pairs that found nothing to release, the reference's ``rmct`` ("unable to remove
    orphaned reference total="); waits for the device.  ``m`` is left as it was: the caller drops it."""
    return index.claim_slots(m, nbuf, slot_len, -1, hash_len=hash_len, stream=stream).missed


def trim(index, m, nbuf: int, slot_len: int, pos: int, length: int, chunk_length: int, hash_len: int = 32,
         stream=None):
    """``trim(pos, len)`` (LongByteArrayMap.java:595-648, from DedupFileChannel.java:755): every
    slot wholly inside [pos, pos + length) releases its pairs and is overwritten with FREE (zeros)
    in ``m``.  A corrupt slot is flagged in the result and keeps its bytes, and the walk goes on
    (the reference logs the exception and stops there).  Returns (first, end) of the slot range and
    the :class:`SlotClaims`, or None for an empty range."""
    first, end = trim_range(pos, length, chunk_length)
    first, end = min(first, nbuf), min(end, nbuf)
    if end <= first:
        return (first, first), None
    sel = _range_mask(m, nbuf, first, end)
    return (first, end), index.claim_slots(m, nbuf, slot_len, -1, sel=sel, free=True, hash_len=hash_len,
                                           stream=stream)


def truncate(index, m, nbuf: int, slot_len: int, size: int, chunk_length: int, hash_len: int = 32, stream=None):
    """``truncate(length)`` (LongByteArrayMap.java:656-688, from DedupFileChannel.truncateFile,
    DedupFileChannel.java:124-155): with k = size // chunk_length (getMapFilePosition's floor, :536-539)
    the slots k .. nbuf release their pairs and the map is cut: returns (``m[:k * slot_len]``, k).  The
    slot of a partial last buffer goes too, as the reference's ``bdb.truncate(fpos)`` drops it.  (A
    caller that wants the walk's counts and per-slot status calls ``index.claim_slots`` with the mask
    of the dropped slots itself.)

    One divergence.  The reference's loop releases the slots with ``iterPos * CHUNK_LENGTH < fpos``
    (:664-672): it compares file bytes with map-file bytes, and so walks from the FRONT of the file
    and releases slots the cut keeps.  Here exactly the slots the cut removes are released."""
    k = min(truncate_keep(size, chunk_length), nbuf)
    if k < nbuf:
        index.claim_slots(m, nbuf, slot_len, -1, sel=_range_mask(m, nbuf, k, nbuf), hash_len=hash_len, stream=stream)
    return m[: k * slot_len], k


def close_map(codec, m, nbuf: int, slot_len: int, stream=None):
    """``LongByteArrayMap.close`` under ``Main.COMPRESS_METADATA`` (LongByteArrayMap.java:1003-1015):
    the closed ``GUID.map`` is replaced by ``GUID.map.lz4`` = ``CompressionUtils.compressFile``.  ``codec``
    is a :class:`sdfs_amd.lz4_stream.HipLz4BlockStream`.  Returns the ``.map.lz4`` image, a uint8
    tensor on the device cut to the stream's length (one host read, of that length)."""
    n = nbuf * slot_len
    out, _, out_lens = codec.compress_files(m, [0], [n], stream=stream)
    return out[: int(out_lens[0])]


def open_map(codec, image, slot_len: int, stream=None):
    """A ``.map.lz4`` opened (LongByteArrayMap.java:141-154, 172-177, 464-469): expanded by
    ``CompressionUtils.decompressFile`` before the first slot is read.  Returns ``(m, nbuf)``.  Raises
    :class:`SdfsCdcError` where ``LZ4BlockInputStream`` throws (naming the flags), and when the decoded
    length is not a whole number of slots."""
    from . import _lib
    from .lz4_stream import flag_names

    if slot_len < 1:
        raise ValueError("slot_len")
    out, _, decoded, status, _ = codec.decompress_files(image, [0], [int(image.shape[0])], stream=stream)
    if status[0]:
        raise _lib.SdfsCdcError(_lib.EINVAL, f".map.lz4 is corrupted: {flag_names(int(status[0]))}")
    n = int(decoded[0])
    if n % slot_len:
        raise _lib.SdfsCdcError(_lib.EINVAL, f".map.lz4 decodes to {n} bytes: not a whole number of {slot_len}-byte slots")
    return out[:n], n // slot_len


def snapshot_compressed(codec, m, nbuf: int, slot_len: int, stream=None):
    """``copy(dest, index=false)`` under ``Main.COMPRESS_METADATA`` (LongByteArrayMap.java:897-940; the
    copy is written as ``dest.lz4``, :937-938): the slots as a ``.map.lz4`` image, not indexed — the
    copy counts only once it is opened and :func:`index_map` runs over it."""
    return close_map(codec, m, nbuf, slot_len, stream)
