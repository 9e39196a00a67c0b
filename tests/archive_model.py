"""Plain-Python model of the chunk store layer's rules — TEST INFRASTRUCTURE ONLY.

A literal restatement of the reference, one ``bytearray`` per archive:

* ``next_prime_i``: NextPrime.getNextPrimeI (NextPrime.java:56-88) line by line, with its
  ``isPrime`` flag that is set when ``j == root``;
* ``SlotMap``: SimpleByteArrayLongMap's file image (SimpleByteArrayLongMap.java:224-261: version 0
  = slots ``[key][BE32 value]``, version > 0 = ``[BE32 6442][BE32 version][8 zero bytes]`` then slots
  ``[key][BE64 value]``), ``insertionIndex`` / ``insertKeyRehash`` (:427-498: home ``h % size`` with
  ``h = BE32(key[8:12]) & 0x7fffffff``, then backwards by ``1 + h % (size - 2)``), ``put``
  (:509-539), ``index`` / ``get`` (:340-400,562-599), ``next`` in slot order (:136-170) and
  ``getWMaxSz`` (:187-189);
* ``Archive.put``: HashBlobArchive.putChunk's two "full" checks (HashBlobArchive.java:1305-1316),
  the map value (:1334-1350) and the record ``[BE32 hash.length][hash][BE32 len][record]``
  (:1399-1411); the header of a VERSION > 0 archive ``[BE32 VERSION][IV][zeros]`` to 1024 bytes
  (:299-301,1023-1033);
* ``Store.put``: a full archive is closed and the record opens the next one (:740-764);
* ``compact``: HashBlobArchive.compact (:2064-2186): the map in slot order, the keys still
  wanted, re-put into an archive with blocksz = the old length and a map of 2 * live + 5.
"""
from __future__ import annotations

import math
import struct

MAGIC = 6442
HEADER = 1024
ALIGN = 4096
INT_MAX = 2 ** 31 - 1


def next_prime_i(inp: int) -> int:
    """0 where the reference throws."""
    is_prime = False
    if inp <= 2:
        return 2
    k = 3
    while k < 9:
        if inp <= k:
            return k
        k += 2
    if inp == ((inp >> 1) << 1):
        inp += 1
    i = inp
    while True:
        root = int(math.sqrt(i))
        j = 3
        while j <= root:
            if i == (i // j) * j:
                is_prime = False
                break
            if j == root:
                is_prime = True
            j += 1
        if is_prime:
            if i > INT_MAX:
                return 0
            return i
        i += 2


class ArchiveFull(Exception):
    pass


class SlotMap:
    def __init__(self, sz: int, version: int, hash_len: int):
        self.size = next_prime_i(sz)
        self.version, self.hash_len = version, hash_len
        self.slots = [None] * self.size  # (key, value)
        self.current = 0

    def w_max(self) -> int:
        return int(self.size * .75)

    @staticmethod
    def _hash(key: bytes) -> int:
        return struct.unpack(">i", key[8:12])[0] & 0x7FFFFFFF

    def insertion_index(self, key: bytes) -> int:
        h = self._hash(key)
        idx = h % self.size
        cur = self.slots[idx]
        if cur is None:
            return idx
        if cur[0] == key:
            return -idx - 1
        probe = 1 + (h % (self.size - 2))
        loop = idx
        while True:
            idx -= probe
            if idx < 0:
                idx += self.size
            cur = self.slots[idx]
            if cur is None:
                return idx
            if cur[0] == key:
                return -idx - 1
            if idx == loop:
                raise RuntimeError("No free or removed slots available. Key set full?!!")

    def put(self, key: bytes, value: int) -> bool:
        pos = self.insertion_index(key)
        if pos < 0:
            return False
        self.slots[pos] = (bytes(key), value)
        self.current += 1
        return True

    def index(self, key: bytes) -> int:
        h = self._hash(key)
        idx = h % self.size
        cur = self.slots[idx]
        if cur is not None and cur[0] == key:
            return idx
        if cur is None:
            return -1
        probe = 1 + (h % (self.size - 2))
        loop = idx
        while True:
            idx -= probe
            if idx < 0:
                idx += self.size
            cur = self.slots[idx]
            if cur is not None and cur[0] == key:
                return idx
            if cur is None or idx == loop:
                return -1

    def get(self, key: bytes) -> int:
        i = self.index(key)
        return -1 if i < 0 else self.slots[i][1]

    def entries(self):
        """next(): the filled slots in slot order."""
        return [s for s in self.slots if s is not None]

    def image(self) -> bytes:
        el = self.hash_len + (8 if self.version else 4)
        out = bytearray()
        if self.version:
            out += struct.pack(">ii", MAGIC, self.version) + bytes(8)
        for s in self.slots:
            if s is None:
                out += bytes(el)
            else:
                out += s[0] + (struct.pack(">q", s[1]) if self.version else struct.pack(">i", s[1]))
        return bytes(out)

    @classmethod
    def from_image(cls, img: bytes, version: int, hash_len: int) -> "SlotMap":
        """setUp() on an existing file: size from its length."""
        el = hash_len + (8 if version else 4)
        off = 16 if version else 0
        if version:
            assert struct.unpack(">ii", img[:8]) == (MAGIC, version) and img[8:16] == bytes(8)
        m = cls.__new__(cls)
        m.size, m.version, m.hash_len = (len(img) - off) // el, version, hash_len
        assert off + m.size * el == len(img)
        m.slots, m.current = [], 0
        for i in range(m.size):
            e = img[off + i * el: off + (i + 1) * el]
            if e[:hash_len] == bytes(hash_len):
                m.slots.append(None)
            else:
                v = struct.unpack(">q", e[hash_len:])[0] if version else struct.unpack(">i", e[hash_len:])[0]
                m.slots.append((e[:hash_len], v))
                m.current += 1
        return m


class Archive:
    def __init__(self, map_sz: int, blocksz: int, version: int, hash_len: int, iv: bytes = bytes(16)):
        self.blocksz, self.version, self.hash_len = blocksz, version, hash_len
        self.map = SlotMap(map_sz, version, hash_len)
        self.data = bytearray()
        if version > 0:
            self.data += struct.pack(">i", version) + bytes(iv) + bytes(HEADER - 20)
        self.np = len(self.data)
        self.iv = bytes(iv)
        self.order = []  # keys in put order

    def put(self, key: bytes, record: bytes) -> int:
        """-> position of the record's bytes (cp + 8 + hash_len)."""
        if self.np >= self.blocksz or self.map.current >= self.map.w_max():
            raise ArchiveFull()
        cp = self.np
        value = cp + 4 + len(key)
        if self.version:
            value = (value << 32) | len(record)
        if not self.map.put(key, value):
            raise KeyError("HashExistsException")
        self.np = cp + 4 + len(key) + 4 + len(record)
        self.data += struct.pack(">i", len(key)) + key + struct.pack(">i", len(record)) + record
        assert len(self.data) == self.np
        self.order.append(bytes(key))
        return cp + 8 + len(key)

    def get_record(self, key: bytes):
        """getChunk's lookup: the stored record of ``key``, or None."""
        v = self.map.get(key)
        if v == -1:
            return None
        pos = (v >> 32) if self.version else v
        n = struct.unpack(">i", self.data[pos: pos + 4])[0]
        if self.version:
            assert n == v & 0xFFFFFFFF
        return bytes(self.data[pos + 4: pos + 4 + n])

    def walk(self):
        """[len][hash][len][record] from the header to the end -> [(key, record, record position)]."""
        out, p = [], HEADER if self.version > 0 else 0
        while p < len(self.data):
            hl = struct.unpack(">i", self.data[p: p + 4])[0]
            key = bytes(self.data[p + 4: p + 4 + hl])
            n = struct.unpack(">i", self.data[p + 4 + hl: p + 8 + hl])[0]
            out.append((key, bytes(self.data[p + 8 + hl: p + 8 + hl + n]), p + 8 + hl))
            p += 8 + hl + n
        assert p == len(self.data)
        return out


class Store:
    """The writable archive and the closed ones before it.  blocksz: list, archive a takes
    blocksz[min(a, len - 1)]; ivs: callable(a) -> 16 bytes."""

    def __init__(self, map_sz: int, blocksz, version: int, hash_len: int, ivs=None):
        self.map_sz, self.version, self.hash_len = map_sz, version, hash_len
        self.blocksz = list(blocksz) if isinstance(blocksz, (list, tuple)) else [blocksz]
        self.ivs = ivs or (lambda a: bytes(16))
        self.archives = []
        self.where = []  # per put: (archive, position)

    def _open(self):
        a = len(self.archives)
        self.archives.append(Archive(self.map_sz, self.blocksz[min(a, len(self.blocksz) - 1)], self.version,
                                     self.hash_len, self.ivs(a)))

    def put(self, key: bytes, record: bytes):
        if not self.archives:
            self._open()
        try:
            pos = self.archives[-1].put(key, record)
        except ArchiveFull:
            self._open()
            pos = self.archives[-1].put(key, record)
        self.where.append((len(self.archives) - 1, pos))
        return self.where[-1]


def bases(archives):
    out, end = [], 0
    for a in archives:
        b = (end + ALIGN - 1) // ALIGN * ALIGN
        out.append(b)
        end = b + len(a.data)
    return out, end


def store_image(archives) -> bytes:
    """Every archive at its base (multiples of 4096), zeros between; ends with the last image."""
    bs, end = bases(archives)
    img = bytearray(end)
    for b, a in zip(bs, archives):
        img[b: b + len(a.data)] = a.data
    return bytes(img)


def compact(arc: Archive, wanted, iv: bytes = bytes(16), recode=None):
    """-> the new archive, or None when nothing is left.  wanted(key) -> bool.  recode(record):
    getChunk followed by putChunk (identity without encryption)."""
    ar = [(k, v) for k, v in arc.map.entries() if wanted(k)]
    if not ar:
        return None
    new = Archive(len(ar) * 2 + 5, len(arc.data), arc.version, arc.hash_len, iv)
    for k, _ in ar:
        rec = arc.get_record(k)
        new.put(k, recode(rec) if recode else rec)
    return new
