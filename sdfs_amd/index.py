"""Device-resident dedup-hit index (include/sdfs_index.h) — the step SDFS runs right after
getChunks: group a buffer's chunks by fingerprint, put each distinct one into the hash store
with its claim count, and mark every chunk duplicate or new with its hashloc
(SparseDedupFile.java:435-446,487-564; RocksDBMap.put, RocksDBMap.java:785-870).

:class:`HipHashesMap` mirrors the parts of ``org.opendedup.collections.AbstractHashesMap`` this
step uses (``put`` -> ``InsertRecord``, ``get``, ``containsKey``, ``getSize``, ``getMaxSize``) for a
whole batch of fingerprint records at once, and the way back: ``claimKey`` with a negative or
positive count (DedupFileStore.removeRef / addRef, DedupFileStore.java:130-141,161-172;
RocksDBMap.claimKey, RocksDBMap.java:388-509) and ``claimRecords``, the collection pass
(RocksDBMap.java:630-714).  An unreferenced fingerprint stays in the index, findable, until a
sweep removes it (include/sdfs_index.h).  No CPU fallback: it needs the HIP library and a
gfx950 device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib


@dataclass
class InsertRecord:
    """org.opendedup.collections.InsertRecord: was the fingerprint inserted, and where it lives."""

    inserted: bool
    pos: int


@dataclass
class IndexStats:
    """Fingerprints held (unreferenced ones not yet swept included), tombstones left by sweeps,
    and the number of slots that may be filled (both count against it)."""

    live: int
    tombstones: int
    capacity: int


@dataclass
class SlotClaims:
    """What ``claim_slots`` did (device tensors; reading a property waits for the device)."""

    counts: object       # int64 [4]: pairs applied, pairs missed, corrupt slots, selected slots with a pair
    slot_status: object  # int32 [nslots]: 0 or READ_CORRUPT
    slot_missed: object  # int32 [nslots]: pairs whose digest is not held at their hashloc

    applied = property(lambda self: int(self.counts[0].item()))
    missed = property(lambda self: int(self.counts[1].item()))
    corrupt = property(lambda self: int(self.counts[2].item()))
    nonempty = property(lambda self: int(self.counts[3].item()))


@dataclass
class Recount:
    """What ``recount`` found (device tensors), describing the state before any repair."""

    counts: object       # int64 [8]: counted, missed, corrupt slots, under, over, unnamed, equal, listed
    slot_status: object  # int32 [nslots]
    slot_missed: object  # int32 [nslots]
    digests: object      # uint8 [cap, 32]: the first counts[7] rows of these four are the mismatches,
    pos: object          # int64 [cap]       in table-slot order
    have: object         # int64 [cap]: the index's count
    want: object         # int64 [cap]: the pairs that name the fingerprint

    counted = property(lambda self: int(self.counts[0].item()))
    missed = property(lambda self: int(self.counts[1].item()))
    corrupt = property(lambda self: int(self.counts[2].item()))
    under = property(lambda self: int(self.counts[3].item()))
    over = property(lambda self: int(self.counts[4].item()))
    unnamed = property(lambda self: int(self.counts[5].item()))
    equal = property(lambda self: int(self.counts[6].item()))
    listed = property(lambda self: int(self.counts[7].item()))

    def mismatches(self):
        """[(digest bytes, pos, have, want)] of the listed entries (a host read)."""
        k = self.listed
        d = self.digests[:k].cpu().numpy()
        return [(d[i].tobytes(), p, h, w) for i, (p, h, w) in
                enumerate(zip(self.pos[:k].tolist(), self.have[:k].tolist(), self.want[:k].tolist()))]


class HipHashesMap:
    def __init__(self, capacity: int, device: int = 0):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.sdfs_cdc_index_create(int(device), int(capacity), ctypes.byref(h)))
        self._h = h
        self.device = device

    def destroy(self) -> None:
        if self._h:
            self._lib.sdfs_cdc_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # --- batch path (device tensors) -------------------------------------------------------
    def put_records(self, records, count=None, pos_base: int = 0, stream=None):
        """Apply fingerprint records (torch uint8 [n, 48] on the device, buffer order).

        ``count``: optional device int32[1] holding the number of valid records (the engine's
        ``total``).  Returns device tensors (dup u8[n], hashloc int64[n], new_list int32[n],
        new_count int64[1]); enqueued on ``stream`` (default: torch's current stream)."""
        import torch

        n = int(records.shape[0])
        dev = records.device
        dup = torch.empty(n, dtype=torch.uint8, device=dev)
        hashloc = torch.empty(n, dtype=torch.int64, device=dev)
        new_list = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        new_count = torch.zeros(1, dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.sdfs_cdc_index_put_records(
            self._h, records.data_ptr() if n else None, n, count.data_ptr() if count is not None else None,
            int(pos_base), dup.data_ptr() if n else None, hashloc.data_ptr() if n else None,
            new_list.data_ptr(), new_count.data_ptr(), s))
        return dup, hashloc, new_list, new_count

    def get_digests(self, digests, stream=None):
        """Look up digests (torch uint8 [n, 32] on the device): (pos int64[n], -1 when absent;
        refcount int64[n])."""
        import torch

        n = int(digests.shape[0])
        pos = torch.empty(n, dtype=torch.int64, device=digests.device)
        ref = torch.empty(n, dtype=torch.int64, device=digests.device)
        if n:
            s = stream if stream is not None else torch.cuda.current_stream(digests.device).cuda_stream
            _lib.check(self._lib.sdfs_cdc_index_get(self._h, digests.data_ptr(), n, pos.data_ptr(),
                                                    ref.data_ptr(), s))
        return pos, ref

    def claim_digests(self, digests, delta, expect_pos=None, stream=None):
        """AbstractHashesMap.claimKey for a batch (RocksDBMap.java:388-509): add ``delta`` (device
        int64[n], or one int for every item) to the count of each digest (torch uint8 [n, 32] on
        the device) that is present and, where ``expect_pos`` (device int64[n], -1 = any) names
        one, lives at that position.  Returns pos int64[n], -1 where nothing was claimed.
        Enqueued on ``stream`` (default: torch's current stream; an int ``delta`` is expanded on
        torch's current stream, so pass a tensor when ``stream`` is another one)."""
        import torch

        n = int(digests.shape[0])
        dev = digests.device
        pos = torch.empty(n, dtype=torch.int64, device=dev)
        if n:
            if not isinstance(delta, torch.Tensor):
                delta = torch.full((n,), int(delta), dtype=torch.int64, device=dev)
            delta = delta.to(device=dev, dtype=torch.int64).contiguous()
            if delta.shape[0] != n:
                raise ValueError("one delta per digest")
            if expect_pos is not None:
                expect_pos = expect_pos.to(device=dev, dtype=torch.int64).contiguous()
                if expect_pos.shape[0] != n:
                    raise ValueError("one expected position per digest")
            digests = digests.contiguous()
            s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self._lib.sdfs_cdc_index_claim(
                self._h, digests.data_ptr(), expect_pos.data_ptr() if expect_pos is not None else None,
                delta.data_ptr(), n, pos.data_ptr(), s))
        return pos

    def sweep(self, cap=None, stream=None):
        """AbstractHashesMap.claimRecords (RocksDBMap.java:630-714): remove up to ``cap`` (default:
        all) fingerprints whose count is <= 0.  Returns (digests u8[k, 32], pos int64[k] — what
        the chunk store may now drop, in no particular order — and the number of dead
        fingerprints left behind).  Waits for the sweep to finish (k comes from the device)."""
        if cap is None:
            cap = self.stats().live
        digests, pos, counts = self.sweep_device(int(cap), stream)
        self.stats()  # synchronises the sweep's stream
        k, left = (int(v) for v in counts.tolist())
        return digests[:k], pos[:k], left

    def sweep_device(self, cap: int, stream=None):
        """:meth:`sweep` without the wait: enqueues the sweep on ``stream`` (default, and where
        given the stream torch is currently on: the outputs are allocated there) and returns the
        device tensors (digests u8[cap, 32], pos int64[cap], counts int64[2] = removed, left
        behind); the first counts[0] rows are valid once the stream has got there."""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        digests = torch.empty(max(cap, 1), 32, dtype=torch.uint8, device=dev)
        pos = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.sdfs_cdc_index_sweep(self._h, digests.data_ptr(), pos.data_ptr(), int(cap),
                                                  counts.data_ptr(), s))
        return digests, pos, counts

    # --- map-file walks, the audit, the way in and out (sdfs_cdc_index_claim_slots ...) --------
    @staticmethod
    def _slots_view(m, nslots: int, slot_len: int, sel):
        """The image's first nslots * slot_len bytes (contiguous uint8) and the mask as uint8."""
        import torch

        if m.numel() < nslots * slot_len:
            raise ValueError(f"map holds {m.numel()} bytes, {nslots} slots of {slot_len} need {nslots * slot_len}")
        if m.dtype != torch.uint8 or not m.is_contiguous():
            raise ValueError("the slot image is a contiguous uint8 tensor")
        if sel is not None:
            sel = sel.to(device=m.device, dtype=torch.uint8).contiguous()
            if sel.shape[0] != nslots:
                raise ValueError("one selection flag per slot")
        return sel

    def claim_slots(self, m, nslots: int, slot_len: int, delta: int, sel=None, free: bool = False,
                    hash_len: int = 32, stream=None) -> "SlotClaims":
        """``claimKey(hash, hashloc, delta)`` for every pair of the selected slots of the image
        ``m`` (device uint8, nslots slots of slot_len bytes), read straight from the image by
        ``parse_map_slots``' rule.  ``sel``: device mask [nslots] (None: every slot).  ``free``:
        selected slots that parsed are then overwritten with zeros in ``m`` (FREE).  No host wait:
        the result's tensors are valid once the stream has got there."""
        import torch

        sel = self._slots_view(m, nslots, slot_len, sel)
        dev = m.device
        status = torch.empty(max(nslots, 1), dtype=torch.int32, device=dev)
        missed = torch.empty(max(nslots, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.check(self._lib.sdfs_cdc_index_claim_slots(
            self._h, m.data_ptr() if nslots else None, int(nslots), int(slot_len), int(hash_len), _lib.ptr(sel),
            int(delta), 1 if free else 0, status.data_ptr(), missed.data_ptr(), counts.data_ptr(),
            _lib.stream_of(m, stream)))
        return SlotClaims(counts, status[:nslots], missed[:nslots])

    def recount(self, m, nslots: int, slot_len: int, sel=None, repair: bool = False, cap: int = 1024,
                hash_len: int = 32, stream=None) -> "Recount":
        """The audit (``sdfs_cdc_index_recount``): counts every pair of the image ``m`` — which must
        hold every persisted slot of the volume — into a shadow count per fingerprint and compares
        it with the index's count.  The first ``cap`` mismatching entries come back in table-slot
        order; with ``repair`` every count is then set to what the slots say.  No host wait."""
        import torch

        sel = self._slots_view(m, nslots, slot_len, sel)
        dev = m.device
        cap = int(cap)
        status = torch.empty(max(nslots, 1), dtype=torch.int32, device=dev)
        missed = torch.empty(max(nslots, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        dg = torch.empty(max(cap, 1), 32, dtype=torch.uint8, device=dev)
        pos, have, want = (torch.empty(max(cap, 1), dtype=torch.int64, device=dev) for _ in range(3))
        _lib.check(self._lib.sdfs_cdc_index_recount(
            self._h, m.data_ptr() if nslots else None, int(nslots), int(slot_len), int(hash_len), _lib.ptr(sel),
            1 if repair else 0, status.data_ptr(), missed.data_ptr(), dg.data_ptr(), pos.data_ptr(), have.data_ptr(),
            want.data_ptr(), cap, counts.data_ptr(), _lib.stream_of(m, stream)))
        return Recount(counts, status[:nslots], missed[:nslots], dg, pos, have, want)

    def load(self, digests, pos, ref, stream=None):
        """``sdfs_cdc_index_load``: entries with the caller's positions (digests uint8 [n, 32], pos and
        ref int64 [n] on the device).  Returns status uint8 [n]: 0 = the item's count was added to
        the entry at its pos, 1 = conflict (the digest lives at another pos; nothing added)."""
        import torch

        n = int(digests.shape[0])
        dev = digests.device
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            digests = digests.contiguous()
            pos = pos.to(device=dev, dtype=torch.int64).contiguous()
            ref = ref.to(device=dev, dtype=torch.int64).contiguous()
            if pos.shape[0] != n or ref.shape[0] != n:
                raise ValueError("one pos and one count per digest")
            _lib.check(self._lib.sdfs_cdc_index_load(self._h, digests.data_ptr(), pos.data_ptr(), ref.data_ptr(), n,
                                                     status.data_ptr(), _lib.stream_of(digests, stream)))
        return status

    def export(self, cap=None, stream=None):
        """``sdfs_cdc_index_export``: every held entry, those with count <= 0 included, in
        table-slot order: (digests uint8 [k, 32], pos int64 [k], ref int64 [k], held) with k =
        min(cap, held).  Waits for the export to finish (k comes from the device)."""
        import torch

        if cap is None:
            cap = self.stats().live
        cap = int(cap)
        dev = torch.device(f"cuda:{self.device}")
        dg = torch.empty(max(cap, 1), 32, dtype=torch.uint8, device=dev)
        pos = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        ref = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        n = torch.empty(2, dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.sdfs_cdc_index_export(self._h, dg.data_ptr(), pos.data_ptr(), ref.data_ptr(), cap,
                                                   n.data_ptr(), s))
        self.stats()  # synchronises the export's stream
        k, held = (int(v) for v in n.tolist())
        return dg[:k], pos[:k], ref[:k], held

    def compact(self, stream=None) -> None:
        """Rebuild the table now, dropping the tombstones (needs as much free device memory as
        the index holds; put_records does this by itself when a batch would not fit otherwise)."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.sdfs_cdc_index_compact(self._h, s))

    def stats(self) -> "IndexStats":
        live, tomb, cap = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._lib.sdfs_cdc_index_stats(self._h, ctypes.byref(live), ctypes.byref(tomb),
                                                  ctypes.byref(cap)))
        return IndexStats(live.value, tomb.value, cap.value)

    # --- AbstractHashesMap-style conveniences (host bytes) -------------------------------------
    def claimKey(self, key: bytes, val: int, ct: int) -> int:
        """AbstractHashesMap.claimKey(hash, val, ct): add ct (negative: DedupFileStore.removeRef,
        positive: addRef) to the count of ``key`` if it lives at ``val`` (-1: wherever it lives);
        its pos, or -1."""
        import torch

        expect = torch.tensor([int(val)], dtype=torch.int64, device=f"cuda:{self.device}")
        return int(self.claim_digests(self._digest_tensor([key]), int(ct), expect)[0].item())

    def claimRecords(self) -> list:
        """AbstractHashesMap.claimRecords: remove every unreferenced fingerprint; [(digest, pos)]."""
        digests, pos, _ = self.sweep()
        d = digests.cpu().numpy()
        return [(d[i].tobytes(), p) for i, p in enumerate(pos.tolist())]

    def _digest_tensor(self, keys):
        import torch

        buf = bytearray(32 * len(keys))
        for i, k in enumerate(keys):
            if len(k) > 32:
                raise ValueError("fingerprints are at most 32 bytes")
            buf[32 * i:32 * i + len(k)] = k
        return torch.frombuffer(buf, dtype=torch.uint8).reshape(-1, 32).to(f"cuda:{self.device}")

    def get(self, key: bytes) -> int:
        """AbstractHashesMap.get: the fingerprint's pos, or -1."""
        pos, _ = self.get_digests(self._digest_tensor([key]))
        return int(pos[0].item())

    def containsKey(self, key: bytes) -> bool:
        return self.get(key) != -1

    def refcount(self, key: bytes) -> int:
        _, ref = self.get_digests(self._digest_tensor([key]))
        return int(ref[0].item())

    def clear(self, stream=None) -> None:
        """AbstractHashesMap.clear: drop every fingerprint (enqueued on `stream`)."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.sdfs_cdc_index_clear(self._h, s))

    def getSize(self) -> int:
        used, cap = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._lib.sdfs_cdc_index_size(self._h, ctypes.byref(used), ctypes.byref(cap)))
        return used.value

    def getMaxSize(self) -> int:
        used, cap = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._lib.sdfs_cdc_index_size(self._h, ctypes.byref(used), ctypes.byref(cap)))
        return cap.value
