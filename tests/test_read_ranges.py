"""Ranged reads (include/sdfs_read.h): DedupFileChannel.read for batches of byte ranges.

CPU: the host split (sdfs_cdc_read_split) against the plain-Python model (tests/range_model.py,
restated from DedupFileChannel.java:499-608 and WritableCacheBuffer.java:217-245) on hand-worked and
seeded random requests, its capacity and argument rules, the argument refusals of the two device
entry points, and the split's own text as a host program under AddressSanitizer and UBSan
(tests/cpu/read_split_check.cpp).  GPU: the piece plan and the piece gather against the model —
every alignment, the placement rules, status confinement (the one stated divergence from the
reference), the slice property against the whole-buffer read, windows above and below the LDS limit,
the fetch list — and the write -> store -> ranged read round trip at the product's own shape.
Parity status: pinned by the reference's own request walk and placement code (no fixtures)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import range_model as RM
from tests import read_model as R
from tests import test_read_path as T  # the hand-built images' helpers: _dev, _slots, _raw_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = T.PB
NONE = RM.NONE


# ------------------------------------------------------------------------------------------- CPU

def _split(files, requests, cl):
    from sdfs_amd.read import split_requests

    p = split_requests(files, requests, cl)
    pieces = list(zip(p.req.tolist(), p.row.tolist(), p.start.tolist(), p.len.tolist(), p.out_off.tolist()))
    return p.n_read.tolist(), pieces, p.rows.tolist()


def _same_as_model(files, requests, cl):
    got = _split(files, requests, cl)
    want = RM.split(files, requests, cl)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    return got


def test_split_hand_worked_cases():
    cl = 1000
    one = [(0, 4, 4000)]
    # inside one buffer
    assert _same_as_model(one, [(0, 1100, 200, 7)], cl) == ([200], [(0, 0, 100, 200, 7)], [1])
    # ending exactly on a boundary: no empty piece after it
    assert _same_as_model(one, [(0, 900, 100, 0)], cl) == ([100], [(0, 0, 900, 100, 0)], [0])
    assert _same_as_model(one, [(0, 1000, 1000, 0)], cl) == ([1000], [(0, 0, 0, 1000, 0)], [1])
    # spanning three buffers; the outputs follow each other from out_off
    assert _same_as_model(one, [(0, 950, 1100, 16)], cl) == (
        [1100], [(0, 0, 950, 50, 16), (0, 1, 0, 1000, 66), (0, 2, 0, 50, 1066)], [0, 1, 2])
    # file_pos == file_len: -1, nothing else; file_len - 1: one byte
    assert _same_as_model(one, [(0, 4000, 10, 0)], cl) == ([-1], [], [])
    assert _same_as_model(one, [(0, 5000, 10, 0)], cl) == ([-1], [], [])
    assert _same_as_model(one, [(0, 3999, 10, 3)], cl) == ([1], [(0, 0, 999, 1, 3)], [3])
    # siz == 0: 0, not -1, while inside the file
    assert _same_as_model(one, [(0, 5, 0, 0)], cl) == ([0], [], [])
    assert _same_as_model(one, [(0, 4000, 0, 0)], cl) == ([-1], [], [])
    # clipped by file_len in mid-buffer
    assert _same_as_model([(0, 4, 3500)], [(0, 2900, 5000, 0)], cl) == (
        [600], [(0, 0, 900, 100, 0), (0, 1, 0, 500, 100)], [2, 3])
    # a file longer than its map: the pieces past it have no row and the slots past it are no rows
    assert _same_as_model([(5, 2, 3500)], [(0, 1500, 2000, 0)], cl) == (
        [2000], [(0, 0, 500, 500, 0), (0, NONE, 0, 1000, 500), (0, NONE, 0, 500, 1500)], [6])
    assert _same_as_model([(5, 0, 3500)], [(0, 0, 10, 0)], cl) == ([10], [(0, NONE, 0, 10, 0)], [])
    # two files sharing one image; rows ascend whatever the request order is
    two = [(0, 3, 3000), (3, 2, 1500)]
    assert _same_as_model(two, [(1, 900, 400, 0), (0, 2500, 100, 400)], cl) == (
        [400, 100], [(0, 1, 900, 100, 0), (0, 2, 0, 300, 100), (1, 0, 500, 100, 400)], [2, 3, 4])
    # two requests touching the same slot: one row
    assert _same_as_model(one, [(0, 2100, 10, 0), (0, 2990, 20, 10)], cl) == (
        [10, 20], [(0, 0, 100, 10, 0), (1, 0, 990, 10, 10), (1, 1, 0, 10, 20)], [2, 3])
    # files far apart in the image (the rows are found by sorting, not through a table)
    far = [(1 << 40, 2, 2000), (7, 2, 2000), (1 << 50, 1, 1000)]
    assert _same_as_model(far, [(0, 1500, 10, 0), (2, 0, 5, 10), (1, 990, 20, 15), (0, 0, 1, 35)], cl) == (
        [10, 5, 20, 1], [(0, 3, 500, 10, 0), (1, 4, 0, 5, 10), (2, 0, 990, 10, 15), (2, 1, 0, 10, 25), (3, 2, 0, 1, 35)],
        [7, 8, 1 << 40, (1 << 40) + 1, 1 << 50])
    # nothing at all
    assert _same_as_model(one, [], cl) == ([], [], [])
    assert _same_as_model([], [], cl) == ([], [], [])


@pytest.mark.parametrize("cl", [1027, 262144])
def test_split_random_requests_vs_model(cl):
    rng = np.random.default_rng(cl)
    # on a boundary; in mid-buffer; longer than its map and sharing slots 10, 11 with the one before;
    # no map at all; a long one; one byte
    files = [(3, 5, 5 * cl), (8, 4, 4 * cl - 17), (10, 3, 5 * cl + 5), (13, 0, cl // 2), (13, 8, 8 * cl), (2, 2, 1)]
    requests, out = [], 5
    for _ in range(2000):
        f = int(rng.integers(0, len(files)))
        ln = files[f][2]
        pos = int(rng.integers(0, ln + cl))
        k = int(rng.integers(0, 8))
        if k == 0:
            pos = ln
        elif k == 1 and ln:
            pos = ln - 1
        elif k == 2:
            pos = pos // cl * cl
        siz = int(rng.integers(0, 3 * cl)) if rng.integers(0, 4) else int(rng.integers(0, 40))
        if rng.integers(0, 8) == 0:
            siz = (pos // cl + 1 + int(rng.integers(0, 3))) * cl - pos  # ends exactly on a boundary
        requests.append((f, pos, siz, out))
        out += siz + int(rng.integers(0, 3))
    n_read, pieces, rows = _same_as_model(files, requests, cl)
    assert -1 in n_read and 0 in n_read and any(p[1] == NONE for p in pieces) and len(rows) > 8
    assert len(pieces) <= sum(q[2] // cl + 2 for q in requests) and len(rows) <= len(pieces)
    assert sum(p[3] for p in pieces) == sum(n for n in n_read if n > 0)


def _split_raw(files, requests, cl, piece_cap, row_cap):
    """sdfs_cdc_read_split itself, with the capacities the caller names; arrays carry a guard entry."""
    lib = _lib.load()
    f = np.array(files, np.uint64).reshape(-1, 3)
    q = np.array(requests, np.uint64).reshape(-1, 4)
    n_read = np.full(len(q) + 1, 77, np.int64)
    u32 = [np.full(piece_cap + 1, 0xABABABAB, np.uint32) for _ in range(4)]
    out_off = np.full(piece_cap + 1, 0xAB, np.uint64)
    rows = np.full(row_cap + 1, 0xAB, np.uint64)
    n_p, n_r = ctypes.c_uint64(123), ctypes.c_uint64(456)
    ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.sdfs_cdc_read_split(ip(f), len(f), ip(q), len(q), cl, ip(n_read), piece_cap, ip(u32[0]), ip(u32[1]),
                                 ip(u32[2]), ip(u32[3]), ip(out_off), row_cap, ip(rows), ctypes.byref(n_p),
                                 ctypes.byref(n_r))
    return rc, n_p.value, n_r.value, n_read, u32, out_off, rows


def test_split_reports_the_counts_when_room_is_short():
    lib = _lib.load()
    files, cl = [(0, 8, 8000)], 1000
    requests = [(0, 950, 1100, 0), (0, 5500, 10, 1100), (0, 1999, 2, 1110)]  # 3 + 1 + 2 pieces; rows 0 1 2 5
    for piece_cap, row_cap in [(5, 4), (6, 3), (0, 0)]:
        rc, n_p, n_r, n_read, u32, out_off, rows = _split_raw(files, requests, cl, piece_cap, row_cap)
        assert rc == _lib.ECAP and (n_p, n_r) == (6, 4)
        assert b"6 pieces" in lib.sdfs_cdc_last_error()
        assert (u32[0] == 0xABABABAB).all() and (rows == 0xAB).all() and (out_off == 0xAB).all()  # nothing written
    rc, n_p, n_r, n_read, u32, out_off, rows = _split_raw(files, requests, cl, 6, 4)
    assert rc == 0 and (n_p, n_r) == (6, 4) and rows.tolist() == [0, 1, 2, 5, 0xAB]
    assert n_read.tolist() == [1100, 10, 2, 77] and u32[3].tolist() == [50, 1000, 50, 10, 1, 1, 0xABABABAB]
    # the argument rules
    for bad_files, bad_requests, bad_cl in [
        (files, [(1, 0, 10, 0)], cl),                      # a file that is not there
        (files, requests, 0), (files, requests, 1 << 31),  # chunk_length
        (files, [(0, 0, 1 << 63, 0)], cl),                 # siz
        (files, [(0, 0, 10, (1 << 64) - 5)], cl),          # out_off + n_read
        ([((1 << 64) - 2, 8, 8000)], requests, cl),        # first_slot + n_slots
        ([(0, 0, (1 << 64) - 1)], [(0, 0, (1 << 63) - 1, 0)], 1),  # more pieces than a 32-bit index holds
    ]:
        assert _split_raw(bad_files, bad_requests, bad_cl, 8, 8)[0] == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()
    from sdfs_amd.read import split_requests

    with pytest.raises(ValueError):
        split_requests(files, [(0, -1, 10, 0)], cl)
    with pytest.raises(_lib.SdfsCdcError):
        split_requests(files, [(3, 0, 10, 0)], cl)


def test_piece_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    p = T._fake_pairs()
    bad = T._fake_pairs()
    bad.nlen = None
    X = ctypes.c_void_p(0x1000)
    P = ctypes.byref(p)

    def einval(rc):
        assert rc == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()

    plan = lib.sdfs_cdc_read_plan_pieces
    #         dev nbuf pairs base n  dir       n_pieces row start len status  pf fc  src    dst    plain total stream
    einval(plan(0, 1, None, 0, 4, X, X, X, 2, X, X, X, X, X, X, X, X, X, X, None, X, None))
    einval(plan(0, 1, ctypes.byref(bad), 0, 4, X, X, X, 2, X, X, X, X, X, X, X, X, X, X, None, X, None))
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, None, X, X, X, X, X, X, X, X, X, None, X, None))  # piece_row
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, None, X, X, X, X, X, X, X, X, None, X, None))  # piece_start
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, X, None, X, X, X, X, X, X, X, None, X, None))  # piece_len
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, X, X, None, X, X, X, X, X, X, None, X, None))  # piece_status
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, X, X, X, None, X, X, X, X, X, None, X, None))  # pair_fetch
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, X, X, X, X, None, X, X, X, X, None, X, None))  # fetch_count
    einval(plan(0, 1, P, 0, 4, None, X, X, 2, X, X, X, X, X, X, X, X, X, X, None, X, None))  # the directory
    einval(plan(0, 1, P, 0, 4, X, X, X, 2, X, X, X, X, X, X, X, X, X, X, None, None, None))  # total_bytes
    einval(plan(0, 1, P, 0, (1 << 32) - 1, X, X, X, 2, X, X, X, X, X, X, X, X, X, X, None, X, None))
    einval(plan(0, 1, P, 0, 4, X, X, X, 1 << 31, X, X, X, X, X, X, X, X, X, X, None, X, None))
    asm = lib.sdfs_cdc_read_assemble_pieces
    #        dev nbuf cl pairs pf chunks off len n_pieces row start len out_off status req n_req req_status out stream
    einval(asm(0, 1, 4096, None, X, X, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 4096, ctypes.byref(bad), X, X, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 0, P, X, X, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 1 << 31, P, X, X, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 4096, P, None, X, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 4096, P, X, None, X, X, 2, X, X, X, X, X, X, 3, X, X, None))
    einval(asm(0, 1, 4096, P, X, X, X, None, 2, X, X, X, X, X, X, 3, X, X, None))
    for k in (0, 1, 2, 3, 4, 5, 8):  # each piece array, the requests' (with d_req_status), and the output
        args = [X, X, X, X, X, X, 3, X, X]
        args[k] = None
        einval(asm(0, 1, 4096, P, X, X, X, X, 2, *args, None))
    einval(asm(0, 1, (1 << 31) - 1, P, X, X, X, X, 1 << 20, X, X, X, X, X, None, 0, None, X, None))  # too many tiles


def test_model_piece_rules_hand_worked():
    cl, sb = 64, 13 + 56 * 6
    A, B, C = bytes(range(100, 120)), bytes(range(200, 230)), bytes(range(50, 60))
    ck = {5: A, 6: B, 8: None, 9: C}
    img = T._img([(5, 20, 0, 0, 20), (6, 30, 10, 0, 5), (7, 9, 30, 0, 4), (8, 9, 40, 0, 4), (9, 10, 50, 5, 9)])
    rp = lambda start, ln: RM.read_piece(img, sb, 32, cl, ck, start, ln)  # noqa: E731
    assert rp(0, 10) == (0, A[:10], {0})
    assert rp(8, 10) == (0, A[8:10] + B[:5] + A[15:18], {0, 1})  # overlap: the later pos wins
    assert rp(20, 10) == (0, bytes(10), set())                   # a gap fetches nothing
    assert rp(29, 2) == (R.MISSING, bytes(2), set())             # hashloc 7 is outside the directory
    assert rp(34, 6) == (0, bytes(6), set())                     # [30, 34) ended just before
    assert rp(43, 1) == (R.FETCH, bytes(1), {3})
    assert rp(44, 6) == (0, bytes(6), set())
    assert rp(49, 2) == (R.BOUNDS, bytes(2), {4})                # offset 5 + 9 > 10
    assert rp(40, 15) == (R.FETCH, bytes(15), {3, 4})            # FETCH is decided before BOUNDS
    assert rp(25, 20) == (R.MISSING, bytes(20), set())           # MISSING before both
    assert RM.read_piece(None, sb, 32, cl, ck, 3, 5) == (0, bytes(5), set())
    assert RM.read_piece(T._img([(5, 20, 0, 0, 20)], zlen=9), sb, 32, cl, ck, 0, 5) == (R.CORRUPT, bytes(5), set())
    # the terminator ends U: the pair after it is never touched; nlen == 0 never touches
    img = T._img([(5, 20, 0, 0, 4), (0, 20, 10, 0, 4), (7, 9, 20, 0, 4), (7, 9, 30, 0, 0)])
    assert RM.read_piece(img, sb, 32, cl, ck, 0, 64) == (0, A[:4] + bytes(60), {0})
    # the whole-buffer rule fails this buffer on a pair the piece [0, 10) does not touch
    img = T._img([(5, 20, 0, 0, 20), (7, 9, 30, 0, 4)])
    assert R.read_buffer(img, sb, 32, cl, ck) == (R.MISSING, bytes(cl))
    assert RM.read_piece(img, sb, 32, cl, ck, 0, 10) == (0, A[:10], {0})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_split_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "read_split_check"
    src = os.path.join(ROOT, "tests", "cpu", "read_split_check.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    src, "-o", str(exe)], check=True, timeout=240)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr[-6000:]


# ------------------------------------------------------------------------------------------- GPU

CANARY = 0xA5


def _ranges_and_check(images, slot_len, hash_len, cl, chunks, files, requests, out_bytes, verify=False):
    """Reads requests over hand-built images through HipBufferReader.read_ranges over a raw store
    holding `chunks` (entry k = the chunk of hashloc PB + k, None = a record that fails), into an
    output pre-filled with a canary, and compares with the model: n_read, the request and piece
    statuses, every output byte (the canary outside the extents included), the fetch count and
    which pairs carry a fetch.  -> (output bytes, RangeInfo, the model's results)."""
    import torch

    from sdfs_amd.read import HipBufferReader

    store, off, ln, raw = T._raw_store(chunks)
    out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda:0")
    rd = HipBufferReader(cl, hash_len)
    got, n_read, status, info = rd.read_ranges(T._slots(images, slot_len), len(images), slot_len, files, requests,
                                               store, off, ln, raw, PB, out=out)
    torch.cuda.synchronize()
    rd.destroy()
    want = bytearray([CANARY]) * out_bytes
    ck = {PB + k: c for k, c in enumerate(chunks)}
    model = RM.read_ranges(dict(enumerate(images)), slot_len, hash_len, cl, ck, files, requests, want)
    m_n_read, m_req, m_piece, m_needed, m_hashlocs, m_pieces, m_rows = model
    assert n_read.tolist() == m_n_read
    assert info.rows.tolist() == m_rows
    assert info.piece_status.tolist() == m_piece
    assert status.tolist() == m_req
    got = got.cpu().numpy()
    if got.tobytes() != bytes(want):
        diff = np.nonzero(got != np.frombuffer(bytes(want), np.uint8))[0]
        raise AssertionError(f"{len(diff)} output bytes differ, first at {diff[0]}")
    assert info.fetch_count == len(m_hashlocs)
    pf = info.pair_fetch.cpu().numpy()[:len(m_rows)]
    assert {(int(r), int(i)) for r, i in zip(*np.nonzero(pf != -1))} == m_needed
    return got, info, model


@pytest.mark.gpu
def test_gpu_pieces_every_alignment():
    """chunk_length 1027, cap 8: start 0..17 x len 1..40 x output misalignment 0..15, one request
    each, over a row of short pairs with gaps and an overlap; a canary between the extents."""
    rng = np.random.default_rng(17)
    cl, cap = 1027, 8
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(100) for _ in range(4)]
    pairs = [(rng.bytes(32), PB + 0, 100, 0, 3, 9), (rng.bytes(32), PB + 1, 100, 9, 0, 7),
             (rng.bytes(32), PB + 2, 100, 14, 11, 20), (rng.bytes(32), PB + 3, 100, 37, 1, 5),
             (rng.bytes(32), PB + 0, 100, 45, 50, 30)]
    images = [R.build_image(pairs)]
    requests, out = [], 0
    for start in range(18):
        for ln in range(1, 41):
            for mis in range(16):
                out = (out + 15) // 16 * 16 + 16 + mis  # at least one canary byte before each extent
                requests.append((0, start, ln, out))
                out += ln
    _, info, _ = _ranges_and_check(images, slot_len, 32, cl, chunks, [(0, 1, cl)], requests, out + 40)
    assert not info.piece_status.any() and len(requests) == 18 * 40 * 16


@pytest.mark.gpu
def test_gpu_pieces_placement_rules_and_overlap():
    rng = np.random.default_rng(4096)
    cl, cap = 4096, 8
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(1000) for _ in range(4)]
    P = lambda k, pos, off, nlen: (rng.bytes(32), PB + k if k >= 0 else 0, 1000, pos, off, nlen)  # noqa: E731
    images = [
        R.build_image([P(0, 0, 0, 600), P(1, 300, 0, 500), P(2, 350, 7, 50), P(3, 790, 0, 20)]),  # overlaps
        R.build_image([P(0, 100, 0, 5000), P(1, 2000, 40, 0), P(2, 2010, 990, 10), P(3, 3000, 5, 77)]),  # nlen > ck, 0
        R.build_image([P(0, 0, 0, 1000), P(-1, 1000, 0, 1000), P(1, 2000, 0, 1000)]),  # a terminator
        R.build_image([P(0, 10, 0, 100), P(1, 500, 5, 300), P(2, 4000, 900, 96)]),     # gaps
        bytes(slot_len),                                                               # a never-written slot
    ]
    files = [(0, len(images), len(images) * cl)]
    at = lambda b, start, ln: (0, b * cl + start, ln)  # noqa: E731
    ranges = [at(0, 0, 4096), at(0, 290, 70), at(0, 340, 70), at(0, 399, 2), at(0, 780, 40), at(0, 810, 5),
              at(1, 0, 4096), at(1, 1090, 20), at(1, 1100, 900), at(1, 1990, 40), at(1, 2900, 300),
              at(2, 0, 4096), at(2, 990, 20), at(2, 1000, 3000),   # past the terminator: zeros
              at(3, 110, 390), at(3, 800, 3200), at(3, 3990, 106), at(3, 0, 10),  # in gaps: zeros, no fetch
              at(4, 5, 100), at(0, 4000, 5000)]
    requests, out = [], 3
    for f, pos, ln in ranges:
        requests.append((f, pos, ln, out))
        out += ln + 5
    got, info, model = _ranges_and_check(images, slot_len, 32, cl, chunks, files, requests, out)
    assert not info.piece_status.any()
    # pieces that lie in a gap or past the terminator alone fetch nothing
    _, info, model = _ranges_and_check(images, slot_len, 32, cl, chunks, files,
                                       [(0, 2 * cl + 1000, 3000, 0), (0, 3 * cl + 110, 390, 3000), (0, 4 * cl, 50, 3390)],
                                       3440)
    assert info.fetch_count == 0 and not model[3]


@pytest.mark.gpu
def test_gpu_pieces_status_is_confined_to_the_touching_pairs():
    """One row with a pair outside the directory, a pair whose record is damaged and a pair out of
    bounds: each fails exactly the pieces that touch it; the whole-buffer read fails the whole row
    (the stated divergence).  A row that does not parse fails all its pieces."""
    import torch

    from sdfs_amd.read import HipBufferReader

    rng = np.random.default_rng(99)
    cl, cap = 4096, 8
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(500) for _ in range(3)] + [None]
    P = lambda loc, pos, off, nlen: (rng.bytes(32), loc, 500, pos, off, nlen)  # noqa: E731
    row = [P(PB + 0, 0, 0, 500), P(PB + 77, 600, 0, 200),   # MISSING
           P(PB + 1, 1000, 0, 500), P(PB + 3, 1600, 0, 200),  # FETCH
           P(PB + 2, 2000, 10, 500), P(PB + 1, 2600, 400, 200),  # BOUNDS: offset + c > ck.length
           P(PB + 2, 3000, 0, 500)]
    images = [R.build_image(row), R.build_image([P(PB + 0, 0, 0, 100), P(PB + 1, 200, -1, 100)]),
              R.build_image([P(PB + 1, 0, 0, 500)])]
    files = [(0, 3, 3 * cl)]
    cases = [((0, 500), 0), ((550, 100), R.MISSING), ((799, 2), R.MISSING), ((800, 200), 0), ((1000, 500), 0),
             ((1500, 101), R.FETCH), ((1799, 500), R.FETCH), ((1800, 200), 0), ((2000, 500), R.BOUNDS),
             ((2499, 102), R.BOUNDS), ((2700, 200), R.BOUNDS), ((2800, 1296), 0), ((3000, 500), 0),
             ((700, 1000), R.MISSING), ((1700, 400), R.FETCH), ((500, 100), 0),
             ((cl + 0, 10), R.CORRUPT), ((cl + 3000, 10), R.CORRUPT), ((2 * cl, 500), 0)]
    requests, out = [], 1
    for (pos, ln), _ in cases:
        requests.append((0, pos, ln, out))
        out += ln + 3
    got, info, model = _ranges_and_check(images, slot_len, 32, cl, chunks, files, requests, out)
    assert info.piece_status.tolist() == [st for _, st in cases]
    for ((pos, ln), st), q in zip(cases, requests):
        data = got[q[3]: q[3] + ln]
        assert (not data.any()) == (st != 0 or pos in (800, 1800, 500)), (pos, ln)
    # the whole-buffer read of the same rows: row 0 fails as a whole
    store, off, ln, raw = T._raw_store(chunks)
    rd = HipBufferReader(cl, 32)
    buf, status, _ = rd.read(T._slots(images, slot_len), 3, slot_len, store, off, ln, raw, PB)
    torch.cuda.synchronize()
    rd.destroy()
    assert status.tolist() == [R.MISSING, R.CORRUPT, 0] and not buf[0].any()
    assert R.read_buffer(images[0], slot_len, 32, cl, {PB + k: c for k, c in enumerate(chunks)})[0] == R.MISSING


@pytest.mark.gpu
def test_gpu_pieces_are_slices_of_the_whole_buffer_read():
    """Seeded random images whose whole-buffer status is 0: random pieces equal the slice of
    HipBufferReader.read's buffer, and the model."""
    import torch

    from sdfs_amd.read import HipBufferReader

    rng = np.random.default_rng(2024)
    cl, cap = 5003, 24
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(int(rng.integers(1, 700))) for _ in range(12)]
    images = []
    for b in range(6):
        pairs, pos = [], int(rng.integers(0, 30))
        for _ in range(int(rng.integers(0, cap + 1))):
            k = int(rng.integers(0, len(chunks)))
            n = len(chunks[k])
            off = int(rng.integers(0, n))
            nlen = int(rng.integers(0, n - off + 1)) if rng.integers(0, 5) else 5000  # nlen > ck.length at offset 0
            if nlen == 5000:
                off = 0
            if pos + min(nlen, n) > cl:
                break
            pairs.append((rng.bytes(32), PB + k, n, pos, off, nlen))
            pos += max(1, min(nlen, n) + int(rng.integers(-60, 200)))
        images.append(R.build_image(pairs))
    store, off, ln, raw = T._raw_store(chunks)
    rd = HipBufferReader(cl, 32)
    whole, status, _ = rd.read(T._slots(images, slot_len), len(images), slot_len, store, off, ln, raw, PB)
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any()
    whole = whole.cpu().numpy().reshape(-1)
    file_len = len(images) * cl - 1234
    requests, out = [], 0
    for _ in range(300):
        pos = int(rng.integers(0, file_len))
        siz = int(rng.integers(1, 200)) if rng.integers(0, 3) else int(rng.integers(1, 3 * cl))
        requests.append((0, pos, siz, out))
        out += min(siz, file_len - pos) + int(rng.integers(0, 4))
    got, info, model = _ranges_and_check(images, slot_len, 32, cl, chunks, [(0, len(images), file_len)], requests, out + 8)
    assert not info.piece_status.any()
    for (_, pos, siz, o), n in zip(requests, model[0]):
        assert n == min(siz, file_len - pos) and (got[o:o + n] == whole[pos:pos + n]).all(), (pos, siz)


@pytest.mark.gpu
def test_gpu_pieces_windows_above_and_below_the_lds_limit():
    """Slots of 1100 pairs (chunk_length 30011): a piece covering the whole buffer has a window of
    more than 1024 pairs and is gathered from global memory; small pieces of the same row stage
    their few pairs in LDS; a run of pieces whose windows grow by one pair each across the limit."""
    rng = np.random.default_rng(1100)
    cl, cap = 30011, 1100
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(300) for _ in range(16)]
    images, all_pairs = [], []
    for b in range(2):
        pairs, pos = [], int(rng.integers(0, 20))
        for _ in range(1050):
            n = int(rng.integers(1, 40))
            if pos + n > cl:
                break
            pairs.append((rng.bytes(32), PB + int(rng.integers(0, 16)), 300, pos, int(rng.integers(0, 200)), n))
            pos += max(1, n + int(rng.integers(-8, 9)))
        assert len(pairs) > 1024
        images.append(R.build_image(pairs))
        all_pairs.append(pairs)
    p0 = all_pairs[0]
    ranges = [(0, cl), (cl, cl), (5, 2 * cl - 100), (100, 1), (7000, 300), (cl - 50, 100), (cl + 12345, 4096)]
    # pairs 10 .. last start inside; the window also holds the few earlier pairs that reach pos[10]
    ranges += [(p0[10][3], p0[last][3] + 1 - p0[10][3]) for last in range(1026, 1038)]
    requests, out = [], 9
    for pos, ln in ranges:
        requests.append((0, pos, ln, out))
        out += ln + 7
    _, info, _ = _ranges_and_check(images, slot_len, 32, cl, chunks, [(0, 2, 2 * cl)], requests, out)
    assert not info.piece_status.any()


@pytest.mark.gpu
def test_gpu_piece_plan_lists_only_the_touched_records_once():
    import torch

    from sdfs_amd.read import parse_map_slots, plan_pieces, plan_reads

    rng = np.random.default_rng(3)
    cap, n_store, cl = 8, 12, 1000
    slot_len = 13 + 56 * cap
    raw = np.array([100 + 17 * k for k in range(n_store)], np.int32)
    slen = raw + 4 + np.arange(n_store, dtype=np.int32) % 3
    soff = (np.arange(n_store, dtype=np.int64) * 1000 + 5)
    P = lambda loc, pos: (rng.bytes(32), loc, 50, pos, 0, 50)  # noqa: E731
    uses = [[5, 2, 7, 11], [2, 9, 7], [7, 0, 5, 1]]  # pair i of a row at pos 100 * i
    images = [R.build_image([P(PB + k, 100 * i) for i, k in enumerate(u)]) for u in uses]
    images.append(R.build_image([P(PB + 6, 0), P(0, 100), P(PB + 4, 200)]))  # a terminator before entry 4
    images.append(R.build_image([P(PB + 3, 0), P(PB + n_store, 100)]))       # one pair outside the directory
    nrows = len(images)
    # (row, start, len): several pieces and rows name entries 2, 5 and 7
    pieces = [(0, 0, 120), (0, 149, 52), (1, 0, 50), (1, 199, 2), (2, 0, 1), (2, 149, 51), (0, 100, 50),
              (3, 0, 1000), (4, 0, 50), (4, 50, 60), (-1, 0, 1000), (2, 400, 600)]
    pr, ps, pl = (T._dev(np.array(c, np.int32), None) for c in zip(*pieces))
    p = parse_map_slots(T._slots(images, slot_len), nrows, slot_len, 32)
    dirs = (T._dev(soff, torch.int64), T._dev(slen, torch.int32), T._dev(raw, torch.int32))
    plan = plan_pieces(p, pr, ps, pl, *dirs, PB)
    whole = plan_reads(parse_map_slots(T._slots(images, slot_len), nrows, slot_len, 32), *dirs, PB)
    torch.cuda.synchronize()
    want = [0, 2, 3, 5, 6, 7]  # the model's needed set: 1, 4, 9 and 11 are touched by no piece
    ck = {PB + k: bytes(int(raw[k])) for k in range(n_store)}
    needed, hashlocs = set(), set()
    for row, start, ln in pieces:
        st, _, need = RM.read_piece(None if row < 0 else images[row], slot_len, 32, cl, ck, start, ln)
        needed |= {(row, i) for i in need}
        hashlocs |= {R.parse(images[row], slot_len, 32)[1][i][1] for i in need}
    assert sorted(h - PB for h in hashlocs) == want
    k = int(plan["fetch_count"].item())
    assert k == len(want) < int(whole["fetch_count"].item()) == 8
    assert plan["src_off"][:k].tolist() == [int(soff[i]) for i in want]
    assert plan["src_len"][:k].tolist() == [int(slen[i]) for i in want]
    assert plan["dst_cap"][:k].tolist() == [int(raw[i]) for i in want]
    r16 = lambda v: (int(v) + 15) // 16 * 16  # noqa: E731
    assert plan["dst_off"][:k].tolist() == [sum(r16(raw[j]) for j in want[:i]) for i in range(k)]
    assert plan["plain_off"][:k].tolist() == [sum(r16(slen[j]) for j in want[:i]) for i in range(k)]
    assert plan["total_bytes"].tolist() == [sum(r16(raw[j]) for j in want), sum(r16(slen[j]) for j in want)]
    assert plan["piece_status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, R.MISSING, 0, 0]
    assert not p.status.any()  # only what the parse wrote
    pf = plan["pair_fetch"].cpu().numpy()
    rank = {idx: f for f, idx in enumerate(want)}
    got = {(int(r), int(i)): int(pf[r, i]) for r, i in zip(*np.nonzero(pf != -1))}
    assert set(got) == needed
    for (row, i), f in got.items():
        assert f == rank[R.parse(images[row], slot_len, 32)[1][i][1] - PB]


# ---- the product's own shape: 8 buffers of 256 KiB through HipBufferWriter.write at its defaults

_KEY = bytes(range(7, 39))
_WRITTEN = {}
L, NBUF = 262144, 8
FILE_LEN = NBUF * L - 100_003  # ends in mid-buffer


def _written(variant, algo="sha256"):
    """variant: raw (uncompressed records), lz4, aes (LZ4 + AES-256, archives with IVs of their own).
    Written once per variant and shared; a test that damages the store works on a copy."""
    if (variant, algo) in _WRITTEN:
        return _WRITTEN[(variant, algo)]
    import torch

    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    hl = 16 if algo == "md5" else 32
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=L)
    batch.fill_streams(first_stream=777, bufs_per_stream=2)
    v = batch.data.view(NBUF, L)
    v[1, 20000:120000] = 0
    v[6].copy_(v[2])
    ix = HipHashesMap(1 << 12)
    aes = variant == "aes"
    wr = HipBufferWriter(ix, hash_len=hl, compress=variant != "raw", aes=_KEY if aes else None, version=1 if aes else 0)
    m, arcs = wr.write(batch, PB)
    torch.cuda.synchronize()
    assert int(arcs.extra["overflow"].item()) == 0
    counts, st, ln, dg, total = batch.host_results()
    w = dict(engine=e, hl=hl, m=m, arcs=arcs, data=batch.data.cpu().numpy().reshape(-1).copy(), variant=variant,
             slot_len=slot_bytes(hl, L, 4095), counts=counts, starts=st, lens=ln,
             loc=arcs.extra["hashloc"].cpu().numpy()[:total])
    wr.destroy()
    _WRITTEN[(variant, algo)] = w
    return w


def _reader(w):
    from sdfs_amd.read import HipBufferReader

    aes = w["variant"] == "aes"
    return HipBufferReader(L, w["hl"], aes=_KEY if aes else None, record_ivs=aes, engine=w["engine"])


def _random_requests(rng, n):
    requests, out = [], 0
    for i in range(n):
        k = int(rng.integers(0, 10))
        siz = int(rng.integers(1, 600 * 1024 + 1)) if k < 3 else int(rng.integers(1, 131073)) if k < 7 else int(
            rng.integers(1, 4097))
        pos = int(rng.integers(0, FILE_LEN + 200_000))      # some at or past the end of the file
        if i == 0:
            pos, siz = FILE_LEN - 5000, 20_000              # straddles the end
        elif i == 1:
            pos = FILE_LEN
        requests.append((0, pos, siz, out))
        out += max(0, min(siz, FILE_LEN - pos)) + int(rng.integers(0, 3))
    return requests, out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_write_store_read_ranges_round_trip(variant, algo):
    import torch

    w = _written(variant, algo)
    arcs = w["arcs"]
    rng = np.random.default_rng(len(variant) + len(algo))
    requests, out_bytes = _random_requests(rng, 200)
    out = torch.full((out_bytes + 16,), CANARY, dtype=torch.uint8, device="cuda:0")
    rd = _reader(w)
    got, n_read, status, info = rd.read_ranges(w["m"], NBUF, w["slot_len"], [(0, NBUF, FILE_LEN)], requests, arcs.store,
                                               *arcs.directory(), PB, verify=True, out=out,
                                               store_ivs=arcs.record_ivs())
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any() and not info.piece_status.any()
    assert not info.bad_count.any() and not info.pair_bad.any()
    want = np.full(out_bytes + 16, CANARY, np.uint8)
    for r, (_, pos, siz, o) in enumerate(requests):
        n = -1 if pos >= FILE_LEN else min(siz, FILE_LEN - pos)
        assert int(n_read[r]) == n, r
        if n > 0:
            want[o:o + n] = w["data"][pos:pos + n]
    assert n_read[0] == 5000 and n_read[1] == -1 and (n_read == -1).sum() > 2
    assert (got.cpu().numpy() == want).all()


@pytest.mark.gpu
def test_gpu_ranged_verify_marks_a_flipped_chunk_only_where_it_is_touched():
    """Payload byte 10 of one stored record flipped (an uncompressed store, so the record still
    decodes): verify marks exactly the needed pairs of that record, the requests that touch the
    chunk carry the flipped byte, and every other request is clean."""
    import torch

    w = _written("raw")
    arcs = w["arcs"]
    # a chunk of buffer 3 (not shared with any other buffer), at least 64 bytes long
    first = int(w["counts"][:3].sum())
    i = next(i for i in range(int(w["counts"][3])) if w["lens"][3, i] >= 64 and 0 < i)
    hashloc = int(w["loc"][first + i])
    assert (w["loc"] == hashloc).sum() == 1
    cpos = 3 * L + int(w["starts"][3, i])  # the chunk's file position
    off = int(arcs.store_off[hashloc - PB].item())
    store = arcs.store.clone()
    store[off + 4 + 10] ^= 0x40
    requests = [(0, cpos + 5, 20, 0), (0, cpos - 100, 50, 20), (0, cpos + 11, 5, 70), (0, 2 * L + 7, 4096, 75),
                (0, cpos - 4000, 4011, 4171), (0, 5 * L, 1000, 8182)]
    rd = _reader(w)
    got, n_read, status, info = rd.read_ranges(w["m"], NBUF, w["slot_len"], [(0, NBUF, FILE_LEN)], requests, store,
                                               *arcs.directory(), PB, verify=True)
    torch.cuda.synchronize()
    assert not status.any()  # the reference only logs the mismatch
    data = w["data"].copy()
    data[cpos + 10] ^= 0x40
    got = got.cpu().numpy()
    for _, pos, siz, o in requests:
        assert (got[o:o + siz] == data[pos:pos + siz]).all(), pos
    assert info.rows.tolist() == [2, 3, 5]
    bad = info.pair_bad.cpu().numpy()
    want = np.zeros_like(bad)
    want[1, i] = 1
    assert (bad == want).all() and info.bad_count.tolist() == [0, 1, 0]
    # requests that do not touch the chunk: nothing is marked, the record is not even fetched
    clean = [q for q in requests if q[1] + q[2] <= cpos or q[1] >= cpos + int(w["lens"][3, i])]
    assert len(clean) == 3
    got, n_read, status, info = rd.read_ranges(w["m"], NBUF, w["slot_len"], [(0, NBUF, FILE_LEN)], clean, store,
                                               *arcs.directory(), PB, verify=True)
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any() and not info.pair_bad.any() and not info.bad_count.any()
    assert int(info.pair_fetch[info.rows.tolist().index(3), i].item()) == -1


@pytest.mark.gpu
def test_gpu_read_ranges_with_nothing_to_read():
    import torch

    w = _written("lz4")
    arcs = w["arcs"]
    rd = _reader(w)
    args = (arcs.store, *arcs.directory(), PB)
    files = [(0, NBUF, FILE_LEN)]
    out = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda:0")
    for requests, want in [([], []), ([(0, FILE_LEN, 10, 0), (0, FILE_LEN + L, 1, 10)], [-1, -1]),
                           ([(0, 5, 0, 3)], [0])]:
        got, n_read, status, info = rd.read_ranges(w["m"], NBUF, w["slot_len"], files, requests, *args, verify=True, out=out)
        torch.cuda.synchronize()
        assert n_read.tolist() == want and status.tolist() == [0] * len(want)
        assert info.fetch_count == 0 and len(info.pieces.req) == 0 and info.rows.numel() == 0
        assert (out == CANARY).all()
    got, n_read, status, info = rd.read_ranges(w["m"], NBUF, w["slot_len"], files, [], *args)
    assert got.numel() == 0
    rd.destroy()


@pytest.mark.gpu
def test_gpu_read_file_returns_none_at_eof_and_raises_on_a_damaged_record():
    import torch

    w = _written("lz4")
    arcs = w["arcs"]
    rd = _reader(w)
    rf = lambda pos, siz, store=arcs.store: rd.read_file(w["m"], NBUF, w["slot_len"], FILE_LEN, pos, siz, store,  # noqa: E731
                                                         *arcs.directory(), PB)
    assert rf(FILE_LEN, 10) is None and rf(FILE_LEN + 1, 0) is None
    assert rf(10, 0) == b""
    assert rf(L - 7, 20) == w["data"][L - 7:L + 13].tobytes()
    assert rf(FILE_LEN - 3, 100) == w["data"][FILE_LEN - 3:FILE_LEN].tobytes()
    # the record of a chunk of buffer 3 cut down to its length header: its fetch fails
    first = int(w["counts"][:3].sum())
    hashloc = int(w["loc"][first + 1])
    cpos = 3 * L + int(w["starts"][3, 1])
    store_len = arcs.store_len.clone()
    store_len[hashloc - PB] = 2
    with pytest.raises(_lib.SdfsCdcError):
        rd.read_file(w["m"], NBUF, w["slot_len"], FILE_LEN, cpos + 1, 10, arcs.store, arcs.store_off, store_len,
                     arcs.raw_len, PB)
    # a range of the same buffer that does not touch it still reads
    assert rd.read_file(w["m"], NBUF, w["slot_len"], FILE_LEN, 3 * L, 100, arcs.store, arcs.store_off, store_len,
                        arcs.raw_len, PB) == w["data"][3 * L:3 * L + 100].tobytes()
    torch.cuda.synchronize()
    rd.destroy()
