"""Map files at rest: the LZ4Block stream (include/sdfs_lz4_stream.h; CompressionUtils.compressFile /
decompressFile, CompressionUtils.java:127-151 = lz4-java 1.3.0's LZ4BlockOutputStream / InputStream).

CPU: the pure-Python model (tests/stream_model.py) — XXH32 against the published vectors, the
``xxhash`` module and liblz4's frame content checksum; the golden streams (tests/golden/lz4_stream.json);
the level table and the bound; write -> read of every GPU case; the reader's flag for every corruption.
GPU: the HIP writer, header walk and reader through the C-ABI and through Python, byte for byte and
word for word against the model, with canary bytes around every output extent.
Parity status: unpinned — the format is restated from lz4-java's sources (the jar is not here); XXH32
is pinned three ways, the LZ4 blocks are the LZ4 tests' (R123 unpinned in two rules, V19 pinned)."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from oracle import cdc_oracle as C
from oracle import lz4_oracle as Z
from sdfs_amd import _lib
from tests import stream_model as M
from tests.golden.make_lz4_stream_golden import XXH_INPUTS, random_input

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "lz4_stream.json")))
EDGE_LENS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 63, 64, 65535, 65536, 65537]
KINDS = ["zeros", "text", "rand"]


def _gen(kind, n, stream=1):
    if kind == "rand":
        return C.synth(7, stream, 0, n).tobytes()
    if kind == "zeros":
        return bytes(n)
    return Z.text_like(7, stream, n).tobytes()


def _framing_lens(B):
    return [0, 1, 15, 16, 17, 63, 64, 65, B - 1, B, B + 1, 2 * B + 5]


def framing_files(B):
    """One batch per block size: every length of the list for the three data kinds."""
    return [_gen(k, n, stream=100 * ki + i) for ki, k in enumerate(KINDS) for i, n in enumerate(_framing_lens(B))]


def reference_files():
    """B = 65 536: the lengths around one block and 3 blocks + 100, three data kinds."""
    return [_gen(k, n, stream=300 + 10 * ki + i) for ki, k in enumerate(KINDS)
            for i, n in enumerate((65535, 65536, 65537, 3 * 65536 + 100))]


def wide_file():
    """B = 131 072 (level 7): a first block past 64 KiB + 11, where the LZ4 kernels switch to 32-bit tables."""
    return _gen("text", 131072 + 12, stream=77)


# ---- corruptions: name -> (stream bytes, the flag lz4-java's reader stops with, by its rules)

def _set_i32(s, at, v):
    return s[:at] + struct.pack("<I", v & 0xFFFFFFFF) + s[at + 4:]


def _flip(s, at, bit=1):
    return s[:at] + bytes([s[at] ^ bit]) + s[at + 1:]


def corruptions():
    lz = M.write(_gen("text", 300, 5), 65536)      # one LZ4 block, level 6
    raw = M.write(_gen("rand", 300, 6), 65536)     # one RAW block, level 6
    three = M.write(_gen("text", 2500, 8), 1024)   # three blocks, level 0
    b3 = M.read(three)["blocks"]
    assert lz[8] == 0x26 and raw[8] == 0x16 and len(b3) == 3
    lz_olen = struct.unpack_from("<I", lz, 13)[0]
    out = {
        "magic_block0": (_flip(lz, 3), M.MAGIC_BAD),
        "magic_block2_of_3": (_flip(three, b3[2][0] - 21 + 7, 0x40), M.MAGIC_BAD),
        "method_0x30": (lz[:8] + b"\x36" + lz[9:], M.HEADER_BAD),
        "original_len_above_level": (_set_i32(lz, 13, (1 << 16) + 1), M.HEADER_BAD),
        "compressed_len_negative": (_set_i32(lz, 9, -5), M.HEADER_BAD),
        "original_len_negative": (_set_i32(lz, 13, -lz_olen), M.HEADER_BAD),
        "raw_unequal_lengths": (_set_i32(raw, 13, 299), M.HEADER_BAD),
        "compressed_len_0_original_5": (_set_i32(_set_i32(lz, 9, 0), 13, 5), M.HEADER_BAD),
        "end_mark_check_1": (_set_i32(lz, len(lz) - 4, 1), M.HEADER_BAD),
        "cut_at_10": (lz[:10], M.TRUNCATED),
        "cut_at_21_plus_3": (lz[:24], M.TRUNCATED),
        "cut_before_end_mark": (lz[:-21], M.TRUNCATED),
        "compressed_len_past_file": (_set_i32(lz, 9, len(lz) - 21 + 1), M.TRUNCATED),
        "check_bit31": (_flip(lz, 20, 0x80), M.CHECKSUM),
        "raw_payload_flip": (_flip(raw, 21 + 150), M.CHECKSUM),
        "lz4_payload_flip": (_flip(lz, 21 + 40, 0x10), None),  # DECODE or CHECKSUM: whichever the model says
        "junk_after_end_mark": (lz + bytes(range(100)), 0),
    }
    return out


CORRUPTIONS = corruptions()


# =============================================================================================== CPU

def test_xxh32_anchors():
    for v in GOLDEN["xxh32"]:
        assert "%08X" % M.xxh32(XXH_INPUTS[v["input"]], int(v["seed"], 16)) == v["xxh32"], v
    # the same anchors, spelled out
    assert M.xxh32(b"") == 0x02CC5D05 and M.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F
    assert M.xxh32(b"abc", 0x9747B28C) == 0x4D4CB222 and M.xxh32(bytes(range(64)), 0x9747B28C) == 0x7DCA2BF8


def test_xxh32_against_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    for n in EDGE_LENS:
        d = _gen("rand", n, 40 + n % 7)
        for seed in (0, M.SEED, 0xFFFFFFFF):
            assert M.xxh32(d, seed) == xxhash.xxh32(d, seed=seed).intdigest(), (n, seed)


class _FramePrefs(ctypes.Structure):
    """LZ4F_preferences_t (lz4frame.h, liblz4 >= 1.8)."""

    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def test_xxh32_against_liblz4_frame_content_checksum():
    """An LZ4 frame written with the content-checksum flag ends with XXH32(content, seed 0), little-endian."""
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("no liblz4.so.1")
    L.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    L.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.POINTER(_FramePrefs)]
    L.LZ4F_compressFrame.restype = ctypes.c_size_t
    L.LZ4F_compressFrame.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(_FramePrefs)]
    L.LZ4F_isError.argtypes = [ctypes.c_size_t]
    for n in EDGE_LENS:
        d = _gen("text", n, 50 + n % 5)
        prefs = _FramePrefs()
        prefs.contentChecksumFlag = 1
        cap = L.LZ4F_compressFrameBound(n, ctypes.byref(prefs))
        buf = ctypes.create_string_buffer(cap)
        k = L.LZ4F_compressFrame(buf, cap, d, n, ctypes.byref(prefs))
        assert not L.LZ4F_isError(k)
        assert struct.unpack("<I", buf.raw[k - 4: k])[0] == M.xxh32(d, 0), n


def test_golden_streams():
    for s in GOLDEN["streams"]:
        d = bytes.fromhex(s["input_hex"])
        w = M.write(d, 65536, Z.R123)
        assert w.hex() == s["stream_hex"]
        r = M.read(w)
        assert r["status"] == 0 and r["data"] == d and r["consumed"] == len(w)
    # the same anchors, spelled out
    end = "4c5a34426c6f636b16000000000000000000000000"
    assert M.write(b"").hex() == end
    assert M.write(b"abc").hex() == "4c5a34426c6f636b16030000000300000022b24c0d616263" + end
    assert M.write(b"a" * 20).hex() == "4c5a34426c6f636b260a000000140000005c328e0e1a610100506161616161" + end
    zeros, rnd = GOLDEN["sizes"]
    assert (zeros["stream_len"], rnd["stream_len"], rnd["tokens"]) == (930, 70063, [0x16, 0x16])
    assert len(M.write(bytes(200000))) == 930
    w = M.write(random_input())
    assert len(w) == 70063 and [b[3] | 6 for b in M.read(w)["blocks"]] == [0x16, 0x16]


LEVELS = {64: 0, 100: 0, 1024: 0, 1025: 1, 2048: 1, 65535: 6, 65536: 6, 65537: 7, 131072: 7, 1 << 25: 15}


def test_level_table():
    lib = _lib.load()
    for b, lv in LEVELS.items():
        assert M.level(b) == lv and lib.sdfs_cdc_lz4_stream_level(b) == lv, b
    for b in (0, 1, 63, (1 << 25) + 1, 0xFFFFFFFF):
        assert lib.sdfs_cdc_lz4_stream_level(b) == -1 and lib.sdfs_cdc_lz4_stream_bound(1000, b) == 0
        with pytest.raises(ValueError):
            M.level(b)


def test_stream_bound():
    lib = _lib.load()
    for B in (64, 100, 1024, 65536, 131072, 1 << 25):
        for n in (0, 1, B - 1, B, B + 1, 2 * B + 5, 200000, 29413376, (1 << 33) + 7):
            want = n + 21 * (-(-n // B) + 1)
            assert lib.sdfs_cdc_lz4_stream_bound(n, B) == want == M.bound(n, B), (B, n)
    assert lib.sdfs_cdc_lz4_stream_bound(0, 65536) == 21 and lib.sdfs_cdc_lz4_stream_bound(200000, 65536) == 200105
    # incompressible input reaches the bound exactly; nothing passes it
    for B, n in ((64, 200), (1024, 3000), (65536, 70000)):
        assert len(M.write(_gen("rand", n, 9), B)) == M.bound(n, B)
    for n in (0, 21, 22, 43, 44, 1000):
        assert lib.sdfs_cdc_lz4_stream_max_blocks(n) == n // 22 + 1


@pytest.mark.parametrize("mode", [Z.R123, Z.V19])
def test_model_round_trip_of_every_gpu_case(mode):
    cases = [(B, d) for B in (64, 100, 1024) for d in framing_files(B)]
    cases += [(65536, d) for d in reference_files()] + [(131072, wide_file())]
    for B, d in cases:
        w = M.write(d, B, mode)
        assert len(w) <= M.bound(len(d), B)
        r = M.read(w)
        assert r["status"] == 0 and r["data"] == d and r["consumed"] == len(w), (B, len(d))
        assert r["n_blocks"] == -(-len(d) // B) and r["decoded_len"] == len(d)
        assert all(b[3] | M.level(B) == w[b[0] - 13] for b in r["blocks"])
    assert M.write(wide_file(), 131072)[8] == 0x27


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_model_reader_flags_every_corruption(name):
    s, want = CORRUPTIONS[name]
    r = M.read(s)
    if want is None:
        assert r["status"] in (M.DECODE, M.CHECKSUM)
    else:
        assert r["status"] == want, M.flag_names(r["status"])
    assert (r["data"] is None) == (r["status"] != 0)
    if name == "junk_after_end_mark":
        assert r["consumed"] == len(s) - 100 and r["data"] == _gen("text", 300, 5)
    if name == "magic_block2_of_3":
        assert r["n_blocks"] == 2 and r["decoded_len"] == 2048


# =============================================================================================== GPU

CANARY = 0xC3
GAP = 48  # canary bytes before, between and behind the extents (also the room the block kernels' wide loads may touch)


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_state = {}


def _codec(mode=Z.R123):
    from sdfs_amd.lz4 import HipLz4Compressor
    from sdfs_amd.lz4_stream import HipLz4BlockStream

    if mode not in _state:
        _state[mode] = HipLz4BlockStream(HipLz4Compressor(mode))
    return _state[mode]


def _lay(files, first=GAP, step=1):
    """The files in one host image at offsets that walk through every alignment, canaries between."""
    offs, at = [], first
    for i, d in enumerate(files):
        offs.append(at)
        at += len(d) + GAP + (i * step) % 4
    img = np.full(at + GAP, CANARY, np.uint8)
    for o, d in zip(offs, files):
        img[o: o + len(d)] = np.frombuffer(d, np.uint8)
    return img, np.array(offs, np.uint64), np.array([len(d) for d in files], np.uint64)


def _canaries_intact(host, offs, lens):
    """Everything of ``host`` outside the extents still holds the canary."""
    mask = np.ones(len(host), bool)
    for o, k in zip(offs, lens):
        mask[int(o): int(o) + int(k)] = False
    return bool((host[mask] == CANARY).all())


def capi_compress(codec, files, B):
    """sdfs_cdc_lz4_stream_compress_device into canary-filled room: the streams, after checking
    that nothing outside [out_off, out_off + produced) was written."""
    torch = _torch()
    lib = _lib.load()
    img, offs, lens = _lay(files)
    d = torch.from_numpy(img).cuda()
    room = [int(lib.sdfs_cdc_lz4_stream_bound(int(k), B)) for k in lens]
    out_img, out_offs, _ = _lay([bytes(r) for r in room], step=3)
    out = torch.full((len(out_img),), CANARY, dtype=torch.uint8, device="cuda")
    out_lens = torch.full((len(files),), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.sdfs_cdc_lz4_stream_compress_device(
        codec.z._h, d.data_ptr(), offs.ctypes.data, lens.ctypes.data, len(files), B, out.data_ptr(),
        out_offs.ctypes.data, out_lens.data_ptr(), torch.cuda.current_stream().cuda_stream))
    got_lens = out_lens.cpu().numpy()
    host = out.cpu().numpy()
    assert (d.cpu().numpy() == img).all()
    assert all(0 < int(k) <= r for k, r in zip(got_lens, room))
    assert _canaries_intact(host, out_offs, got_lens)
    return [host[int(o): int(o) + int(k)].tobytes() for o, k in zip(out_offs, got_lens)]


def capi_read(codec, streams, exact_blocks=True, info=None):
    """scan + decompress through the C-ABI with canaries around every decoded extent.  Returns per
    file (walk dict, final status, decoded bytes); info (a dict) receives the block bound passed."""
    torch = _torch()
    lib = _lib.load()
    img, offs, lens = _lay(streams)
    d = torch.from_numpy(img).cuda()
    n = len(streams)
    cap = np.array([int(lib.sdfs_cdc_lz4_stream_max_blocks(int(k))) for k in lens], np.uint64)
    base = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    files = torch.full((n, 3), -1, dtype=torch.int64, device="cuda")
    blocks = torch.full((int(cap.sum()), 4), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sdfs_cdc_lz4_stream_scan_device(codec.z._h, d.data_ptr(), offs.ctypes.data, lens.ctypes.data, n,
                                                   files.data_ptr(), blocks.data_ptr(), base.ctypes.data, s))
    f = files.cpu().numpy().view(np.uint64)
    bl = blocks.cpu().numpy().view(np.uint64)
    walks = []
    for i in range(n):
        nb = int(f[i, 0] >> 32)
        tab = bl[int(base[i]): int(base[i]) + nb]
        walks.append(dict(status=int(f[i, 0] & 0xFFFFFFFF), n_blocks=nb, decoded_len=int(f[i, 1]), consumed=int(f[i, 2]),
                          blocks=[(int(e[0]) - int(offs[i]), int(e[1] & 0xFFFFFFFF), int(e[1] >> 32),
                                   int(e[2] & 0xFFFFFFFF), int(e[2] >> 32)) for e in tab],
                          decoded_offs=[int(e[3]) for e in tab]))
        assert (bl[int(base[i]) + nb: int(base[i]) + int(cap[i])] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    decoded = np.array([w["decoded_len"] for w in walks], np.uint64)
    out_img, out_offs, _ = _lay([bytes(int(k)) for k in decoded], step=1)
    out = torch.full((len(out_img),), CANARY, dtype=torch.uint8, device="cuda")
    total = sum(w["n_blocks"] for w in walks)
    max_blocks = total if exact_blocks else int(cap.sum())
    if info is not None:
        info["max_blocks"] = max_blocks
    _lib.check(lib.sdfs_cdc_lz4_stream_decompress_device(
        codec.z._h, d.data_ptr(), n, files.data_ptr(), blocks.data_ptr(), base.ctypes.data,
        max_blocks, out.data_ptr(), out_offs.ctypes.data, decoded.ctypes.data, s))
    f2 = files.cpu().numpy().view(np.uint64)
    host = out.cpu().numpy()
    assert (d.cpu().numpy() == img).all()
    assert _canaries_intact(host, out_offs, decoded)
    assert (f2[:, 1:] == f[:, 1:]).all() and ((f2[:, 0] >> 32) == (f[:, 0] >> 32)).all()
    return [(w, int(f2[i, 0] & 0xFFFFFFFF), host[int(out_offs[i]): int(out_offs[i]) + int(decoded[i])].tobytes())
            for i, w in enumerate(walks)]


def _same_walk(got, want):
    return all(got[k] == want[k] for k in ("n_blocks", "decoded_len", "consumed", "blocks"))


def _check_batch(codec, files, B, mode=Z.R123):
    want = [M.write(d, B, mode) for d in files]
    got = capi_compress(codec, files, B)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (B, i, len(files[i]), len(g), len(w))
    for i, (walk, status, data) in enumerate(capi_read(codec, got)):
        m = M.read(want[i])
        assert status == 0 and walk["status"] == 0 and _same_walk(walk, m), (B, i)
        assert walk["decoded_offs"] == [j * B for j in range(walk["n_blocks"])]
        assert data == files[i], (B, i)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 100, 1024])
def test_gpu_framing_and_xxh32_edges(B):
    _check_batch(_codec(), framing_files(B), B)


def _real_map():
    """emit_map_slots output of a 6-buffer write, as tests/test_mapfile.py builds its store."""
    torch = _torch()
    from sdfs_amd import HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    if "map" not in _state:
        e = HipVariableSha256HashEngine()
        batch = DeviceBatch(e, nbuf=6, buf_len=262144)
        batch.fill_streams(first_stream=6260, bufs_per_stream=1)
        batch.data.view(6, 262144)[3:].copy_(batch.data.view(6, 262144)[:3])
        ix = HipHashesMap(1 << 13)
        m, arcs = HipBufferWriter(ix, compress=True, blocksz=[200000, 260000, 150000]).write(batch, 1 << 33)
        torch.cuda.synchronize()
        assert int(arcs.extra["overflow"].item()) == 0
        _state["map"] = (m, 6, slot_bytes(32, 262144, 4095))
        _state["keep"] = (e, ix)
    return _state["map"]


@pytest.mark.gpu
def test_gpu_reference_block_size_and_a_real_map():
    m, nbuf, sl = _real_map()
    image = m.cpu().numpy().tobytes()
    assert len(image) == nbuf * sl and any(image)
    _check_batch(_codec(), reference_files() + [image], 65536)


@pytest.mark.gpu
def test_gpu_32bit_table_route():
    codec = _codec()
    d = wide_file()
    got = capi_compress(codec, [d], 131072)
    assert got[0] == M.write(d, 131072) and got[0][8] == 0x27
    (walk, status, data), = capi_read(codec, got)
    assert status == 0 and data == d and walk["n_blocks"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [Z.R123, Z.V19])
def test_gpu_modes(mode):
    files = [_gen(k, n, 500 + i) for i, (k, n) in enumerate((k, n) for k in KINDS for n in (70000, 65536 + 12))]
    _check_batch(_codec(mode), files, 65536, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 0x9747B28C])
def test_gpu_xxh32_alone(seed):
    torch = _torch()
    codec = _codec()
    B = 1024
    lens = _framing_lens(B)
    base = np.frombuffer(_gen("rand", 4 * sum(lens) + 4 * 16 * len(lens) + 64, 21), np.uint8)
    offs, at = [], 0
    for a in range(4):           # start offset mod 4 = a
        for n in lens:
            at = (at + 3) // 4 * 4 + a
            offs.append(at)
            at += n
    ln = lens * 4
    assert at <= len(base) and sorted({o % 4 for o in offs}) == [0, 1, 2, 3]
    got = codec.xxh32(torch.from_numpy(base.copy()).cuda(), torch.tensor(offs, dtype=torch.int64, device="cuda"),
                      torch.tensor(ln, dtype=torch.int32, device="cuda"), seed).cpu().numpy().view(np.uint32)
    want = [M.xxh32(base[o: o + n].tobytes(), seed) for o, n in zip(offs, ln)]
    assert got.tolist() == want
    # a device count below n_max: the rest is not written
    from sdfs_amd.lz4_stream import xxh32

    cnt = torch.tensor([5], dtype=torch.int32, device="cuda")
    part = codec.xxh32(torch.from_numpy(base.copy()).cuda(), torch.tensor(offs, dtype=torch.int64, device="cuda"),
                       torch.tensor(ln, dtype=torch.int32, device="cuda"), seed, count=cnt)
    assert part.cpu().numpy().view(np.uint32)[:5].tolist() == want[:5]
    assert xxh32(b"abc", seed) == M.xxh32(b"abc", seed) and xxh32(b"", seed) == M.xxh32(b"", seed)


@pytest.mark.gpu
def test_gpu_round_trip_map_and_host_bytes():
    torch = _torch()
    from sdfs_amd import SdfsCdcError, close_map, compressFile, decompressFile, open_map, snapshot_compressed

    codec = _codec()
    m, nbuf, sl = _real_map()
    image = close_map(codec, m, nbuf, sl)
    assert image.cpu().numpy().tobytes() == M.write(m.cpu().numpy().tobytes(), 65536)
    back, n = open_map(codec, image, sl)
    assert n == nbuf and torch.equal(back, m[: nbuf * sl])
    assert torch.equal(snapshot_compressed(codec, m, nbuf, sl), image)
    with pytest.raises(SdfsCdcError, match="whole number"):
        open_map(codec, image, sl + 1)
    bad = image.clone()
    bad[3] ^= 1
    with pytest.raises(SdfsCdcError, match="MAGIC"):
        open_map(codec, bad, sl)
    for d in (b"", b"abc", b"a" * 20, _gen("text", 200000, 3), random_input()):
        s = compressFile(d)
        assert s == M.write(d, 65536) and decompressFile(s) == d
    assert compressFile(b"a" * 20).hex() == GOLDEN["streams"][2]["stream_hex"]
    with pytest.raises(SdfsCdcError, match="TRUNCATED"):
        decompressFile(compressFile(b"abc")[:-1])
    # through the Python batch calls, a table sized by the bound instead of the exact block count
    streams = [M.write(_gen(k, 3000, 30 + i), 1024) for i, k in enumerate(KINDS)]
    for (walk, status, data), k in zip(capi_read(codec, streams, exact_blocks=False), KINDS):
        assert status == 0 and data == _gen(k, 3000, 30 + KINDS.index(k))


@pytest.mark.gpu
def test_gpu_reader_on_the_split_route():
    """The reader passes its block bound to the LZ4 decode as the batch capacity, and the decode
    chooses its route by capacity: with the bound the C-ABI documents (the sum of
    stream_max_blocks = len / 22 + 1) a batch above ~1.08 MB of streams takes the split decode
    with bare 64 KiB blocks, with the exact block count it takes the wave kernel.  Text files,
    64 KiB random files (RAW blocks: zero-length entries in the decode batch) and every
    corruption beside good neighbours: statuses, walks and bytes equal the model on both."""
    codec = _codec()
    lib = _lib.load()
    thr = int(lib.sdfs_cdc_lz4_hybrid_min_items(codec.z._h))
    assert thr > 0
    texts = [M.write(_gen("text", n, 910 + i), B)
             for i, (n, B) in enumerate(((5000, 1024), (70000, 65536), (300, 64), (20000, 65536)))]
    rnd = [M.write(_gen("rand", 65536, 920 + i), 65536) for i in range(2)]
    streams = []
    for i, name in enumerate(sorted(CORRUPTIONS)):
        streams += [texts[i % 4], CORRUPTIONS[name][0]]
    streams += texts
    i = 0
    while sum(len(s) // 22 + 1 for s in streams) < thr + 1:
        streams.append(rnd[i % 2])
        i += 1
    assert sum(len(s) for s in streams) > 22 * thr and i >= 4
    split, wave = {}, {}
    res_split = capi_read(codec, streams, exact_blocks=False, info=split)
    res_wave = capi_read(codec, streams, exact_blocks=True, info=wave)
    assert split["max_blocks"] >= thr > wave["max_blocks"] > 0, (split, wave, thr)
    model = {}
    for i, s in enumerate(streams):
        m = model.setdefault(s, M.read(s))
        for route, res in (("split", res_split), ("wave", res_wave)):
            walk, status, data = res[i]
            assert M.flag_names(status) == M.flag_names(m["status"]), (route, i)
            assert _same_walk(walk, m), (route, i)
            if m["status"] == 0:
                assert data == m["data"], (route, i)
        assert res_split[i][:2] == res_wave[i][:2], i
    assert sum(model[s]["status"] != 0 for s in streams) >= 15


@pytest.mark.gpu
def test_gpu_batch_isolation():
    codec = _codec()
    good = [_gen(k, n, 60 + i) for i, (k, n) in enumerate([("text", 5000), ("rand", 3000), ("zeros", 70000),
                                                             ("text", 65536), ("rand", 1)])]
    streams = [M.write(d, 65536) for d in good]
    bad = [CORRUPTIONS[k][0] for k in ("magic_block2_of_3", "raw_payload_flip", "compressed_len_past_file")]
    batch = [streams[0], bad[0], streams[1], streams[2], bad[1], bad[2], streams[3], streams[4]]
    res = capi_read(codec, batch)
    for i, d in zip((0, 2, 3, 6, 7), good):
        assert res[i][1] == 0 and res[i][2] == d, i
    for i, s in zip((1, 4, 5), bad):
        assert res[i][1] == M.read(s)["status"] != 0, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_gpu_corruptions(name):
    codec = _codec()
    s, _ = CORRUPTIONS[name]
    left, right = _gen("text", 700, 1), _gen("rand", 90, 2)
    res = capi_read(codec, [M.write(left, 1024), s, M.write(right, 64)])
    assert res[0][1] == 0 and res[0][2] == left and res[2][1] == 0 and res[2][2] == right
    walk, status, data = res[1]
    m = M.read(s)
    assert M.flag_names(status) == M.flag_names(m["status"])
    assert _same_walk(walk, m), (walk, m)
    if m["status"] == 0:
        assert data == m["data"] and walk["consumed"] == len(s) - 100
    # the walk's own word: what is wrong with a header; what decoding finds comes on top of it
    assert walk["status"] == (m["status"] if m["status"] in (M.TRUNCATED, M.MAGIC_BAD, M.HEADER_BAD) else 0)
