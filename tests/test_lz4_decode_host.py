"""The one-lane LZ4 decoder of the split decode (sdfs_amd/csrc/lz4_decode.h) as a host program
under AddressSanitizer and UBSan (tests/cpu/lz4_decode_fuzz.cpp): 200 000 encoder, emitter and
damaged blocks plus the structural edges, bare and framed, caps from len - 8 to len + 20, against
the program's own byte-at-a-time model — same verdict, same bytes, guard bytes intact, and no
sanitizer report.  The wave decoder cannot run on the host; tests/test_lz4_decode.py runs both
on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_decoder_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "lz4_decode_fuzz"
    src = os.path.join(ROOT, "tests", "cpu", "lz4_decode_fuzz.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    src, "-o", str(exe), "-ldl"], check=True, timeout=240)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr[-6000:]
