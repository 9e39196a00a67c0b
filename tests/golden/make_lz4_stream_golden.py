"""Regenerate tests/golden/lz4_stream.json — anchors of the LZ4Block stream tests.

    python tests/golden/make_lz4_stream_golden.py

XXH32 vectors (seed 0: the published ones; seed 0x9747b28c: the stream's) and whole streams of
small inputs in hex, with the lengths and tokens of two larger ones, all from the pure-Python model
(tests/stream_model.py) over the R123 LZ4 oracle at block size 65 536.  The XXH32 values are
asserted here against the ``xxhash`` module when it imports.  lz4-java's jar is not available, so
the streams are the restated format's, not bytes a JVM wrote.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import cdc_oracle as C  # noqa: E402
from oracle import lz4_oracle as Z  # noqa: E402
from tests import stream_model as M  # noqa: E402

XXH_INPUTS = {"empty": b"", "a": b"a", "abc": b"abc", "spam": b"Nobody inspects the spammish repetition",
              "range64": bytes(range(64))}
RANDOM_SPEC = dict(seed=1, stream=4242, len=70000)  # oracle.cdc_oracle.synth


def random_input() -> bytes:
    return C.synth(RANDOM_SPEC["seed"], RANDOM_SPEC["stream"], 0, RANDOM_SPEC["len"]).tobytes()


def main() -> None:
    try:
        import xxhash
    except ImportError:
        xxhash = None
    xxh = []
    for seed, names in ((0, ["empty", "a", "abc", "spam"]), (M.SEED, ["empty", "a", "abc", "range64"])):
        for name in names:
            v = M.xxh32(XXH_INPUTS[name], seed)
            if xxhash is not None:
                assert v == xxhash.xxh32(XXH_INPUTS[name], seed=seed).intdigest(), (name, seed)
            xxh.append(dict(input=name, seed="%08x" % seed, xxh32="%08X" % v))
    streams = [dict(input_hex=d.hex(), stream_hex=M.write(d, 65536, Z.R123).hex()) for d in (b"", b"abc", b"a" * 20)]
    zeros = M.write(bytes(200000), 65536, Z.R123)
    rnd = M.write(random_input(), 65536, Z.R123)
    sizes = [dict(input="zeros", len=200000, stream_len=len(zeros), tokens=[b[3] | M.level(65536) for b in M.read(zeros)["blocks"]]),
             dict(input="random", spec=RANDOM_SPEC, stream_len=len(rnd),
                  tokens=[b[3] | M.level(65536) for b in M.read(rnd)["blocks"]])]
    with open(os.path.join(HERE, "lz4_stream.json"), "w") as f:
        json.dump(dict(note="tests/stream_model.py over oracle/lz4_ref.c (R123), block size 65536; lz4-java 1.3.0's "
                            "LZ4BlockOutputStream restated, not pinned against the jar",
                       xxh32=xxh, streams=streams, sizes=sizes), f, indent=1)
        f.write("\n")
    print(json.dumps(sizes))


if __name__ == "__main__":
    main()
