"""Seeded SparseDataChunk slot images of every kind the walks must tell apart — TEST
INFRASTRUCTURE ONLY (shared by tests/test_mapfile.py and tests/test_slot_walk.py)."""
from tests import read_model as R

KINDS = ["plain", "zero", "zlen0", "full", "over", "negzlen", "negfield", "repeat"]


def digest(rng, hl=32):
    return bytes(rng.getrandbits(8) for _ in range(hl))


def held(rng, n, hl, pos0=0):
    """n entries; positions 0 and 1 are real positions here (pos_base = 0)."""
    return [(digest(rng, hl).ljust(32, b"\0"), pos0 + i) for i in range(n)]


def seeded_image(rng, held, hl, cap):
    """One image in IMAGE order and its slot kind; ``held``: [(digest, pos)] the index holds."""
    kind = rng.choice(["plain"] * 6 + ["zero", "zlen0", "full", "over", "negzlen", "negfield", "repeat"])
    if kind == "zero":
        return b"", kind

    def pair(i):
        u = rng.random()
        d, loc = rng.choice(held)
        if u < 0.1:
            d = digest(rng, hl)        # not held
        elif u < 0.2:
            loc ^= 0x10000             # the wrong archive
        return (d[:hl], loc, 10, i * 10, 0, 10)

    n = {"zlen0": 0, "full": cap, "over": cap}.get(kind, rng.randint(1, cap))
    pairs = [pair(i) for i in range(n)]
    zlen = None
    if kind == "over":
        zlen = cap + 1
    elif kind == "negzlen":
        zlen = -rng.randint(1, 5)
    elif kind == "negfield":
        p = list(pairs[-1])
        p[rng.choice([2, 3, 4, 5])] = -rng.randint(1, 1 << 30)
        pairs[-1] = tuple(p)
    elif kind == "repeat" and n >= 2:
        for _ in range(rng.randint(1, 3)):
            i, j = rng.sample(range(n), 2)
            p = list(pairs[i])
            p[3] = pairs[j][3]
            pairs[i] = tuple(p)
        rng.shuffle(pairs)
    return R.build_image(pairs, flags=rng.randrange(256), doop=rng.randrange(1 << 20), zlen=zlen), kind
