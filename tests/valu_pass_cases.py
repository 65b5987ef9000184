"""TEST INFRASTRUCTURE: writer-made streams (tests/deflate_writer.py) that sit on the edges of phase B (strip_step_b) and of the
groups (seq_group) of pure_zlib_amd/csrc/inflate_core.h -- the two bodies whose instructions the VALU pass rewrites.  Where an
edge depends on where the kernel cuts its strips and groups (which a stream cannot dictate), the streams SWEEP the quantity
through every value around it instead: every distance around the ring's near / far boundary, every alignment of a run against
the ring's end, every literal-run length against the 16-byte literal groups and the 4 / 8 records of a store.

cases(ring_bits) -> [(name, data, raw DEFLATE)]; zlib_wrap / gzip_wrap put the container around a raw stream."""
import random
import struct
import zlib

import deflate_writer as W

RUNS = (3, 4, 5, 8, 9, 15, 16, 17)            # literal runs placed across the ring's end
FAR_LENS = (3, 4, 7, 8, 9, 16, 17, 32, 33)    # match lengths around the dwords of a copy, SEQ_CAP = 32 and one more
SEQ_GLIM = 768                                # output bytes of a group at the most (inflate_core.h)


class Tokens:
    """tokens and the bytes they produce, side by side"""

    def __init__(self, seed):
        self.rng, self.t, self.out = random.Random(seed), [], bytearray()

    def lit(self, b):
        self.t.append(b)
        self.out.append(b)

    def lits(self, n, alphabet=range(32, 127)):
        for _ in range(n):
            self.lit(self.rng.choice(alphabet))

    def match(self, ln, dist):
        assert 3 <= ln <= 258 and 1 <= dist <= min(len(self.out), 32768), (ln, dist, len(self.out))
        self.t.append((ln, dist))
        for _ in range(ln):
            self.out.append(self.out[-dist])

    def fill_to(self, target, dist=lambda rng: rng.randint(40, 250)):
        """matches alone (no literal: the next run's count stays what the case wants) up to output offset `target`"""
        gap = target - len(self.out)
        assert gap == 0 or gap >= 6, gap
        while gap > 0:
            if gap > 64:
                ln = self.rng.choice((32, 31, 24, 12))
            elif gap > 32:
                ln = gap // 2
            else:
                ln = gap
            self.match(ln, dist(self.rng))
            gap -= ln

    def deflate(self, kind="dynamic", seed=1):
        w, blk = W.BitWriter(), W.Block(kind)
        blk.tokens = self.t
        W.write_block(w, blk, True, random.Random(seed), {"hlit": None, "hdist": None})
        return bytes(self.out), w.bytes()


def zlib_wrap(data, raw):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


def gzip_wrap(data, raw):
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def lit_runs_across_ring_end(ring, every_offset):
    """Literal runs of RUNS bytes (a match in front, a match behind: the record counts exactly that many) that start j bytes in
    front of a multiple of the ring's size, j = 1 .. L - 1 (every_offset) or L // 2: the run's destination wraps the ring's end."""
    k = Tokens(11 * ring)
    k.lits(300)
    edge = 0
    for ln in RUNS:
        for j in (range(1, ln) if every_offset else (ln // 2,)):
            edge += ring
            k.fill_to(edge - j)
            k.lits(ln)
            k.match(k.rng.choice((3, 4, 9, 20)), k.rng.randint(40, 250))
    return k.deflate()


def far_sweep(ring, lens, lo, hi, seed):
    """Matches of the given lengths at EVERY distance lo .. hi: with lo .. hi around ring - SEQ_GLIM .. ring, each length meets the
    distance at which its source ends exactly where the near matches' begin (a group's extent decides where that is: every value
    0 .. SEQ_GLIM is swept), and, further out, where it ends 128, 127, 129 ... bytes below the flushed part's end."""
    k = Tokens(seed)
    k.lits(300)
    k.fill_to(hi + 64)
    for ln in lens:
        for d in range(lo, hi + 1):
            if d > len(k.out) or d > 32768:
                break
            k.lits(k.rng.choice((0, 0, 1, 2)))
            k.match(ln, d)
    return k.deflate()


def record_edges(seed, kind):
    """Sequences whose literal runs go through 0 .. 18 and whose matches through 3 .. 12 bytes in two periods that are coprime: a
    lane's strip ends behind its 1st, 2nd, ... 9th ... record, on a match and inside a run, between the two literals of a step, and
    its literal count passes every value modulo 16 (two literals that would straddle a 16-byte group are taken one by one)."""
    k = Tokens(seed)
    k.lits(200)
    i = 0
    while len(k.out) < 48000:
        k.lits(i % 19, alphabet=range(97, 105))
        k.match(3 + i % 10, 1 + (i * 7) % min(len(k.out), 700))
        i += 1
    k.lits(5)
    return k.deflate(kind)


def out_of_steps(seed):
    """One-bit literals: a byte so frequent that its code is one bit long, in runs between stretches of ordinary tokens -- the strips
    are cut for the block's mean token, and the lanes inside a run have more tokens than steps (STRIP_TMAX): the span ends there."""
    k = Tokens(seed)
    for rep in range(6):
        k.lits(1500, alphabet=range(32, 96))
        for _ in range(40):
            k.match(k.rng.randint(3, 30), k.rng.randint(1, 1000))
            k.lits(k.rng.randint(0, 6), alphabet=range(32, 96))
        for _ in range(9000):
            k.lit(0x61)
    return k.deflate()


def cases(ring_bits):
    ring = 1 << ring_bits
    out = [("lit_runs_wrap", *lit_runs_across_ring_end(ring, every_offset=ring_bits <= 12))]
    if ring_bits < 15:  # (the hybrid window: sources older than the ring come from the flushed output)
        for n, lens in enumerate((FAR_LENS[0:3], FAR_LENS[3:6], FAR_LENS[6:9])):
            out.append(("far_sweep_%d" % n, *far_sweep(ring, lens, ring - SEQ_GLIM - 100, ring + 200, 100 + n)))
        out.append(("far_deep", *far_sweep(ring, FAR_LENS, 2 * ring + 1, 2 * ring + 140, 104)))
    else:        # (the 32 KiB ring: sources the group itself would overwrite go through seq_solo)
        out.append(("far_sweep_0", *far_sweep(ring, FAR_LENS[2:9:3], ring - SEQ_GLIM - 100, ring, 105)))
    out.append(("records_dynamic", *record_edges(7, "dynamic")))
    out.append(("records_fixed", *record_edges(8, "fixed")))
    out.append(("out_of_steps", *out_of_steps(9)))
    return out
