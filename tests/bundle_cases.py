"""TEST INFRASTRUCTURE: zlib streams of the FIXED code written token by token (tests/deflate_writer.py), aimed at the edges of the
bundles (pure_zlib_amd/csrc/bundle_core.h: 64 streams to a wavefront, one lane per stream): the near/far switch of the lane's
512-byte window (NEAR_MAX = 496), matches that overlap themselves, the two far landing registers, steps of 49 bits, 9-bit
literals at every literal position of a step, blocks that end at every bit offset, streams cut or padded at their tails,
capacities that end inside a token, and the size limits.  Reference semantics: Deflate.hs:79-82, 106-120, 241-251.

all_cases() -> [Case]; the first three fields of a Case are (name, data, stream).  Every case says whether it is PLAIN -- valid, of
the fixed code only, capacity at or above the need, length and capacity below MAX_BYTES: what a lane must decode -- or not (what a
lane must leave to the ordinary kernel; a wrong trailer alone is a lane's to report).  Everything is seeded; each base stream is
checked against the system zlib when it is built."""
import collections
import functools
import random
import zlib

import deflate_writer as W

MAX_BYTES = 1 << 20  # Bundle::MAX_BYTES
NEAR_MAX = 496       # Bundle::NEAR_MAX
PHASE = 4            # Bundle::PHASE

Case = collections.namedtuple("Case", "name data stream cap plain wrong_trailer family")

ALT = "284+31"  # (258, distance, ALT): the length written as symbol 284 with five extra bits (227 + 31), not as symbol 285

GRID_DISTS = list(range(1, 20)) + list(range(480, 530)) + [1000, 4095, 4096, 4097, 32767, 32768]
GRID_LENS = [3, 4, 5, 7, 8, 9, 15, 16, 17, 130, 131, 257, 258]
WIDE_DISTS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 480, 495, 496, 497, 498, 511, 512, 513, 528, 1000, 4096, 32768]
WIDE_LENS = [3, 8, 9, 16, 17, 258]


def write_fixed(w, tokens, final):
    """One block of the fixed code from explicit tokens (deflate_writer.write_block, and the ALT spelling of length 258 beside it)."""
    if not any(isinstance(t, tuple) and len(t) == 3 for t in tokens):
        b = W.Block("fixed")
        b.tokens = tokens
        W.write_block(w, b, final, None, {})
        return
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            w.code(W.FIXED_LIT[t])
            continue
        if len(t) == 3:
            assert t[0] == 258 and t[2] == ALT
            w.code(W.FIXED_LIT[284])
            w.put(31, 5)
        else:
            s, ev, eb = W._LEN_SYM[t[0]]
            w.code(W.FIXED_LIT[s])
            w.put(ev, eb)
        d, dv, db = W.dist_sym(t[1])
        w.code(W.FIXED_DIST[d])
        w.put(dv, db)
    w.code(W.FIXED_LIT[256])


def expand(tokens, out):
    """What the tokens decode to, appended to the bytearray `out` (RFC 1951 3.2.3)."""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        ln, d = t[0], t[1]
        assert 3 <= ln <= 258 and 1 <= d <= min(len(out), 32768), (t, len(out))
        s = len(out) - d
        if d >= ln:
            out += out[s:s + ln]
        else:
            for k in range(ln):
                out.append(out[s + k])


def zstream(blocks, eob_at=None):
    """(data, zlib stream) of the token lists `blocks`, one block of the fixed code each, the last one final.  eob_at: a list that
    receives the bit position of every block's end-of-block code, counted from the stream's first byte."""
    out = bytearray()
    w = W.BitWriter()
    for i, tokens in enumerate(blocks):
        expand(tokens, out)
        write_fixed(w, tokens, i == len(blocks) - 1)
        if eob_at is not None:
            eob_at.append(16 + w.bitpos() - 7)
    data = bytes(out)
    z = bytes([0x78, 0x9c]) + w.bytes() + zlib.adler32(data).to_bytes(4, "big")
    assert zlib.decompress(z) == data
    return data, z


@functools.lru_cache(maxsize=None)
def _history(n, seed):
    """Tokens that decode to exactly n bytes with no period: random literals, then random matches and literals."""
    rng = random.Random(1000003 * seed + n)
    tokens, have = [], 0
    while have < n:
        left = n - have
        if have < 48 or left < 3 or rng.random() < 0.3:
            tokens.append(rng.randrange(256))
            have += 1
            continue
        ln = min(left, rng.choice([3, 4, 5, 8, 11, 30, 70, 130, 200, 258, 258]))
        top = min(have, 32768)
        d = rng.randint(1, top) if rng.random() < 0.5 else rng.randint(1, min(top, 1 << rng.randint(0, 15)))
        tokens.append((ln, d))
        have += ln
    return tuple(tokens)


def history(n, seed=0):
    return list(_history(n, seed))


def lits9(rng, n):
    return [rng.randrange(144, 256) for _ in range(n)]


def lits8(rng, n):
    return [rng.randrange(0, 144) for _ in range(n)]


class _Set:
    def __init__(self):
        self.cases, self.names = [], set()

    def add(self, family, name, data, stream, cap=None, plain=True, wrong_trailer=False):
        name = family + "/" + name
        assert name not in self.names, name
        self.names.add(name)
        self.cases.append(Case(name, data, stream, len(data) if cap is None else cap, plain, wrong_trailer, family))

    def tokens(self, family, name, blocks):
        data, z = zstream(blocks)
        self.add(family, name, data, z)


def _grid_case(dist, ln, lead):
    rng = random.Random(dist * 70001 + ln * 131 + lead)
    base = max(16, (dist + 15) // 16 * 16)  # the first match starts `lead` bytes into a 16-byte flush group
    ln2 = GRID_LENS[(GRID_LENS.index(ln) + 5) % len(GRID_LENS)] if ln in GRID_LENS else 3 + (ln * 7 + lead) % 256
    return [history(base, dist % 7) + [rng.randrange(256) for _ in range(lead)] + [(ln, dist)] + lits9(rng, 3) + [(ln2, dist), rng.randrange(256)]]


def _window_grid(s):
    for dist in GRID_DISTS:
        for ln in GRID_LENS:
            for lead in range(4):
                s.tokens("grid", "d%d_l%d_s%d" % (dist, ln, lead), _grid_case(dist, ln, lead))
    for dist in WIDE_DISTS:
        for ln in WIDE_LENS:
            for lead in range(4, 16):
                s.tokens("grid", "d%d_l%d_s%d" % (dist, ln, lead), _grid_case(dist, ln, lead))


def _handover(s):
    rng = random.Random(0x4A0)
    fars = [497, 498, 504, 512, 513, 600, 1999, 2400]
    lens = [3, 5, 8, 9, 16, 17, 33, 258]
    for d1 in fars:
        for ln in lens:
            d2 = fars[(fars.index(d1) + 3) % len(fars)]
            ln2 = lens[(lens.index(ln) + 3) % len(lens)]
            pre = history(2400 + (d1 + ln) % 16, 1)
            s.tokens("handover", "far_far_d%d_l%d" % (d1, ln), [pre + [(ln, d1), (ln2, d2), (ln, d1), 200]])
            near = [1, 3, 8, 100, 495, 496][(d1 + ln) % 6]
            s.tokens("handover", "far_near_far_d%d_l%d" % (d1, ln), [pre + [(ln, d1), (ln2, near), (ln, d2), (3, 496), (ln2, 497), 7]])
    # a far match of 258 bytes that begins in every step of a phase: j matches of three bytes in front of it, one step each
    for j in range(2 * PHASE):
        for d in (497, 700, 5000):
            pre = history(5008 + j, 2)
            s.tokens("handover", "phase_j%d_d%d" % (j, d), [pre + [(3, 5)] * j + [(258, d), (258, d + 1), 201, (258, 497)]])
    # the nearest far source right behind a long run of literals (nothing of the window's content comes from a match)
    for ln in GRID_LENS:
        for run in (600, 601, 602, 603, 1111):
            lit = [rng.randrange(256) for _ in range(run)]
            s.tokens("handover", "lits%d_d497_l%d" % (run, ln), [lit + [(ln, 497), 150, (ln, 496), 250, (ln, 498)]])
    # a distance equal to the bytes produced so far: the source is byte 0 of the extent
    for have in list(range(1, 21)) + [495, 496, 497, 498, 511, 512, 513, 1000, 4096, 32767, 32768]:
        for ln in (3, 8, 9, 258):
            pre = history(have, 3)
            s.tokens("handover", "from_byte0_n%d_l%d" % (have, ln), [pre + [(ln, have), 222, (ln, min(have + ln + 1, 32768))]])


def _overlap(s):
    rng = random.Random(0x0E1)
    for d in range(1, 9):
        for ln in list(range(3, 25)) + [258]:
            for at in range(4):
                pre = [rng.randrange(256) for _ in range(16 + at)]
                s.tokens("overlap", "d%d_l%d_at%d" % (d, ln, at), [pre + [(ln, d)] + lits9(rng, 2) + [(ln, d), (3 + (ln + at) % 22, d)]])


def _bitrate(s):
    for v in range(4):
        rng = random.Random(0xB17 + v)
        # 49 bits a step: two 9-bit literals, length 258 as symbol 284 + 5 extra bits, distance 32768 (13 extra bits)
        pre = history(32768 + v, 4 + v)
        body = []
        for _ in range(256 + 16 * v):
            body += lits9(rng, 2) + [(258, 32768, ALT)]
        s.tokens("bitrate", "49bits_%d" % v, [pre + body + lits9(rng, 3)])
        s.tokens("bitrate", "nines_%d" % v, [lits9(rng, 3000 + 1000 * v + v)])
        # the fewest bits a step: distance 1, length 258
        s.tokens("bitrate", "ones_%d" % v, [[65 + v] + [(258, 1)] * (270 + 10 * v)])
        # 8- and 9-bit literals mixed: the second and third literal of a step at every place they can start
        s.tokens("bitrate", "mixed_literals_%d" % v, [[rng.randrange(256) for _ in range(5000 + v)]])
        # the ALT spelling next to near and far distances, behind one, two and three literals
        body = history(3000, 9 + v)
        for _ in range(60):
            body += [rng.randrange(256) for _ in range(rng.randrange(0, 5))] + [(258, rng.choice([1, 7, 8, 496, 497, 3000]), ALT)]
        s.tokens("bitrate", "alt258_%d" % v, [body])


def _pad_to(w_bits, target):
    """(a, b): a 8-bit and b 9-bit literals move a bit position `w_bits` to `target` modulo 64."""
    b = (target - w_bits) % 8
    a = ((target - w_bits - 9 * b) // 8) % 8
    return a, b


def _blocks(s):
    for nblocks in (2, 5, 64):
        for t in range(64):
            rng = random.Random(nblocks * 64 + t)
            blocks, pos, have = [], 16, 0  # pos: the bit position in the stream, from its first byte
            want = []
            for i in range(nblocks):
                pos += 3
                tokens = []
                if have >= 8 and i % 3 == 1:  # a match across the block boundary
                    ln, d = rng.choice([3, 9, 40]), rng.randint(1, have)
                    tokens.append((ln, d))
                    s9, ev, eb = W._LEN_SYM[ln]
                    pos += W.FIXED_LIT[s9][1] + eb + 5 + W.dist_sym(d)[2]
                    have += ln
                target = (t + 11 * i) % 64
                a, b = _pad_to(pos, target)
                if i == 0 and a + b == 0:
                    a = 8
                lit = lits8(rng, a) + lits9(rng, b)
                rng.shuffle(lit)
                tokens += lit
                pos += 8 * a + 9 * b
                have += a + b
                want.append(pos)
                pos += 7
                blocks.append(tokens)
            at = []
            data, z = zstream(blocks, at)
            assert at == want and all((p - (t + 11 * i)) % 64 == 0 for i, p in enumerate(at)), (nblocks, t)
            s.add("blocks", "n%d_eob%d" % (nblocks, t), data, z)
    rng = random.Random(0xB10C)
    s.tokens("blocks", "empty_final", [history(700, 5) + [(20, 600)], []])
    s.tokens("blocks", "empty_in_between", [history(100, 6), [], [], lits9(rng, 7), []])
    data, z = zstream([[]])
    assert len(z) == 8
    s.add("blocks", "only_an_empty_block", data, z)


def _tail_bases():
    bases = []
    for r in range(4):
        rng = random.Random(0x7A11 + r)
        tokens = history(1500, 10 + r) + [(100, 1200), 5, (9, 3)] + lits9(rng, 4)
        for extra in range(5):  # (a literal of eight bits makes the stream one byte longer)
            data, z = zstream([tokens + lits8(rng, extra)])
            if len(z) % 4 == r:
                break
        assert len(z) % 4 == r
        bases.append((data, z))
    return bases


def _tails(s):
    for r, (data, z) in enumerate(_tail_bases()):
        rng = random.Random(0x7A12 + r)
        s.add("tails", "base_mod%d" % r, data, z)
        for cut in range(1, 13):
            s.add("tails", "mod%d_cut%d" % (r, cut), data, z[:-cut], plain=False)
        for more in range(1, 10):
            s.add("tails", "mod%d_plus%d" % (r, more), data, z + bytes(rng.randrange(256) for _ in range(more)))
        for i in range(4):
            bad = bytearray(z)
            bad[len(z) - 4 + i] ^= 1 << rng.randrange(8)
            s.add("tails", "mod%d_trailer%d" % (r, i), data, bytes(bad), plain=False, wrong_trailer=True)


def _capacity(s):
    rng = random.Random(0xCA9)
    bases = [("literals", [lits8(rng, 20) + lits9(rng, 20)], [2, 4, 5, 22]),          # (a step takes three literals: 1, 2, 4, 5 end between two of one step)
             ("matches", [lits8(rng, 10) + [(20, 5)] + lits9(rng, 5) + [(258, 12), 9, 9, (8, 1)]], [9, 11, 12, 29, 30, 31, 36, 135, 292, 294, 296]),
             ("far", [history(1000, 20) + [(100, 900), 1, 2, 3, (258, 1000)]], [1001, 1007, 1008, 1009, 1050, 1099, 1101, 1102, 1110, 1360])]
    for name, blocks, inside in bases:
        data, z = zstream(blocks)
        need = len(data)
        for cap in sorted(set([need, need - 1, 0, 1, 15, 16, 17] + inside)):
            assert cap <= need
            s.add("capacity", "%s_cap%d" % (name, cap), data, z, cap=cap, plain=cap >= need)
        for cap in (need + 1, need + 17):
            s.add("capacity", "%s_cap%d" % (name, cap), data, z, cap=cap)


def _literal_stream(n, seed):
    """n literals of eight bits in one block: a stream of exactly n + 8 bytes, written in one piece."""
    rng = random.Random(seed)
    data = bytes(rng.randrange(144) for _ in range(n))
    codes = bytes(W.FIXED_LIT[b][0] for b in range(144)) + bytes(112)
    w = W.BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    w.put(int.from_bytes(data.translate(codes), "little"), 8 * n)
    w.code(W.FIXED_LIT[256])
    z = bytes([0x78, 0x9c]) + w.bytes() + zlib.adler32(data).to_bytes(4, "big")
    assert len(z) == n + 8 and zlib.decompress(z) == data
    return data, z


def _sizes(s):
    data, z = _literal_stream(MAX_BYTES - 9, 1)
    s.add("sizes", "in_len_max_minus_1", data, z)
    data, z = _literal_stream(MAX_BYTES - 8, 2)
    assert len(z) == MAX_BYTES
    s.add("sizes", "in_len_max", data, z, plain=False)
    for need, name in ((MAX_BYTES - 1, "cap_max_minus_1"), (MAX_BYTES, "cap_max")):
        n, rest = divmod(need - 1, 258)
        data, z = zstream([[77] + [(258, 1)] * n + ([(rest, 1)] if rest >= 3 else [78] * rest)])
        assert len(data) == need
        s.add("sizes", name, data, z, plain=need < MAX_BYTES)


FAMILIES = [("grid", _window_grid), ("handover", _handover), ("overlap", _overlap), ("bitrate", _bitrate), ("blocks", _blocks),
            ("tails", _tails), ("capacity", _capacity), ("sizes", _sizes)]


@functools.lru_cache(maxsize=None)
def _all():
    s = _Set()
    for _name, make in FAMILIES:
        make(s)
    for c in s.cases:
        # (the label is given where a case is built; this is what it has to mean)
        assert c.plain == (_valid(c) and c.cap >= len(c.data) and len(c.stream) < MAX_BYTES and c.cap < MAX_BYTES), c.name
        assert not (c.plain and c.wrong_trailer), c.name
    return tuple(s.cases)


def _valid(c):
    try:
        d = zlib.decompressobj()
        return d.decompress(c.stream) == c.data and d.eof
    except zlib.error:
        return False


def all_cases():
    return list(_all())


def family(name):
    return [c for c in _all() if c.family == name]
