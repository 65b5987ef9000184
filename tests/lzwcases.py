"""LZW test material, shared by the CPU model test, the sanitized program's test and the GPU tests of pzg_unlzw_many.

decode() is the reference: a classic table decoder written from the rules in include/pzg.h (the comment of pzg_unlzw_many), not from
the kernel's core, which keeps no table.  codes_of() / pack() are a writer with the knobs the tests need: early change on and off, a
Clear after any number of codes or never (the table then stays full), no leading Clear, no EOI, and hand-made code lists for what no
encoder writes.  all_cases() builds every case once and decodes it once with the reference."""
import functools
from dataclasses import dataclass

import numpy as np

OK, E_TRUNCATED, E_LZW = 0, 1, 25
CLEAR, EOI, FIRST = 256, 257, 258


def width_for(f, early_change):
    """The width of the code read while f is the next free entry."""
    for w in (9, 10, 11):
        if f <= (1 << w) - 1 - early_change:
            return w
    return 12


def decode(stream, cap, early_change=1):
    """(status, output bytes, d0, d1) of one stream by the header's rules."""
    stream = bytes(stream)
    total = 8 * len(stream)
    value = int.from_bytes(stream, "big") if stream else 0
    out = bytearray()
    entries = {}
    f, prev, at = FIRST, None, 0
    while True:
        if len(out) >= cap:
            return OK, bytes(out[:cap]), 0, 0
        w = width_for(f, early_change)
        if at + w > total:
            return E_TRUNCATED, bytes(out), 0, 0
        c = (value >> (total - at - w)) & ((1 << w) - 1)
        at += w
        if c == CLEAR:
            entries, f, prev = {}, FIRST, None
            continue
        if c == EOI:
            return OK, bytes(out), 0, 0
        if c < CLEAR:
            s = bytes([c])
        elif FIRST <= c < f:
            s = entries[c]
        elif c == f and prev is not None and f <= 4095:
            s = prev + prev[:1]
        else:
            return E_LZW, bytes(out), c, len(out)
        if prev is not None and f <= 4095:
            entries[f] = prev + s[:1]
            f += 1
        out += s
        prev = s


def codes_of(data, clear_every=None, leading_clear=True, eoi=True):
    """The codes of a greedy encoder.  clear_every: a Clear after that many codes since the last one (None: never -- once the table
    is full nothing is added and coding goes on)."""
    data = bytes(data)
    codes = [CLEAR] if leading_clear else []
    table = {}
    j, i, n = 0, 0, len(data)
    while i < n:
        cur = data[i]
        i += 1
        while i < n and (cur, data[i]) in table:
            cur = table[(cur, data[i])]
            i += 1
        codes.append(cur)
        if i < n and FIRST + j <= 4095:
            table[(cur, data[i])] = FIRST + j
        j += 1
        if clear_every is not None and j >= clear_every and i < n:
            codes.append(CLEAR)
            table = {}
            j = 0
    if eoi:
        codes.append(EOI)
    return codes


def pack(codes, early_change=1):
    """Codes to bytes, most significant bit first, every code at the width the header's rule gives its place."""
    value, bits, j = 0, 0, 0
    for c in codes:
        f = min(FIRST + max(j - 1, 0), 4096)
        w = width_for(f, early_change)
        assert c < (1 << w), (c, w)
        value = (value << w) | c
        bits += w
        j = 0 if c == CLEAR else j + 1
    pad = -bits % 8
    return ((value << pad).to_bytes((bits + pad) // 8, "big")) if bits else b""


def encode(data, early_change=1, clear_every=3837, leading_clear=True, eoi=True):
    return pack(codes_of(data, clear_every, leading_clear, eoi), early_change)


@dataclass
class Case:
    name: str
    stream: bytes
    cap: int
    early_change: int
    status: int = 0
    out: bytes = b""
    d0: int = 0
    d1: int = 0


def _rng(seed):
    return np.random.default_rng(seed)


def text_like(n, seed=3):
    words = [b"strip", b"tile", b"wave", b"lane", b"code", b"clear", b"scan", b" ", b" the ", b"\n", b"0123", b"predictor"]
    r = _rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(len(words)))]
    return bytes(out[:n])


def image_like(n, seed=5):
    r = _rng(seed)
    return (np.cumsum(r.integers(-2, 3, n)) // 2 % 256).astype(np.uint8).tobytes()


def _build():
    cases = []

    def add(name, stream, cap, ec=1):
        cases.append(Case(name, bytes(stream), int(cap), ec))

    rnd = _rng(11).integers(0, 256, 40000, dtype=np.uint8).tobytes()
    # runs: every code is the entry just made, the dependency chain of a step 64 deep, and strings far longer than 64 bytes
    for ec in (1, 0):
        for period in (1, 2, 3, 7):
            data = bytes(range(1, period + 1)) * (6000 // period) if period > 1 else bytes(6000)
            add("period %d ec %d" % (period, ec), encode(data, ec), len(data), ec)
    add("zeros 40000", encode(bytes(40000)), 40000)
    add("zeros no clear at all", encode(bytes(3000), leading_clear=False), 3000)
    # random bytes: the table fills and is cleared, or fills and stays full
    for ec in (1, 0):
        add("random cleared ec %d" % ec, encode(rnd, ec), len(rnd), ec)
        add("random table stays full ec %d" % ec, encode(rnd[:12000], ec, clear_every=None), 12000, ec)
    add("random cleared when full", encode(rnd[:9000], clear_every=3839), 9000)
    add("random no leading clear no eoi", encode(rnd[:3000], leading_clear=False, eoi=False), 3000)
    add("text", encode(text_like(20000)), 20000)
    add("text table stays full", encode(text_like(30000), clear_every=None), 30000)
    add("image-like", encode(image_like(30000)), 30000)
    add("image-like ec 0", encode(image_like(9000), 0), 9000, 0)
    # the width switches: streams that end a few codes around f = 510/511/512, 1022.., 2046.., and the table's end
    codes = codes_of(rnd[:8000], clear_every=None, eoi=False)
    for ec in (1, 0):
        for around in (254, 766, 1790, 3838):
            for ncodes in range(around - 2, around + 4):
                cs = codes[: 1 + ncodes] + [EOI]
                st = pack(cs, ec)
                add("width switch %d codes ec %d" % (ncodes, ec), st, 8192, ec)
    # a Clear at every lane position of a step
    for every in (64, 65, 95, 126, 127, 128, 1, 2, 63):
        add("clear every %d (text)" % every, encode(text_like(3000, every), clear_every=every), 3000)
        add("clear every %d (zeros)" % every, encode(bytes(2000), clear_every=every), 2000)
    # capacities
    data = text_like(700, 9)
    st = encode(data)
    for cap in (0, 1, len(data) - 1, len(data), len(data) + 1):
        add("text cap %d" % cap, st, cap)
    z = encode(bytes(5000))
    for cap in (0, 1, 63, 64, 65, 2000, 2017, 4999, 5001):
        add("zeros cap %d (a string crosses it)" % cap, z, cap)
    add("garbage behind the capacity", encode(data, eoi=False) + b"\xff\xff\xff\xff\xff", len(data))
    add("garbage behind the capacity, zeros", encode(bytes(1000), eoi=False) + b"\xff\xf0\x0f", 1000)
    # inputs cut at every byte of a short stream
    short = encode(text_like(90, 4) + bytes(40))
    for cut in range(len(short)):
        add("cut at %d" % cut, short[:cut], 256)
    add("empty input", b"", 100)
    add("empty input, no room", b"", 0)
    # what no encoder writes
    add("bad first code after a Clear", pack([CLEAR, 65, 66, CLEAR, 300, 67]), 100)
    add("bad first code of the stream", pack([258, 65]), 100)
    add("first entry as the first code", pack([CLEAR, 258]), 100)
    add("f + 1", pack([CLEAR, 65, 66, 260, 67]), 100)
    add("f + 1 ec 0", pack([CLEAR, 65, 66, 260, 67], 0), 100, 0)
    add("f exactly", pack([CLEAR, 65, 66, 259, 67, EOI]), 100)
    add("far beyond", pack([CLEAR] + list(range(70)) + [400] + [1, 2]), 1000)
    add("bad code in lane 63", pack([CLEAR] + [7] * 63 + [500, 1]), 1000)
    add("bad code behind the capacity", pack([CLEAR, 65, 66, 300]), 2)
    add("eoi first", pack([EOI]), 10)
    add("clear only", pack([CLEAR]), 10)
    add("clears only", pack([CLEAR] * 70 + [65, EOI]), 10)
    add("data behind eoi", pack([CLEAR, 65, EOI, 66, 67]), 10)
    add("entries of entries", pack([CLEAR, 65, 258, 259, 260, 258, 66, 263, 264, 262, EOI]), 1000)
    add("an old entry and the one just made", pack([CLEAR] + [1, 2, 3, 4] * 16 + [258, 259, 321, 322, 323, 324, 258, EOI]), 1000)
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _build()
    for c in cases:
        c.status, c.out, c.d0, c.d1 = decode(c.stream, c.cap, c.early_change)
    return tuple(cases)


FILL = 0xCD


def layout(c, i):
    """(mis, out_off, dst_bytes) of case c as test number i places it: every input alignment, output offsets that are not 16-aligned."""
    mis = i % 4
    out_off = (5 * i + 3) % 23
    return mis, out_off, out_off + c.cap + 9


def expected_dst(c, i):
    """The whole destination afterwards: FILL but for the delivered bytes."""
    _, out_off, nbytes = layout(c, i)
    want = np.full(nbytes, FILL, np.uint8)
    want[out_off:out_off + len(c.out)] = np.frombuffer(c.out, np.uint8)
    return want


def batch(cases):
    """One call's arrays: (in_buf, in_off, in_len, out_bytes, out_off, out_cap, want_out, want_len, want_status, want_detail)."""
    in_parts, in_off, in_len, out_off, out_cap = [], [], [], [], []
    ip = op = 0
    want = []
    for i, c in enumerate(cases):
        pad = (i % 4 - ip) % 4
        in_parts.append(bytes(pad))
        ip += pad
        in_off.append(ip)
        in_len.append(len(c.stream))
        in_parts.append(c.stream)
        ip += len(c.stream)
        op += (5 * i + 3) % 23
        out_off.append(op)
        out_cap.append(c.cap)
        want.append((op, c.out))
        op += c.cap + 5
    in_buf = np.frombuffer(b"".join(in_parts) + bytes(4), np.uint8).copy()
    want_out = np.full(op + 16, FILL, np.uint8)
    for at, b in want:
        want_out[at:at + len(b)] = np.frombuffer(b, np.uint8)
    u64 = lambda x: np.array(x, np.uint64)
    return (in_buf, u64(in_off), u64(in_len), op + 16, u64(out_off), u64(out_cap), want_out, u64([len(c.out) for c in cases]),
            np.array([c.status for c in cases], np.int32), np.array([[c.d0, c.d1] for c in cases], np.uint32))


# ---- LZW pages for tests/tiffcases.py's writer ---------------------------------------------------------------------------------------------
def relzw(then=None, **enc):
    """A hook for the writer's pages: the stream it deflated, stored as LZW instead.  then(k, stream): what a test does to it afterwards."""
    import zlib

    def edit(k, z):
        out = encode(zlib.decompress(z), **enc)
        return then(k, out) if then else out
    return edit


def lzw_page(data, then=None, enc=None, **kw):
    """A Page of `data` with Compression 5 for write_tiff (Predictor 1 or 2, any layout the writer has)."""
    import tiffcases as T
    return T.Page(data, compression=5, edit=relzw(then, **(enc or {})), **kw)


def lzw_float_page(data, big_endian, then=None, **kw):
    """The same with Predictor 3 (tests/fpcases.py encodes the rows)."""
    import fpcases as F
    return F.float_page(data, big_endian, then=relzw(then), compression=5, **kw)
