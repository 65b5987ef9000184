"""Shared by tests/test_model_resume_formats.py (CPU) and tests/test_gpu_resume_formats.py (GPU): the cases of the resumable gzip
and raw decoders (pzg_decoder_create_format), the driver that feeds one decoder piece by piece, and the rule every case is held to.

THE RULE (include/pzg.h, pzg_decoder_create_format): take any input and any way of cutting it into feeds and of sizing the rooms; the
concatenation of the delivered bytes, the terminal state and detail, the last adler and the sum of the in_used of all calls equal what
the batch path (pzg_decompress_many with the same flag) gives over the whole input as one stream with enough capacity.

A case is a dict: name, fmt ("gzip" | "raw"), stream (all its bytes), pieces (the feeds; their concatenation is the stream), final
(the last piece is fed with final_in set; otherwise an EMPTY feed with final_in follows the last piece if the decoder still wants
input), room (bytes of output room per call), zpieces (or None: the same DEFLATE body as a zlib stream, cut at the same body
positions -- oracle.trace of it says how many 32 KiB chunks the reference has published after each feed)."""
import struct
import zlib

import corpus
from conftest import REF_CASES, read_case

GZIP, RAW = 4, 32
FLAG = {"gzip": GZIP, "raw": RAW}
NEED_INPUT, OUT_FULL = 101, 102
# include/pzg.h leaves in_used[] of a FAILED batch stream unspecified, and for an error met inside the blocks it is: the batch
# kernels have read ahead of the token that fails by then (windows, strips), further than a feed may even have reached.  For these
# states the sum of in_used is not compared with the batch path's (include/pzg.h says of the decoders what it says of the batch call:
# unspecified, never more than a call was given -- which Driver.take() asserts for every call); it is compared for every other state,
# failures in headers and trailers included.
READ_AHEAD_ERRORS = (5, 6, 7, 8, 9, 11, 12, 13)
HDR10 = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def member(body, data, hdr=HDR10, crc=None, isize=None):
    return hdr + body + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) & 0xffffffff if isize is None else isize)


def rich_header():
    """FEXTRA + FNAME + FCOMMENT + FHCRC."""
    h = bytearray(b"\x1f\x8b\x08\x1e" + struct.pack("<I", 1234567) + b"\x02\x03")
    h += struct.pack("<H", 9) + b"\x41\x70\x05\x00hello"
    h += b"a file name.txt\x00" + b"a comment, somewhat longer than the name\x00"
    h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xffff)
    return bytes(h)


def cut(stream, positions):
    ps = [0] + sorted(set(p for p in positions if 0 < p < len(stream))) + [len(stream)]
    return [stream[a:b] for a, b in zip(ps, ps[1:])]


def by_step(stream, step):
    return cut(stream, range(step, len(stream), step))


def wrapped_pieces(z, fmt, step, hdr=HDR10):
    """The zlib stream z re-wrapped, cut every `step` bytes of its DEFLATE body; and z itself cut at the same body positions."""
    body, data_len = z[2:-4], None
    cuts = list(range(step, len(body), step))
    if fmt == "gzip":
        data = zlib.decompress(z)
        s = member(body, data, hdr)
        return s, cut(s, [len(hdr) + c for c in cuts]), cut(z, [2 + c for c in cuts])
    return body, cut(body, cuts), cut(z, [2 + c for c in cuts])


def case(name, fmt, stream, pieces, final=False, room=1 << 18, zpieces=None):
    assert b"".join(pieces) == stream
    if zpieces is not None:
        assert len(zpieces) == len(pieces), name
    return dict(name=name, fmt=fmt, stream=stream, pieces=pieces, final=final, room=room, zpieces=zpieces)


def fixture_cases(steps_for):
    """The nine reference fixtures re-wrapped as gzip and as raw; steps_for(len(z)) -> the piece sizes."""
    out = []
    for name in REF_CASES:
        z, _gold = read_case(name)
        for fmt in ("gzip", "raw"):
            for k, step in enumerate(steps_for(len(z))):
                s, pieces, zp = wrapped_pieces(z, fmt, step)
                out.append(case("%s/%s/%d" % (name, fmt, step), fmt, s, pieces, final=bool(k & 1), room=4096 if step in (7, 4096) else 1 << 18, zpieces=zp))
    return out


def three_members(seed=3, sizes=(5000, 3000, 7000)):
    datas = [corpus.mixed_data(n, seed + k) for k, n in enumerate(sizes)]
    bodies = [zlib.compress(d, 6)[2:-4] for d in datas]
    return datas, bodies


def corner_cases():
    """Everything but the fixtures: headers, trailers, member boundaries, garbage, wrong checksums and lengths, truncation, a raw
    stream that ends mid-byte -- with rooms of 4,096 bytes among them (PZG_DEC_OUT_FULL interleaves)."""
    out = []
    data = corpus.zipf_text(9000, 11)
    z = zlib.compress(data, 6)
    body = z[2:-4]
    # a header with every optional field, cut at every byte of it (the header is read as a whole: suspension at its first byte)
    rh = rich_header()
    s = member(body, data, rh)
    for c in range(1, len(rh) + 1):
        out.append(case("header cut %d" % c, "gzip", s, cut(s, [c]), final=bool(c & 1), room=4096 if c % 3 == 0 else 1 << 16,
                        zpieces=[z[:2], z[2:]]))
    out.append(case("header byte by byte", "gzip", s, cut(s, range(1, len(rh) + 3)), final=True))
    # a trailer cut at each of its 8 bytes
    s = member(body, data)
    for c in range(8):
        at = len(s) - 8 + c
        out.append(case("trailer cut %d" % c, "gzip", s, cut(s, [at]), final=bool(c & 1), room=4096 if c & 2 else 1 << 16,
                        zpieces=[z[:-4], z[-4:]]))
    # three members back to back: every split inside the middle member's trailer and the next member's first two bytes
    datas, bodies = three_members()
    ms = [member(b, d, rich_header() if k == 1 else HDR10) for k, (b, d) in enumerate(zip(bodies, datas))]
    s = b"".join(ms)
    t0 = len(ms[0]) + len(ms[1]) - 8
    for c in range(0, 11):
        out.append(case("three members, split %d" % c, "gzip", s, cut(s, [t0 + c]), final=bool(c & 1), room=4096 if c % 3 == 1 else 1 << 16))
    out.append(case("three members, two splits", "gzip", s, cut(s, [t0 + 3, t0 + 9]), room=4096))
    out.append(case("three members by 1000", "gzip", s, by_step(s, 1000), final=True, room=4096))
    # an empty member between two others (no output, op stays where it was)
    e = member(zlib.compress(b"")[2:-4], b"")
    s2 = ms[0] + e + ms[2]
    out.append(case("empty member in the middle", "gzip", s2, by_step(s2, 777)))
    s2 = e + ms[0]
    out.append(case("empty member first", "gzip", s2, by_step(s2, 5), room=4096))
    # trailing garbage after a member, with and without final_in (one byte of it: whether a member follows is not known before the end)
    one = member(body, data)
    for g in (b"\x00", b"\x1f", b"\x1f\x8c tail", b"garbage behind the member" * 3):
        for final in (False, True):
            s = one + g
            out.append(case("garbage %r final=%d" % (g[:4], final), "gzip", s, cut(s, [len(one) - 3, len(one)]), final=final))
            out.append(case("garbage %r final=%d whole" % (g[:4], final), "gzip", s, [s], final=final, room=4096))
    # 1f 8b behind a member and nothing else: a header that never comes
    s = one + b"\x1f\x8b"
    out.append(case("a member that never comes", "gzip", s, cut(s, [len(one)]), final=True))
    s = one + b"\x1f\x8b\x07\x00rest of a bad header"
    out.append(case("a bad second header", "gzip", s, cut(s, [len(one) + 1]), final=False))
    # a wrong CRC in member 1 of 3: reported at the end, as the batch path does
    bad = [ms[0], member(bodies[1], datas[1], crc=zlib.crc32(datas[1]) ^ 0x10000), ms[2]]
    s = b"".join(bad)
    out.append(case("wrong crc in member 1 of 3", "gzip", s, by_step(s, 1500), final=True))
    out.append(case("wrong crc in member 1 of 3, small rooms", "gzip", s, by_step(s, 4000), final=False, room=4096))
    # a wrong ISIZE alone, and together with a wrong CRC
    s = member(body, data, isize=len(data) + 1)
    out.append(case("wrong isize", "gzip", s, by_step(s, 900), final=True, room=4096))
    s = ms[0] + member(bodies[1], datas[1], isize=5) + ms[2]
    out.append(case("wrong isize in member 1 of 3", "gzip", s, by_step(s, 2500), final=False))
    s = member(body, data, crc=12345, isize=len(data) + 1)
    out.append(case("wrong isize and wrong crc", "gzip", s, by_step(s, 900), final=True))
    s = ms[0] + member(bodies[1], datas[1], crc=7, isize=5)
    out.append(case("wrong isize and wrong crc in member 1 of 2", "gzip", s, cut(s, [len(s) - 4]), final=False, room=4096))
    # truncation with final_in inside a header, a block and a trailer
    s = member(body, data, rh)
    for name, n in (("header", 20), ("header fixed part", 7), ("block", len(rh) + len(body) // 2), ("trailer", len(s) - 5), ("no trailer", len(s) - 8)):
        out.append(case("truncated in the " + name, "gzip", s[:n], by_step(s[:n], 1200), final=True, room=4096 if n & 1 else 1 << 16))
        out.append(case("truncated in the %s, end signalled late" % name, "gzip", s[:n], by_step(s[:n], 1200), final=False))
    s = ms[0] + ms[1][:9]
    out.append(case("truncated in the second header", "gzip", s, by_step(s, 3000), final=True))
    for name, n in (("block", len(body) // 2), ("last byte", len(body) - 1), ("nothing", 0)):
        out.append(case("raw truncated: " + name, "raw", body[:n], by_step(body[:n], 1100), final=True, room=4096))
        out.append(case("raw truncated: %s, end signalled late" % name, "raw", body[:n], by_step(body[:n], 1100), final=False))
    # header errors (PZG_E_GZIP_HEADER with the batch path's detail words)
    for name, h in (("magic", b"\x1f\x8c" + HDR10[2:]), ("method", b"\x1f\x8b\x07" + HDR10[3:]), ("flags", b"\x1f\x8b\x08\x20" + HDR10[4:]),
                    ("fhcrc", rh[:-2] + bytes([rh[-2] ^ 1, rh[-1]]))):
        s = h + body + one[-8:]
        out.append(case("bad header: " + name, "gzip", s, cut(s, [1, 3, len(h) - 1, len(h) + 50]), final=False))
    # errors inside the blocks (what the batch path reports, where it reports it)
    for seed in range(6):
        b = bytearray(one)
        b[len(HDR10) + 40 + 300 * seed] ^= 0x24
        out.append(case("flipped bits %d" % seed, "gzip", bytes(b), by_step(bytes(b), 700 + 97 * seed), final=bool(seed & 1), room=4096 if seed & 2 else 1 << 16))
        rb = bytearray(body)
        rb[40 + 300 * seed] ^= 0x24
        out.append(case("raw flipped bits %d" % seed, "raw", bytes(rb), by_step(bytes(rb), 700 + 97 * seed), final=bool(seed & 1), room=4096 if seed & 2 else 1 << 16))
    # a raw stream whose final block ends mid-byte, followed by other bytes: in_used stops at the byte that holds its last bit
    n = 0
    for seed in range(40):
        d = corpus.mixed_data(300 + 131 * seed, seed)
        co = zlib.compressobj(1 + seed % 9, zlib.DEFLATED, -15, 8, zlib.Z_FIXED if seed & 1 else zlib.Z_DEFAULT_STRATEGY)
        b = co.compress(d) + co.flush()
        if n < 6:
            n += 1
            for tail in (b"\xff\xff\xff", b"\x00", b):
                s = b + tail
                out.append(case("raw mid-byte end %d + %d" % (seed, len(tail)), "raw", s, cut(s, [len(b) - 1, len(b)]), final=bool(seed & 1), room=4096))
                out.append(case("raw mid-byte end %d + %d whole" % (seed, len(tail)), "raw", s, [s], final=False))
    # stored blocks and many small blocks through small rooms, both formats
    d = corpus.random_bytes(70000, 5)
    zs = zlib.compress(d, 0)
    for fmt in ("gzip", "raw"):
        s, pieces, zp = wrapped_pieces(zs, fmt, 9000)
        out.append(case("stored/" + fmt, fmt, s, pieces, final=True, room=4096, zpieces=zp))
        zv = corpus.compress_variant(corpus.mixed_data(150000, 9), 9)
        s, pieces, zp = wrapped_pieces(zv, fmt, 5000)
        out.append(case("variant/" + fmt, fmt, s, pieces, final=False, room=4096 if fmt == "raw" else 70000, zpieces=zp))
    return out


class Outcome:
    """What a driven decoder came to."""

    def __init__(self):
        self.data = bytearray()
        self.status = NEED_INPUT
        self.detail = (0, 0)
        self.adler = None
        self.in_used = 0
        self.chunks_after_piece = []  # the cumulative chunk count when each piece had been taken
        self.calls = 0


class Driver:
    """One decoder of a case, stepped one PIECE at a time (so that many of them can share a launch): next_input() is what the next
    call gets, take() is handed that call's results."""

    def __init__(self, c):
        self.c = c
        self.o = Outcome()
        self.tail = b""
        self.k = 0                   # pieces handed out
        self.pending = None          # (data, final) of a call to repeat (out of room)
        self.closing = False
        self.done = False
        self.chunks = 0

    def next_input(self):
        """(bytes, final_in) of the next call, or None when the decoder is finished."""
        if self.done:
            return None
        if self.pending is not None:
            return self.pending
        pieces = self.c["pieces"]
        if self.k < len(pieces):
            data = self.tail + pieces[self.k]
            self.k += 1
            fin = 1 if (self.c["final"] and self.k == len(pieces)) else 0
        else:  # every piece is in and the decoder still wants input: the end is signalled with an empty feed
            data, fin = self.tail, 1
            self.closing = True
        self.pending = (data, fin)
        return self.pending

    def take(self, status, detail, adler, out_len, in_used, chunks, delivered):
        data, fin = self.pending
        o = self.o
        o.calls += 1
        assert len(delivered) == out_len and out_len <= self.c["room"] and in_used <= len(data), (self.c["name"], status, out_len, in_used)
        assert chunks >= self.chunks
        self.chunks = chunks
        o.data += delivered
        o.in_used += in_used
        o.adler = adler
        if status == OUT_FULL:
            assert o.calls < 100000
            self.pending = (data[in_used:], fin)
            return
        self.pending = None
        self.tail = data[in_used:]
        o.status, o.detail = status, tuple(detail)
        if not self.closing:
            o.chunks_after_piece.append(chunks)
        if status != NEED_INPUT:
            self.done = True
        else:
            assert not fin, (self.c["name"], "wants input after final_in")


def expected_chunks(O, c, n_taken):
    """The cumulative count of published 32 KiB chunks after each of the first n_taken pieces, from the oracle's event trace of the
    same body as a zlib stream (the publication rule does not depend on the wrapper)."""
    events, _r, _o = O.trace(c["zpieces"])
    counts, chunks, need = [], 0, 0
    for e in events:
        if e[0] == "Chunk":
            chunks += 1
        elif e[0] == "NeedMore":
            need += 1
            if need >= 2:
                counts.append(chunks)
        elif e[0] == "Done":
            counts.append(chunks - 1)  # (the last Chunk is the rest, handed over by finalize)
        else:
            counts.append(chunks)
    return counts[:n_taken]


def check_rule(O, c, o, batch):
    """o: the Outcome of the driven decoder; batch = (status, d0, d1, adler, in_used, bytes): the batch path over the whole stream."""
    what = c["name"]
    st, d0, d1, adler, in_used, data = batch
    assert o.status == st, (what, o.status, st)
    assert bytes(o.data) == data, (what, len(o.data), len(data))
    assert o.detail == (d0, d1), (what, st, o.detail, (d0, d1))
    assert o.adler == adler, (what, st, hex(o.adler), hex(adler))
    if st not in READ_AHEAD_ERRORS:
        assert o.in_used == in_used, (what, st, o.in_used, in_used)
    if c["zpieces"] is not None:
        want = expected_chunks(O, c, len(o.chunks_after_piece))
        # (a gzip decoder may end a feed later than the zlib one: behind a trailer it waits for two bytes or the end of the input)
        assert o.chunks_after_piece[:len(want)] == want, (what, o.chunks_after_piece, want)
        assert all(x == want[-1] for x in o.chunks_after_piece[len(want):]), (what, o.chunks_after_piece, want)


def check_independent(O, c, o):
    """Sources that share no code with the kernels: system zlib for what it accepts, the oracle's gzip reader for one member."""
    s = c["stream"]
    d = zlib.decompressobj(31 if c["fmt"] == "gzip" else -15)
    try:
        data = d.decompress(s)
        while c["fmt"] == "gzip" and d.eof and d.unused_data[:2] == b"\x1f\x8b":  # the members that follow
            rest = d.unused_data
            d = zlib.decompressobj(31)
            data += d.decompress(rest)
        ok = d.eof
    except zlib.error:
        ok = False
    if ok:
        assert o.status == 0 and bytes(o.data) == data and o.in_used == len(s) - len(d.unused_data), (c["name"], o.status, o.in_used)
        assert o.adler == (zlib.crc32(data) if c["fmt"] == "gzip" else zlib.adler32(data)), c["name"]
    elif c["fmt"] == "gzip":
        assert o.status != 0, c["name"]
        r, oo = O.gzip_decompress(s, 1 << 21)
        if r.status != 0:  # (the oracle reads a series of members too; a stream it rejects, it rejects as the decoder does)
            assert o.status == r.status and bytes(o.data) == oo, (c["name"], o.status, r.status)
    else:
        assert o.status != 0, c["name"]
