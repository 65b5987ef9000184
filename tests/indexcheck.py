"""Shared by tests/test_model_segments.py (CPU) and tests/test_gpu_indexed.py (GPU): the inputs of the index tests, the host model of
the segment decoder (tests/model/model_seg.cpp), how an index cuts a stream into segments, and the INDEPENDENT check of an access
point -- system zlib only, nothing of the code under test:

    the compressed body as one integer, shifted right by in_bit and packed to bytes again, is a raw stream of its own (an empty block
    goes in front of it, so that its stored blocks find their byte boundaries where the stream has them);
    zlib.decompressobj(-15, zdict=window) over it must yield exactly reference[out_pos:].
"""
import ctypes as C
import os
import random
import subprocess
import zlib

WINDOW = 32768
GUARD = bytes(range(0x40, 0x80))  # 64 bytes that must stay as they are in front of and behind a segment's room
E_TRUNCATED, E_OUT_TOO_SMALL, E_SEGMENT = 1, 14, 21
BLOCK_LEVEL = (1, 5, 6, 7, 8, 9, 11, 12, 13)  # what a decoder that reads on past its segment may meet instead of PZG_E_SEGMENT


def _phase_prefix(phase):
    """(bits as an integer, their number): an EMPTY non-final dynamic block of the writer's whose length is `phase` modulo 8."""
    import deflate_writer as W
    for hlit in range(257, 265):  # (written without run lengths, every further code length of 0 costs the header one bit)
        w = W.BitWriter()
        W.write_block(w, W.Block("dynamic"), False, random.Random(0), dict(codes="huffman", rle="plain", hlit=hlit, hdist=1))
        nbits = w.bitpos()
        if nbits % 8 == phase:
            return int.from_bytes(w.bytes(), "little") & ((1 << nbits) - 1), nbits
    raise AssertionError(phase)


def check_point(body, in_bit, out_pos, window, reference, what=None):
    """The bits from in_bit on, behind an empty block that puts them at the bit offset inside a byte they have in the stream (shifted
    to bit 0 they would decode alike but for stored blocks, whose LEN is found by skipping to the next byte boundary OF THE STREAM)."""
    pre, nbits = _phase_prefix(in_bit & 7)
    whole = pre | ((int.from_bytes(body, "little") >> in_bit) << nbits)
    shifted = whole.to_bytes((nbits + 8 * len(body) - in_bit + 7) // 8, "little")
    o = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    got = o.decompress(shifted)
    assert o.eof and got == reference[out_pos:], (what, in_bit, out_pos)


def raw_of(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def tiny_blocks(seed=11, nblocks=400, lo=1, hi=700):
    """(data, raw stream) from the writer: nblocks blocks of lo..hi bytes -- dynamic, fixed and stored -- ending at every bit offset."""
    import deflate_writer as W
    rng = random.Random(0x1D + seed)
    out, blocks = bytearray(), []
    prof = dict(alphabet=list(b"etaoin shrdlu ETAOIN.,;\n") * 3 + list(range(32, 127)), lens=[3, 3, 4, 5, 8, 17, 40, 258], dists="any", p_match=0.35)
    for _ in range(nblocks):
        r = rng.random()
        if r < 0.1:
            b = W.Block("stored")
            b.raw = bytes(rng.getrandbits(8) for _ in range(rng.randint(lo, hi)))
            out.extend(b.raw)
        else:
            b = W.Block("dynamic" if r < 0.75 else "fixed")
            b.tokens = W.gen_tokens(rng, out, rng.randint(lo, hi), prof)
        blocks.append(b)
    w = W.BitWriter()
    for i, b in enumerate(blocks):
        w_opts = dict(codes="huffman", rle="rle")
        W.write_block(w, b, i == len(blocks) - 1, rng, w_opts)
    return bytes(out), w.bytes()


def seam_stream(first):
    """(data, raw stream): a 32768-byte block of literals, then a block that OPENS with the match `first` = (length, distance) --
    with span = 32768 the second segment starts at that match, whose source is the window alone."""
    import deflate_writer as W
    rng = random.Random(0x5EA + first[1])
    out = bytearray()
    a, b = W.Block("dynamic"), W.Block("dynamic")
    prof = dict(alphabet=list(range(256)), lens=[3], dists="any", p_match=0.0)
    a.tokens = W.gen_tokens(rng, out, WINDOW, prof)
    assert len(out) == WINDOW
    ln, d = first
    b.tokens = [first]
    for k in range(ln):
        out.append(out[len(out) - d])
    b.tokens += W.gen_tokens(rng, out, 900, dict(prof, lens=[3, 9, 258], p_match=0.3))
    w = W.BitWriter()
    W.write_block(w, a, False, rng, dict(codes="huffman", rle="rle"))
    W.write_block(w, b, True, rng, dict(codes="huffman", rle="rle"))
    return bytes(out), w.bytes()


def big_inputs():
    """[(name, raw stream, data)]: the six streams of the GPU tests (all under 1 MiB decoded)."""
    import corpus
    text = corpus.zipf_text(300 << 10, 21)
    tiny = tiny_blocks()
    rnd = corpus.random_bytes(256 << 10, 5)
    return [("text6", raw_of(text, 6), text), ("text1", raw_of(text, 1), text), ("fixed", raw_of(text, 6, zlib.Z_FIXED), text),
            ("stored", raw_of(text, 0), text), ("tiny400", tiny[1], tiny[0]), ("random6", raw_of(rnd, 6), rnd)]


def model_inputs():
    """[(name, raw stream, data)]: every stream of rawcheck.stream_pool() that system zlib accepts (cut where it ends), the big inputs
    and a level-9 stream."""
    import corpus
    import rawcheck
    ins = []
    for name, d in rawcheck.stream_pool():
        z = rawcheck.zlib_raw(d)
        if z is not None:
            ins.append((name, d[:z[1]], z[0]))
    ins += big_inputs()
    text = corpus.zipf_text(300 << 10, 21)
    ins.append(("text9", raw_of(text, 9), text))
    return ins


def segments(points, body_len, out_len):
    """The pieces an index cuts a stream into: [(in_off, in_len, start_bit, end_bit, a, b)] -- input bytes in_off .. + in_len, the first
    block's header at bit start_bit of the first of them, the last block ending at bit end_bit counted from that byte's bit 0 (0: the
    final block), producing bytes a .. b of the output."""
    cuts = [(0, 0)] + [tuple(p) for p in points]
    segs = []
    for k, (bit, a) in enumerate(cuts):
        off = bit >> 3
        if k + 1 < len(cuts):
            end = cuts[k + 1][0] - 8 * off
            segs.append((off, (end + 7) >> 3, bit & 7, end, a, cuts[k + 1][1]))
        else:
            segs.append((off, body_len - off, bit & 7, 0, a, out_len))
    return segs


def expected_points(all_ends, span):
    """What the rule records at `span`, from the stream's non-final block ends (the points of a span = 1 build)."""
    got, last = [], 0
    for bit, pos in all_ends:
        if pos - last >= span:
            got.append((bit, pos))
            last = pos
    return got


def error_cases(d, data, pts):
    """[(what, input, start_bit, end_bit, window, capacity, check(status, d0, out_len))] around the segments of one stream."""
    segs = segments(pts, len(d), len(data))
    assert len(segs) >= 4
    off, ln, sb, eb, a, b = segs[1]
    win = data[max(0, a - WINDOW):a]
    loff, lln, lsb, _leb, la, lb = segs[-1]
    lwin = data[max(0, la - WINDOW):la]
    past = lambda st, d0, n: (st == E_SEGMENT and d0 == 2) or st in BLOCK_LEVEL
    return [
        ("one bit more", d[off:], sb, eb + 1, win, b - a, past),
        ("one bit less", d[off:], sb, eb - 1, win, b - a, past),
        ("beyond the final block", d[loff:] + b"\0" * 8, lsb, 8 * lln + 40, lwin, lb - la, lambda st, d0, n: (st, d0, n) == (E_SEGMENT, 1, lb - la)),
        ("cut one byte short", d[off:off + ln - 1], sb, eb, win, b - a, lambda st, d0, n: st == E_TRUNCATED and n <= b - a),
        ("capacity - 1", d[off:off + ln], sb, eb, win, b - a - 1, lambda st, d0, n: (st, n) == (E_OUT_TOO_SMALL, b - a)),
        ("capacity 0", d[off:off + ln], sb, eb, win, 0, lambda st, d0, n: (st, n) == (E_OUT_TOO_SMALL, b - a)),
    ], (a, b, la, lb)


class R(C.Structure):
    _fields_ = [("status", C.c_int32), ("detail0", C.c_uint32), ("detail1", C.c_uint32), ("adler", C.c_uint32),
                ("out_len", C.c_uint64), ("in_used", C.c_uint64)]


class SegModel:
    """The host build of Decoder<15, false, false, true, true>."""

    def __init__(self):
        from conftest import ROOT
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelseg.so")
        srcs = [os.path.join(d, "model_seg.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "inflate_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pzm_seg_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(R)]

    def _run(self, d, start_bit, end_bit, zdict, cap, span, max_points):
        room = C.create_string_buffer(GUARD + b"\xa5" * cap + GUARD, cap + 2 * len(GUARD))
        pts = (C.c_uint64 * (2 * max_points + 2))(*([0xDEADBEEF] * (2 * max_points + 2)))
        r, n = R(), C.c_uint32(0)
        assert self.M.pzm_seg_decompress(d, len(d), start_bit, end_bit, zdict, len(zdict), C.addressof(room) + len(GUARD), cap, span, pts, max_points,
                                         C.byref(n), C.byref(r)) == 0
        raw = room.raw
        assert raw[:len(GUARD)] == GUARD and raw[len(GUARD) + cap:] == GUARD, ("written outside the capacity", cap, r.status, r.out_len)
        assert list(pts[2 * max_points:]) == [0xDEADBEEF] * 2, "a point stored past max_points"
        stored = min(n.value, max_points)
        return r, raw[len(GUARD):len(GUARD) + min(r.out_len, cap)], n.value, [(pts[2 * k], pts[2 * k + 1]) for k in range(stored)]

    def build(self, d, cap, span, max_points=4096):
        """(result, bytes, npoints, the points stored) of one index build over the raw stream d."""
        return self._run(d, 0, 0, b"", cap, span, max_points)

    def segment(self, d, start_bit, end_bit, zdict, cap):
        """(result, bytes) of one segment."""
        r, out, _n, _p = self._run(d, start_bit, end_bit, zdict, cap, 0, 0)
        return r, out
