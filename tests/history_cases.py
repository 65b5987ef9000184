"""TEST INFRASTRUCTURE: writer-made streams (tests/deflate_writer.py) on the edges of the HISTORY IN FRONT OF THE OUTPUT of
pure_zlib_amd/csrc/inflate_core.h -- install_dictionary() lays the last min(dict_len, 32768) bytes of a dictionary (or a segment's
window) into the ring in front of output byte 0 and sets hist_extra; the head-token checks of emit_body and seq_solo, the SRC_OUT
predicate of a segment and the BAD predicate of a group compare a distance with op + hist_extra; MIX (32 KiB ring only) is live
from output byte 0 once the history is full.  A compressor never writes a match that reaches the oldest byte of the history from
output byte 0, a distance one too large, or a match on the MIX threshold; these streams do.

The writer's bytearray is seeded with the dictionary, so its tokens reach into the history and its own bytes behind the history
are the expected output, independent of any decoder.  cases() -> [case]; a case is a dict:
    name    what it is
    zdict   the history bytes (the whole dictionary: above 32768 bytes only its tail is history, the DICTID covers all of it)
    raw     the DEFLATE body (one final block)
    data    the writer's bytes behind the history, or the prefix delivered before the planned failure
    expect  ("ok",) or ("bad_distance", distance, op)
and beside these: nbits (the body's length in bits), tokens and bits (every token and the bit it starts at), where (of a failing
token: "first" | "first64" | "behind600" | None), path (the path the case is named for: "head" | "segment" | "group" | "mix" |
None), nodict (what the same body gives with an EMPTY history: ("ok", data) or ("bad_distance", distance, op, prefix)).
zlib_wrap / plain_wrap / seg_wrap put the containers around a body; self_check() holds the list against system zlib."""
import random
import struct
import zlib

import deflate_writer as W

RING = 32768
SEQ_GLIM = 768  # inflate_core.h: `#define PZG_SEQ_GLIM 768` -- output bytes of a group at the most; MIX is m - dist < SEQ_GLIM - RING
MIX_EDGE = SEQ_GLIM - RING  # = -32000: a match at m (from the group's start) with m - dist BELOW this value is MIX
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 258, 259, 32767, 32768, 32769, 40000)  # dict_adler steps by 64; the ring holds 32768
KS = (0, 1, 2, 15, 16, 17, 127, 128, 129, 600)  # literals in front of the edge match
# With these histories the match behind 600 literals lies more than 32000 bytes in front of its group's start: it is MIX, the group
# ends in front of it and seq_solo decodes it -- the one way a VALID match at the oldest byte of the history (dist == op +
# hist_extra) meets seq_solo's own comparison.  k = 600 only.
SOLO_LENGTHS = (32100, 32160)
PRINT = list(range(32, 127))
BYTES = list(range(256))  # eight bits a literal: 600 of them are 600 bytes of body
TEXT = list(b"etaoin shrdlu ETAOIN.,;\n") * 3 + PRINT

_DICTS = {}


def zdict_of(length, kind="random"):
    """One dictionary per length (shared by its cases): random bytes, so that a source one byte off shows in the output."""
    if (length, kind) not in _DICTS:
        _DICTS[length, kind] = b"\xff" * length if kind == "ff" else random.Random(0xD1C7 + length).randbytes(length)
    return _DICTS[length, kind]


class _Marked(list):
    """tokens that note the writer's bit position as each is written (write_block's last pass over them is the one that writes)"""

    def __init__(self, tokens, w):
        super().__init__(tokens)
        self.w, self.bits = w, [0] * len(tokens)

    def __iter__(self):
        for i, t in enumerate(list.__iter__(self)):
            self.bits[i] = self.w.bitpos()
            yield t


def deflate(tokens, kind="dynamic", seed=1):
    """(body, its length in bits, the bit at which each token starts): one final block"""
    w, blk = W.BitWriter(), W.Block(kind)
    blk.tokens = _Marked(tokens, w)
    W.write_block(w, blk, True, random.Random(seed), {"hlit": None, "hdist": None})
    nbits = w.bitpos()
    return w.bytes(), nbits, blk.tokens.bits


class Hist:
    """tokens and the bytes they produce behind a history, side by side"""

    def __init__(self, zdict, seed):
        self.zdict, self.base, self.rng = zdict, len(zdict), random.Random(seed)
        self.out, self.t = bytearray(zdict), []
        self.fail = None    # (distance, op, token index, the bytes before it) of the planned failure
        self.reach = None   # the same for the first token that an EMPTY history fails
        self.path = None

    @property
    def op(self):
        return len(self.out) - self.base

    def lit(self, b):
        self.t.append(b)
        self.out.append(b)

    def lits(self, n, alphabet=PRINT):
        for _ in range(n):
            self.lit(self.rng.choice(alphabet))

    def _note_reach(self, dist):
        if self.reach is None and dist > self.op:
            self.reach = (dist, self.op, len(self.t), bytes(self.out[self.base:]))

    def match(self, ln, dist):
        assert 3 <= ln <= 258 and 1 <= dist <= min(len(self.out), RING), (ln, dist, len(self.out))
        self._note_reach(dist)
        self.t.append((ln, dist))
        for _ in range(ln):
            self.out.append(self.out[-dist])

    def bad(self, ln, dist):
        """a match one byte or more in front of the history (what follows it in the stream is never decoded)"""
        assert self.fail is None and len(self.out) < dist <= RING, (dist, len(self.out))
        self._note_reach(dist)
        self.fail = (dist, self.op, len(self.t), bytes(self.out[self.base:]))
        self.t.append((ln, dist))
        self.out += bytes(ln)

    def tail(self, n, dists="near", p_match=0.4, lens=(3, 4, 5, 8, 17, 40, 258)):
        at, op = len(self.t), self.op
        self.t += W.gen_tokens(self.rng, self.out, n, dict(alphabet=TEXT, lens=list(lens), dists=dists, p_match=p_match))
        for tk in self.t[at:]:  # (the first of them that reaches in front of output byte 0, for the empty history)
            if not isinstance(tk, int):
                if self.reach is None and tk[1] > op:
                    self.reach = (tk[1], op, at, bytes(self.out[self.base:self.base + op]))
                op += tk[0]
            else:
                op += 1
            at += 1

    def case(self, name, kind="dynamic"):
        raw, nbits, bits = deflate(self.t, kind)
        c = dict(name=name, zdict=self.zdict, raw=raw, nbits=nbits, tokens=list(self.t), bits=bits, path=self.path, where=None)
        if self.fail:
            dist, op, at, before = self.fail
            c.update(data=before, expect=("bad_distance", dist, op))
            c["where"] = "first" if at == 0 else "first64" if at < 64 else "behind600" if bits[at] >= 8 * 600 else None
        else:
            c.update(data=bytes(self.out[self.base:]), expect=("ok",))
        c["nodict"] = ("bad_distance", self.reach[0], self.reach[1], self.reach[3]) if self.reach else ("ok", c["data"])
        return c


# ---- the containers ---------------------------------------------------------------------------------------------------

FDICT_HDR = b"\x78\xbb"  # CMF 78, FLG bb: FDICT (bit 5) set, 0x78bb % 31 == 0


def zlib_wrap(c, dictid=None):
    """RFC 1950 with FDICT: header, DICTID (the Adler-32 of the WHOLE dictionary) big-endian, body, Adler-32 of the data alone"""
    return FDICT_HDR + struct.pack(">I", zlib.adler32(c["zdict"]) if dictid is None else dictid) + c["raw"] + struct.pack(">I", zlib.adler32(c["data"]))


def plain_wrap(c):
    """the same body WITHOUT FDICT: a decoder that is handed a dictionary for it must ignore it"""
    return b"\x78\x9c" + c["raw"] + struct.pack(">I", zlib.adler32(c["nodict"][-1]))


_PREFIX = {}


def _prefix(window, start_bit):
    """(bits as an integer, their number P with P % 8 == start_bit): a non-final block whose output is `window` -- a stored block
    (it ends on a byte boundary: start bit 0), or a fixed block of literals behind an empty block that puts its end at start_bit."""
    key = (window, start_bit)
    if key not in _PREFIX:
        import indexcheck
        w = W.BitWriter()
        if start_bit == 0:
            b = W.Block("stored")
            b.raw = window
        else:
            b = W.Block("fixed")
            b.tokens = list(window)
            pre, nbits = indexcheck._phase_prefix((start_bit - 10 - sum(W.FIXED_LIT[x][1] for x in window)) % 8)
            w.put(pre, nbits)
        W.write_block(w, b, False, None, {})
        p = w.bitpos()
        assert p % 8 == start_bit
        _PREFIX[key] = (int.from_bytes(w.bytes(), "little") & ((1 << p) - 1), p)
    return _PREFIX[key]


def seg_wrap(c, start_bit):
    """The body as a SEGMENT (pzg_decompress_many_segments): behind a block that produces the window, from the byte that holds that
    block's end bit.  -> dict(inp, start_bit, end_bit (exact: 0 means "the final block" as well), window, whole (the stream from its
    first block on: system zlib decodes it to window + data), in_used)"""
    window = c["zdict"][-RING:]
    pre, p = _prefix(window, start_bit)
    total = p + c["nbits"]
    whole = (pre | (int.from_bytes(c["raw"], "little") << p)).to_bytes((total + 7) // 8, "little")
    inp = whole[p >> 3:]
    return dict(inp=inp, start_bit=start_bit, end_bit=start_bit + c["nbits"], window=window, whole=whole, in_used=len(inp))


def truncated(c):
    """(the body cut at 2/3 of its bytes, the bytes of the tokens that lie inside the cut whole): PZG_E_TRUNCATED delivers these"""
    cut = len(c["raw"]) * 2 // 3
    out = bytearray(c["zdict"])
    for k, tk in enumerate(c["tokens"]):
        end = c["bits"][k + 1] if k + 1 < len(c["tokens"]) else c["nbits"] - 1
        if end > 8 * cut:
            break
        if isinstance(tk, int):
            out.append(tk)
        else:
            for _ in range(tk[0]):
                out.append(out[-tk[1]])
    return c["raw"][:cut], bytes(out[len(c["zdict"]):])


def truncated_segment(c, s):
    """(the segment s = seg_wrap(c, ...) with the last third of its input cut off, the bytes of the tokens that lie inside the cut
    whole): in the segment's input token k starts at bit start_bit + bits[k]"""
    cut = len(s["inp"]) * 2 // 3
    out = bytearray(c["zdict"])
    for k, tk in enumerate(c["tokens"]):
        end = s["start_bit"] + (c["bits"][k + 1] if k + 1 < len(c["tokens"]) else c["nbits"] - 1)
        if end > 8 * cut:
            break
        if isinstance(tk, int):
            out.append(tk)
        else:
            for _ in range(tk[0]):
                out.append(out[-tk[1]])
    return s["inp"][:cut], bytes(out[len(c["zdict"]):])


# ---- the cases --------------------------------------------------------------------------------------------------------

def _first_match(length, k, bad):
    """k literals, then a match of 3 bytes at the oldest byte of the history (or one in front of it), then ordinary tokens"""
    use = min(length, RING)
    dist = k + use + (1 if bad else 0)
    if dist > RING:
        return None
    # (the valid stream and its failing twin: the same literals.  Where the strips end a span is their business -- a lane whose
    # guessed start never meets the chain of tokens cuts it --, and with the first seed's literals the span of L = 64, k = 600 ends
    # in front of the match: those two streams draw other literals.  tests/test_model_history.py holds every k = 600 stream to
    # its group by the model's counters.)
    h = Hist(zdict_of(length), 1000 * length + 2 * k + (500 if (length, k) == (64, 600) else 0))
    h.lits(k, BYTES if k >= 127 else PRINT)
    (h.bad if bad else h.match)(3, dist)
    # (behind 600 bytes of body the block goes on long enough for a span of strips; elsewhere a short tail)
    h.tail(2500 if k == 600 else 150)
    h.path = ("head" if k == 0 else "segment" if k <= 17 else "solo" if length in SOLO_LENGTHS else "group" if k == 600 else None)
    return h.case("first_L%d_k%d_%s" % (length, k, "bad" if bad else "ok"))


def _join(length):
    """matches whose source starts in the history and runs into the output they produce (dist < len over the join), and sources
    that end exactly at the join (dist == len) or one byte in front of it (dist == len + 1), all at output byte 0"""
    out = []
    for ln, dist in ((258, 1), (258, 2), (258, 3), (258, 16), (10, 4), (3, 3), (16, 16), (258, 258), (3, 4), (16, 17), (257, 258)):
        if dist > min(length, RING):
            continue
        h = Hist(zdict_of(length), 77 * length + 300 * ln + dist)
        h.match(ln, dist)
        h.tail(120)
        h.path = "head"
        out.append(h.case("join_L%d_len%d_dist%d" % (length, ln, dist)))
    return out


def _full_window(length):
    """a full 32 KiB history: source and destination at the same ring positions, and next to that, at the first bytes of output"""
    out = []
    for at in (0, 1, 257, 258):
        for ln, dist in ((258, RING), (258, RING - 1), (3, RING)):
            if (ln, dist) == (258, RING) and at:
                continue
            h = Hist(zdict_of(length), 31 * length + 1000 * at + ln + dist)
            h.lits(at)
            h.match(ln, dist)
            h.tail(200, dists="max")
            h.path = "head" if at == 0 else None
            out.append(h.case("full_L%d_op%d_len%d_dist%d" % (length, at, ln, dist)))
    return out


MIX_MS = (0, 1, 255, 500, 764, 765)  # (m + 3 <= SEQ_GLIM: the match still fits the group that starts behind the anchor)


def _mix(length, m, delta):
    """Behind 700 bytes of body (the strips and groups engage): a match at distance 32768, which is MIX wherever its group starts
    (m < SEQ_GLIM always) and so is decoded on its own -- the next group starts right behind it; then m literals and a match with
    m - dist = MIX_EDGE + delta: -1 is MIX, 0 and +1 are not.  The three streams of one m differ in the extra bits of that one
    distance only.  Then literals up to the group's limit, whose last bytes lie where the ring holds that match's source."""
    h = Hist(zdict_of(length), 5000 + m)
    h.lits(700, BYTES)
    h.match(3, RING)
    h.lits(m, BYTES)
    dist = m - (MIX_EDGE + delta)
    h.match(3, dist)
    h.lits(SEQ_GLIM + 40 - m, BYTES)
    h.tail(2000)
    h.path = "mix"
    return h.case("mix_L%d_m%d_%s" % (length, m, {-1: "below", 0: "at", 1: "above"}[delta]))


def _evicted():
    """70,000 bytes behind a full history: early matches at the far end of a history the ring is overwriting, late ones in output"""
    h = Hist(zdict_of(RING), 4242)
    h.tail(35000, dists="max", p_match=0.3, lens=(3, 4, 5, 6, 33, 64, 258))
    h.tail(35000, dists="far", p_match=0.3)
    return h.case("evicted_L32768")


_CASES = None
CONTRACT = ("first_L65_k16_ok", "first_L32768_k0_ok", "join_L258_len258_dist16", "full_L40000_op257_len258_dist32767", "mix_L32768_m255_at",
            "evicted_L32768", "ff_L40000")


def cases():
    global _CASES
    if _CASES is None:
        out = []
        for length in LENGTHS:
            for k in KS:
                for bad in (0, 1):
                    c = _first_match(length, k, bad)
                    if c:
                        out.append(c)
        for length in SOLO_LENGTHS:
            out += [_first_match(length, 600, bad) for bad in (0, 1)]
        for length in (1, 2, 3, 16, 17, 258, 259, 32768, 40000):
            out += _join(length)
        for length in (RING, 40000):
            out += _full_window(length)
            for m in MIX_MS:  # (m + 32001 <= 32768: every distance can be written)
                out += [_mix(length, m, d) for d in (-1, 0, 1)]
        out.append(_evicted())
        h = Hist(zdict_of(40000, "ff"), 9)  # 40000 x 0xff: the largest sums dict_adler meets
        h.match(258, RING)
        h.tail(300)
        out.append(h.case("ff_L40000"))
        assert len({c["name"] for c in out}) == len(out) and set(CONTRACT) <= {c["name"] for c in out}
        _CASES = out
    return _CASES


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def self_check():
    """The list against system zlib and against what it claims to hold: every ("ok",) case decodes to exactly `data` in the zlib and
    in the raw form, and as a segment's stream (window + data); every ("bad_distance", ...) case is rejected; a body cut at 2/3
    gives zlib the planned prefix; the failing tokens sit at the first token, inside the first 64 tokens and behind 600 bytes of
    body; every history length, every k, the MIX numbers and the sizes are there."""
    cs = cases()
    for c in cs:
        z, zd = zlib_wrap(c), c["zdict"]
        assert z[1] & 0x20 and (z[0] * 256 + z[1]) % 31 == 0
        if c["expect"] == ("ok",):
            o = zlib.decompressobj(15, zdict=zd)
            assert o.decompress(z) == c["data"] and o.eof and not o.unused_data, c["name"]
            o = zlib.decompressobj(-15, zdict=zd)
            assert o.decompress(c["raw"]) == c["data"] and o.eof and not o.unused_data, c["name"]
        else:
            kind, dist, op = c["expect"]
            assert kind == "bad_distance" and dist == op + min(len(zd), RING) + 1 and len(c["data"]) == op, c["name"]
            for wbits, s in ((15, z), (-15, c["raw"])):
                o = zlib.decompressobj(wbits, zdict=zd)
                try:
                    o.decompress(s)
                    raise AssertionError((c["name"], "system zlib accepts it"))
                except zlib.error as e:
                    assert "distance too far back" in str(e), (c["name"], str(e))
        assert len(c["data"]) < 110000 and (c["nbits"] + 7) // 8 == len(c["raw"]), c["name"]
        # the empty history: zlib itself says whether the body needs one
        o = zlib.decompressobj(-15)
        try:
            got = o.decompress(c["raw"])
            assert c["nodict"] == ("ok", got) and o.eof, c["name"]
        except zlib.error:
            assert c["nodict"][0] == "bad_distance" and c["nodict"][1] > c["nodict"][2] == len(c["nodict"][3]), c["name"]
    for k, c in enumerate(cs):  # as segments: all eight start bits over the list, every one of the big windows once at bit 0
        s = seg_wrap(c, k % 8)
        o = zlib.decompressobj(-15)
        if c["expect"] == ("ok",):
            assert o.decompress(s["whole"]) == s["window"] + c["data"] and o.eof, c["name"]
            assert s["in_used"] == (s["end_bit"] + 7) // 8 and s["end_bit"] - c["nbits"] == s["start_bit"] == k % 8, c["name"]
    some = 0
    for name in CONTRACT:
        c = by_name(name)
        cut, prefix = truncated(c)
        o = zlib.decompressobj(-15, zdict=c["zdict"])
        assert o.decompress(cut) == prefix and not o.eof and len(prefix) < len(c["data"]), name
        some += len(prefix) > 0  # (a short body is cut inside its block header: nothing is delivered)
        s = seg_wrap(c, 5)
        scut, sprefix = truncated_segment(c, s)
        o = zlib.decompressobj(-15)
        assert o.decompress(s["whole"][: len(s["whole"]) - (len(s["inp"]) - len(scut))]) == s["window"] + sprefix and not o.eof, name
    assert some >= 4
    bad = [c for c in cs if c["expect"] != ("ok",)]
    assert {c["where"] for c in bad} >= {"first", "first64", "behind600"}
    assert {c["path"] for c in bad} >= {"head", "segment", "group"} and {c["path"] for c in cs if c["expect"] == ("ok",)} >= {"head", "segment", "group", "mix", "solo"}
    for length in LENGTHS:
        ks_ok = {c["name"] for c in cs if c["name"].startswith("first_L%d_" % length) and c["name"].endswith("_ok")}
        assert len(ks_ok) == sum(1 for k in KS if k + min(length, RING) <= RING), length
        if length < RING:
            assert "first_L%d_k0_bad" % length in {c["name"] for c in cs}
    mix = [c for c in cs if c["path"] == "mix"]
    assert len(mix) >= 2 * 3 * 4 and all(c["bits"][701] >= 8 * 600 for c in mix)
    for c in mix:  # the numbers themselves: token 700 is the anchor, m literals, then the match on the threshold
        m = int(c["name"].split("_m")[1].split("_")[0])
        ln, dist = c["tokens"][701 + m]
        assert c["tokens"][700] == (3, RING) and m - dist - MIX_EDGE == {"below": -1, "at": 0, "above": 1}[c["name"].rsplit("_", 1)[1]], c["name"]
    assert len(by_name("evicted_L32768")["data"]) >= 70000
    return len(cs)
