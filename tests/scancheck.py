"""Shared by tests/test_model_scan.py (CPU) and tests/test_gpu_scan.py (GPU): the parallel index scan (pzg_index_scan) restated.

  * is_candidate(body, p): the finder's predicate in plain Python, written from its specification (include/pzg.h), nothing of the
    code under test; all_candidates / first_candidate over it (numpy only narrows down where the plain predicate is asked);
  * reference windows: a point's window is the 32 KiB of system zlib's output in front of it, and indexcheck.check_point decodes
    from the point with that window -- the marker pass and the chain walk are checked against those, not against themselves;
  * ScanModel: tests/model/model_scan.cpp, the three passes of pure_zlib_amd/csrc/scan_core.h as a host program between guards;
  * false_candidate_stream(): a stored block whose payload begins, at a chunk boundary, with a real dynamic block.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

WINDOW = 32768
NONE = (1 << 64) - 1
NEXT_FINAL, NEXT_FAIL = 0xffffffff, 0x80000000
E_SCAN, E_TRUNCATED = 22, 1
BLOCK_STATUS = (1, 5, 6, 7, 9, 12, 13)  # what d0 of PZG_E_SCAN may be besides 0 (a dead wave)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _bits(body, p, n):
    """n <= 24 bits from bit p of the body, zeros past its end."""
    i = p >> 3
    return (int.from_bytes(body[i:i + 4], "little") >> (p & 7)) & ((1 << n) - 1)


def _kraft(lengths):
    """The Kraft sum of the nonzero lengths in units of 2^-15."""
    return sum(1 << (15 - l) for l in lengths if l)


def is_candidate(body, p):
    """Does a non-final dynamic block's header that passes every check of the specification start at bit p?"""
    end = 8 * len(body)
    if _bits(body, p, 3) != 4:  # BFINAL = 0, BTYPE = 2
        return False
    hlit, hdist, hclen = _bits(body, p + 3, 5), _bits(body, p + 8, 5), _bits(body, p + 13, 4) + 4
    if hlit > 29 or hdist > 29:
        return False
    q = p + 17
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = _bits(body, q, 3)
        q += 3
    if _kraft(cl) != 1 << 15:
        return False
    code, codes = 0, {}
    for l in range(1, 8):  # canonical codes, first bit first
        for s in range(19):
            if cl[s] == l:
                codes[l, code] = s
                code += 1
        code <<= 1
    total = hlit + 257 + hdist + 1
    lens = []
    while len(lens) < total:
        c, l = 0, 0
        while True:
            c = (c << 1) | _bits(body, q, 1)
            q += 1
            l += 1
            if (l, c) in codes:
                s = codes[l, c]
                break
            assert l < 7  # (a complete code: some code matches)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                return False
            rep, v = 3 + _bits(body, q, 2), lens[-1]
            q += 2
        elif s == 17:
            rep, v = 3 + _bits(body, q, 3), 0
            q += 3
        else:
            rep, v = 11 + _bits(body, q, 7), 0
            q += 7
        if len(lens) + rep > total:
            return False
        lens += [v] * rep
    if q > end:
        return False
    lit, dist = lens[:hlit + 257], lens[hlit + 257:]
    if lit[256] == 0 or _kraft(lit) != 1 << 15:
        return False
    nd = [l for l in dist if l]
    return _kraft(dist) == 1 << 15 or nd == [1] or nd == []


_CACHE = {}


def all_candidates(body):
    """Every candidate position of the body, ascending.  numpy applies the first three rules (BFINAL/BTYPE, HLIT/HDIST and the
    code-length code's Kraft sum) to all positions at once; is_candidate() decides about what is left."""
    key = (len(body), zlib.crc32(body))
    if key not in _CACHE:
        b = np.unpackbits(np.frombuffer(body, dtype=np.uint8), bitorder="little").astype(np.int64)
        n = len(b)
        b = np.concatenate([b, np.zeros(96, dtype=np.int64)])
        f = lambda off, w: sum(b[off + i:off + i + n] << i for i in range(w))
        ok = (f(0, 3) == 4) & (f(3, 5) <= 29) & (f(8, 5) <= 29)
        hclen = f(13, 4) + 4
        ks = np.zeros(n, dtype=np.int64)
        for i in range(19):
            l = f(17 + 3 * i, 3)
            ks += np.where((i < hclen) & (l > 0), 128 >> l, 0)
        ok &= ks == 128
        _CACHE[key] = [int(p) for p in np.nonzero(ok)[0] if is_candidate(body, int(p))]
    return _CACHE[key]


def first_candidate(body, from_bit, to_bit):
    """The smallest candidate position in [from_bit, to_bit), or None."""
    import bisect
    c = all_candidates(body)
    i = bisect.bisect_left(c, from_bit)
    return c[i] if i < len(c) and c[i] < to_bit else None


def expected_candidates(body, chunk):
    n = max(1, -(-len(body) // chunk))
    return [0] + [first_candidate(body, 8 * k * chunk, min(8 * (k + 1) * chunk, 8 * len(body))) for k in range(1, n)]


def false_candidate_stream(chunk=1024):
    """(raw stream, data, bit): stored blocks pad up to a chunk boundary, where the payload of a further stored block begins with the
    bytes of a real non-final dynamic block (a sync-flushed deflate of a small text); a final dynamic block ends the stream.  `bit`
    is that boundary: a candidate that is no block start."""
    import corpus
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    inner = co.compress(corpus.zipf_text(3000, 77)) + co.flush(zlib.Z_SYNC_FLUSH)
    assert inner[0] & 7 == 4
    stored = lambda payload: b"\0" + len(payload).to_bytes(2, "little") + (len(payload) ^ 0xffff).to_bytes(2, "little") + payload
    front = bytearray()
    filler = corpus.zipf_text(2 * chunk, 79)
    front += stored(filler[:chunk - 5 - 37])   # ends at chunk - 37
    front += stored(filler[:37 - 10])          # ends at chunk - 5: the next block's five bytes of header end AT the boundary
    assert len(front) == chunk - 5
    payload = inner + filler[:200]
    body = bytes(front) + stored(payload)
    data = filler[:chunk - 42] + filler[:27] + payload
    co = zlib.compressobj(6, zlib.DEFLATED, -15)  # three more dynamic blocks behind it, each after a full flush, and the final one
    for seed in (80, 81, 82):
        piece = corpus.zipf_text(9000, seed)
        body += co.compress(piece) + co.flush(zlib.Z_FULL_FLUSH)
        data += piece
    piece = corpus.zipf_text(9000, 83)
    body += co.compress(piece) + co.flush()
    data += piece
    assert zlib.decompressobj(-15).decompress(body) == data
    return body, data, 8 * chunk


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("d0", C.c_uint32), ("d1", C.c_uint32), ("npoints", C.c_uint32), ("out_len", C.c_uint64),
                ("in_used", C.c_uint64)]


class ScanModel:
    """The host build of scan_core.h (tests/model/model_scan.cpp)."""

    def __init__(self):
        from conftest import ROOT
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelscan.so")
        self.srcs = [os.path.join(d, "model_scan.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "scan_core.h"),
                     os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, self.srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, self.srcs[0]])
        self.M = C.CDLL(so)
        vp = C.c_void_p
        self.M.pzs_scan.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.POINTER(Result), vp, vp, vp,
                                    vp, vp]
        self.M.pzs_find.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]
        self.M.pzs_find.restype = C.c_uint64

    def find(self, d, from_bit, to_bit, mis=0):
        q = self.M.pzs_find(d, len(d), mis, from_bit, to_bit)
        return None if q == NONE else q

    def scan(self, d, chunk, span, max_points=4096, mis=0, rings=False):
        """The whole scan: a dict of the result block, the points and windows stored, and the passes' arrays."""
        n = max(1, -(-len(d) // chunk))
        pts = np.full((max_points + 1, 2), 0xDEADBEEF, dtype=np.uint64)
        win = np.full((max_points + 1, WINDOW), 0x5A, dtype=np.uint8)
        cand, nxt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        count, endbit = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        rg = np.zeros((n, WINDOW), dtype=np.uint16) if rings else None
        r = Result()
        rc = self.M.pzs_scan(d, len(d), mis, chunk, span, pts.ctypes.data, max_points, win.ctypes.data, C.byref(r), cand.ctypes.data,
                             nxt.ctypes.data, count.ctypes.data, endbit.ctypes.data, rg.ctypes.data if rings else None)
        assert rc == 0, ("written outside a buffer: guard %d" % (rc - 1), chunk, span)
        assert (pts[max_points] == 0xDEADBEEF).all() and (win[max_points] == 0x5A).all(), "a point stored past max_points"
        stored = min(r.npoints, max_points)
        return dict(status=r.status, d0=r.d0, d1=r.d1, npoints=r.npoints, out_len=r.out_len, in_used=r.in_used,
                    points=[(int(a), int(b)) for a, b in pts[:stored]], windows=win[:stored].copy(), cand=[None if c == NONE else int(c) for c in cand],
                    next=[int(x) for x in nxt], count=[int(x) for x in count], endbit=[int(x) for x in endbit], rings=rg)


def chain(res):
    """[(k, start bit, out_pos at its start)] of the segments on the true chain of a scan that succeeded, in order."""
    k, pos, links = 0, 0, []
    while True:
        links.append((k, res["cand"][k], pos))
        pos += res["count"][k]
        if res["next"][k] == NEXT_FINAL:
            return links
        assert not res["next"][k] & NEXT_FAIL and res["next"][k] > k, (k, res["next"][k])
        k = res["next"][k]


def check_windows(res, data, what=None):
    """Every stored window is system zlib's output in front of its point; what lies in front of a short one was left alone."""
    for (bit, pos), w in zip(res["points"], res["windows"]):
        n = min(pos, WINDOW)
        assert w[WINDOW - n:].tobytes() == data[pos - n:pos], (what, bit, pos)
        assert (w[:WINDOW - n] == 0x5A).all(), (what, bit, pos)
