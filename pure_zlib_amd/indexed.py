"""EXTENSION: ONE large DEFLATE stream, indexed -- decoded by a wavefront per segment, or read at any offset.

A stream is one wavefront's work (pure_zlib_amd.zlib.decompress).  An Index of access points (include/pzg.h, pzg_index_build: a
block boundary about every `span` output bytes -- its bit position, its output position, the 32 KiB of output in front of it) cuts
it into segments that decode independently (pzg_decompress_many_segments):

    index, result = Index.build(data, kind="zlib")     # one sequential pass; result is decompress(data)'s Either
    index, result = Index.build_parallel(data)         # the same, the points found in parallel (pzg_index_scan) and verified
    index.save("big.z.pzi"); index = Index.load("big.z.pzi")
    index.decompress(data)                             # every segment in one launch, the trailer's checksum verified
    index.read(data, offset, length)                   # only the segments that cover the range

kind: "zlib" (RFC 1950: the 2-byte header, Adler-32 trailer), "gzip" (RFC 1952: ONE member; CRC-32 and ISIZE trailer) or "raw"
(RFC 1951: no trailer -- the Adler-32 the build pass saw stands in for it).  The wrapper is parsed here, on the host; the DEFLATE
body is decoded on the device and nowhere else.
"""
import ctypes as C
import zlib as _syszlib  # (crc32 of 128 KiB of the COMPRESSED file, to pair an index with its file: nothing is inflated on the CPU)
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from .zlib import (ChecksumError, Context, DecompressionError, DecompressionError_, Either, HeaderError, Left, Right, default_context,
                   error_from_status)

WINDOW = 32768
ADLER_MOD = 65521
KINDS = ("zlib", "gzip", "raw")


# ---- checksums of a concatenation from the checksums of its parts -------------------------------------------------------------

def adler32_combine(a1: int, a2: int, len2: int) -> int:
    """Adler-32 of A + B from adler32(A), adler32(B) and len(B)."""
    rem = len2 % ADLER_MOD
    s1, s2 = a1 & 0xffff, (a1 >> 16) & 0xffff
    b1, b2 = a2 & 0xffff, (a2 >> 16) & 0xffff
    # B's sums started from 1: its bytes see s1 instead -- (s1 - 1) more in the low sum, len2 times that in the high sum
    lo = (s1 + b1 - 1) % ADLER_MOD
    hi = (s2 + b2 + rem * (s1 - 1)) % ADLER_MOD
    return (hi << 16) | lo


def _gf2_times(mat, vec):
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1
        i += 1
    return s


def _gf2_square(mat):
    return [_gf2_times(mat, mat[n]) for n in range(32)]


def _crc_zero_operators():
    """Entry k: the operator of 2^k zero BYTES (k < 64: every length a uint64 holds)."""
    bit = [0xedb88320] + [1 << n for n in range(31)]  # one zero bit
    ops = [_gf2_square(_gf2_square(_gf2_square(bit)))]
    while len(ops) < 64:
        ops.append(_gf2_square(ops[-1]))
    return tuple(ops)


_CRC_ZEROS = _crc_zero_operators()  # made once, at import, and never changed: a combine is one product per set bit of the length


def crc32_combine(c1: int, c2: int, len2: int) -> int:
    """CRC-32 (RFC 1952) of A + B from crc32(A), crc32(B) and len(B): crc32(A) advanced over len(B) zero bytes -- the operator for
    one zero bit as a 32 x 32 matrix over GF(2), squared once per bit of the length -- plus crc32(B)."""
    if len2 <= 0:
        return c1
    k = 0
    while len2:
        if len2 & 1:
            c1 = _gf2_times(_CRC_ZEROS[k], c1)
        len2 >>= 1
        k += 1
    return c1 ^ c2


# ---- the wrappers (host) ---------------------------------------------------------------------------------------------------------

_TRUNCATED = "Ran out of data mid-decompression 2."


def parse_zlib_header(data) -> int:
    """Offset of the DEFLATE body of a zlib stream (2), or raises the reference's HeaderError (Zlib.hs:55-68: FCHECK, CM, CINFO)."""
    if len(data) < 2:
        raise DecompressionError_(_TRUNCATED)
    cmf, flg = data[0], data[1]
    if ((cmf << 8) | flg) % 31 != 0:
        raise HeaderError("Header checksum failed")
    if cmf & 15 != 8:
        raise HeaderError("Bad compression method: %d" % (cmf & 15))
    if cmf >> 4 > 7:
        raise HeaderError("Window size too big: %d" % (cmf >> 4))
    if flg & 0x20:
        raise HeaderError("preset dictionary (FDICT): such a stream cannot be indexed")
    return 2


def parse_gzip_header(data) -> int:
    """Offset of the DEFLATE body of a gzip member (RFC 1952 2.3: FEXTRA, FNAME, FCOMMENT, FHCRC), or raises HeaderError."""
    def need(n):
        if len(data) < n:
            raise DecompressionError_(_TRUNCATED)
    need(10)
    if data[0] != 0x1f or data[1] != 0x8b:
        raise HeaderError("gzip: bad magic")
    if data[2] != 8:
        raise HeaderError("gzip: bad compression method: %d" % data[2])
    flg = data[3]
    if flg & 0xe0:
        raise HeaderError("gzip: reserved flag bits set")
    p = 10
    if flg & 4:
        need(p + 2)
        p += 2 + (data[p] | (data[p + 1] << 8))
        need(p)
    for bit in (8, 16):
        if flg & bit:
            while True:
                need(p + 1)
                p += 1
                if data[p - 1] == 0:
                    break
    if flg & 2:
        need(p + 2)
        if (data[p] | (data[p + 1] << 8)) != (_syszlib.crc32(bytes(data[:p])) & 0xffff):
            raise HeaderError("gzip: header crc mismatch")
        p += 2
    return p


def _fingerprint(data, end: int) -> Tuple[int, int]:
    """(end, CRC-32 of the first and the last 64 KiB) of the compressed file up to `end`, where its trailer starts (the trailer is
    what decompress() checks, and reports as a checksum error): an index loaded next to another file says so."""
    data = data[:end]
    return len(data), _syszlib.crc32(bytes(data[-65536:]), _syszlib.crc32(bytes(data[:65536])))


def _np(data) -> np.ndarray:
    return np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, dtype=np.uint8)


def segments_of(points, body_len: int, out_len: int):
    """The segments the access points cut a body of body_len bytes and out_len decoded bytes into:
    [(in_off, in_len, start_bit, end_bit, a, b)] -- input bytes of the BODY, the bit its first block starts at inside the first of
    them, the bit its last block ends at counted from that byte (0: the final block), and the output range it produces."""
    cuts = [(0, 0)] + [(int(b), int(p)) for b, p in points]
    segs = []
    for k, (bit, a) in enumerate(cuts):
        off = bit >> 3
        if k + 1 < len(cuts):
            end = cuts[k + 1][0] - 8 * off
            segs.append((off, (end + 7) >> 3, bit & 7, end, a, cuts[k + 1][1]))
        else:
            segs.append((off, body_len - off, bit & 7, 0, a, out_len))
    return segs


def window_extent(k: int, out_pos: int, first_row: int = 0):
    """(offset, length) of the dictionary of segment k of a stream inside its windows (rows of 32768 bytes from row first_row on):
    segment k > 0 starts at point k - 1, whose window is the last min(out_pos, 32768) bytes of that point's row; segment 0 has none."""
    if k == 0 or out_pos == 0:
        return 0, 0
    w = min(out_pos, WINDOW)
    return (first_row + k - 1) * WINDOW + (WINDOW - w), w


class Index:
    """The access points of one stream.  points: uint64 [n, 2] (in_bit from bit 0 of the body, out_pos); windows: uint8 [n, 32768]
    (point k's window at the END of row k: its last min(out_pos, 32768) bytes)."""

    def __init__(self, kind, span, points, windows, out_len, body_off, body_len, expect, fingerprint):
        self.kind, self.span = kind, int(span)
        self.points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2)
        self.windows = np.ascontiguousarray(windows, dtype=np.uint8).reshape(-1, WINDOW)
        self.out_len, self.body_off, self.body_len = int(out_len), int(body_off), int(body_len)
        self.expect = int(expect)  # zlib: the trailer's Adler-32; gzip: its CRC-32; raw: the Adler-32 of the build pass
        self.fingerprint = (int(fingerprint[0]), int(fingerprint[1]))

    # -- building ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def build(data, kind: str = "zlib", span: int = 1 << 20, ctx: Optional[Context] = None,
              size_hint: Optional[int] = None) -> Tuple[Optional["Index"], Either]:
        """One sequential decode (one wavefront) that records the access points.  Returns (index, Right(decoded bytes)) -- the build
        pass produces them anyway -- or (None, Left(error)).  zlib: the trailer's Adler-32 is checked here; gzip: ISIZE is, the
        CRC-32 by index.decompress()."""
        if kind not in KINDS:
            raise ValueError("kind must be one of %r" % (KINDS,))
        if span < 1:
            raise ValueError("span must be positive")
        data = bytes(data)
        ctx = ctx or default_context()
        try:
            body_off = 0 if kind == "raw" else parse_zlib_header(data) if kind == "zlib" else parse_gzip_header(data)
        except DecompressionError as e:
            return None, Left(e)
        body = _np(data)[body_off:]
        if kind == "gzip" and size_hint is None and len(data) >= body_off + 8:
            size_hint = int.from_bytes(data[-4:], "little")  # (ISIZE: right for a file under 4 GiB, a first guess otherwise)
        cap = int(size_hint) if size_hint is not None else max(1 << 16, 4 * len(body))
        max_points = max(16, cap // span + 16)
        L = _ffi.lib()
        for _attempt in range(8):
            out = np.empty(cap + 16, dtype=np.uint8)
            points = np.zeros((max_points, 2), dtype=np.uint64)
            windows = np.zeros((max_points, WINDOW), dtype=np.uint8)
            npoints, status, adler = C.c_uint32(0), C.c_int32(-1), C.c_uint32(0)
            out_len, in_used = C.c_uint64(0), C.c_uint64(0)
            detail = (C.c_uint32 * 2)(0, 0)
            inp = body if len(body) else np.zeros(1, dtype=np.uint8)
            _ffi.check(L.pzg_index_build(ctx.handle, inp.ctypes.data, len(body), out.ctypes.data, cap, span, points.ctypes.data, max_points,
                                         C.byref(npoints), windows.ctypes.data, C.byref(out_len), C.byref(status), detail, C.byref(in_used),
                                         C.byref(adler), 0), ctx.handle)
            if status.value == _ffi.E_OUT_TOO_SMALL and out_len.value > cap:
                cap = int(out_len.value)
                max_points = max(max_points, cap // span + 16)
                continue
            if status.value != _ffi.OK:
                return None, Left(error_from_status(bytes(body), status.value, detail))
            if npoints.value > max_points:  # more points than room: twice the room
                max_points = max(2 * max_points, int(npoints.value))
                continue
            break
        else:
            raise _ffi.PzgError("pzg_index_build: no capacity settled after 8 attempts")
        n, used, total = int(npoints.value), int(in_used.value), int(out_len.value)
        trailer = data[body_off + used:]
        expect = int(adler.value)
        if kind == "zlib":
            if len(trailer) < 4:
                return None, Left(DecompressionError_(_TRUNCATED))
            expect = int.from_bytes(trailer[:4], "big")
            if expect != adler.value:
                return None, Left(ChecksumError("checksum mismatch: %x != %x" % (expect, adler.value)))
        elif kind == "gzip":
            if len(trailer) < 8:
                return None, Left(DecompressionError_(_TRUNCATED))
            expect = int.from_bytes(trailer[:4], "little")
            isize = int.from_bytes(trailer[4:8], "little")
            if isize != total & 0xffffffff:
                return None, Left(ChecksumError("gzip: length mismatch: %u != %u" % (isize, total & 0xffffffff)))
            if trailer[8:10] == b"\x1f\x8b":
                return None, Left(HeaderError("gzip: a second member follows: only a file of ONE member can be indexed"))
        index = Index(kind, span, points[:n].copy(), windows[:n].copy(), total, body_off, used, expect, _fingerprint(data, body_off + used))
        return index, Right(out[:total].tobytes())

    @staticmethod
    def build_parallel(data, kind: str = "zlib", span: int = 1 << 20, chunk: Optional[int] = None,
                       ctx: Optional[Context] = None) -> Tuple[Optional["Index"], Either]:
        """build() without the sequential pass: pzg_index_scan finds the access points in parallel (a wavefront per `chunk`
        compressed bytes; None: the library's 128 KiB), then index.decompress() decodes every segment and checks the combined checksum
        against the trailer -- that decode is what proves the points.  Returns what build() returns.  Whenever the parallel path
        does not end in a verified success (PZG_E_SCAN, a segment's error, a checksum or length mismatch) the result is
        Index.build(data, ...)'s: a broken stream reports the reference's own error, found by the sequential decode.  The points
        are block boundaries about `span` apart, in general not the ones build() picks."""
        if kind not in KINDS:
            raise ValueError("kind must be one of %r" % (KINDS,))
        if span < 1:
            raise ValueError("span must be positive")
        if chunk is not None and chunk < 256:
            raise ValueError("chunk must be 256 or more")
        data = bytes(data)
        ctx = ctx or default_context()
        sequential = lambda: Index.build(data, kind, span, ctx)
        try:
            body_off = 0 if kind == "raw" else parse_zlib_header(data) if kind == "zlib" else parse_gzip_header(data)
        except DecompressionError as e:
            return None, Left(e)
        body = _np(data)[body_off:]
        max_points = max(16, 4 * len(body) // span + 16)
        L = _ffi.lib()
        for _attempt in range(8):
            points = np.zeros((max_points, 2), dtype=np.uint64)
            windows = np.zeros((max_points, WINDOW), dtype=np.uint8)
            npoints, status = C.c_uint32(0), C.c_int32(-1)
            out_len, in_used = C.c_uint64(0), C.c_uint64(0)
            detail = (C.c_uint32 * 2)(0, 0)
            inp = body if len(body) else np.zeros(1, dtype=np.uint8)
            _ffi.check(L.pzg_index_scan(ctx.handle, inp.ctypes.data, len(body), chunk or 0, span, points.ctypes.data, max_points,
                                        C.byref(npoints), windows.ctypes.data, C.byref(out_len), C.byref(status), detail, C.byref(in_used), 0),
                       ctx.handle)
            if status.value != _ffi.OK:
                return sequential()
            if npoints.value > max_points:  # more points than room: twice the room
                max_points = max(2 * max_points, int(npoints.value))
                continue
            break
        else:
            raise _ffi.PzgError("pzg_index_scan: no capacity settled after 8 attempts")
        n, used, total = int(npoints.value), int(in_used.value), int(out_len.value)
        trailer = data[body_off + used:]
        if kind == "gzip":
            if len(trailer) < 8 or int.from_bytes(trailer[4:8], "little") != total & 0xffffffff:
                return sequential()
            if trailer[8:10] == b"\x1f\x8b":
                return None, Left(HeaderError("gzip: a second member follows: only a file of ONE member can be indexed"))
        index = Index(kind, span, points[:n].copy(), windows[:n].copy(), total, body_off, used, 0, _fingerprint(data, body_off + used))
        if kind == "raw":  # no trailer: the segments' combined Adler-32 stands in for it, as the build pass's does in build()
            err, out, _base, sums, segs = index._decode(data, 0, n + 1, ctx, crc32=False)
            if err is not None:
                return sequential()
            expect = 1
            for j, s in enumerate(segs):
                expect = adler32_combine(expect, int(sums[j]), s[5] - s[4])
            index.expect = expect
            return index, Right(out.tobytes())
        r = index.decompress(data, ctx)
        if not r.is_right():
            return sequential()
        index.expect = int.from_bytes(trailer[:4], "big" if kind == "zlib" else "little")
        return index, r

    # -- the segments --------------------------------------------------------------------------------------------------------------
    def segments(self):
        """[(in_off, in_len, start_bit, end_bit, a, b)]: input bytes of the BODY, the bit its first block starts at inside the first of
        them, the bit its last block ends at counted from that byte (0: the final block), and the output range it produces."""
        return segments_of(self.points, self.body_len, self.out_len)

    def _check_pair(self, data) -> Optional[DecompressionError]:
        if _fingerprint(data, self.body_off + self.body_len) != self.fingerprint:
            return DecompressionError_("index does not match the stream")
        return None

    def _decode(self, data, first: int, last: int, ctx: Optional[Context], crc32: bool):
        """Segments first .. last - 1 in ONE launch into one contiguous buffer: (error or None, buffer, its output offset, sums, segs)."""
        ctx = ctx or default_context()
        segs = self.segments()[first:last]
        m = len(segs)
        body = _np(data)[self.body_off:self.body_off + self.body_len]
        base = segs[0][4]
        total = segs[-1][5] - base
        in_off = np.array([s[0] for s in segs], dtype=np.uint64)
        in_len = np.array([s[1] for s in segs], dtype=np.uint64)
        start_bit = np.array([s[2] for s in segs], dtype=np.uint8)
        end_bit = np.array([s[3] for s in segs], dtype=np.uint64)
        out_off = np.array([s[4] - base for s in segs], dtype=np.uint64)
        out_cap = np.array([s[5] - s[4] for s in segs], dtype=np.uint64)
        ext = [window_extent(first + j, s[4]) for j, s in enumerate(segs)]
        dict_off = np.array([e[0] for e in ext], dtype=np.uint64)
        w = np.array([e[1] for e in ext], dtype=np.uint64)
        windows = self.windows if len(self.windows) else np.zeros((1, WINDOW), dtype=np.uint8)
        out = np.empty(total + 16, dtype=np.uint8)
        out_len = np.zeros(m, dtype=np.uint64)
        status = np.full(m, -1, dtype=np.int32)
        detail = np.zeros((m, 2), dtype=np.uint32)
        in_used = np.zeros(m, dtype=np.uint64)
        sums = np.zeros(m, dtype=np.uint32)
        inp = body if len(body) else np.zeros(1, dtype=np.uint8)
        _ffi.check(_ffi.lib().pzg_decompress_many_segments(
            ctx.handle, inp.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, start_bit.ctypes.data, end_bit.ctypes.data,
            windows.ctypes.data, dict_off.ctypes.data, w.ctypes.data, out.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data,
            out_len.ctypes.data, status.ctypes.data, detail.ctypes.data, in_used.ctypes.data, sums.ctypes.data, m,
            _ffi.CRC32 if crc32 else 0), ctx.handle)
        for j, s in enumerate(segs):
            if int(status[j]) == _ffi.E_OUT_TOO_SMALL or (int(status[j]) == _ffi.OK and int(out_len[j]) != s[5] - s[4]):
                return DecompressionError_("index does not match the stream"), None, base, None, segs
            if int(status[j]) != _ffi.OK:
                return error_from_status(bytes(body[s[0]:s[0] + s[1]]), int(status[j]), detail[j]), None, base, None, segs
        return None, out[:total], base, sums, segs

    def decompress(self, data, ctx: Optional[Context] = None) -> Either:
        """The whole stream, every segment in one launch; the segments' checksums, combined, must be the trailer's."""
        data = bytes(data)
        err = self._check_pair(data)
        if err is not None:
            return Left(err)
        gz = self.kind == "gzip"
        err, out, _base, sums, segs = self._decode(data, 0, len(self.points) + 1, ctx, crc32=gz)
        if err is not None:
            return Left(err)
        total = 0 if gz else 1
        for j, s in enumerate(segs):
            total = (crc32_combine if gz else adler32_combine)(total, int(sums[j]), s[5] - s[4])
        trailer = data[self.body_off + self.body_len:]
        expect = self.expect
        if self.kind == "zlib":
            if len(trailer) < 4:
                return Left(DecompressionError_(_TRUNCATED))
            expect = int.from_bytes(trailer[:4], "big")
        elif gz:
            if len(trailer) < 8:
                return Left(DecompressionError_(_TRUNCATED))
            expect = int.from_bytes(trailer[:4], "little")
            isize = int.from_bytes(trailer[4:8], "little")
            if isize != self.out_len & 0xffffffff and expect == total:
                return Left(ChecksumError("gzip: length mismatch: %u != %u" % (isize, self.out_len & 0xffffffff)))
        if expect != total:
            return Left(ChecksumError("checksum mismatch: %x != %x" % (expect, total)))
        return Right(out.tobytes())

    def read(self, data, offset: int, length: int, ctx: Optional[Context] = None) -> bytes:
        """decompress(data)[offset:offset + length], decoding only the segments that cover the range.  Raises the DecompressionError
        a segment fails with.  (A partial read has no trailer to check against: decompress() is the verifying pass.)"""
        data = bytes(data)
        err = self._check_pair(data)
        if err is not None:
            raise err
        lo = max(0, min(int(offset), self.out_len))
        hi = max(lo, min(lo + max(0, int(length)), self.out_len))
        if hi == lo:
            return b""
        starts = np.concatenate(([0], self.points[:, 1])).astype(np.uint64)
        first = int(np.searchsorted(starts, lo, side="right")) - 1
        last = int(np.searchsorted(starts, hi, side="left"))
        err, out, base, _sums, _segs = self._decode(data, first, last, ctx, crc32=False)
        if err is not None:
            raise err
        return out[lo - base:hi - base].tobytes()

    # -- on disk -------------------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One .npz archive (whatever the file is called)."""
        with open(path, "wb") as f:
            np.savez(f, points=self.points, windows=self.windows, kind=np.array(KINDS.index(self.kind), dtype=np.int64),
                     lengths=np.array([self.span, self.out_len, self.body_off, self.body_len, self.expect, *self.fingerprint], dtype=np.uint64))

    @staticmethod
    def load(path) -> "Index":
        with open(path, "rb") as f, np.load(f) as z:
            ln = [int(x) for x in z["lengths"]]
            points, windows = z["points"], z["windows"]
            if len(ln) != 7 or points.ndim != 2 or points.shape[1] != 2 or windows.shape != (len(points), WINDOW):
                raise ValueError("%s: not an index" % (path,))
            return Index(KINDS[int(z["kind"])], ln[0], points, windows, ln[1], ln[2], ln[3], ln[4], (ln[5], ln[6]))
