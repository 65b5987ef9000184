"""EXTENSION: a gzip FILE of many members -- BGZF (bgzip: .vcf.gz, .bam), WARC, rotated logs, `cat a.gz b.gz` -- decoded with a
wavefront per member in one launch.

A member starts with an empty window, so nothing has to be indexed: the members are found and laid out on the device
(pzg_gzip_find_members, pzg_gzip_layout; pure_zlib_amd/csrc/member_core.h) and the gzip kernel decodes them side by side:

    decompress_gzip_file(data)                      # Either: exactly gzip_decompress_many([data])[0], for every input
    index, result = decompress_gzip_file(data, return_index=True)
    index.read(data, offset, length)                # only the members that cover the range
    index.save("big.gz.pzm"); index = MemberIndex.load("big.gz.pzm"); index.decompress(data)

What the finder returns are CANDIDATES (the bytes of a member header can occur inside a member: in a stored block, or by chance).
A candidate counts as a member only when the chain of good members from position 0 reaches it: member j is good when it decodes
without an error, fills exactly the room its ISIZE promised and ends exactly where candidate j + 1 starts (the kernel has checked
its CRC-32 and ISIZE by then).  The first member that is not good is repaired: when it decoded without an error but stopped short
or went on, the rest of the file goes to the one-stream decode, which does the same; otherwise candidate j + 1 is dropped and the
members from j on are laid out and decoded again.  Beyond MAX_DROPS drops in a row for one member or MAX_REPAIRS repair launches the
whole file goes to the one-stream decode, whose result -- and error text -- is then the file's.

A LARGE member (decompress_gzip_file's `split`: that many compressed bytes or more) is not left to one wavefront: the large members
of a launch are scanned in one call (pzg_index_scan_many) and their segments decoded in one launch, straight into their places
(pure_zlib_amd/split.py).  Only a member whose size and CRC-32 come out as its trailer says is taken from that; every other one is
decoded by the gzip launch as before, so the acceptance chain, the repairs and every error text are untouched.

Limits: a member of 4 GiB or more, whose ISIZE has wrapped, ends in the one-stream decode; MemberIndex.read() decodes a member it
touches on one wavefront, however large.
"""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _ffi
from . import split as _split
from . import zlib as _z
from .indexed import _fingerprint, parse_gzip_header
from .zlib import Context, DecompressionError_, Either, Left, Right, default_context, error_from_status

MAX_DROPS = 4     # candidates dropped in a row behind one member
MAX_REPAIRS = 16  # launches after the first


def _padded(data: bytes) -> np.ndarray:
    buf = np.zeros(len(data) + 16, dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return buf


def find_members(buf: np.ndarray, n: int, ctx: Context, chunk: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """pzg_gzip_find_members over buf[:n] (host memory): (starts uint64, bsize uint32), repeated with more room when there are more
    candidates than room."""
    L = _ffi.lib()
    room = max(64, n >> 12)
    for _attempt in range(3):
        starts, bsize = np.zeros(room, dtype=np.uint64), np.zeros(room, dtype=np.uint32)
        count = C.c_uint32(0)
        _ffi.check(L.pzg_gzip_find_members(ctx.handle, buf.ctypes.data, n, chunk or 0, starts.ctypes.data, bsize.ctypes.data, room,
                                           C.byref(count), 0), ctx.handle)
        if count.value <= room:
            return starts[:count.value], bsize[:count.value]
        room = int(count.value)
    raise _ffi.PzgError("pzg_gzip_find_members: the count did not settle")


def prune_bgzf(starts, bsize) -> List[int]:
    """The list without the candidates that lie strictly inside a member that states its own size (the BGZF 'BC' subfield)."""
    keep, until = [], 0
    for s, b in zip(starts.tolist(), bsize.tolist()):
        if s < until:
            continue
        keep.append(s)
        until = s + b if b else 0
    return keep


def layout(buf: np.ndarray, n: int, starts, ctx: Context):
    """pzg_gzip_layout of the members that start at `starts`, the output from offset 0: (in_off, in_len, out_off, out_cap, total)."""
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    m = len(st)
    arrays = [np.zeros(m, dtype=np.uint64) for _ in range(4)]
    total = C.c_uint64(0)
    _ffi.check(_ffi.lib().pzg_gzip_layout(ctx.handle, buf.ctypes.data, n, st.ctypes.data, m, 0, *[a.ctypes.data for a in arrays],
                                          C.byref(total), 0), ctx.handle)
    return (*arrays, int(total.value))


def _launch(buf, in_off, in_len, out_off, out_cap, total, ctx, split=0, split_chunk=None):
    """The members in ONE PZG_GZIP launch: (out, out_len, status, detail, in_used).  split: the members of that many bytes or more go
    to split.split_decode first, many wavefronts each; one that comes back verified is filled in as the gzip kernel would have
    filled it in, every other one is decoded by the launch with the rest."""
    out = np.empty(total + 16, dtype=np.uint8)
    m = len(in_off)
    rest = np.arange(m)
    bodies, which = [], []
    if split:
        for j in np.flatnonzero(in_len >= split).tolist():
            body = _large_body(buf, int(in_off[j]), int(in_len[j]), int(out_off[j]), int(out_cap[j]))
            if body is not None:
                bodies.append(body)
                which.append(j)
    if not bodies:
        out_len, status, detail, in_used, _crc = ctx.decompress_many_raw(buf, in_off, in_len, out, out_off, out_cap, gzip=True)
        return out, out_len, status, detail, in_used
    done = _split.split_decode(buf, bodies, out, ctx, split_chunk)
    taken = np.array([j for j, ok in zip(which, done) if ok], dtype=np.int64)
    rest = np.setdiff1d(rest, taken)
    out_len, status = np.zeros(m, dtype=np.uint64), np.full(m, -1, dtype=np.int32)
    detail, in_used = np.zeros((m, 2), dtype=np.uint32), np.zeros(m, dtype=np.uint64)
    out_len[taken], status[taken], in_used[taken] = out_cap[taken], _ffi.OK, in_len[taken]
    out_len[rest], status[rest], detail[rest], in_used[rest], _crc = ctx.decompress_many_raw(
        buf, in_off[rest], in_len[rest], out, out_off[rest], out_cap[rest], gzip=True)
    return out, out_len, status, detail, in_used


def _large_body(buf, off, length, out_off, out_cap):
    """The raw body of the member buf[off : off + length] as a split.Body, its size and CRC-32 from the trailer; None when the extent
    does not read as header | body | trailer, or its ISIZE is more than the room the layout gave it (no sound member's is)."""
    extent = buf[off:off + length]
    try:  # (a header longer than this reads as cut short: such a member is not split)
        h = parse_gzip_header(extent[:1 << 17].tobytes())
    except _z.DecompressionError:
        return None
    if length < h + 8:
        return None
    crc = int.from_bytes(extent[length - 8:length - 4].tobytes(), "little")
    isize = int.from_bytes(extent[length - 4:].tobytes(), "little")
    if isize != out_cap:
        return None
    return _split.Body(off + h, length - h - 8, isize, crc, out_off)


def decompress_gzip_file(data, ctx: Optional[Context] = None, chunk: Optional[int] = None, return_index: bool = False,
                         split: Optional[int] = None, split_chunk: Optional[int] = None):
    """The members of a gzip file decoded in parallel.  Returns what gzip_decompress_many([data])[0] returns -- the same bytes for a
    Right, the same show() text for a Left -- or, with return_index, (MemberIndex or None, that).
    split: members of that many compressed bytes or more are decoded by many wavefronts each (pure_zlib_amd.split; split_chunk: the
    compressed bytes per wavefront of their scan); None: split.DEFAULT_SPLIT; 0: none, every member is one wavefront's work.  Only
    the time depends on it.  The MemberIndex does not record the split: index.read() of a range inside a large member still decodes
    that member on one wavefront."""
    if chunk is not None and chunk < 64:
        raise ValueError("chunk must be 64 or more")
    if split_chunk is not None and split_chunk < 256:
        raise ValueError("split_chunk must be 256 or more")
    split = _split.DEFAULT_SPLIT if split is None else int(split)
    if split < 0:
        raise ValueError("split must not be negative")
    data = bytes(data)
    ctx = ctx or default_context()
    n = len(data)

    def done(result, starts=None, sizes=None):
        if not return_index:
            return result
        index = None
        if result.is_right() and starts is not None:
            index = MemberIndex(starts, np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.uint64)))), _fingerprint(data, n))
        return index, result

    def one_stream(d):
        return _z.gzip_decompress_many([d], ctx)[0]

    buf = _padded(data)
    cands = prune_bgzf(*find_members(buf, n, ctx, chunk))
    pieces, starts, sizes = [], [], []  # what is final: the output, the members' starts and decoded sizes
    first, drops = 0, 0                 # cands[first] is the first member that is not final yet
    for _launch_no in range(1 + MAX_REPAIRS):
        sub = cands[first:]
        m = len(sub)
        in_off, in_len, out_off, out_cap, total = layout(buf, n, sub, ctx)
        out, out_len, status, _detail, in_used = _launch(buf, in_off, in_len, out_off, out_cap, total, ctx, split, split_chunk)
        good = (status == _ffi.OK) & (out_len == out_cap) & (in_used == in_len)
        bad = np.flatnonzero(~good)
        j = int(bad[0]) if len(bad) else m
        if j == m - 1 and status[j] == _ffi.OK and out_len[j] <= out_cap[j] and in_used[j] <= in_len[j]:
            j = m  # the last member may end in front of its extent's end: trailing bytes are ignored, as the one-stream decode ignores them
        upto = m if j == m else j
        end = int(out_off[upto - 1] + out_len[upto - 1]) if upto else 0
        pieces.append(out[:end].tobytes())
        starts += sub[:upto]
        sizes += out_len[:upto].tolist()
        if j == m:
            return done(Right(b"".join(pieces)), starts, sizes)
        if status[j] == _ffi.OK or j + 1 == m:
            # it stopped in front of its extent's end, or went on past its room -- or it is the last and nothing is left to drop: the
            # one-stream decode from here on does what it would have done there
            if sub[j] == 0:
                return done(one_stream(data))
            tail = one_stream(data[sub[j]:])
            if not tail.is_right():
                break
            return done(Right(b"".join(pieces) + tail.value), starts + [sub[j]], sizes + [len(tail.value)])
        drops = drops + 1 if j == 0 else 1
        if drops > MAX_DROPS:
            break
        del cands[first + j + 1]
        first += j
    return done(one_stream(data))


class MemberIndex:
    """The members of a verified file: starts (uint64 [m], input offsets) and offsets (uint64 [m + 1], cumulative output offsets).
    An entry is what one wavefront decodes: one member, or -- where the file's tail went to the one-stream decode -- the tail."""

    def __init__(self, starts, offsets, fingerprint):
        self.starts = np.ascontiguousarray(starts, dtype=np.uint64)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.fingerprint = (int(fingerprint[0]), int(fingerprint[1]))
        self.out_len = int(self.offsets[-1])

    def _decode(self, data: bytes, a: int, b: int, ctx: Optional[Context]) -> np.ndarray:
        """Entries a .. b - 1 in one launch; raises what does not decode as the index says."""
        if _fingerprint(data, len(data)) != self.fingerprint:
            raise DecompressionError_("index does not match the stream")
        ctx = ctx or default_context()
        ends = np.concatenate((self.starts[1:], [len(data)])).astype(np.uint64)
        in_off, in_len = self.starts[a:b].copy(), (ends - self.starts)[a:b].copy()
        base = self.offsets[a]
        out_off, out_cap = self.offsets[a:b] - base, (self.offsets[1:] - self.offsets[:-1])[a:b].copy()
        buf = _padded(data)
        out, out_len, status, detail, _used = _launch(buf, in_off, in_len, out_off, out_cap, int(self.offsets[b] - base), ctx)
        for k in range(b - a):
            if int(status[k]) not in (_ffi.OK, _ffi.E_OUT_TOO_SMALL):
                lo = int(in_off[k])
                raise error_from_status(data[lo:lo + int(in_len[k])], int(status[k]), detail[k])
            if int(status[k]) != _ffi.OK or out_len[k] != out_cap[k]:
                raise DecompressionError_("index does not match the stream")
        return out[:int(self.offsets[b] - base)]

    def decompress(self, data, ctx: Optional[Context] = None) -> Either:
        """The whole file, every entry in one launch (each member's CRC-32 and ISIZE checked by the kernel)."""
        try:
            return Right(self._decode(bytes(data), 0, len(self.starts), ctx).tobytes())
        except _z.DecompressionError as e:
            return Left(e)

    def read(self, data, offset: int, length: int, ctx: Optional[Context] = None) -> bytes:
        """decompress(data)[offset:offset + length], decoding only the members that cover the range.  Raises the DecompressionError
        a member fails with."""
        lo = max(0, min(int(offset), self.out_len))
        hi = max(lo, min(lo + max(0, int(length)), self.out_len))
        if hi == lo:
            return b""
        a = int(np.searchsorted(self.offsets, lo, side="right")) - 1
        b = int(np.searchsorted(self.offsets, hi, side="left"))
        base = int(self.offsets[a])
        return self._decode(bytes(data), a, b, ctx)[lo - base:hi - base].tobytes()

    def save(self, path) -> None:
        """One .npz archive (whatever the file is called)."""
        with open(path, "wb") as f:
            np.savez(f, starts=self.starts, offsets=self.offsets, fingerprint=np.array(self.fingerprint, dtype=np.uint64))

    @staticmethod
    def load(path) -> "MemberIndex":
        with open(path, "rb") as f, np.load(f) as z:
            starts, offsets, fp = z["starts"], z["offsets"], z["fingerprint"]
            if starts.ndim != 1 or offsets.shape != (len(starts) + 1,) or fp.shape != (2,):
                raise ValueError("%s: not a member index" % (path,))
            return MemberIndex(starts, offsets, fp)
