"""EXTENSION: the LARGE members of a container -- a gzip file's, a ZIP archive's -- decoded by many wavefronts each.

A member is a raw DEFLATE body whose decoded size and CRC-32 the container states.  One wavefront decodes it at the rate of the
plain decode; split_decode() scans the bodies of all large members in one call (pzg_index_scan_many: a wavefront per chunk over all
of them), decodes all their segments in one launch straight into the members' places in the output
(pzg_decompress_many_segments with PZG_CRC32) and combines each body's segment CRCs.  The scan's points are proven by nothing but
that decode, so a body counts as done only when everything agrees -- the scan succeeded and used the whole body, every segment
decoded and filled exactly its room, the sizes add up to the stated size and the combined CRC-32 is the stated one.  Anything else
-- a broken member, a false chain, a device without the memory -- is "not split": the caller decodes that member on its ordinary
path, and the statuses, the error text and the bytes delivered are that path's.

DEFAULT_SPLIT and DEFAULT_CHUNK come from profiles/split.txt (tests/tools/split_bench.py): on a file of 8 equal members splitting
first beats a wavefront per member by more than 10 % and the spreads at members of 5 MiB, rounded up to 8 MiB; below that nothing is
split.  A 64 KiB chunk is best or within the spreads of the best from there on.
"""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _ffi
from .indexed import WINDOW, crc32_combine, segments_of, window_extent
from .zlib import Context

DEFAULT_SPLIT = 8 << 20     # members of this many compressed bytes or more are split; 0: none
DEFAULT_CHUNK = 64 << 10    # compressed bytes per scan chunk
SPAN = 1 << 20              # decoded bytes per segment, about
MAX_CHUNKS = 8192           # per scan call: the chip's 6,656 resident stream-waves rounded up -- more chunks gain no parallelism, and
                            # 8,192 chunks bound a call's scratch at 512 MiB


class Body(NamedTuple):
    """One large member's raw DEFLATE body inside the input buffer, what its container says it holds and where its bytes go."""
    off: int       # in the input buffer
    length: int
    size: int      # decoded bytes expected
    crc: int       # CRC-32 expected
    out_off: int   # in the output buffer


def _calls(bodies: Sequence[Body], chunk: int) -> List[List[int]]:
    """The bodies' indices grouped into scan calls of at most MAX_CHUNKS chunks (a body of more than that is a call of its own)."""
    calls, cur, used = [], [], 0
    for i, b in enumerate(bodies):
        c = max(1, -(-b.length // chunk))
        if cur and used + c > MAX_CHUNKS:
            calls.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += c
    if cur:
        calls.append(cur)
    return calls


def split_decode(buf: np.ndarray, bodies: Sequence[Body], out: np.ndarray, ctx: Context, chunk: Optional[int] = None,
                 span: Optional[int] = None) -> List[bool]:
    """For every body: True -- out[out_off : out_off + size] holds its decoded bytes, verified against size and crc; False -- not
    split (that range of `out` may hold anything: the caller decodes the member over it)."""
    chunk, span = int(chunk or DEFAULT_CHUNK), int(span or SPAN)
    n = len(bodies)
    done = [False] * n
    if n == 0:
        return done
    # 1. the scans: points and windows of every body that scanned as its container says
    pts, wins, rows = [None] * n, [], 0  # pts[i]: (its points, the row of its first window in the concatenated windows)
    for call in _calls(bodies, chunk):
        rooms = [bodies[i].size // span + 2 for i in call]  # (points lie `span` or more decoded bytes apart)
        point_off = np.concatenate(([0], np.cumsum(rooms))).astype(np.uint64)
        if int(point_off[-1]) >= 1 << 32:
            continue
        try:
            p, w, npoints, out_len, status, _detail, in_used = ctx.index_scan_many(
                buf, [bodies[i].off for i in call], [bodies[i].length for i in call], point_off, chunk, span)
        except _ffi.PzgError:
            continue  # (PZG_RC_NO_MEMORY among them: these bodies are not split)
        for j, i in enumerate(call):
            b = bodies[i]
            if int(status[j]) != _ffi.OK or int(in_used[j]) != b.length or int(out_len[j]) != b.size or int(npoints[j]) > rooms[j]:
                continue
            lo = int(point_off[j])
            pts[i] = (p[lo:lo + int(npoints[j])], rows + lo)
        wins.append(w)
        rows += len(w)
    live = [i for i in range(n) if pts[i] is not None]
    if not live:
        return done
    windows = wins[0] if len(wins) == 1 else np.concatenate(wins)
    if len(windows) == 0:
        windows = np.zeros((1, WINDOW), dtype=np.uint8)
    # 2. every segment of every such body in one launch, straight into its place
    owner, in_off, in_len, start_bit, end_bit, dict_off, dict_len, out_off, out_cap = ([] for _ in range(9))
    for i in live:
        b, (p, row) = bodies[i], pts[i]
        for k, (off, ln, sbit, ebit, a, e) in enumerate(segments_of(p, b.length, b.size)):
            d_off, d_len = window_extent(k, a, row)
            owner.append(i)
            in_off.append(b.off + off)
            in_len.append(ln)
            start_bit.append(sbit)
            end_bit.append(ebit)
            dict_off.append(d_off)
            dict_len.append(d_len)
            out_off.append(b.out_off + a)
            out_cap.append(e - a)
    m = len(owner)
    u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
    in_off, in_len, end_bit, dict_off, dict_len, out_off, out_cap = map(u64, (in_off, in_len, end_bit, dict_off, dict_len, out_off, out_cap))
    start_bit = np.array(start_bit, dtype=np.uint8)
    out_len, status = np.zeros(m, dtype=np.uint64), np.full(m, -1, dtype=np.int32)
    detail, in_used, crc = np.zeros((m, 2), dtype=np.uint32), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
    rc = _ffi.lib().pzg_decompress_many_segments(
        ctx.handle, buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, start_bit.ctypes.data, end_bit.ctypes.data,
        windows.ctypes.data, dict_off.ctypes.data, dict_len.ctypes.data, out.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data,
        out_len.ctypes.data, status.ctypes.data, detail.ctypes.data, in_used.ctypes.data, crc.ctypes.data, m, _ffi.CRC32)
    if rc != _ffi.RC_OK:
        return done
    # 3. a body is done when every segment is sound and exactly full and the CRCs, combined, are the container's
    full = (status == _ffi.OK) & (out_len == out_cap)
    total, sound = {i: 0 for i in live}, {i: True for i in live}
    for j, i in enumerate(owner):
        sound[i] = sound[i] and bool(full[j])
        if sound[i]:
            total[i] = crc32_combine(total[i], int(crc[j]), int(out_cap[j]))
    for i in live:
        done[i] = sound[i] and total[i] == bodies[i].crc & 0xffffffff
    return done
