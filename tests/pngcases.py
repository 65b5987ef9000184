"""Shared by the PNG tests (no GPU): a PNG WRITER over the system's zlib.compress that applies a chosen filter to each row -- so every
filter and every mix is reachable -- and can cut IDAT at chosen places, write a chosen filter byte, a wrong chunk CRC, a short
stream or a row too many; a plain-Python REFERENCE UNFILTER written from the PNG specification (section 9) alone, which shares
nothing with pure_zlib_amd/csrc/unfilter_core.h; and the cases of pzg_unfilter_many that the CPU model (tests/test_model_unfilter.py)
and the device (tests/test_gpu_png.py) both run: the smallest shapes at which the kernel can go wrong."""
import functools
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

E_TRUNCATED, E_FILTER = 1, 23

BPPS = (1, 2, 3, 4, 6, 8)
HEIGHTS = (1, 2, 63, 64, 65, 129)  # one row, the group boundary, two boundaries


def row_bytes_of(bpp):
    """A row shorter than the lag, one unit, and rows around the dword and group edges."""
    return sorted({rb for rb in (bpp - 1, bpp, bpp + 1, 63, 64, 65, 257) if rb >= 1})


# ---- the reference unfilter: PNG specification 9.2 - 9.4, byte by byte ----------------------------------------------------------------
def paeth_predictor(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    if pb <= pc:
        return b
    return c


def unfilter(stream: bytes, row_bytes: int, height: int, bpp: int) -> List[bytes]:
    """The rows of `stream` (height rows of a filter byte and row_bytes bytes) reconstructed; raises ValueError at a filter byte > 4."""
    rows, prior = [], bytes(row_bytes)
    for y in range(height):
        at = y * (1 + row_bytes)
        ft, line = stream[at], stream[at + 1:at + 1 + row_bytes]
        recon = bytearray(row_bytes)
        if ft == 0:
            recon[:] = line
        elif ft == 1:
            for j in range(row_bytes):
                recon[j] = (line[j] + (recon[j - bpp] if j >= bpp else 0)) & 255
        elif ft == 2:
            for j in range(row_bytes):
                recon[j] = (line[j] + prior[j]) & 255
        elif ft == 3:
            for j in range(row_bytes):
                recon[j] = (line[j] + (((recon[j - bpp] if j >= bpp else 0) + prior[j]) >> 1)) & 255
        elif ft == 4:
            for j in range(row_bytes):
                a = recon[j - bpp] if j >= bpp else 0
                c = prior[j - bpp] if j >= bpp else 0
                recon[j] = (line[j] + paeth_predictor(a, prior[j], c)) & 255
        else:
            raise ValueError("row %d has filter type %d" % (y, ft))
        rows.append(bytes(recon))
        prior = rows[-1]
    return rows


# ---- the writer ------------------------------------------------------------------------------------------------------------------------
def _shift(rows: np.ndarray, bpp: int) -> np.ndarray:
    out = np.zeros_like(rows)
    out[:, bpp:] = rows[:, :-bpp] if rows.shape[1] > bpp else out[:, bpp:]
    return out


def filtered_candidates(raw: np.ndarray, bpp: int) -> np.ndarray:
    """raw: (H, row_bytes) uint8.  (5, H, row_bytes): every row filtered by every filter (the forward filters take raw neighbours)."""
    x = raw.astype(np.int32)
    a = _shift(x, bpp)
    b = np.vstack([np.zeros((1, x.shape[1]), np.int32), x[:-1]])
    c = _shift(b, bpp)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - pred]).astype(np.uint8)


def filter_stream(raw: np.ndarray, bpp: int, filters) -> bytes:
    """The filtered stream of `raw`: filters is one filter type for all rows, a sequence of one per row, or "adaptive" (the usual
    encoder's rule: per row the filter with the smallest sum of absolute values of the filtered bytes taken as signed)."""
    h = raw.shape[0]
    cand = filtered_candidates(raw, bpp)
    if isinstance(filters, str):
        assert filters == "adaptive"
        fts = np.abs(cand.view(np.int8).astype(np.int32)).sum(axis=2).argmin(axis=0)
    else:
        fts = np.full(h, filters) if np.isscalar(filters) else np.asarray(filters)
    out = np.empty((h, 1 + raw.shape[1]), np.uint8)
    out[:, 0] = fts
    out[:, 1:] = cand[fts, np.arange(h)]
    return out.tobytes()


def chunk(kind: bytes, body: bytes, bad_crc: bool = False) -> bytes:
    crc = zlib.crc32(body, zlib.crc32(kind)) ^ (1 if bad_crc else 0)
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", crc)


CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


def geometry(width, color_type, depth):
    """(row_bytes, bpp)"""
    bits = CHANNELS[color_type] * depth
    return (width * bits + 7) // 8, max(1, bits // 8)


def write_png(width, height, color_type, depth, raw: np.ndarray, filters="adaptive", idat=None, level=6, interlace=0, bad_crc=None,
              stream_edit=None, palette=None, trns=None) -> bytes:
    """raw: (height', row_bytes) uint8, the rows as the file stores them (height' may differ from height: a row too many or too few).
    idat: None -- one chunk; k -- chunks of k bytes.  bad_crc: the kind of a chunk whose CRC is written wrong.  stream_edit: a function
    of the filtered stream, applied before it is compressed (a chosen filter byte); of the zlib stream when it returns a tuple
    ("z", f)."""
    rb, bpp = geometry(width, color_type, depth)
    assert raw.shape[1] == rb
    stream = filter_stream(raw, bpp, filters)
    z_edit = None
    if stream_edit is not None:
        r = stream_edit(stream)
        if isinstance(r, tuple):
            z_edit = r[1]
        else:
            stream = r
    z = zlib.compress(stream, level)
    if z_edit is not None:
        z = z_edit(z)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, 0, 0, interlace), bad_crc == b"IHDR")
    if color_type == 3 or palette is not None:
        out += chunk(b"PLTE", palette if palette is not None else bytes(range(48)), bad_crc == b"PLTE")
    if trns is not None:
        out += chunk(b"tRNS", trns)
    pieces = [z] if idat is None else [z[i:i + idat] for i in range(0, len(z), idat)]
    for k, p in enumerate(pieces):
        out += chunk(b"IDAT", p, bad_crc == b"IDAT" and k == len(pieces) // 2)
    return out + chunk(b"IEND", b"")


# ---- the cases of pzg_unfilter_many ----------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    bpp: int
    row_bytes: int
    height: int
    stream: bytes            # what the call is given (src_len = len(stream))
    status: int              # what it must answer
    d0: int
    d1: int
    rows: List[bytes]        # the rows it must deliver, [0, len(rows)); the others stay as they were


def _raw(rng, h, rb, kind="random"):
    if kind == "ties":  # few values: a = b = c, pa = pb < pc and pb = pc < pa all happen (checked in the CPU suite)
        return rng.choice(np.array([5, 6, 10, 12], np.uint8), size=(h, rb))
    if kind == "high":  # Average with a + b >= 256
        return rng.integers(200, 256, size=(h, rb), dtype=np.uint8)
    return rng.integers(0, 256, size=(h, rb), dtype=np.uint8)


def _sound(name, bpp, rb, h, raw, filters) -> Case:
    stream = filter_stream(raw, bpp, filters)
    rows = unfilter(stream, rb, h, bpp)
    assert rows == [r.tobytes() for r in raw], name  # the writer and the reference agree: what the file stores comes back
    return Case(name, bpp, rb, h, stream, 0, 0, 0, rows)


@functools.lru_cache(maxsize=None)
def shape_cases() -> List[Case]:
    """Every bpp x row_bytes x height with a seeded random filter per row (246 images, each of another shape)."""
    rng = np.random.default_rng(20261019)
    out = []
    for bpp in BPPS:
        for rb in row_bytes_of(bpp):
            for h in HEIGHTS:
                out.append(_sound("random-filters bpp%d rb%d h%d" % (bpp, rb, h), bpp, rb, h, _raw(rng, h, rb), rng.integers(0, 5, size=h)))
    return out


@functools.lru_cache(maxsize=None)
def filter_cases() -> List[Case]:
    """Each filter on every row -- row 0 included, whose row above is zeros -- for every bpp and row_bytes at heights 2 and 65; Paeth on
    bytes where its ties occur; Average where a + b >= 256."""
    rng = np.random.default_rng(77)
    out = []
    for bpp in BPPS:
        for rb in row_bytes_of(bpp):
            for h in (2, 65):
                for ft in range(5):
                    out.append(_sound("filter%d bpp%d rb%d h%d" % (ft, bpp, rb, h), bpp, rb, h, _raw(rng, h, rb), ft))
        for rb in (bpp + 1, 65):
            out.append(_sound("paeth-ties bpp%d rb%d" % (bpp, rb), bpp, rb, 66, _raw(rng, 66, rb, "ties"), 4))
            out.append(_sound("average-high bpp%d rb%d" % (bpp, rb), bpp, rb, 66, _raw(rng, 66, rb, "high"), 3))
    return out


@functools.lru_cache(maxsize=None)
def error_cases() -> List[Case]:
    """A filter byte of 5 or 255 on row 0, on row 64 and on the last row; src_len cut mid-row and at a row boundary; both at once."""
    rng = np.random.default_rng(5)
    out = []
    for bpp, rb in ((1, 1), (3, 65), (4, 64), (8, 257)):
        for h in (65, 129):
            raw = _raw(rng, h, rb)
            good = _sound("", bpp, rb, h, raw, rng.integers(0, 5, size=h))
            for row in (0, 64, h - 1):
                for byte in (5, 255):
                    s = bytearray(good.stream)
                    s[row * (1 + rb)] = byte
                    out.append(Case("filter-byte %d row %d bpp%d rb%d h%d" % (byte, row, bpp, rb, h), bpp, rb, h, bytes(s), E_FILTER, row, byte, good.rows[:row]))
            for whole, extra in ((0, 0), (0, rb), (63, 1 + rb // 2), (64, 0), (64, rb), (h - 1, 0), (h - 1, rb)):
                cut = whole * (1 + rb) + extra
                out.append(Case("cut at %d+%d bpp%d rb%d h%d" % (whole, extra, bpp, rb, h), bpp, rb, h, good.stream[:cut], E_TRUNCATED, whole, 0, good.rows[:whole]))
            s = bytearray(good.stream[:64 * (1 + rb) + 1])  # a bad filter byte in a whole row wins; one in the cut row is not looked at
            s[3 * (1 + rb)] = 9
            out.append(Case("cut and filter-byte bpp%d rb%d h%d" % (bpp, rb, h), bpp, rb, h, bytes(s), E_FILTER, 3, 9, good.rows[:3]))
            s = bytearray(good.stream[:64 * (1 + rb) + 1])
            s[64 * (1 + rb)] = 9
            out.append(Case("filter-byte in the cut row bpp%d rb%d h%d" % (bpp, rb, h), bpp, rb, h, bytes(s), E_TRUNCATED, 64, 0, good.rows[:64]))
    return out


def empty_case() -> Case:
    return Case("empty", 1, 7, 0, b"", 0, 0, 0, [])


FILL = 0xCD


@dataclass
class Batch:
    cases: List[Case]
    src: np.ndarray
    src_off: np.ndarray
    src_len: np.ndarray
    dst_want: np.ndarray     # the whole destination as it must be afterwards: FILL wherever nothing is delivered
    dst_off: np.ndarray
    stride: np.ndarray
    row_bytes: np.ndarray
    height: np.ndarray
    bpp: np.ndarray
    status: np.ndarray
    detail: np.ndarray


def batch(cases: List[Case], stride_extra: int = 5) -> Batch:
    """One call's arrays: src_off at every misalignment 0-3 in turn, dst_off off the 16-byte boundaries, dst_stride = row_bytes +
    stride_extra, FILL between the rows and between the extents."""
    n = len(cases)
    src_off, dst_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    s_at, d_at = 0, 0
    for i, c in enumerate(cases):
        s_at = (s_at + 3) // 4 * 4 + i % 4
        src_off[i] = s_at
        s_at += len(c.stream) + 2
        d_at = (d_at + 15) // 16 * 16 + (1, 7, 12, 3, 0)[i % 5]
        dst_off[i] = d_at
        d_at += c.height * (c.row_bytes + stride_extra) + 6
    src = np.full(s_at + 8, 0xEE, np.uint8)
    dst = np.full(d_at + 32, FILL, np.uint8)
    for i, c in enumerate(cases):
        src[int(src_off[i]):int(src_off[i]) + len(c.stream)] = np.frombuffer(c.stream, np.uint8)
        for r, row in enumerate(c.rows):
            at = int(dst_off[i]) + r * (c.row_bytes + stride_extra)
            dst[at:at + c.row_bytes] = np.frombuffer(row, np.uint8)
    return Batch(cases, src, src_off, np.array([len(c.stream) for c in cases], np.uint64), dst, dst_off,
                 np.array([c.row_bytes + stride_extra for c in cases], np.uint64), np.array([c.row_bytes for c in cases], np.uint32),
                 np.array([c.height for c in cases], np.uint32), np.array([c.bpp for c in cases], np.uint8),
                 np.array([c.status for c in cases], np.int32), np.array([[c.d0, c.d1] for c in cases], np.uint32).reshape(n, 2))


def first_difference(got: np.ndarray, b: Batch) -> Optional[str]:
    """None, or which image (or gap) of the batch differs from what must be there."""
    if np.array_equal(got, b.dst_want):
        return None
    at = int(np.flatnonzero(got != b.dst_want)[0])
    i = int(np.searchsorted(b.dst_off, at, side="right")) - 1
    name = b.cases[i].name if i >= 0 else "(in front of the first extent)"
    return "byte %d (%s, %d behind its dst_off): %#x, not %#x" % (at, name, at - int(b.dst_off[max(i, 0)]), int(got[at]), int(b.dst_want[at]))
