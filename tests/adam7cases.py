"""Shared by the Adam7 tests (no GPU): a plain-Python REFERENCE of Adam7 interlacing written from the PNG specification (section 8.2)
alone -- split() takes an image apart into its seven reduced images by the 8 x 8 pattern of the specification, weave() puts reduced
images back by the passes' starts and steps -- which shares nothing with pure_zlib_amd/csrc/adam7_core.h; an interlaced PNG WRITER
over pngcases.filter_stream and pngcases.chunk, each pass filtered on its own; and the cases of pzg_adam7_many that the CPU model
(tests/test_model_adam7.py), the sanitizer program (tests/test_sanitized_adam7.py) and the device (tests/test_gpu_adam7.py) all run:
the smallest shapes at which the kernel can go wrong."""
import functools
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import pngcases as PC

E_FILTER = 23
BAD_ARGS = 0xffffffff
PIXEL_BITS = (1, 2, 4, 8, 16, 24, 32, 48, 64)
ROW_SLICES = 16  # Adam7::SLICES of adam7_core.h: the waves that share an image's rows (tests/test_model_adam7.py holds the two together)
FILL = PC.FILL

# PNG specification, section 8.2: the pass of each pixel of an 8 x 8 tile
PATTERN = ((1, 6, 4, 6, 2, 6, 4, 6),
           (7, 7, 7, 7, 7, 7, 7, 7),
           (5, 6, 5, 6, 5, 6, 5, 6),
           (7, 7, 7, 7, 7, 7, 7, 7),
           (3, 6, 4, 6, 3, 6, 4, 6),
           (7, 7, 7, 7, 7, 7, 7, 7),
           (5, 6, 5, 6, 5, 6, 5, 6),
           (7, 7, 7, 7, 7, 7, 7, 7))
# ... and the same as the starts and steps of the passes: (x0, y0, dx, dy)
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def row_bytes_of(width, bits):
    return (width * bits + 7) // 8


def pass_sizes(width, height, bits):
    """[(pw, ph, prb)] of the seven passes; a pass without pixels is (0, 0, 0)."""
    out = []
    for x0, y0, dx, dy in PASSES:
        pw, ph = max(0, -(-(width - x0) // dx)), max(0, -(-(height - y0) // dy))
        out.append((pw, ph, row_bytes_of(pw, bits)) if pw and ph else (0, 0, 0))
    return out


def extent(width, height, bits):
    return sum(ph * prb for _pw, ph, prb in pass_sizes(width, height, bits))


# ---- pixels <-> packed rows ----------------------------------------------------------------------------------------------------------
def unpack(rows: np.ndarray, width: int, bits: int) -> np.ndarray:
    """(h, row_bytes) uint8 -> (h, width, k) uint8: a pixel is k = bits / 8 bytes, or below 8 bits its `bits` bits, one a byte."""
    h = rows.shape[0]
    if bits >= 8:
        return rows.reshape(h, width, bits // 8)
    return np.unpackbits(rows, axis=1)[:, :width * bits].reshape(h, width, bits)


def pack(pix: np.ndarray, bits: int, rng=None) -> np.ndarray:
    """The inverse: (h, row_bytes).  The padding bits of a row's last byte are 0, or random with a generator."""
    h, w = pix.shape[:2]
    if bits >= 8:
        return np.ascontiguousarray(pix).reshape(h, w * (bits // 8))
    flat = pix.reshape(h, w * bits)
    padding = -(w * bits) % 8
    tail = rng.integers(0, 2, size=(h, padding), dtype=np.uint8) if rng is not None else np.zeros((h, padding), np.uint8)
    return np.packbits(np.hstack([flat, tail]), axis=1)


# ---- the reference: PNG specification 8.2 ------------------------------------------------------------------------------------------------
def split(pix: np.ndarray) -> List[Optional[np.ndarray]]:
    """The seven reduced images of (h, w, k) pixels, by the pattern: pass p is the pixels the pattern gives p, row by row."""
    h, w = pix.shape[:2]
    out = []
    for p in range(1, 8):
        ys = [y for y in range(h) if p in PATTERN[y & 7]]
        xs = [x for x in range(w) if ys and PATTERN[ys[0] & 7][x & 7] == p]
        out.append(pix[np.ix_(ys, xs)] if ys and xs else None)
    return out


def weave(stream: bytes, width: int, height: int, bits: int) -> np.ndarray:
    """(height, row_bytes): the image of the dense reduced images in `stream`, by the passes' starts and steps."""
    k = bits // 8 if bits >= 8 else bits
    pix = np.zeros((height, width, k), np.uint8)
    at = 0
    for (x0, y0, dx, dy), (pw, ph, prb) in zip(PASSES, pass_sizes(width, height, bits)):
        if not pw:
            continue
        rows = np.frombuffer(stream, np.uint8, ph * prb, at).reshape(ph, prb)
        pix[y0::dy, x0::dx] = unpack(rows, pw, bits)
        at += ph * prb
    assert at == len(stream)
    return pack(pix, bits)


def interlace(raw: np.ndarray, width: int, bits: int, rng=None) -> List[Optional[np.ndarray]]:
    """The reduced images of the image whose rows are `raw`, as packed rows (padding bits random with a generator)."""
    return [None if p is None else pack(p, bits, rng) for p in split(unpack(raw, width, bits))]


# ---- the writer ------------------------------------------------------------------------------------------------------------------------
def write_png(width, height, color_type, depth, raw: np.ndarray, filters="adaptive", idat=None, level=6, stream_edit=None, palette=None,
              trns=None) -> bytes:
    """An Adam7 PNG of the image whose rows are raw (height, row_bytes), as pngcases.write_png writes a plain one: each pass is
    filtered on its own -- filters: one type for all rows, "adaptive", or a function of a pass's height that gives its rows' types --
    and the seven streams are compressed as one.  stream_edit: as there."""
    bits = PC.CHANNELS[color_type] * depth
    rb, bpp = PC.geometry(width, color_type, depth)
    assert raw.shape == (height, rb)
    stream = b""
    for p in interlace(raw, width, bits):
        if p is not None:
            stream += PC.filter_stream(p, bpp, filters(p.shape[0]) if callable(filters) else filters)
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
    out = b"\x89PNG\r\n\x1a\n" + PC.chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, 0, 0, 1))
    if color_type == 3 or palette is not None:
        out += PC.chunk(b"PLTE", palette if palette is not None else bytes(range(48)))
    if trns is not None:
        out += PC.chunk(b"tRNS", trns)
    for piece in ([z] if idat is None else [z[i:i + idat] for i in range(0, len(z), idat)]):
        out += PC.chunk(b"IDAT", piece)
    return out + PC.chunk(b"IEND", b"")


def filtered_pass_offsets(width, height, bits):
    """Where each pass starts in the FILTERED stream of an interlaced image (None: an empty pass), and the stream's length."""
    at, out = 0, []
    for pw, ph, prb in pass_sizes(width, height, bits):
        out.append(at if pw else None)
        at += ph * (1 + prb)
    return out, at


# ---- the cases of pzg_adam7_many -------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    width: int
    height: int
    bits: int
    src: bytes               # the reduced images, dense, in pass order
    status: int              # what the call must answer
    d0: int
    d1: int
    rows: List[bytes]        # the rows it must deliver (none where status is not 0)

    @property
    def row_bytes(self):
        return row_bytes_of(self.width, self.bits)


def _case(rng, name, w, h, bits) -> Case:
    raw = rng.integers(0, 256, size=(h, row_bytes_of(w, bits)), dtype=np.uint8)
    if bits < 8 and (w * bits) % 8:
        raw[:, -1] &= (0xff << (8 - (w * bits) % 8)) & 0xff
    src = b"".join(p.tobytes() for p in interlace(raw, w, bits, rng) if p is not None)
    assert len(src) == extent(w, h, bits), name
    assert np.array_equal(weave(src, w, h, bits), raw), name  # the two halves of the reference agree
    return Case(name, w, h, bits, src, 0, 0, 0, [r.tobytes() for r in raw])


@functools.lru_cache(maxsize=None)
def small_cases() -> List[Case]:
    """Every (w, h) in 1..9 x 1..9 for each pixel_bits: every combination of empty passes (729 images)."""
    rng = np.random.default_rng(20261020)
    return [_case(rng, "%dx%d bits%d" % (w, h, bits), w, h, bits) for bits in PIXEL_BITS for w in range(1, 10) for h in range(1, 10)]


@functools.lru_cache(maxsize=None)
def edge_cases() -> List[Case]:
    """For every pixel_bits 67 x 65, 33 x 131 (passes 6 and 7 have 66 and 65 rows) and 257 x 10; one narrow image taller than one
    round of the kernel's row slices."""
    rng = np.random.default_rng(8)
    out = [_case(rng, "%dx%d bits%d" % (w, h, bits), w, h, bits) for bits in PIXEL_BITS for w, h in ((67, 65), (33, 131), (257, 10))]
    h = 2 * ROW_SLICES + 5
    out.append(_case(rng, "3x%d bits24, taller than a round of the %d row slices" % (h, ROW_SLICES), 3, h, 24))
    return out


def all_cases() -> List[Case]:
    return small_cases() + edge_cases()


def empty_cases() -> List[Case]:
    return [Case("no width", 0, 5, 8, b"", 0, 0, 0, []), Case("no height", 5, 0, 24, b"", 0, 0, 0, [])]


def bad_geometry_cases() -> List[Case]:
    """What the device refuses: nothing of such an image is read or written (its source is not even there)."""
    out = [Case("bits %d" % b, 5, 3, b, b"", E_FILTER, BAD_ARGS, b, []) for b in (0, 3, 12, 40, 65, 255)]
    out.append(Case("width 2^31", 1 << 31, 1, 8, b"", E_FILTER, BAD_ARGS, 8, []))
    out.append(Case("height 2^31", 1, 1 << 31, 8, b"", E_FILTER, BAD_ARGS, 8, []))
    return out


@dataclass
class Batch:
    cases: List[Case]
    src: np.ndarray
    src_off: np.ndarray
    dst_want: np.ndarray     # the whole destination as it must be afterwards: FILL wherever nothing is delivered
    dst_off: np.ndarray
    stride: np.ndarray
    width: np.ndarray
    height: np.ndarray
    bits: np.ndarray
    status: np.ndarray
    detail: np.ndarray


def stride_of(c: Case, stride_extra: int) -> int:
    """row_bytes + stride_extra; of an image that cannot be laid out (2^31 pixels a side) just that of one pixel a row."""
    return (c.row_bytes if c.width < 1 << 31 else 1) + stride_extra


def batch(cases: List[Case], stride_extra: int = 5) -> Batch:
    """One call's arrays, laid out as pngcases.batch lays out the unfilter's: src_off at every misalignment 0-3 in turn, dst_off off
    the 16-byte boundaries, dst_stride = row_bytes + stride_extra, FILL between the rows and between the extents."""
    n = len(cases)
    src_off, dst_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    s_at, d_at = 0, 0
    for i, c in enumerate(cases):
        s_at = (s_at + 3) // 4 * 4 + i % 4
        src_off[i] = s_at
        s_at += len(c.src) + 2
        d_at = (d_at + 15) // 16 * 16 + (1, 7, 12, 3, 0)[i % 5]
        dst_off[i] = d_at
        d_at += len(c.rows) * stride_of(c, stride_extra) + 6
    src = np.full(s_at + 8, 0xEE, np.uint8)
    dst = np.full(d_at + 32, FILL, np.uint8)
    for i, c in enumerate(cases):
        src[int(src_off[i]):int(src_off[i]) + len(c.src)] = np.frombuffer(c.src, np.uint8)
        for r, row in enumerate(c.rows):
            at = int(dst_off[i]) + r * stride_of(c, stride_extra)
            dst[at:at + len(row)] = np.frombuffer(row, np.uint8)
    return Batch(cases, src, src_off, dst, dst_off, np.array([stride_of(c, stride_extra) for c in cases], np.uint64),
                 np.array([c.width for c in cases], np.uint32), np.array([c.height for c in cases], np.uint32),
                 np.array([c.bits for c in cases], np.uint8), np.array([c.status for c in cases], np.int32),
                 np.array([[c.d0, c.d1] for c in cases], np.uint32).reshape(n, 2))


def first_difference(got: np.ndarray, b: Batch) -> Optional[str]:
    """None, or which image (or gap) of the batch differs from what must be there."""
    if np.array_equal(got, b.dst_want):
        return None
    at = int(np.flatnonzero(got != b.dst_want)[0])
    i = int(np.searchsorted(b.dst_off, at, side="right")) - 1
    name = b.cases[i].name if i >= 0 else "(in front of the first extent)"
    return "byte %d (%s, %d behind its dst_off): %#x, not %#x" % (at, name, at - int(b.dst_off[max(i, 0)]), int(got[at]), int(b.dst_want[at]))
