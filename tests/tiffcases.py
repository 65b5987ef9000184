"""Shared by the TIFF tests (no GPU): a plain-numpy REFERENCE for pzg_unpredict_many written from the rules include/pzg.h states -- np.cumsum
along the row at the sample's dtype in the file's byte order, then the window; it shares nothing with pure_zlib_amd/csrc/unpredict_core.h
-- the cases that the CPU model (tests/test_model_unpredict.py), the sanitized program (tests/test_sanitized_unpredict.py) and the
device (tests/test_gpu_unpredict.py) all run, and a TIFF WRITER from numpy and the system's zlib (II / MM, classic and BigTIFF, strips
and tiles, Predictor 1 / 2, PlanarConfiguration 1 / 2, Compression 8 / 32946, several pages) for tests/test_gpu_tiff.py.
The kernel goes wrong at edges, not at size: every sample width and pixel size in both byte orders at widths around the run, the
wave and one past a wave's reach, heights around the rows a wave takes at once, every source misalignment, destinations off the
dword and 16-byte boundaries, padded strides, windows clipped on every side, sources cut short, empty jobs, illegal geometry."""
import functools
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

OK, E_TRUNCATED, E_FILTER = 0, 1, 23
BAD_ARGS = 0xffffffff
FILL = 0xCD
LANES = 64

SAMPLE_BYTES = (1, 2, 4, 8)
SAMPLES = (1, 2, 3, 4)
WIDTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 129)  # pixels; one more per pixel size: one past a wave's reach (reach_pixels() + 1)

# pzg_unpredict_desc, stated a second time (include/pzg.h gives the offsets)
DESC = np.dtype({"names": ["src_off", "dst_off", "dst_stride", "src_row_bytes", "rows", "win_row", "win_rows", "win_byte", "win_bytes", "predictor",
                           "sample_bytes", "samples", "big_endian"],
                 "formats": ["<u8", "<u8", "<u8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "u1", "u1", "u1", "u1"],
                 "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 49, 50, 51], "itemsize": 64})


def run_bytes(sb: int, s: int) -> int:
    """The bytes of a row a lane owns: lcm(16, the bytes of a pixel), as unpredict_core.h states it (the model says so:
    tests/test_model_unpredict.py holds pzu_run() against this)."""
    p = sb * s
    return 48 if p % 3 == 0 else 32 if p > 16 else 16


def reach_pixels(sb: int, s: int) -> int:
    """The pixels of a row one wave reaches at once."""
    return LANES * run_bytes(sb, s) // (sb * s)


def rows_per_wave(row_bytes: int, sb: int, s: int) -> int:
    return LANES // min(LANES, -(-row_bytes // run_bytes(sb, s)))


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def sample_dtype(sb: int, big_endian: bool) -> np.dtype:
    return np.dtype("u1") if sb == 1 else np.dtype((">" if big_endian else "<") + "u%d" % sb)


def reconstruct(stored: np.ndarray, predictor: int, sb: int, s: int, big_endian: bool) -> np.ndarray:
    """stored: (rows, row_bytes) uint8 as the strip or tile decodes.  The reconstructed rows, the same shape: with predictor 2 the
    running sum of every channel along the row, modulo 2^(8 sb), taken and written in the file's byte order."""
    stored = np.ascontiguousarray(stored, np.uint8)
    if predictor != 2 or stored.size == 0:
        return stored.copy()
    rows = stored.shape[0]
    dt = sample_dtype(sb, big_endian)
    a = stored.view(dt).reshape(rows, -1, s).astype("u%d" % sb)  # native integers
    out = np.cumsum(a, axis=1, dtype="u%d" % sb).astype(dt)      # (an unsigned sum wraps)
    return out.reshape(rows, -1).view(np.uint8).reshape(stored.shape).copy()


def difference(actual: np.ndarray, sb: int, s: int, big_endian: bool) -> np.ndarray:
    """What a writer stores for the rows `actual` (rows, row_bytes) uint8 with predictor 2."""
    rows = actual.shape[0]
    dt = sample_dtype(sb, big_endian)
    a = np.ascontiguousarray(actual, np.uint8).view(dt).reshape(rows, -1, s).astype("u%d" % sb)
    d = a.copy()
    d[:, 1:] = a[:, 1:] - a[:, :-1]
    return d.astype(dt).reshape(rows, -1).view(np.uint8).reshape(actual.shape).copy()


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    predictor: int
    sb: int
    s: int
    big_endian: int
    stored: np.ndarray             # (rows, src_row_bytes) uint8; (0, 0) where the job has no stored byte
    rows: int                      # what the descriptor says (stored.shape where the job is sound)
    srb: int
    window: Tuple[int, int, int, int]  # win_row, win_rows, win_byte, win_bytes
    src_len: Optional[int] = None  # None: rows * srb
    status: int = OK
    d0: int = 0
    d1: int = 0
    dst_short: int = 0             # the stride falls this much short of win_bytes (illegal geometry)

    @property
    def legal(self):
        return self.status in (OK, E_TRUNCATED)

    @property
    def slen(self):
        return self.rows * self.srb if self.src_len is None else self.src_len

    @property
    def readable(self):
        """The bytes of the source the job may read."""
        return min(self.slen, self.stored.size) if self.legal else 0

    def delivered(self) -> np.ndarray:
        """(rows delivered, win_bytes) uint8: the window's rows that lie wholly inside src_len, from the reference."""
        wr, wn, wb, wbn = self.window
        if not self.legal or wn == 0 or wbn == 0 or self.srb == 0 or self.rows == 0:
            return np.zeros((0, wbn), np.uint8)
        inside = min(self.rows, self.slen // self.srb)
        end = min(wr + wn, inside)
        if end <= wr:
            return np.zeros((0, wbn), np.uint8)
        return reconstruct(self.stored[wr:end], self.predictor, self.sb, self.s, bool(self.big_endian))[:, wb:wb + wbn]


def window_of(kind: int, rows: int, srb: int, pixel: int, i: int) -> Tuple[int, int, int, int]:
    """0 full; 1 right and bottom clipped; 2 left and top clipped by an odd number of bytes; 3 one pixel (or, every other time, one
    byte) in the last corner."""
    if kind == 0:
        return 0, rows, 0, srb
    if kind == 1:
        return 0, max(1, rows - 1 - i % 2), 0, max(1, srb - (1, 3, pixel, 5)[i % 4])
    if kind == 2:
        top, left = min(rows - 1, 1 + i % 2), min(srb - 1, (1, 3, 5, 7)[i % 4])
        return top, rows - top, left, srb - left
    one = pixel if i % 2 == 0 else 1
    return rows - 1, 1, srb - one, one


def _random_stored(rng, rows, srb):
    """Uniformly random bytes: the samples are uniform over their full range, sums wrap and carries cross every byte."""
    return rng.integers(0, 256, size=(rows, srb), dtype=np.uint8)


def _heights(srb, sb, s):
    rpw = rows_per_wave(srb, sb, s)
    return (1, 2, max(1, rpw - 1), rpw + 1)


@functools.lru_cache(maxsize=None)
def shape_cases() -> List[Case]:
    """Predictor 2: every sample width x pixel size x byte order at every width, the heights and the windows in turn; predictor 1 at
    every width for four pixel sizes."""
    rng = np.random.default_rng(20261021)
    out, i = [], 0
    for sb in SAMPLE_BYTES:
        for s in SAMPLES:
            for be in (0, 1):
                for w in WIDTHS + (reach_pixels(sb, s) + 1,):
                    srb = w * sb * s
                    rows = _heights(srb, sb, s)[i % 4]
                    win = window_of((i // 4 + i) % 4, rows, srb, sb * s, i)
                    out.append(Case("p2 sb%d s%d be%d %dx%d win%s" % (sb, s, be, w, rows, win), 2, sb, s, be, _random_stored(rng, rows, srb), rows, srb, win))
                    i += 1
    for sb, s in ((1, 1), (1, 3), (2, 4), (8, 3)):
        for w in WIDTHS + (reach_pixels(1, 1) // (sb * s) + 1,):
            srb = w * sb * s
            rows = _heights(srb, 1, 1)[i % 4]
            win = window_of((i // 4 + i) % 4, rows, srb, sb * s, i)
            out.append(Case("p1 sb%d s%d %dx%d win%s" % (sb, s, w, rows, win), 1, sb, s, i % 2, _random_stored(rng, rows, srb), rows, srb, win))
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def special_cases() -> List[Case]:
    rng = np.random.default_rng(8)
    out = []
    # every height and every window at two widths of the common formats
    for sb, s in ((1, 3), (2, 1), (1, 4), (4, 1)):
        for w in (5, 65):
            srb = w * sb * s
            for rows in sorted(set(_heights(srb, sb, s))):
                for kind in range(4):
                    win = window_of(kind, rows, srb, sb * s, len(out))
                    out.append(Case("heights sb%d s%d %dx%d win%s" % (sb, s, w, rows, win), 2, sb, s, len(out) % 2, _random_stored(rng, rows, srb), rows, srb, win))
    # the carry's direction: 0x..00ff, then deltas of +1, in both byte orders -- and down again with deltas of -1
    for sb in (2, 4, 8):
        for be in (0, 1):
            dt = sample_dtype(sb, bool(be))
            up = np.array([[0xff] + [1] * 20, [(1 << (8 * sb)) - 0x100] + [(1 << (8 * sb)) - 1] * 20], "u%d" % sb).astype(dt)
            stored = up.view(np.uint8).reshape(2, -1)
            c = Case("carry sb%d be%d" % (sb, be), 2, sb, 1, be, stored, 2, stored.shape[1], (0, 2, 0, stored.shape[1]))
            got = c.delivered().view(dt).reshape(2, -1)
            assert [int(v) for v in got[0, :3]] == [0xff, 0x100, 0x101] and int(got[1, 1]) == (1 << (8 * sb)) - 0x101
            out.append(c)
    # long rows: several chunks of a wave's reach, the sums and the last dword carried over each boundary; a strip of many rows
    for sb, s, be in ((1, 3, 0), (2, 1, 1), (1, 4, 0), (8, 4, 1), (4, 3, 0)):
        w = 2 * reach_pixels(sb, s) + 3
        srb = w * sb * s
        out.append(Case("long sb%d s%d be%d %dx3" % (sb, s, be, w), 2, sb, s, be, _random_stored(rng, 3, srb), 3, srb, window_of(len(out) % 3, 3, srb, sb * s, 1)))
    out.append(Case("many rows rgb8 7x300", 2, 1, 3, 0, _random_stored(rng, 300, 21), 300, 21, (3, 295, 2, 17)))
    out.append(Case("many rows copy 40x300", 1, 1, 1, 0, _random_stored(rng, 300, 40), 300, 40, (0, 300, 0, 40)))
    # a source that holds more than the job
    out.append(Case("src_len beyond the job", 2, 2, 3, 1, _random_stored(rng, 4, 54), 4, 54, (0, 4, 0, 54), src_len=4 * 54 + 5))
    return out


@functools.lru_cache(maxsize=None)
def truncated_cases() -> List[Case]:
    """src_len cut in the middle of a row and at a row boundary: d0 is the rows wholly inside, those of the window are delivered."""
    rng = np.random.default_rng(9)
    out = []
    for sb, s, be, w, rows in ((1, 3, 0, 17, 9), (2, 2, 1, 65, 5), (4, 1, 0, 33, 70), (1, 1, 0, 700, 4)):
        srb = w * sb * s
        stored = _random_stored(rng, rows, srb)
        for cut_rows, extra in ((rows - 1, srb // 2), (rows - 2, 0), (0, srb - 1), (0, 0), (1, 1)):
            for win in ((0, rows, 0, srb), (1, rows - 1, 3, srb - 4)):
                slen = cut_rows * srb + extra
                out.append(Case("cut sb%d s%d %dx%d at %d+%d win%s" % (sb, s, w, rows, cut_rows, extra, win), 2 if len(out) % 3 else 1, sb, s, be, stored, rows, srb, win,
                                src_len=slen, status=E_TRUNCATED, d0=cut_rows))
    return out


def empty_cases() -> List[Case]:
    none = np.zeros((0, 0), np.uint8)
    some = np.arange(12, dtype=np.uint8).reshape(2, 6)
    return [Case("no rows", 2, 1, 3, 0, none, 0, 6, (0, 0, 0, 6)), Case("no bytes", 2, 1, 3, 0, none, 2, 0, (0, 2, 0, 0)),
            Case("no window rows", 2, 1, 3, 0, some, 2, 6, (1, 0, 0, 6)), Case("no window bytes", 2, 1, 3, 0, some, 2, 6, (0, 2, 3, 0)),
            Case("no rows of an illegal predictor", 7, 3, 9, 0, none, 0, 6, (0, 0, 0, 6))]


def bad_geometry_cases() -> List[Case]:
    """Every illegal geometry include/pzg.h names: PZG_E_FILTER with (0xffffffff, predictor << 16 | sample_bytes << 8 | samples),
    nothing read or written."""
    none = np.zeros((0, 0), np.uint8)

    def mk(name, predictor=2, sb=1, s=3, rows=3, srb=12, win=(0, 3, 0, 12), **kw):
        return Case(name, predictor, sb, s, 0, none, rows, srb, win, status=E_FILTER, d0=BAD_ARGS, d1=predictor << 16 | sb << 8 | s, **kw)
    return [mk("predictor 0", predictor=0), mk("predictor 3", predictor=3), mk("predictor 255", predictor=255),
            mk("sample_bytes 0", sb=0), mk("sample_bytes 3", sb=3), mk("sample_bytes 16", sb=16), mk("sample_bytes 3 with predictor 1", predictor=1, sb=3),
            mk("samples 0", s=0), mk("samples 5", s=5), mk("samples 5 with predictor 1", predictor=1, s=5),
            mk("row no multiple of the pixel", srb=13, win=(0, 3, 0, 13)), mk("row no multiple of the pixel, 16-bit rgba", sb=2, s=4, srb=12),
            mk("window below the job", win=(1, 3, 0, 12)), mk("window's first row outside", win=(3, 1, 0, 12)),
            mk("window's rows wrap", win=(0xffffffff, 2, 0, 12)), mk("window right of the row", win=(0, 3, 1, 12)),
            mk("window's first byte outside", win=(0, 3, 12, 1)), mk("window's bytes wrap", win=(0, 3, 0xffffffff, 2)),
            mk("dst stride one short", dst_short=1), mk("dst stride one short, copy", predictor=1, sb=1, s=1, dst_short=1)]


def all_cases() -> List[Case]:
    return shape_cases() + special_cases() + truncated_cases() + empty_cases() + bad_geometry_cases()


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
DST_OFFS = (0, 1, 3, 7, 12, 16, 2)


def layout_of(i: int) -> Tuple[int, int, int]:
    """(source misalignment, destination offset modulo 16, what the destination stride adds to win_bytes)"""
    return i % 4, DST_OFFS[i % 7], (5, 0, 1, 16)[(i // 2) % 4]


def stride_of(c: Case, extra: int) -> int:
    return c.window[3] - c.dst_short if c.dst_short else c.window[3] + extra


def descriptor(c: Case, src_off, dst_off, dst_stride) -> np.ndarray:
    d = np.zeros(1, DESC)
    d["src_off"], d["dst_off"], d["dst_stride"], d["src_row_bytes"], d["rows"] = src_off, dst_off, dst_stride, c.srb, c.rows
    d["win_row"], d["win_rows"], d["win_byte"], d["win_bytes"] = c.window
    d["predictor"], d["sample_bytes"], d["samples"], d["big_endian"] = c.predictor, c.sb, c.s, c.big_endian
    return d


def source_bytes(c: Case) -> np.ndarray:
    return c.stored.reshape(-1)[:c.readable].copy()


def paint(want: np.ndarray, c: Case, dst_off: int, dst_stride: int):
    got = c.delivered()
    for r in range(got.shape[0]):
        want[dst_off + r * dst_stride:dst_off + r * dst_stride + got.shape[1]] = got[r]


def extent_rows(c: Case) -> int:
    return c.window[1] if c.legal and c.window[3] and c.srb and c.rows else 0


def single(c: Case, i: int):
    """One job alone, for the model and the sanitized program: (desc, the source bytes it may read, mis, want) with the destination of
    len(want) bytes, the window at desc.dst_off in it and 9 bytes behind it."""
    mis, doff, extra = layout_of(i)
    stride = stride_of(c, extra)
    want = np.full(doff + extent_rows(c) * stride + 9, FILL, np.uint8)
    paint(want, c, doff, stride)
    return descriptor(c, 0, doff, stride), source_bytes(c), mis, want


@dataclass
class Batch:
    cases: List[Case]
    src: np.ndarray
    src_len: np.ndarray
    desc: np.ndarray
    dst_want: np.ndarray
    dst_off: np.ndarray


def batch(cases: List[Case], shift: int = 0) -> Batch:
    """One call's arrays: the layouts of layout_of(i + shift), 0xEE between the sources, FILL between the rows and between the extents."""
    n = len(cases)
    desc = np.zeros(n, DESC)
    srcs, places, s_at, d_at = [], [], 0, 0
    for i, c in enumerate(cases):
        mis, doff, extra = layout_of(i + shift)
        stride = stride_of(c, extra)
        sb = source_bytes(c)
        s_at = (s_at + 3) // 4 * 4 + mis
        d_at = (d_at + 15) // 16 * 16 + doff
        desc[i] = descriptor(c, s_at, d_at, stride)[0]
        srcs.append((s_at, sb))
        places.append((d_at, stride))
        s_at += len(sb) + 2
        d_at += extent_rows(c) * stride + 6
    src = np.full(s_at + 8, 0xEE, np.uint8)
    for at, sb in srcs:
        src[at:at + len(sb)] = sb
    want = np.full(d_at + 32, FILL, np.uint8)
    for c, (at, stride) in zip(cases, places):
        paint(want, c, at, stride)
    return Batch(cases, src, np.array([c.slen for c in cases], np.uint64), desc, want, np.array([p[0] for p in places], np.uint64))


def first_difference(got: np.ndarray, b: Batch) -> Optional[str]:
    diff = got != b.dst_want
    if not diff.any():
        return None
    at = int(np.flatnonzero(diff)[0])
    i = int(np.searchsorted(b.dst_off, at, side="right")) - 1
    name = b.cases[i].name if i >= 0 else "(in front of the first extent)"
    return "byte %d (%s, %d behind its dst_off): %#x, not %#x" % (at, name, at - int(b.dst_off[max(i, 0)]), int(got[at]), int(b.dst_want[at]))


# ---- the TIFF writer --------------------------------------------------------------------------------------------------------------------
@dataclass
class Page:
    """One image to write.  data: (H, W, S) of the sample's dtype (any byte order: the writer stores the file's); or, bits < 8,
    (H, ceil(W * bits / 8)) uint8 packed rows with `width` given."""
    data: np.ndarray
    tile: Optional[Tuple[int, int]] = None   # (TileWidth, TileLength); None: strips
    rows_per_strip: Optional[int] = None     # None: the whole image (the tag is left out)
    predictor: int = 1
    planar: int = 1
    compression: int = 8
    bits: Optional[int] = None
    width: Optional[int] = None
    sample_format: Optional[int] = None      # None: by dtype (1 unsigned, 2 signed, 3 float)
    photometric: Optional[int] = None
    extra_samples: Tuple[int, ...] = ()
    colormap: Optional[np.ndarray] = None    # (3 << bits,) uint16
    orientation: Optional[int] = None
    fill_order: Optional[int] = None
    subsampling: Optional[Tuple[int, int]] = None
    level: int = 6
    more_tags: Tuple[Tuple[int, int, Tuple[int, ...]], ...] = ()  # (tag, type, values) written as they stand
    edit: Optional[object] = None            # edit(k, stream) -> the bytes stored for strip / tile k


SHORT, LONG, LONG8 = 3, 4, 16
_TYPE_FMT = {1: "B", 3: "H", 4: "I", 16: "Q"}


def _chunks(p: Page, big_endian: bool, rng) -> Tuple[List[bytes], dict]:
    """The strips or tiles of a page as they are compressed, in the file's order, and the page's geometry."""
    packed = p.bits is not None and p.bits < 8
    if packed:
        h, w, s, bits = p.data.shape[0], p.width, 1, p.bits
        sb, raw = 1, np.ascontiguousarray(p.data, np.uint8).reshape(h, -1, 1)
    else:
        h, w, s = p.data.shape
        sb, bits = p.data.dtype.itemsize, 8 * p.data.dtype.itemsize
        raw = np.ascontiguousarray(p.data.astype(p.data.dtype.newbyteorder(">" if big_endian else "<"))).view(np.uint8).reshape(h, -1, s * sb)
        raw = raw.reshape(h, w, s, sb)
    planes = [raw] if p.planar == 1 or packed else [raw[:, :, k:k + 1] for k in range(s)]
    ps = s if p.planar == 1 else 1  # the samples of a stored pixel
    out = []
    for plane in planes:
        rows = plane.reshape(h, -1)  # (H, row bytes)
        if p.tile is not None:
            tw, tl = p.tile
            tb = tw * bits * ps // 8 if packed else tw * ps * sb
            for y0 in range(0, h, tl):
                for x0 in range(0, w, tw):
                    b0 = x0 * bits * ps // 8 if packed else x0 * ps * sb
                    t = rng.integers(0, 256, size=(tl, tb), dtype=np.uint8)  # the padding is random, and differenced with the rest
                    part = rows[y0:y0 + tl, b0:b0 + tb]
                    t[:part.shape[0], :part.shape[1]] = part
                    out.append(t)
        else:
            rps = p.rows_per_strip or h
            for y0 in range(0, h, rps):
                out.append(rows[y0:y0 + rps])
    streams = []
    for k, t in enumerate(out):
        stored = difference(t, sb, ps, big_endian) if p.predictor == 2 else t
        z = zlib.compress(stored.tobytes(), p.level)
        streams.append(p.edit(k, z) if p.edit else z)
    fmt = p.sample_format
    if fmt is None:
        fmt = 1 if packed else {"u": 1, "i": 2, "f": 3}[p.data.dtype.kind]
    return streams, dict(width=w, height=h, samples=s, bits=bits, sample_format=fmt)


def write_tiff(pages: List[Page], big_endian: bool = False, bigtiff: bool = False, seed: int = 0) -> bytes:
    """A TIFF file of the pages, each with its own IFD, the data of a page in front of its IFD."""
    rng = np.random.default_rng(seed)
    e = ">" if big_endian else "<"
    buf = bytearray((b"MM" if big_endian else b"II") + (struct.pack(e + "HHHQ", 43, 8, 0, 0) if bigtiff else struct.pack(e + "HI", 42, 0)))
    link = 8 if bigtiff else 4  # where the offset of the next IFD goes
    osz, ofmt, otype = (8, "Q", LONG8) if bigtiff else (4, "I", LONG)
    for p in pages:
        streams, g = _chunks(p, big_endian, rng)
        offsets = []
        for z in streams:
            if len(buf) % 2:
                buf += b"\0"
            offsets.append(len(buf))
            buf += z
        photometric = p.photometric if p.photometric is not None else (3 if p.colormap is not None else 2 if g["samples"] >= 3 else 1)
        tags = [(256, LONG, (g["width"],)), (257, LONG, (g["height"],)), (258, SHORT, (g["bits"],) * g["samples"]), (259, SHORT, (p.compression,)),
                (262, SHORT, (photometric,)), (277, SHORT, (g["samples"],)), (284, SHORT, (p.planar,)), (339, SHORT, (g["sample_format"],) * g["samples"])]
        if p.predictor != 1:
            tags.append((317, SHORT, (p.predictor,)))
        if p.tile is not None:
            tags += [(322, LONG, (p.tile[0],)), (323, LONG, (p.tile[1],)), (324, otype, tuple(offsets)), (325, otype, tuple(len(z) for z in streams))]
        else:
            tags += [(273, otype, tuple(offsets)), (279, otype, tuple(len(z) for z in streams))]
            if p.rows_per_strip is not None:
                tags.append((278, LONG, (p.rows_per_strip,)))
        if p.extra_samples:
            tags.append((338, SHORT, tuple(p.extra_samples)))
        if p.colormap is not None:
            tags.append((320, SHORT, tuple(int(v) for v in p.colormap)))
        if p.orientation is not None:
            tags.append((274, SHORT, (p.orientation,)))
        if p.fill_order is not None:
            tags.append((266, SHORT, (p.fill_order,)))
        if p.subsampling is not None:
            tags.append((530, SHORT, tuple(p.subsampling)))
        tags += list(p.more_tags)
        tags.sort()
        entries = []
        for tag, typ, values in tags:
            body = struct.pack(e + "%d%s" % (len(values), _TYPE_FMT[typ]), *values)
            if len(body) > osz:
                if len(buf) % 2:
                    buf += b"\0"
                at = len(buf)
                buf += body
                body = struct.pack(e + ofmt, at)
            entries.append(struct.pack(e + ("HHQ" if bigtiff else "HHI"), tag, typ, len(values)) + body.ljust(osz, b"\0"))
        if len(buf) % 2:
            buf += b"\0"
        ifd = len(buf)
        buf[link:link + osz] = struct.pack(e + ofmt, ifd)
        buf += struct.pack(e + ("Q" if bigtiff else "H"), len(entries)) + b"".join(entries)
        link = len(buf)
        buf += b"\0" * osz
    return bytes(buf)
