"""Shared by the floating-point predictor's tests (no GPU): a plain-numpy REFERENCE for pzg_unshuffle_many written from the rules
include/pzg.h states -- np.cumsum at uint8 along the row per channel, then the planes, reversed or not, transposed; it shares nothing
with pure_zlib_amd/csrc/unshuffle_core.h -- its inverse, the ENCODER, the cases that the CPU model (tests/test_model_unshuffle.py), the
sanitized program (tests/test_sanitized_unshuffle.py) and the device (tests/test_gpu_unshuffle.py) all run, laid out as
tests/tiffcases.py lays its own out, and the hook that makes tiffcases.write_tiff write Predictor 3 pages.
The kernel goes wrong at edges, not at size: every element size x sum stride x plane order at element counts around a lane's run, a
wave's reach and past it, heights around the rows a wave takes at once, every source misalignment (odd counts make the planes' own
misalignments differ), destinations off the dword and 16-byte boundaries, padded strides, windows clipped on every side and inside
an element, sums that cross every plane and chunk boundary, sources cut short, empty jobs, illegal geometry."""
import functools
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

import tiffcases as T
from tiffcases import BAD_ARGS, E_FILTER, E_TRUNCATED, FILL, LANES, OK, Batch, first_difference, layout_of  # noqa: F401 (the tests take them from here)

ELEM_BYTES = (2, 4, 8)
SUM_STRIDES = (0, 1, 2, 3, 4)
RUN = 8                 # the elements of a row a lane owns, as unshuffle_core.h states it (the model says so: pzs_run())
REACH = LANES * RUN     # the elements of a row one wave reaches at once
COUNTS = (1, 2, 3, RUN - 1, RUN, RUN + 1, REACH - 1, REACH, REACH + 1, 2 * REACH + 3)  # elements; each taken as a multiple of S

# pzg_unshuffle_desc, stated a second time (include/pzg.h gives the offsets)
DESC = np.dtype({"names": ["src_off", "dst_off", "dst_stride", "src_row_bytes", "rows", "win_row", "win_rows", "win_byte", "win_bytes", "elem_bytes",
                           "sum_stride", "reverse", "reserved0"],
                 "formats": ["<u8", "<u8", "<u8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "u1", "u1", "u1", "u1"],
                 "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 49, 50, 51], "itemsize": 64})


def rows_per_wave(n: int) -> int:
    return LANES // min(LANES, -(-n // RUN))


# ---- the reference and the encoder ------------------------------------------------------------------------------------------------------
def reconstruct(stored: np.ndarray, b: int, s: int, reverse: bool) -> np.ndarray:
    """stored: (rows, n * b) uint8 as the strip or tile decodes.  The reconstructed rows, the same shape: the running sum modulo 256 of
    every channel over the whole row (s = 0: none), then the row's b planes of n bytes, the last first where `reverse`, transposed."""
    stored = np.ascontiguousarray(stored, np.uint8)
    if stored.size == 0:
        return stored.copy()
    rows = stored.shape[0]
    t = stored if s == 0 else np.cumsum(stored.reshape(rows, -1, s), axis=1, dtype=np.uint8).reshape(rows, -1)
    planes = t.reshape(rows, b, -1)
    if reverse:
        planes = planes[:, ::-1]
    return np.ascontiguousarray(planes.transpose(0, 2, 1)).reshape(rows, -1)


def encode(actual: np.ndarray, b: int, s: int, reverse: bool) -> np.ndarray:
    """What a writer stores for the rows `actual` (rows, n * b) uint8: the inverse of reconstruct()."""
    actual = np.ascontiguousarray(actual, np.uint8)
    rows = actual.shape[0]
    planes = actual.reshape(rows, -1, b).transpose(0, 2, 1)
    if reverse:
        planes = planes[:, ::-1]
    t = np.ascontiguousarray(planes).reshape(rows, -1)
    if s == 0:
        return t
    a = t.reshape(rows, -1, s)
    d = a.copy()
    d[:, 1:] = a[:, 1:] - a[:, :-1]
    return d.reshape(rows, -1)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    b: int
    s: int
    reverse: int
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
        return reconstruct(self.stored[wr:end], self.b, self.s, bool(self.reverse))[:, wb:wb + wbn]


def _random_stored(rng, rows, srb):
    """Uniformly random bytes: every sum wraps."""
    return rng.integers(0, 256, size=(rows, srb), dtype=np.uint8)


def _count(n: int, s: int) -> int:
    return n if s == 0 else -(-n // s) * s


def _heights(n):
    rpw = rows_per_wave(n)
    return (1, 2, max(1, rpw - 1), rpw + 1)


@functools.lru_cache(maxsize=None)
def shape_cases() -> List[Case]:
    """Every element size x sum stride x plane order at every element count, the heights and the windows in turn."""
    rng = np.random.default_rng(20261021)
    out, i = [], 0
    for b in ELEM_BYTES:
        for s in SUM_STRIDES:
            for rev in (0, 1):
                for n0 in COUNTS:
                    n = _count(n0, s)
                    srb = n * b
                    rows = _heights(n)[i % 4]
                    win = T.window_of((i // 4 + i) % 4, rows, srb, b, i)
                    out.append(Case("b%d s%d rev%d %dx%d win%s" % (b, s, rev, n, rows, win), b, s, rev, _random_stored(rng, rows, srb), rows, srb, win))
                    i += 1
    return out


@functools.lru_cache(maxsize=None)
def special_cases() -> List[Case]:
    rng = np.random.default_rng(8)
    out = []
    # every height and every window at two widths of the common formats
    for b, s in ((4, 1), (4, 3), (2, 1), (8, 1), (4, 0)):
        for n0 in (5, 65):
            n = _count(n0, s)
            srb = n * b
            for rows in sorted(set(_heights(n))):
                for kind in range(4):
                    win = T.window_of(kind, rows, srb, b, len(out))
                    out.append(Case("heights b%d s%d %dx%d win%s" % (b, s, n, rows, win), b, s, len(out) % 2, _random_stored(rng, rows, srb), rows, srb, win))
    # the sum crosses every plane and chunk boundary: only byte 0 of the row is stored non-zero, and every byte of its channel equals it
    for b in ELEM_BYTES:
        for n0 in (6, REACH + 3, 2 * REACH + 3):
            for s in (1, 3):
                n = _count(n0, s)
                stored = np.zeros((2, n * b), np.uint8)
                stored[0, 0], stored[1, 0] = 0xa7, 0x5b
                c = Case("carry b%d s%d n%d" % (b, s, n), b, s, n % 2, stored, 2, n * b, (0, 2, 0, n * b))
                got = c.delivered().reshape(2, n, b)
                assert (got[0, 0::s] == 0xa7).all() and (got[1, 0::s] == 0x5b).all() and (s == 1 or not got[:, 1::s].any() and not got[:, 2::s].any())
                out.append(c)
    for b, s, value in ((4, 1, 0xff), (4, 2, 0x01), (8, 3, 0xff), (2, 4, 0x01), (8, 4, 0xff)):
        n = _count(2 * REACH + 3, s)
        out.append(Case("rows of %#x b%d s%d" % (value, b, s), b, s, 1, np.full((2, n * b), value, np.uint8), 2, n * b, (0, 2, 0, n * b)))
    # long rows in every window, a strip of many rows
    for b, s, rev in ((4, 1, 1), (4, 3, 0), (2, 2, 1), (8, 4, 0), (4, 0, 1), (8, 3, 1)):
        n = _count(3 * REACH + 5, s)
        srb = n * b
        out.append(Case("long b%d s%d rev%d %dx3" % (b, s, rev, n), b, s, rev, _random_stored(rng, 3, srb), 3, srb, T.window_of(len(out) % 4, 3, srb, b, 1)))
    out.append(Case("many rows f32 rgb 7x300", 4, 3, 1, _random_stored(rng, 300, 84), 300, 84, (3, 295, 2, 79)))
    out.append(Case("many rows shuffle 10x300", 8, 0, 0, _random_stored(rng, 300, 80), 300, 80, (0, 300, 0, 80)))
    # a source that holds more than the job
    out.append(Case("src_len beyond the job", 4, 3, 1, _random_stored(rng, 4, 108), 4, 108, (0, 4, 0, 108), src_len=4 * 108 + 5))
    return out


@functools.lru_cache(maxsize=None)
def truncated_cases() -> List[Case]:
    """src_len cut in the middle of a row and at a row boundary: d0 is the rows wholly inside, those of the window are delivered."""
    rng = np.random.default_rng(9)
    out = []
    for b, s, rev, n, rows in ((4, 1, 1, 17, 9), (2, 2, 0, 66, 5), (4, 3, 1, 33, 70), (8, 0, 0, 9, 6), (4, 1, 0, 700, 4)):
        srb = n * b
        stored = _random_stored(rng, rows, srb)
        for cut_rows, extra in ((rows - 1, srb // 2), (rows - 2, 0), (0, srb - 1), (0, 0), (1, 1)):
            for win in ((0, rows, 0, srb), (1, rows - 1, 3, srb - 4)):
                slen = cut_rows * srb + extra
                out.append(Case("cut b%d s%d %dx%d at %d+%d win%s" % (b, s, n, rows, cut_rows, extra, win), b, s, rev, stored, rows, srb, win,
                                src_len=slen, status=E_TRUNCATED, d0=cut_rows))
    return out


def empty_cases() -> List[Case]:
    none = np.zeros((0, 0), np.uint8)
    some = np.arange(24, dtype=np.uint8).reshape(2, 12)
    return [Case("no rows", 4, 3, 1, none, 0, 12, (0, 0, 0, 12)), Case("no bytes", 4, 3, 1, none, 2, 0, (0, 2, 0, 0)),
            Case("no window rows", 4, 3, 1, some, 2, 12, (1, 0, 0, 12)), Case("no window bytes", 4, 3, 1, some, 2, 12, (0, 2, 3, 0)),
            Case("no rows of an illegal element", 3, 9, 7, none, 0, 12, (0, 0, 0, 12))]


def bad_geometry_cases() -> List[Case]:
    """Every illegal geometry include/pzg.h names: PZG_E_FILTER with (0xffffffff, elem_bytes << 16 | sum_stride << 8 | reverse),
    nothing read or written."""
    none = np.zeros((0, 0), np.uint8)

    def mk(name, b=4, s=3, rev=1, rows=3, srb=24, win=(0, 3, 0, 24), **kw):
        return Case(name, b, s, rev, none, rows, srb, win, status=E_FILTER, d0=BAD_ARGS, d1=b << 16 | s << 8 | rev, **kw)
    return [mk("elem_bytes 0", b=0), mk("elem_bytes 1", b=1), mk("elem_bytes 3", b=3), mk("elem_bytes 16", b=16), mk("elem_bytes 255", b=255),
            mk("sum_stride 5", s=5, srb=40, win=(0, 3, 0, 40)), mk("sum_stride 255", s=255), mk("reverse 2", rev=2), mk("reverse 255", rev=255),
            mk("row no multiple of the element", srb=26, win=(0, 3, 0, 26)), mk("row no multiple of the element, 8 bytes", b=8, s=1, srb=28, win=(0, 3, 0, 28)),
            mk("elements no multiple of the sum's stride", srb=28, win=(0, 3, 0, 28)), mk("elements no multiple of the sum's stride, 2", b=2, s=2, srb=6, win=(0, 3, 0, 6)),
            mk("window below the job", win=(1, 3, 0, 24)), mk("window's first row outside", win=(3, 1, 0, 24)),
            mk("window's rows wrap", win=(0xffffffff, 2, 0, 24)), mk("window right of the row", win=(0, 3, 1, 24)),
            mk("window's first byte outside", win=(0, 3, 24, 1)), mk("window's bytes wrap", win=(0, 3, 0xffffffff, 2)),
            mk("dst stride one short", dst_short=1), mk("dst stride one short, no sum", s=0, dst_short=1)]


def all_cases() -> List[Case]:
    return shape_cases() + special_cases() + truncated_cases() + empty_cases() + bad_geometry_cases()


# ---- layouts (those of tiffcases.py) -------------------------------------------------------------------------------------------------------
def descriptor(c: Case, src_off, dst_off, dst_stride) -> np.ndarray:
    d = np.zeros(1, DESC)
    d["src_off"], d["dst_off"], d["dst_stride"], d["src_row_bytes"], d["rows"] = src_off, dst_off, dst_stride, c.srb, c.rows
    d["win_row"], d["win_rows"], d["win_byte"], d["win_bytes"] = c.window
    d["elem_bytes"], d["sum_stride"], d["reverse"] = c.b, c.s, c.reverse
    return d


def single(c: Case, i: int):
    """One job alone, for the model and the sanitized program: (desc, the source bytes it may read, mis, want) with the destination of
    len(want) bytes, the window at desc.dst_off in it and 9 bytes behind it."""
    mis, doff, extra = T.layout_of(i)
    stride = T.stride_of(c, extra)
    want = np.full(doff + T.extent_rows(c) * stride + 9, FILL, np.uint8)
    T.paint(want, c, doff, stride)
    return descriptor(c, 0, doff, stride), T.source_bytes(c), mis, want


def batch(cases: List[Case], shift: int = 0) -> Batch:
    """One call's arrays: the layouts of layout_of(i + shift), 0xEE between the sources, FILL between the rows and between the extents."""
    n = len(cases)
    desc = np.zeros(n, DESC)
    srcs, places, s_at, d_at = [], [], 0, 0
    for i, c in enumerate(cases):
        mis, doff, extra = T.layout_of(i + shift)
        stride = T.stride_of(c, extra)
        sb = T.source_bytes(c)
        s_at = (s_at + 3) // 4 * 4 + mis
        d_at = (d_at + 15) // 16 * 16 + doff
        desc[i] = descriptor(c, s_at, d_at, stride)[0]
        srcs.append((s_at, sb))
        places.append((d_at, stride))
        s_at += len(sb) + 2
        d_at += T.extent_rows(c) * stride + 6
    src = np.full(s_at + 8, 0xEE, np.uint8)
    for at, sb in srcs:
        src[at:at + len(sb)] = sb
    want = np.full(d_at + 32, FILL, np.uint8)
    for c, (at, stride) in zip(cases, places):
        T.paint(want, c, at, stride)
    return Batch(cases, src, np.array([c.slen for c in cases], np.uint64), desc, want, np.array([p[0] for p in places], np.uint64))


# ---- Predictor 3 pages through tiffcases.write_tiff -------------------------------------------------------------------------------------
def float_page(data: np.ndarray, big_endian: bool, then=None, **kw) -> T.Page:
    """A Page of float `data` (H, W, S) with Predictor 3 for write_tiff(..., big_endian): the writer leaves such rows undifferenced, so
    the hook inflates what it stored -- the plain rows of strip or tile k -- encodes them with the page's row geometry and deflates
    again.  then(k, stream): what a test does to a stream after that."""
    assert data.dtype.kind == "f" and data.dtype.itemsize in (2, 4, 8)
    b = data.dtype.itemsize
    tile, planar = kw.get("tile"), kw.get("planar", 1)
    s = data.shape[2] if planar == 1 else 1
    srb = (tile[0] if tile else data.shape[1]) * s * b

    def edit(k, z):
        rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(-1, srb)
        out = zlib.compress(encode(rows, b, s, not big_endian).tobytes(), kw.get("level", 6))
        return then(k, out) if then else out
    return T.Page(data, predictor=3, edit=edit, **kw)


def float_data(rng, shape, dtype) -> np.ndarray:
    """Random floats with NaN, infinities, zeros of both signs and subnormals among them, and a smooth ramp under it so that the
    stored bytes look like a real raster's."""
    dt = np.dtype(dtype)
    a = (np.linspace(-3.0, 900.0, int(np.prod(shape))).reshape(shape) + rng.normal(0.0, 1.0, size=shape)).astype(dt)
    flat = a.reshape(-1)
    bits = flat.view("u%d" % dt.itemsize)
    special = rng.integers(0, flat.size, size=max(4, flat.size // 16))
    flat[special[0::4]] = np.nan
    flat[special[1::4]] = np.inf
    flat[special[2::4]] = -0.0
    bits[special[3::4]] = rng.integers(0, 1 << 16, size=len(special[3::4])).astype(bits.dtype)  # subnormals, and NaN payloads below
    bits[special[:2]] |= np.array(1, bits.dtype)  # (a NaN with a payload bit)
    return a
