"""Shared by the pixel-expansion tests (no GPU): a plain-numpy REFERENCE written from the rules include/pzg.h states for
pzg_expand_many -- it shares nothing with pure_zlib_amd/csrc/expand_core.h -- and the cases that the CPU model
(tests/test_model_expand.py), the sanitized program (tests/test_sanitized_expand.py) and the device (tests/test_gpu_expand.py) all
run.  The kernel goes wrong at edges, not at size: every image type with both formats, with and without a colour key or palette
alpha, at widths around the byte, the 16-byte unit and the wave's 64 lanes, heights of 1, 2 and one more than the row slices, every
source misalignment, destinations off the 16-byte boundaries, padded strides, padding bits set, bad palette indices, empty images
and every illegal geometry."""
import functools
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

OK, E_FILTER, E_PALETTE = 0, 23, 24
BAD_ARGS = 0xffffffff
RGBA8, RGB8 = 0, 1
FILL = 0xCD
ROW_SLICES = 16  # Expand::SLICES (the model says so: tests/test_model_expand.py)

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
TYPES = [(ct, d) for ct, ds in DEPTHS.items() for d in ds]
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 257)
HEIGHTS = (1, 2, 17)
PALETTE_SIZES = (1, 2, 16, 255, 256)

# pzg_expand_desc, stated a second time (include/pzg.h gives the offsets)
DESC = np.dtype({"names": ["src_off", "src_stride", "dst_off", "dst_stride", "width", "height", "pal_off", "pal_len", "key", "color_type", "bit_depth",
                           "out_format", "has_key"],
                 "formats": ["<u8", "<u8", "<u8", "<u8", "<u4", "<u4", "<u4", "<u2", ("<u2", (3,)), "u1", "u1", "u1", "u1"],
                 "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 46, 52, 53, 54, 55], "itemsize": 64})


def src_row_bytes(width, ct, depth):
    return (width * CHANNELS.get(ct, 1) * depth + 7) // 8


def out_bytes(fmt):
    return 3 if fmt == RGB8 else 4


class BadIndex(Exception):
    def __init__(self, row, x, index):
        super().__init__("row %d, pixel %d: index %d" % (row, x, index))
        self.row, self.x, self.index = row, x, index


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def samples_of(rows: np.ndarray, width: int, ct: int, depth: int) -> np.ndarray:
    """(H, W, channels) integers: the samples of rows (H, row_bytes) uint8 as PNG packs them.  Padding bits are cut off."""
    h, ch = rows.shape[0], CHANNELS[ct]
    if depth < 8:
        bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(h, width, depth).astype(np.uint32)
        return (bits << np.arange(depth - 1, -1, -1, dtype=np.uint32)).sum(axis=2).reshape(h, width, 1)
    if depth == 8:
        return rows[:, :width * ch].reshape(h, width, ch).astype(np.uint32)
    b = rows[:, :2 * width * ch].reshape(h, width, ch, 2).astype(np.uint32)
    return b[..., 0] * 256 + b[..., 1]


def expand_reference(width, height, ct, depth, rows, fmt=RGBA8, palette=None, key=None) -> np.ndarray:
    """rows: (height, row_bytes) uint8 as the file stores them.  palette: (N, 4) uint8 R, G, B, A, PLTE and tRNS merged (type 3).
    key: the tRNS colour key at the source depth, one value (type 0) or three (type 2), or None.  Returns (height, width, 4 | 3)
    uint8; raises BadIndex for the first pixel in row-major order whose index is outside the palette."""
    s = samples_of(np.asarray(rows, np.uint8).reshape(height, -1), width, ct, depth)
    out = np.empty((height, width, 4), np.uint8)
    reduce8 = (lambda v: v * (255 // ((1 << depth) - 1))) if depth < 8 else (lambda v: v >> (depth - 8))  # bit replication; the high byte
    if ct == 3:
        pal = np.asarray(palette, np.uint8).reshape(-1, 4)
        bad = np.argwhere(s[..., 0] >= len(pal))
        if len(bad):
            raise BadIndex(int(bad[0][0]), int(bad[0][1]), int(s[bad[0][0], bad[0][1], 0]))
        out[:] = pal[s[..., 0]]
    elif ct in (0, 4):
        out[..., 0] = out[..., 1] = out[..., 2] = reduce8(s[..., 0])
        out[..., 3] = reduce8(s[..., 1]) if ct == 4 else 255
    else:
        out[..., :3] = reduce8(s[..., :3])
        out[..., 3] = reduce8(s[..., 3]) if ct == 6 else 255
    if key is not None and ct in (0, 2):
        k = np.asarray(key, np.uint32).reshape(-1)[:CHANNELS[ct]]
        out[..., 3] = np.where((s == k).all(axis=2), 0, 255)
    return out[..., :3].copy() if fmt == RGB8 else out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    width: int
    height: int
    ct: int
    depth: int
    fmt: int
    rows: np.ndarray                  # (height, src_row_bytes) uint8; (0, 0) where nothing may be read
    palette: Optional[np.ndarray]     # (pal_len,) uint32, bytes in memory R, G, B, A; None: no palette
    key: Optional[Tuple[int, ...]]
    status: int = OK
    d0: int = 0
    d1: int = 0
    out: Optional[np.ndarray] = None  # (height, width, C) where status is OK and the image has pixels
    pal_len: Optional[int] = None     # what the descriptor says where it is not len(palette)
    src_short: int = 0                # the strides fall this much short of a row (illegal geometry)
    dst_short: int = 0

    @property
    def orb(self):
        return self.width * out_bytes(self.fmt) if self.fmt in (RGBA8, RGB8) else 0

    @property
    def srb(self):
        return self.rows.shape[1] if self.rows.size else 0

    @property
    def delivers(self):
        return self.status == OK and self.width > 0 and self.height > 0

    @property
    def touches(self):
        """A bad palette index: the image's own row bytes may hold anything afterwards."""
        return self.status == E_PALETTE


def _pal_u32(rgba: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4).view("<u4").reshape(-1).copy()


def _random_rows(rng, w, h, ct, depth, limit=None):
    """Random samples (an index below `limit`), packed; the padding bits of a packed row are set to 1."""
    rb = src_row_bytes(w, ct, depth)
    if depth >= 8:
        rows = rng.integers(0, 256, size=(h, rb), dtype=np.uint8)
        if limit is not None:
            rows = rng.integers(0, limit, size=(h, rb), dtype=np.uint8)
        return rows
    top = (1 << depth) if limit is None else min(limit, 1 << depth)
    s = rng.integers(0, top, size=(h, w), dtype=np.uint8)
    return pack(s, depth)


def pack(s: np.ndarray, depth: int) -> np.ndarray:
    """(H, W) samples below 8 bits -> (H, row_bytes) packed rows, the padding bits set to 1."""
    h, w = s.shape
    bits = ((s[..., None] >> np.arange(depth - 1, -1, -1, dtype=np.uint8)) & 1).astype(np.uint8).reshape(h, w * depth)
    padn = -(w * depth) % 8
    return np.packbits(np.concatenate([bits, np.ones((h, padn), np.uint8)], axis=1), axis=1)


def _palette(rng, n, alpha):
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    if alpha:
        rgba[:, 3] >>= 1              # (below 255: what it holds is a tRNS alpha)
        rgba[(n + 1) // 2:, 3] = 255  # a tRNS shorter than PLTE, merged
    else:
        rgba[:, 3] = 255
    return rgba


def _sound(name, rng, w, h, ct, depth, fmt, trns, pal_n=None) -> Case:
    palette = key = None
    limit = None
    if ct == 3:
        pal_n = pal_n or min(1 << depth, 16)
        palette, limit = _palette(rng, pal_n, trns), pal_n
    rows = _random_rows(rng, w, h, ct, depth, limit)
    if trns and ct in (0, 2):  # the key is some pixel's samples: it matches that pixel, and whichever others are equal
        s = samples_of(rows, w, ct, depth)
        key = tuple(int(v) for v in s[h // 2, w // 2])
    out = expand_reference(w, h, ct, depth, rows, fmt, palette, key)
    if key is not None:
        assert (out[..., 3] == 0).any() if fmt == RGBA8 else True
    return Case(name, w, h, ct, depth, fmt, rows, None if palette is None else _pal_u32(palette), key, out=out)


@functools.lru_cache(maxsize=None)
def shape_cases() -> List[Case]:
    """Every type x format x (key or palette alpha | none) at every width, the heights in turn: 15 * 2 * 2 * 19 images."""
    rng = np.random.default_rng(20261020)
    out, i = [], 0
    for ct, depth in TYPES:
        for fmt in (RGBA8, RGB8):
            for trns in (False, True):
                for w in WIDTHS:
                    h = HEIGHTS[i % 3]
                    i += 1
                    out.append(_sound("t%d d%d f%d trns%d %dx%d" % (ct, depth, fmt, trns, w, h), rng, w, h, ct, depth, fmt, trns))
    return out


@functools.lru_cache(maxsize=None)
def special_cases() -> List[Case]:
    """Every height at two widths; the palette sizes; the keys that differ from a sample in one byte."""
    rng = np.random.default_rng(7)
    out = []
    for ct, depth in TYPES:
        for h in HEIGHTS:
            for w in (5, 65):
                out.append(_sound("heights t%d d%d %dx%d" % (ct, depth, w, h), rng, w, h, ct, depth, (w + h) % 2, True))
    for n in PALETTE_SIZES:
        for depth in (1, 2, 4, 8):
            for fmt in (RGBA8, RGB8):
                out.append(_sound("palette of %d d%d f%d" % (n, depth, fmt), rng, 33, 2, 3, depth, fmt, True, pal_n=n))
    # 16-bit gray with the key 0x00ff beside 0x01ff and 0x00fe: only the first is transparent
    s = np.array([[0x00ff, 0x01ff, 0x00fe, 0xff00, 0x00ff, 0xffff, 0x0000]], ">u2")
    rows = s.view(np.uint8).reshape(1, 14)
    c = Case("gray16 key 0x00ff", 7, 1, 0, 16, RGBA8, rows, None, (0x00ff,), out=expand_reference(7, 1, 0, 16, rows, RGBA8, None, (0x00ff,)))
    assert c.out[0, :, 3].tolist() == [0, 255, 255, 255, 0, 255, 255] and c.out[0, :3, 0].tolist() == [0, 1, 0]
    out.append(c)
    # 16-bit RGB: each sample of the key off by its low byte, by its high byte, and the key itself
    key = (0x1234, 0xabcd, 0x00ff)
    px = [key, (0x1235, 0xabcd, 0x00ff), (0x1234, 0xaacd, 0x00ff), (0x1234, 0xabcd, 0x01ff), (0x1234, 0xabcd, 0x00fe), key]
    rows = np.array(px, ">u2").reshape(1, 6, 3).view(np.uint8).reshape(1, 36)
    c = Case("rgb16 key near misses", 6, 1, 2, 16, RGBA8, rows, None, key, out=expand_reference(6, 1, 2, 16, rows, RGBA8, None, key))
    assert c.out[0, :, 3].tolist() == [0, 255, 255, 255, 255, 0]
    out.append(c)
    # 8-bit RGB: a pixel that matches the key in two samples of three
    key = (10, 20, 30)
    rows = np.array([[10, 20, 30, 10, 20, 31, 11, 20, 30, 10, 21, 30, 10, 20, 30]], np.uint8)
    c = Case("rgb8 key near misses", 5, 1, 2, 8, RGBA8, rows, None, key, out=expand_reference(5, 1, 2, 8, rows, RGBA8, None, key))
    assert c.out[0, :, 3].tolist() == [0, 255, 255, 255, 0]
    out.append(c)
    # a key no sample of the depth can equal: nothing is transparent
    rows = pack(np.array([[0, 1, 2, 3, 3]], np.uint8), 2)
    c = Case("gray2 key out of range", 5, 1, 0, 2, RGBA8, rows, None, (0x0103,), out=expand_reference(5, 1, 0, 2, rows, RGBA8, None, (0x0103,)))
    assert (c.out[..., 3] == 255).all()
    out.append(c)
    return out


def _bad(name, w, h, depth, pal_n, offenders, fmt=RGBA8) -> Case:
    """A palette image of indices 0 with the offenders [(row, x, index)] put in; the reference names the first."""
    s = np.zeros((h, w), np.uint8)
    for r, x, idx in offenders:
        s[r, x] = idx
    rows = pack(s, depth) if depth < 8 else s
    pal = _palette(np.random.default_rng(pal_n), pal_n, True)
    try:
        expand_reference(w, h, 3, depth, rows, fmt, pal)
    except BadIndex as e:
        return Case(name, w, h, 3, depth, fmt, rows, _pal_u32(pal), None, E_PALETTE, e.row, e.x)
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def bad_index_cases() -> List[Case]:
    out = [
        _bad("first pixel", 33, 18, 8, 16, [(0, 0, 200)]),
        _bad("last pixel", 33, 18, 8, 16, [(17, 32, 16)]),
        _bad("rows 16 and 1", 33, 18, 8, 16, [(16, 5, 99), (1, 30, 17)]),
        _bad("x 70 and x 3 of one row", 129, 3, 8, 16, [(2, 70, 255), (2, 3, 16)]),
        _bad("x 70 and x 3 of one row, rgb", 129, 3, 8, 16, [(2, 70, 255), (2, 3, 16)], RGB8),
        _bad("exactly pal_len", 9, 2, 8, 255, [(1, 4, 255)]),
        _bad("4 bits, 5 entries", 17, 17, 4, 5, [(16, 16, 5), (16, 15, 4)]),
        _bad("2 bits, 3 entries", 7, 2, 2, 3, [(1, 6, 3)]),
        _bad("1 bit, 1 entry", 65, 2, 1, 1, [(1, 64, 1), (0, 63, 1)]),
        _bad("every pixel", 64, 17, 8, 1, [(r, x, 1 + (r + x) % 200) for r in range(17) for x in range(64)]),
    ]
    assert [(c.d0, c.d1) for c in out] == [(0, 0), (17, 32), (1, 30), (2, 3), (2, 3), (1, 4), (16, 16), (1, 6), (0, 63), (0, 0)]
    return out


def empty_cases() -> List[Case]:
    none = np.zeros((0, 0), np.uint8)
    return [Case("no columns", 0, 5, 2, 8, RGBA8, none, None, None), Case("no rows", 5, 0, 3, 8, RGB8, none, None, None, pal_len=4),
            Case("no columns of an illegal type", 0, 5, 7, 9, RGBA8, none, None, None)]


def bad_geometry_cases() -> List[Case]:
    """Every illegal geometry include/pzg.h names: PZG_E_FILTER with (0xffffffff, color_type << 8 | bit_depth), nothing read or written."""
    none = np.zeros((0, 0), np.uint8)
    pal = np.zeros(4, np.uint32)
    mk = lambda name, w, h, ct, d, fmt=RGBA8, **kw: Case(name, w, h, ct, d, fmt, none, kw.pop("palette", None), None, E_FILTER, BAD_ARGS, ct << 8 | d, **kw)  # noqa: E731
    return [mk("rgb at 4 bits", 5, 3, 2, 4), mk("palette at 16 bits", 5, 3, 3, 16, palette=pal), mk("gray at 3 bits", 5, 3, 0, 3),
            mk("colour type 5", 5, 3, 5, 8), mk("colour type 1", 5, 3, 1, 8), mk("gray+alpha at 4 bits", 5, 3, 4, 4), mk("depth 0", 5, 3, 6, 0),
            mk("format 2", 5, 3, 2, 8, 2), mk("format 255", 5, 3, 0, 1, 255),
            mk("dst stride one short", 5, 3, 6, 16, dst_short=1), mk("dst stride one short, rgb", 5, 3, 0, 1, RGB8, dst_short=1),
            mk("src stride one short", 9, 3, 0, 1, src_short=1), mk("src stride one short, rgba16", 5, 3, 6, 16, src_short=1),
            mk("palette of 0", 5, 3, 3, 8, palette=pal, pal_len=0), mk("palette of 257", 5, 3, 3, 2, palette=pal, pal_len=257),
            mk("width 2^31", 1 << 31, 3, 0, 8), mk("height 2^31", 5, 1 << 31, 2, 8)]


def all_cases() -> List[Case]:
    return shape_cases() + special_cases() + bad_index_cases() + empty_cases() + bad_geometry_cases()


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
DST_OFFS = (0, 1, 3, 7, 12, 16)


def layout_of(i: int) -> Tuple[int, int, int, int]:
    """(source misalignment, destination offset modulo 16, what the destination stride adds to a row, what the source stride adds)"""
    return i % 4, DST_OFFS[i % 6], (5, 0)[(i // 2) % 2], (0, 3, 1)[i % 3]


def strides_of(c: Case, dst_extra: int, src_extra: int) -> Tuple[int, int]:
    """(src_stride, dst_stride).  An illegal image has the strides its geometry asks for, whatever the layout adds."""
    legal_srb = src_row_bytes(c.width, c.ct, c.depth) if (c.width >> 31) == 0 else 8
    if c.src_short:
        return legal_srb - c.src_short, c.orb + dst_extra
    if c.dst_short:
        return legal_srb + src_extra, c.orb - c.dst_short
    return (c.srb or legal_srb) + src_extra, (c.orb or 4) + dst_extra


def descriptor(c: Case, src_off, src_stride, dst_off, dst_stride, pal_off) -> np.ndarray:
    d = np.zeros(1, DESC)
    d["src_off"], d["src_stride"], d["dst_off"], d["dst_stride"] = src_off, src_stride, dst_off, dst_stride
    d["width"], d["height"], d["pal_off"] = c.width, c.height, pal_off
    d["pal_len"] = c.pal_len if c.pal_len is not None else (len(c.palette) if c.palette is not None else 0)
    if c.key is not None:
        d["key"][0, :len(c.key)] = c.key
        d["has_key"] = 1
    d["color_type"], d["bit_depth"], d["out_format"] = c.ct, c.depth, c.fmt
    return d


def source_bytes(c: Case, src_stride: int) -> np.ndarray:
    """The image's source extent: its rows at src_stride, 0xEE between them, nothing behind the last row's last byte."""
    if not c.rows.size:
        return np.zeros(0, np.uint8)
    h, rb = c.rows.shape
    buf = np.full((h, src_stride), 0xEE, np.uint8)
    buf[:, :rb] = c.rows
    return buf.reshape(-1)[:(h - 1) * src_stride + rb].copy()


def paint(want: np.ndarray, loose: np.ndarray, c: Case, dst_off: int, dst_stride: int):
    """The image's rows into `want` (what must be there) or, for an image whose bytes are unspecified, into the mask `loose`."""
    if c.delivers:
        flat = c.out.reshape(c.height, c.orb)
        for r in range(c.height):
            want[dst_off + r * dst_stride:dst_off + r * dst_stride + c.orb] = flat[r]
    elif c.touches:
        for r in range(c.height):
            loose[dst_off + r * dst_stride:dst_off + r * dst_stride + c.orb] = True


def single(c: Case, i: int):
    """One image alone, for the model and the sanitized program: (desc, source bytes, mis, palette or None, want, loose) with the
    destination of len(want) bytes, the image at desc.dst_off in it and 9 bytes behind it."""
    mis, doff, dextra, sextra = layout_of(i)
    sstride, dstride = strides_of(c, dextra, sextra)
    rows = c.height if c.delivers or c.touches else 0
    want = np.full(doff + rows * max(dstride, 0) + 9, FILL, np.uint8)
    loose = np.zeros(len(want), bool)
    paint(want, loose, c, doff, dstride)
    return descriptor(c, 0, sstride, doff, dstride, 0), source_bytes(c, sstride), mis, c.palette, want, loose


@dataclass
class Batch:
    cases: List[Case]
    src: np.ndarray
    palette: np.ndarray
    desc: np.ndarray
    dst_want: np.ndarray
    loose: np.ndarray        # bytes that may hold anything afterwards (the rows of an image with a bad palette index)
    dst_off: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))


def batch(cases: List[Case], shift: int = 0) -> Batch:
    """One call's arrays: the layouts of layout_of(i + shift), FILL between the rows and between the extents, every palette just
    behind the one before."""
    n = len(cases)
    desc = np.zeros(n, DESC)
    srcs, pals, s_at, d_at, p_at, places = [], [], 0, 0, 0, []
    for i, c in enumerate(cases):
        mis, doff, dextra, sextra = layout_of(i + shift)
        sstride, dstride = strides_of(c, dextra, sextra)
        sb = source_bytes(c, sstride)
        s_at = (s_at + 3) // 4 * 4 + mis
        d_at = (d_at + 15) // 16 * 16 + doff
        desc[i] = descriptor(c, s_at, sstride, d_at, dstride, p_at)[0]
        srcs.append((s_at, sb))
        places.append((d_at, dstride))
        s_at += len(sb) + 2
        rows = c.height if c.delivers or c.touches else 0
        d_at += rows * dstride + 6
        if c.palette is not None:
            pals.append(c.palette)
            p_at += len(c.palette)
    src = np.full(s_at + 8, 0xEE, np.uint8)
    for at, sb in srcs:
        src[at:at + len(sb)] = sb
    want = np.full(d_at + 32, FILL, np.uint8)
    loose = np.zeros(len(want), bool)
    for c, (at, dstride) in zip(cases, places):
        paint(want, loose, c, at, dstride)
    palette = np.concatenate(pals + [np.zeros(1, np.uint32)]).astype(np.uint32)
    return Batch(cases, src, palette, desc, want, loose, np.array([p[0] for p in places], np.uint64))


def first_difference(got: np.ndarray, b: Batch) -> Optional[str]:
    """None, or which image (or gap) of the batch differs from what must be there."""
    diff = (got != b.dst_want) & ~b.loose
    if not diff.any():
        return None
    at = int(np.flatnonzero(diff)[0])
    i = int(np.searchsorted(b.dst_off, at, side="right")) - 1
    name = b.cases[i].name if i >= 0 else "(in front of the first extent)"
    return "byte %d (%s, %d behind its dst_off): %#x, not %#x" % (at, name, at - int(b.dst_off[max(i, 0)]), int(got[at]), int(b.dst_want[at]))
