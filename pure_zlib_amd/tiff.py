"""Deflate-compressed TIFF files read in batches on the GPU: EXTENSION, the reference has no image reader.

Every strip and every tile of a Deflate TIFF (Compression 8, and the older 32946) is a complete RFC 1950 stream of its own, and the IFD
gives each one's offset, its compressed length and its exact decoded size.  So every strip and tile of every page of every file of a
batch goes into ONE pzg_decompress_many launch with exact capacities -- no capacity guess, no relaunch -- and ONE pzg_unpredict_many
launch behind it on the same stream, which takes the decode's out_len array as its src_len: horizontal differencing (Predictor 2,
TIFF 6.0 section 14) is undone on the device and every tile is clipped to the image as it is delivered into the page's rows.  One
sync, and one copy out of the pixels alone.  The host parses the IFDs; nothing is inflated on the CPU.  Device memory is held in
torch tensors.
With float_predictor=True the floating-point predictor (Predictor 3, TIFF Technical Note 3: what GDAL and libtiff write for elevation
models and other float rasters) is read as well: the strips and tiles of such pages go through ONE pzg_unshuffle_many launch -- a
byte-wise running sum along the row, then the byte planes transposed back into elements -- behind the pzg_unpredict_many launch of
the others, on the same stream and with the same out_len array; a batch without such pages issues the launches it always did.
With lzw=True LZW pages (Compression 5, the post-6.0 bit order: what scanners, Photoshop and older GDAL / libtiff defaults write) are
read through every path a Deflate page has: their strips and tiles go to ONE pzg_unlzw_many launch beside the pzg_decompress_many
launch of the Deflate ones, into the same decode buffer and out_len array, and the stage launches follow as before (a batch that
holds Deflate and LZW jobs for both stages issues the Deflate launch once per stage's run).  LZW has no end-of-data check: a strip
that ends early is "not enough image data" from the stage, a code outside the table is the decoder's own error, and a strip in the
bit order from before TIFF 6.0 is a NotImplementedError for its file.

    parse_tiff(blob)                  -> [TiffPage]               (pure Python, no GPU; ValueError names the page and the tag)
    read_tiff_many(blobs_or_paths)    -> [[TiffImage per page], or the DecompressionError / ValueError / NotImplementedError of that file]
    read_tiff(blob_or_path, page=0)   -> TiffImage                (raises)
    read_tiff_region(blob_or_path, page, y0, x0, h, w) -> np.ndarray   (only the strips or tiles that cover the rectangle are decoded)
    test_tiff_many(blobs_or_paths)    -> [(index_or_name, problem)]   (empty: every file is sound)
    python -m pure_zlib_amd.tiff -t [--float-predictor] [--lzw] A.tif B.tif ...
    (each of the four readers takes float_predictor=False and lzw=False)

Byte orders II and MM, classic TIFF and BigTIFF, strips and tiles, PlanarConfiguration 1 and 2, Predictor 1 and 2, 8/16/32/64-bit
samples of any SampleFormat, and 1/2/4-bit single-sample images as packed rows; with float_predictor=True Predictor 3 on
16/32/64-bit floating-point samples, chunky with up to four samples or as separate planes.  `data` is the samples as the file stores
them, in the file's byte order: PhotometricInterpretation, ExtraSamples, Orientation and ColorMap are reported, not interpreted.  Not
done (NotImplementedError, for that file alone): any other compression (LZW without lzw=True among them), old-style LZW, Predictor 3 (the floating-point predictor) without
float_predictor=True, FillOrder 2, unequal BitsPerSample, bits below 8 with several samples or with Predictor 2, Predictor 2 with bits
outside 8/16/32/64, Predictor 2 or 3 with more than four chunky samples, 24-bit floats, subsampled YCbCr, a strip or tile of 4 GiB or
more.  Predictor 3 on samples that are not floating-point, or on 8-bit ones, is a ValueError (tags 317 / 339): libtiff refuses such
files too.
"""
import os
import struct
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from ._batch import DeviceChain, load
from .zlib import UNPREDICT_DESC, UNSHUFFLE_DESC, Context, DecompressionError, default_context, error_from_status

_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8, 17: 8, 18: 8}
_UINT_FMT = {1: "B", 3: "H", 4: "I", 13: "I", 16: "Q", 18: "Q"}
_TAGS = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation", 266: "FillOrder",
         273: "StripOffsets", 274: "Orientation", 277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration",
         317: "Predictor", 320: "ColorMap", 322: "TileWidth", 323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 338: "ExtraSamples",
         339: "SampleFormat", 530: "YCbCrSubSampling"}
_MAX_PAGES = 65536


@dataclass
class TiffPage:
    """One IFD as parse_tiff found it: the image's shape and where its strips or tiles lie in the file.  A strip-based page has
    tile_width = width and tile_length = RowsPerStrip."""
    index: int
    big_endian: bool
    width: int
    height: int
    samples: int
    bits_per_sample: Tuple[int, ...]
    sample_format: int
    planar: int
    photometric: Optional[int]
    extra_samples: Tuple[int, ...]
    colormap: Optional[Tuple[int, ...]]
    orientation: int
    compression: int
    predictor: int
    fill_order: int
    subsampling: Optional[Tuple[int, ...]]
    tiled: bool
    tile_width: int
    tile_length: int
    offsets: Tuple[int, ...] = field(repr=False)
    byte_counts: Tuple[int, ...] = field(repr=False)

    @property
    def bits(self) -> int:
        return self.bits_per_sample[0]

    @property
    def stored_samples(self) -> int:
        """The samples of a stored pixel: SamplesPerPixel for chunky data, 1 for a separate plane."""
        return self.samples if self.planar == 1 else 1

    @property
    def planes(self) -> int:
        return 1 if self.planar == 1 else self.samples

    @property
    def across(self) -> int:
        return -(-self.width // self.tile_width)

    @property
    def down(self) -> int:
        return -(-self.height // self.tile_length)

    def row_bytes(self, pixels: int) -> int:
        return (pixels * self.stored_samples * self.bits + 7) // 8


@dataclass
class TiffImage:
    width: int
    height: int
    samples: int
    bits: int
    sample_format: int
    planar: int
    photometric: Optional[int]
    extra_samples: Tuple[int, ...]
    colormap: Optional[Tuple[int, ...]]
    tiled: bool
    data: Optional[np.ndarray]  # (H, W, S) chunky | (S, H, W) planar == 2 | (H, row_bytes) packed uint8 below 8 bits; None with device_out


# ---- the parser -----------------------------------------------------------------------------------------------------------------------
def parse_tiff(blob, name: str = "tiff") -> List[TiffPage]:
    """The pages of a TIFF file.  Every offset and count is checked against the blob before it is used: a bad file is a ValueError
    that names the page and the tag, never an IndexError or a struct.error.  What the reader does not support is not an error here."""
    blob = bytes(blob)
    if len(blob) < 8 or blob[:2] not in (b"II", b"MM"):
        raise ValueError("%s: not a TIFF file (bad byte order mark)" % name)
    e = "<" if blob[:2] == b"II" else ">"
    magic, = struct.unpack_from(e + "H", blob, 2)
    if magic == 42:
        big, osz, ofmt, first = False, 4, "I", struct.unpack_from(e + "I", blob, 4)[0]
    elif magic == 43:
        if len(blob) < 16 or struct.unpack_from(e + "HH", blob, 4) != (8, 0):
            raise ValueError("%s: bad BigTIFF header" % name)
        big, osz, ofmt, first = True, 8, "Q", struct.unpack_from(e + "Q", blob, 8)[0]
    else:
        raise ValueError("%s: not a TIFF file (version %d)" % (name, magic))
    cnt_sz, ent_sz = (8, 20) if big else (2, 12)
    pages, seen, at = [], set(), first
    while at:
        p = len(pages)
        where = "%s: page %d" % (name, p)
        if at in seen:
            raise ValueError("%s: the chain of IFDs comes back to offset %d" % (where, at))
        if len(pages) >= _MAX_PAGES:
            raise ValueError("%s: more than %d IFDs" % (where, _MAX_PAGES))
        seen.add(at)
        if at + cnt_sz > len(blob):
            raise ValueError("%s: the IFD at offset %d lies outside the file" % (where, at))
        count, = struct.unpack_from(e + ("Q" if big else "H"), blob, at)
        if at + cnt_sz + count * ent_sz + osz > len(blob):
            raise ValueError("%s: the IFD at offset %d (%d entries) runs past the end of the file" % (where, at, count))
        tags = {}
        for k in range(count):
            tag, typ, n = struct.unpack_from(e + ("HHQ" if big else "HHI"), blob, at + cnt_sz + k * ent_sz)
            if tag not in _TAGS or tag in tags:
                continue
            label = "%s: tag %d (%s)" % (where, tag, _TAGS[tag])
            if typ not in _UINT_FMT:
                raise ValueError("%s: type %d is no unsigned integer" % (label, typ))
            size = _TYPE_SIZE[typ] * n
            vat = at + cnt_sz + k * ent_sz + ent_sz - osz
            if size > osz:
                vat, = struct.unpack_from(e + ofmt, blob, vat)
                if vat + size > len(blob):
                    raise ValueError("%s: %d values at offset %d run past the end of the file" % (label, n, vat))
            tags[tag] = struct.unpack_from("%s%d%s" % (e, n, _UINT_FMT[typ]), blob, vat)
        nxt, = struct.unpack_from(e + ofmt, blob, at + cnt_sz + count * ent_sz)

        def one(tag, default=None):
            v = tags.get(tag)
            if v is None:
                if default is None:
                    raise ValueError("%s: tag %d (%s) is missing" % (where, tag, _TAGS[tag]))
                return default
            if len(v) < 1:
                raise ValueError("%s: tag %d (%s) has no value" % (where, tag, _TAGS[tag]))
            return int(v[0])

        width, height, samples = one(256), one(257), one(277, 1)
        if not (0 < width < 1 << 31 and 0 < height < 1 << 31):
            raise ValueError("%s: tag 256 (ImageWidth) / 257 (ImageLength): an image of %d x %d" % (where, width, height))
        if not 0 < samples <= 65535:
            raise ValueError("%s: tag 277 (SamplesPerPixel): %d" % (where, samples))
        bps = tuple(int(v) for v in tags.get(258, (1,)))
        if len(bps) == 1 and samples > 1:
            bps = bps * samples  # (some writers give one value for all)
        if len(bps) != samples or any(b == 0 or b > 64 for b in bps):
            raise ValueError("%s: tag 258 (BitsPerSample): %d values %s for %d samples" % (where, len(bps), bps[:8], samples))
        planar = one(284, 1)
        if planar not in (1, 2):
            raise ValueError("%s: tag 284 (PlanarConfiguration): %d" % (where, planar))
        tiled = 322 in tags or 324 in tags
        if tiled:
            tw, tl = one(322), one(323)
            if not (0 < tw < 1 << 31 and 0 < tl < 1 << 31):
                raise ValueError("%s: tag 322 (TileWidth) / 323 (TileLength): tiles of %d x %d" % (where, tw, tl))
            otag, ctag = 324, 325
        else:
            tw, tl = width, min(one(278, height), height)
            if tl <= 0:
                raise ValueError("%s: tag 278 (RowsPerStrip): %d" % (where, tl))
            otag, ctag = 273, 279
        for t in (otag, ctag):
            if t not in tags:
                raise ValueError("%s: tag %d (%s) is missing" % (where, t, _TAGS[t]))
        expect = -(-width // tw) * -(-height // tl) * (samples if planar == 2 else 1)
        offsets, counts = tags[otag], tags[ctag]
        for t, v in ((otag, offsets), (ctag, counts)):
            if len(v) != expect:
                raise ValueError("%s: tag %d (%s): %d values for %d %s" % (where, t, _TAGS[t], len(v), expect, "tiles" if tiled else "strips"))
        for k, (o, c) in enumerate(zip(offsets, counts)):
            if o + c > len(blob):
                raise ValueError("%s: tag %d (%s): %s %d (%d bytes at offset %d) runs past the end of the file"
                                 % (where, otag, _TAGS[otag], "tile" if tiled else "strip", k, c, o))
        fmt = tags.get(339, (1,))
        pages.append(TiffPage(p, e == ">", width, height, samples, bps, int(fmt[0]) if len(fmt) else 1, planar,
                              int(tags[262][0]) if tags.get(262) else None, tuple(int(v) for v in tags.get(338, ())),
                              tuple(int(v) for v in tags[320]) if 320 in tags else None, one(274, 1), one(259, 1), one(317, 1), one(266, 1),
                              tuple(int(v) for v in tags[530]) if 530 in tags else None, tiled, tw, tl, tuple(int(v) for v in offsets),
                              tuple(int(v) for v in counts)))
        at = nxt
    if not pages:
        raise ValueError("%s: no IFD" % name)
    return pages


def _check_supported(name: str, pg: TiffPage, float_predictor: bool = False, lzw: bool = False, blob: bytes = b"") -> None:
    where = "%s: page %d" % (name, pg.index)
    if pg.compression not in (8, 32946) and not (lzw and pg.compression == 5):
        raise NotImplementedError("%s: Compression %d (only Deflate, 8 and 32946, is read)" % (where, pg.compression))
    if pg.compression == 5:
        for k, (o, c) in enumerate(zip(pg.offsets, pg.byte_counts)):
            if c >= 2 and blob[o] == 0 and blob[o + 1] & 1:  # (libtiff's test: codes packed from the low bit, written before TIFF 6.0)
                raise NotImplementedError("%s, %s %d: old-style LZW (the bit order from before TIFF 6.0) is not read" % (where, "tile" if pg.tiled else "strip", k))
    if pg.predictor == 3 and not float_predictor:
        raise NotImplementedError("%s: Predictor 3 (the floating-point predictor) is not read" % where)
    if pg.predictor not in (1, 2, 3):
        raise ValueError("%s: tag 317 (Predictor): %d" % (where, pg.predictor))
    if pg.fill_order != 1:
        raise NotImplementedError("%s: FillOrder %d is not read" % (where, pg.fill_order))
    if len(set(pg.bits_per_sample)) != 1:
        raise NotImplementedError("%s: unequal BitsPerSample %s" % (where, pg.bits_per_sample[:8]))
    bits = pg.bits
    if pg.predictor == 3 and (pg.sample_format != 3 or bits <= 8):
        raise ValueError("%s: tag 317 (Predictor) 3 with tag 339 (SampleFormat) %d and %d-bit samples: the floating-point predictor takes "
                         "floating-point samples of 16, 32 or 64 bits" % (where, pg.sample_format, bits))
    if bits < 8:
        if bits not in (1, 2, 4):
            raise NotImplementedError("%s: %d bits per sample" % (where, bits))
        if pg.samples > 1 or pg.predictor == 2:
            raise NotImplementedError("%s: %d-bit samples with %s" % (where, bits, "Predictor 2" if pg.predictor == 2 else "%d samples per pixel" % pg.samples))
        if pg.tiled and pg.tile_width * bits % 8:
            raise NotImplementedError("%s: tiles of %d %d-bit pixels do not end on a byte" % (where, pg.tile_width, bits))
    elif bits not in (8, 16, 32, 64):
        raise NotImplementedError("%s: %d bits per sample" % (where, bits))
    if pg.predictor == 2 and pg.stored_samples > 4:
        raise NotImplementedError("%s: Predictor 2 with %d chunky samples per pixel" % (where, pg.stored_samples))
    if pg.predictor == 3 and pg.stored_samples > 4:
        raise NotImplementedError("%s: Predictor 3 with %d chunky samples per pixel" % (where, pg.stored_samples))
    if pg.photometric == 6 and pg.subsampling not in (None, (1, 1)):
        raise NotImplementedError("%s: YCbCr with subsampling %s" % (where, pg.subsampling))
    if pg.tile_length * pg.row_bytes(pg.tile_width) >= 1 << 32:
        raise NotImplementedError("%s: a %s of 4 GiB or more" % (where, "tile" if pg.tiled else "strip"))


def _dtype(pg: TiffPage) -> np.dtype:
    if pg.bits < 8:
        return np.dtype("u1")
    kind = {1: "u", 2: "i", 3: "f"}.get(pg.sample_format, "u")
    if kind == "f" and pg.bits < 16:
        kind = "u"
    if pg.bits == 8:
        return np.dtype(kind + "1")
    return np.dtype((">" if pg.big_endian else "<") + kind + str(pg.bits // 8))


def _image(pg: TiffPage, flat: Optional[np.ndarray]) -> TiffImage:
    data = None
    if flat is not None:
        if pg.bits < 8:
            data = flat.reshape(pg.height, -1)
        elif pg.planar == 2:
            data = flat.view(_dtype(pg)).reshape(pg.samples, pg.height, pg.width)
        else:
            data = flat.view(_dtype(pg)).reshape(pg.height, pg.width, pg.samples)
    return TiffImage(pg.width, pg.height, pg.samples, pg.bits, pg.sample_format, pg.planar, pg.photometric, pg.extra_samples, pg.colormap, pg.tiled, data)


@dataclass
class _Job:
    """One strip or tile: where its stream lies in its file, and its pzg_unpredict_desc -- with Predictor 3 its pzg_unshuffle_desc:
    sample_bytes is elem_bytes, samples sum_stride, a little-endian file reverse -- but for the offsets the launch gives it."""
    file: int
    page: int
    index: int
    tiled: bool
    blob: bytes = field(repr=False)
    start: int
    length: int
    srb: int
    rows: int
    window: Tuple[int, int, int, int]
    dst_off: int
    dst_stride: int
    predictor: int
    sample_bytes: int
    samples: int
    big_endian: bool
    lzw: bool = False


def _page_jobs(f: int, blob: bytes, pg: TiffPage, base: int, stride: int, plane_bytes: int, rect=None) -> List[_Job]:
    """The jobs of a page whose row y, byte b of plane p goes to base + p * plane_bytes + y * stride + b.  rect = (y0, x0 in bytes, h,
    w in bytes): only the strips or tiles that cover it, each clipped to it, delivered with the rectangle's corner at `base`."""
    out = []
    srb = pg.row_bytes(pg.tile_width)
    image_rb = pg.row_bytes(pg.width)
    ry, rx, rh, rw = rect if rect is not None else (0, 0, pg.height, image_rb)
    sb, s = (pg.bits // 8, pg.stored_samples) if pg.predictor in (2, 3) else (1, 1)
    per_plane = pg.across * pg.down
    for plane in range(pg.planes):
        for ty in range(ry // pg.tile_length, -(-(ry + rh) // pg.tile_length)):
            y0 = ty * pg.tile_length
            rows = pg.tile_length if pg.tiled else min(pg.tile_length, pg.height - y0)
            top, bottom = max(ry, y0), min(ry + rh, y0 + rows, pg.height)
            for tx in range(rx // srb, -(-(rx + rw) // srb)):
                b0 = tx * srb
                left, right = max(rx, b0), min(rx + rw, b0 + srb, image_rb)
                k = plane * per_plane + ty * pg.across + tx
                out.append(_Job(f, pg.index, k, pg.tiled, blob, pg.offsets[k], pg.byte_counts[k], srb, rows, (top - y0, bottom - top, left - b0, right - left),
                                base + plane * plane_bytes + (top - ry) * stride + (left - rx), stride, pg.predictor, sb, s, pg.big_endian,
                                pg.compression == 5))
    return out


def _job_error(j: _Job, st: int, detail, ust: int) -> Optional[DecompressionError]:
    """What the decode (st, its detail pair) and the stage (ust) say of a job, or None."""
    where = "page %d, %s %d: " % (j.page, "tile" if j.tiled else "strip", j.index)
    if st == _ffi.OK and ust == _ffi.OK:
        return None
    if st == _ffi.E_OUT_TOO_SMALL:
        return DecompressionError("FormatError", where + "too much image data", _ffi.E_FILTER)
    if j.lzw and st == _ffi.E_TRUNCATED:  # (an LZW stream that ends early has no message of its own: what counts is whether rows are missing)
        st = _ffi.OK
        if ust == _ffi.OK:
            return None
    if st != _ffi.OK:
        e = error_from_status(j.blob[j.start:j.start + j.length], st, detail)
        return DecompressionError(e.constructor, where + e.message, e.status, e.detail)
    if ust == _ffi.E_TRUNCATED:
        return DecompressionError("FormatError", where + "not enough image data", _ffi.E_FILTER)
    return DecompressionError("FormatError", where + "the rows could not be reconstructed", _ffi.E_FILTER)


def _run(ctx: Context, jobs: List[_Job], total_pix: int, out_ptr: Optional[int]):
    """The decode and the stage launches over the jobs: the Predictor 1 / 2 jobs go to pzg_unpredict_many, the Predictor 3 jobs to
    pzg_unshuffle_many behind it, each launch only where it has jobs.  The decode takes the jobs with each kind contiguous, so that
    both stages find their src_len in its out_len array; errors come back under the jobs' own indices.  Returns (the pixel buffer on
    the host or None, {job: its DecompressionError}).  out_ptr: the jobs' dst_off count from this device address and nothing is
    copied out."""
    # (stable: file order within a kind.  The LZW jobs of the two stages meet in the middle -- unpredict Deflate | unpredict LZW |
    # unshuffle LZW | unshuffle Deflate -- so that they are ONE contiguous run and one launch)
    order = sorted(range(len(jobs)), key=lambda k: (jobs[k].predictor == 3, jobs[k].lzw != (jobs[k].predictor == 3)))
    run = [jobs[k] for k in order]
    n = len(run)
    nu = sum(1 for j in run if j.predictor != 3)
    lz = [j.lzw for j in run]
    l0 = lz.index(True) if True in lz else n           # Deflate [0, l0) | LZW [l0, l1) | Deflate [l1, n)
    l1 = n - lz[::-1].index(True) if True in lz else n
    codecs = None if l0 == n else [("deflate", l0), ("lzw", l1 - l0), ("deflate", n - l1)]
    desc, fdesc = np.zeros(nu, dtype=UNPREDICT_DESC), np.zeros(n - nu, dtype=UNSHUFFLE_DESC)
    for d, j in zip(list(desc) + list(fdesc), run):
        d["dst_off"], d["dst_stride"], d["src_row_bytes"], d["rows"] = j.dst_off, j.dst_stride, j.srb, j.rows
        d["win_row"], d["win_rows"], d["win_byte"], d["win_bytes"] = j.window
        if j.predictor == 3:
            d["elem_bytes"], d["sum_stride"], d["reverse"] = j.sample_bytes, j.samples, int(not j.big_endian)
        else:
            d["predictor"], d["sample_bytes"], d["samples"], d["big_endian"] = j.predictor, j.sample_bytes, j.samples, int(j.big_endian)
    with DeviceChain(ctx, [(j.blob, j.start, j.length) for j in run], [j.rows * j.srb for j in run], codecs) as ch:
        pix = ch.scratch(total_pix + 16) if out_ptr is None else None
        dst = out_ptr if pix is None else pix.data_ptr()
        desc["src_off"], fdesc["src_off"] = ch.dec_off[:nu], ch.dec_off[nu:]  # (job k reads its strip or tile where the decode put it)
        stages = []  # (the wrapper, the descriptors' address, status, detail, the first job, the jobs)
        if nu:
            stages.append((ctx.unpredict_many_device, ch.upload(desc)) + ch.results("unpredict", nu) + (0, nu))
        if n - nu:
            stages.append((ctx.unshuffle_many_device, ch.upload(fdesc)) + ch.results("unshuffle", n - nu) + (nu, n - nu))
        ch.decode()
        for launch, desc_ptr, stage_status, stage_detail, first, count in stages:
            launch(ch.dec_ptr, ch.out_len_ptr + 8 * first, dst, desc_ptr, stage_status, stage_detail, count, sync=False)
        blocks = ch.finish()
        pixels = pix.cpu().numpy() if pix is not None else None  # the one copy out
    status, detail = blocks["decode"]
    ustatus = np.concatenate([blocks[name][0] for name in ("unpredict", "unshuffle") if name in blocks])
    bad = np.flatnonzero((status != _ffi.OK) | (ustatus != _ffi.OK))
    return pixels, {order[int(k)]: _job_error(run[k], int(status[k]), detail[k], int(ustatus[k])) for k in bad}


def _named(name: str, e: DecompressionError) -> DecompressionError:
    return DecompressionError(e.constructor, "%s: %s" % (name, e.message), e.status, e.detail)


def read_tiff_many(blobs_or_paths: Sequence[Union[str, os.PathLike, bytes, bytearray, memoryview]], ctx: Optional[Context] = None,
                   device_out: Optional[Tuple[int, Sequence[int], Sequence[int]]] = None, float_predictor: bool = False, lzw: bool = False) -> List[Union[List[TiffImage], Exception]]:
    """Per file the list of its pages, or in its place the exception that read_tiff would raise for it: a bad file never disturbs its
    neighbours.  float_predictor=True: pages with Predictor 3 are read (floating-point samples of 16, 32 or 64 bits) -- their strips and
    tiles go through one pzg_unshuffle_many launch behind the pzg_unpredict_many launch of the others; without it such a page is the
    NotImplementedError it has always been.  device_out = (ptr, offsets, strides), one entry per page in order -- the pages of all the files that parse_tiff
    reads and the reader supports, counted through the batch: row y of that page lands at ptr + offsets[k] + y * strides[k] (plane p
    of a PlanarConfiguration 2 page H * strides[k] further on for every p) in device memory of the caller's (a torch tensor's
    data_ptr()), nothing is copied out and `data` is None."""
    results: List[Union[List[TiffImage], Exception, None]] = [None] * len(blobs_or_paths)
    names, files, jobs, at, flat = [], [], [], 0, 0  # files: (index, pages, [(pixel offset, bytes) per page])
    for f, src in enumerate(blobs_or_paths):
        name = "#%d" % f
        try:
            path, blob = load(src)
            name = path or name
            pages = parse_tiff(blob, name)
            for pg in pages:
                _check_supported(name, pg, float_predictor, lzw, blob)
            places, mine = [], []
            for pg in pages:
                rb = pg.row_bytes(pg.width)
                if device_out is not None:
                    base, stride = int(device_out[1][flat + len(places)]), int(device_out[2][flat + len(places)])
                    if stride < rb:
                        raise ValueError("device_out: a stride below the page's row bytes")
                else:
                    base, stride = at, rb
                    at += (pg.planes * pg.height * rb + 15) & ~15
                places.append((base, pg.planes * pg.height * rb))
                mine += _page_jobs(f, blob, pg, base, stride, pg.height * stride)
            flat += len(pages)
            jobs += mine
            files.append((f, pages, places))
        except (ValueError, NotImplementedError, OSError) as e:
            results[f] = e
        names.append(name)
    if not jobs:
        return results
    pixels, errors = _run(ctx or default_context(), jobs, at, int(device_out[0]) if device_out is not None else None)
    first_error = {}
    for k in sorted(errors):
        first_error.setdefault(jobs[k].file, errors[k])
    for f, pages, places in files:
        if f in first_error:
            results[f] = _named(names[f], first_error[f])
        else:
            results[f] = [_image(pg, pixels[o:o + nb].copy() if pixels is not None else None) for pg, (o, nb) in zip(pages, places)]
    return results


def read_tiff(blob_or_path, page: int = 0, ctx: Optional[Context] = None, float_predictor: bool = False, lzw: bool = False) -> TiffImage:
    """One page of one file.  Raises what read_tiff_many would put in the file's place."""
    r = read_tiff_many([blob_or_path], ctx, float_predictor=float_predictor, lzw=lzw)[0]
    if isinstance(r, Exception):
        raise r
    if not 0 <= page < len(r):
        raise ValueError("page %d of a file of %d" % (page, len(r)))
    return r[page]


def read_tiff_region(blob_or_path, page: int, y0: int, x0: int, h: int, w: int, ctx: Optional[Context] = None, float_predictor: bool = False, lzw: bool = False) -> np.ndarray:
    """The rectangle of h rows from y0 and w pixels from x0 of a page: read_tiff(...).data[y0:y0 + h, x0:x0 + w] ([:, y0:.., x0:..] of a
    PlanarConfiguration 2 page), decoding only the strips or tiles that cover it; each is clipped to the rectangle on the device."""
    path, blob = load(blob_or_path)
    name = path or "#0"
    pages = parse_tiff(blob, name)
    if not 0 <= page < len(pages):
        raise ValueError("%s: page %d of a file of %d" % (name, page, len(pages)))
    pg = pages[page]
    _check_supported(name, pg, float_predictor, lzw, blob)
    if h <= 0 or w <= 0 or y0 < 0 or x0 < 0 or y0 + h > pg.height or x0 + w > pg.width:
        raise ValueError("%s: page %d: the rectangle %d x %d at (%d, %d) lies outside the image of %d x %d" % (name, page, w, h, x0, y0, pg.width, pg.height))
    if pg.bits < 8:
        raise NotImplementedError("%s: page %d: regions of %d-bit images are not read" % (name, page, pg.bits))
    px = pg.stored_samples * pg.bits // 8
    rb = w * px
    jobs = _page_jobs(0, blob, pg, 0, rb, h * rb, (y0, x0 * px, h, rb))
    pixels, errors = _run(ctx or default_context(), jobs, pg.planes * h * rb, None)
    if errors:
        raise _named(name, errors[min(errors)])
    flat = pixels[:pg.planes * h * rb].copy().view(_dtype(pg))
    return flat.reshape(pg.samples, h, w) if pg.planar == 2 else flat.reshape(h, w, pg.samples)


def test_tiff_many(blobs_or_paths, ctx: Optional[Context] = None, float_predictor: bool = False, lzw: bool = False) -> List[Tuple[Union[int, str], str]]:
    """[(index or path, problem)] for every file read_tiff would refuse."""
    out = []
    for k, (src, r) in enumerate(zip(blobs_or_paths, read_tiff_many(blobs_or_paths, ctx, float_predictor=float_predictor, lzw=lzw))):
        if isinstance(r, Exception):
            out.append((k if isinstance(src, (bytes, bytearray, memoryview)) else os.fspath(src), str(r)))
    return out


test_tiff_many.__test__ = False  # (not a pytest test, whatever imports it)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) >= 2 and argv[0] == "-t":
        files = [a for a in argv[1:] if a not in ("--float-predictor", "--lzw")]
        if not files:
            print("usage: python -m pure_zlib_amd.tiff -t [--float-predictor] [--lzw] A.tif B.tif ...", file=sys.stderr)
            return 2
        bad = test_tiff_many(files, float_predictor="--float-predictor" in argv[1:], lzw="--lzw" in argv[1:])
        for name, why in bad:
            print("%s: %s" % (name, why))
        print("%d file(s): %s" % (len(files), "%d bad" % len(bad) if bad else "OK"))
        return 1 if bad else 0
    print("usage: python -m pure_zlib_amd.tiff -t [--float-predictor] [--lzw] A.tif B.tif ...", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
