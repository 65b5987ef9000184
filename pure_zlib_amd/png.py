"""PNG images decoded in batches on the GPU: EXTENSION, the reference has no image reader.

A PNG's IDAT chunks are ONE RFC 1950 stream and IHDR gives its exact decoded size, height * (1 + row_bytes), so a batch of images
is one pzg_decompress_many launch with exact capacities -- no capacity guess, no relaunch -- and one pzg_unfilter_many launch behind
it on the same stream, which takes the decode's out_len array as its src_len: the scanline filters (PNG specification section 9)
are undone on the device, a wavefront per image, and only the pixels come back, in one copy.  The host parses the chunks and
checks their CRC-32s with the system's zlib; nothing is inflated on the CPU.  Device memory is held in torch tensors.

    read_png_many(blobs_or_paths)  -> [PngImage, or the DecompressionError / ValueError / NotImplementedError of that image]
    read_png(blob_or_path)         -> PngImage                  (raises)
    read_png_batch(blobs_or_paths) -> (one (N, H, W, C) uint8 torch tensor on the device, [(index, exception)])
    test_png_many(blobs_or_paths)  -> [(index_or_name, problem)]   (empty: every image is sound)
    python -m pure_zlib_amd.png -t [--adam7] A.png B.png ...

Colour types 0, 2, 3, 4 and 6 at their legal bit depths.  Without `expand`, `data` is the samples as the file stores them: packed
rows below 8 bits, palette indices, big-endian 16-bit samples, tRNS as raw bytes.  With expand="rgba8" or "rgb8" one more launch,
pzg_expand_many, behind the others on the same stream turns them into (H, W, 4 | 3) uint8 pixels on the device, whatever the file's
type: the palette is looked up (tRNS as its alpha), gray below 8 bits is scaled by bit replication, a 16-bit sample gives its high
byte, gray fans out to R = G = B, a tRNS colour key makes its pixels transparent (compared at the file's depth), and "rgb8" drops
alpha.  The unfilter and Adam7 launches then deliver into a device scratch in the file's format, and the expansion writes the pixel
buffer (or device_out, whose offsets and strides then describe the EXPANDED rows).  Still one sync and one copy out.  Not done:
16-bit or gray output, compositing over a background, gamma, sBIT.  expand=None issues exactly the launches it always did.

Adam7-interlaced images are read with adam7=True (--adam7); without it such an image is NotImplementedError, for that image only,
and nothing else changes.  An interlaced image's stream is its seven reduced images, each filtered on its own, so its exact decoded
size is the sum of ph * (1 + prb) over the passes that have pixels; each such pass is one job of a second pzg_unfilter_many launch
-- its src_off inside the image's decoded stream, its exact size as src_len, delivered dense into a device scratch -- and one
pzg_adam7_many launch behind it on the same stream weaves the passes into the pixel buffer (or into device_out at the caller's
offsets and strides).  Still one sync and one copy out; nothing is deinterlaced on the host, and `data` is what a non-interlaced
file of the same pixels gives.  A batch without interlaced images issues exactly the two launches above.
"""
import os
import struct
import sys
import zlib as _sys_zlib  # crc32 of the chunks only
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from ._batch import DeviceChain, load, pack
from .zlib import EXPAND_DESC, Context, DecompressionError, default_context, error_from_status

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


@dataclass
class PngImage:
    width: int
    height: int
    color_type: int
    bit_depth: int
    palette: Optional[bytes]  # PLTE as it stands (3 bytes an entry), or None
    trns: Optional[bytes]     # tRNS as it stands, or None
    data: Optional[np.ndarray]  # (H, W, C) uint8 | (H, W, C) >u2 | (H, row_bytes) packed uint8 below 8 bits; None with device_out
    expanded: Optional[str] = None  # "rgba8" | "rgb8": data (or device_out) holds (H, W, 4 | 3) uint8 pixels; None: the file's samples

    @property
    def channels(self) -> int:
        return _CHANNELS[self.color_type]

    @property
    def row_bytes(self) -> int:
        return (self.width * self.channels * self.bit_depth + 7) // 8

    @property
    def bpp(self) -> int:
        return max(1, self.channels * self.bit_depth // 8)


def _format_error(msg: str) -> DecompressionError:
    return DecompressionError("FormatError", msg, _ffi.E_FILTER)


# Adam7 (PNG specification 8.2): (x0, y0, dx, dy) of the passes 1 .. 7
_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def _passes(img: PngImage) -> List[Tuple[int, int, int]]:
    """[(pass 1 .. 7, its rows, the bytes of one)] of the passes of an interlaced image that have pixels."""
    out, bits = [], img.channels * img.bit_depth
    for p, (x0, y0, dx, dy) in enumerate(_ADAM7):
        pw, ph = -(-(img.width - x0) // dx), -(-(img.height - y0) // dy)
        if pw > 0 and ph > 0:
            out.append((p + 1, ph, (pw * bits + 7) // 8))
    return out


_EXPAND = {"rgba8": (_ffi.PIX_RGBA8, 4), "rgb8": (_ffi.PIX_RGB8, 3)}  # expand -> (out_format, bytes of a pixel)


def _check_trns(name: str, img: PngImage) -> None:
    """What the expansion needs of tRNS (PNG specification 11.3.2): a key of one or three 16-bit values, or at most one alpha per
    palette entry; none where the image has an alpha channel."""
    if img.trns is None:
        return
    if img.color_type in (4, 6):
        raise ValueError("%s: tRNS in an image of colour type %d, which has an alpha channel" % (name, img.color_type))
    if img.color_type == 3:
        if not 1 <= len(img.trns) <= len(img.palette) // 3:
            raise ValueError("%s: tRNS of %d entries for a palette of %d" % (name, len(img.trns), len(img.palette) // 3))
    elif len(img.trns) != 2 * img.channels:
        raise ValueError("%s: tRNS of %d bytes in an image of colour type %d" % (name, len(img.trns), img.color_type))


def _parse(name: str, blob: bytes, adam7: bool = False, expand: bool = False) -> Tuple[PngImage, bytes, bool]:
    """(the image without its data, its IDAT payloads joined, whether it is interlaced); raises ValueError / NotImplementedError
    naming the image.  expand: tRNS is held to its colour type as well (without it, it is passed on as it stands)."""
    if blob[:8] != SIGNATURE:
        raise ValueError("%s: not a PNG file (bad signature)" % name)
    at, img, idat, seen_idat, idat_closed, palette, trns, laced = 8, None, [], False, False, None, None, False
    while True:
        if at + 12 > len(blob):
            raise ValueError("%s: file ends inside a chunk (no IEND)" % name)
        length, kind = struct.unpack_from(">I4s", blob, at)
        if at + 12 + length > len(blob):
            raise ValueError("%s: chunk %s runs past the end of the file" % (name, kind.decode("latin-1")))
        body = blob[at + 8:at + 8 + length]
        crc, = struct.unpack_from(">I", blob, at + 8 + length)
        have = _sys_zlib.crc32(body, _sys_zlib.crc32(kind))
        if crc != have:
            raise ValueError("%s: chunk %s: checksum mismatch: %08x != %08x" % (name, kind.decode("latin-1"), crc, have))
        at += 12 + length
        if img is None and kind != b"IHDR":
            raise ValueError("%s: the first chunk is %s, not IHDR" % (name, kind.decode("latin-1")))
        if kind == b"IHDR":
            if img is not None or length != 13:
                raise ValueError("%s: bad IHDR" % name)
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if ctype not in _DEPTHS or depth not in _DEPTHS[ctype]:
                raise ValueError("%s: colour type %d with bit depth %d is not a PNG image type" % (name, ctype, depth))
            if w == 0 or h == 0 or w >> 31 or h >> 31 or comp != 0 or filt != 0 or lace > 1:
                raise ValueError("%s: bad IHDR (size %d x %d, compression %d, filter %d, interlace %d)" % (name, w, h, comp, filt, lace))
            if lace == 1 and not adam7:
                raise NotImplementedError("%s: Adam7-interlaced images are read with adam7=True (--adam7) only" % name)
            laced = lace == 1
            img = PngImage(w, h, ctype, depth, None, None, None)
            if img.row_bytes >> 32:
                raise ValueError("%s: a row of %d bytes" % (name, img.row_bytes))
        elif kind == b"IDAT":
            if idat_closed:
                raise ValueError("%s: IDAT chunks are not consecutive" % name)
            seen_idat = True
            idat.append(body)
        elif kind == b"IEND":
            break
        else:
            idat_closed = seen_idat
            if kind == b"PLTE":
                if length % 3 or length == 0 or length > 768 or seen_idat:
                    raise ValueError("%s: bad PLTE" % name)
                palette = body
            elif kind == b"tRNS":
                trns = body
            elif not kind[0] & 0x20:
                raise ValueError("%s: unknown critical chunk %s" % (name, kind.decode("latin-1")))
    if not seen_idat:
        raise ValueError("%s: no IDAT chunk" % name)
    if img.color_type == 3 and palette is None:
        raise ValueError("%s: a palette image without PLTE" % name)
    img.palette, img.trns = palette, trns
    if expand:
        _check_trns(name, img)
    return img, b"".join(idat), laced


def _shape(img: PngImage, flat: np.ndarray) -> np.ndarray:
    if img.bit_depth == 8:
        return flat.reshape(img.height, img.width, img.channels)
    if img.bit_depth == 16:
        return flat.view(">u2").reshape(img.height, img.width, img.channels)
    return flat.reshape(img.height, img.row_bytes)


def _collect(sources, adam7: bool, expand: Optional[str]):
    """Loads and parses.  (names, results with the exception of every source that cannot be read and None elsewhere, good =
    [(index, image, stream)], laced = [(place in good, its passes)] of the interlaced ones)."""
    results: List[Union[PngImage, Exception, None]] = [None] * len(sources)
    names, good, laced = [], [], []
    for k, src in enumerate(sources):
        name = "#%d" % k
        try:
            path, blob = load(src)
            name = path or name
            img, z, lace = _parse(name, blob, adam7, expand is not None)
            if lace:
                laced.append((len(good), _passes(img)))
            good.append((k, img, z))
        except (ValueError, NotImplementedError, OSError) as e:
            results[k] = e
        names.append(name)
    return names, results, good, laced


@dataclass
class _Layout:
    """Where everything of a batch lies, an entry per good image: dec_cap, the exact decoded size; the file's rows, which the
    unfilter and Adam7 launches deliver at (file_off, file_stride) -- into the pixel buffer, or with `expand` dense into a scratch of
    file_total bytes that the expansion reads; the pixels, pix bytes at (pix_off, pix_stride) of a buffer of pix_total bytes, or
    where device_out says (pix_total is None then).  Offsets, strides, dec_cap and pix are u64."""
    dec_cap: np.ndarray
    row_bytes: np.ndarray  # u32
    height: np.ndarray     # u32
    bpp: np.ndarray        # u8
    file_off: np.ndarray
    file_stride: np.ndarray
    file_total: Optional[int]
    pix_off: np.ndarray
    pix_stride: np.ndarray
    pix: np.ndarray
    pix_total: Optional[int]


def _layout(good, laced, expand: Optional[str], device_out) -> _Layout:
    images = [i for _k, i, _z in good]
    row_bytes = np.array([i.row_bytes for i in images], dtype=np.uint32)
    height = np.array([i.height for i in images], dtype=np.uint32)
    rows, file_rb = height.astype(np.uint64), row_bytes.astype(np.uint64)
    dec_cap = rows * (file_rb + np.uint64(1))
    for j, passes in laced:  # the seven reduced images, each row with its filter byte
        dec_cap[j] = sum(ph * (1 + prb) for _p, ph, prb in passes)
    out_rb = file_rb if expand is None else np.array([i.width * _EXPAND[expand][1] for i in images], dtype=np.uint64)
    if device_out is not None:
        pix_off = np.array([device_out[1][k] for k, _i, _z in good], dtype=np.uint64)
        pix_stride, pix_total = np.array([device_out[2][k] for k, _i, _z in good], dtype=np.uint64), None
        if (pix_stride < out_rb).any():
            raise ValueError("device_out: a stride below the image's row_bytes")
    else:
        (pix_off, pix_total), pix_stride = pack(rows * out_rb), out_rb
    if expand is None:
        file_off, file_stride, file_total = pix_off, pix_stride, None
    else:
        (file_off, file_total), file_stride = pack(rows * file_rb), file_rb
    return _Layout(dec_cap, row_bytes, height, np.array([i.bpp for i in images], dtype=np.uint8), file_off, file_stride, file_total,
                   pix_off, pix_stride, rows * out_rb, pix_total)


_PASS_JOB = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst_off", "<u8"), ("row_bytes", "<u4"), ("height", "<u4"), ("bpp", "u1")])
_WEAVE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("dst_stride", "<u8"), ("width", "<u4"), ("height", "<u4"), ("pixel_bits", "u1")])


def _pass_jobs(good, laced, lay: _Layout, dec_off) -> Tuple[np.ndarray, np.ndarray, int]:
    """(_PASS_JOB[m], _WEAVE[len(laced)], the bytes of the scratch between them).  Every pass that has pixels is one unfilter job,
    from its place in the image's decoded stream (dec_off) dense into the scratch; a weave job puts an image's passes into its rows."""
    scr_off, scr_total = pack([sum(ph * prb for _p, ph, prb in passes) for _j, passes in laced])
    jobs = []
    for (j, passes), d_at in zip(laced, scr_off.tolist()):
        s_at = int(dec_off[j])
        for _p, ph, prb in passes:
            jobs.append((s_at, ph * (1 + prb), d_at, prb, ph, int(lay.bpp[j])))
            s_at += ph * (1 + prb)
            d_at += ph * prb
    weave = [(scr_off[i], lay.file_off[j], lay.file_stride[j], good[j][1].width, good[j][1].height, good[j][1].channels * good[j][1].bit_depth)
             for i, (j, _ps) in enumerate(laced)]
    return np.array(jobs, dtype=_PASS_JOB), np.array(weave, dtype=_WEAVE), scr_total


def _run(ctx: Context, good, laced, lay: _Layout, expand: Optional[str], out_ptr: Optional[int]):
    """The launches.  Returns (out_len, {launch: (status, detail)}, the pixel buffer on the host or None, bad_index)."""
    n, plain = len(good), len(laced) < len(good)  # (a batch of interlaced images only has nothing for the first unfilter launch)
    with DeviceChain(ctx, [(z, 0, len(z)) for _k, _i, z in good], lay.dec_cap) as ch:
        pix = ch.scratch(lay.pix_total) if out_ptr is None else None
        pix_ptr = out_ptr if pix is None else pix.data_ptr()
        rows = ch.scratch(lay.file_total) if expand is not None else None
        rows_ptr = pix_ptr if rows is None else rows.data_ptr()
        if plain:
            height = lay.height.copy()
            height[[j for j, _ps in laced]] = 0  # (no rows: this launch neither reads nor writes an interlaced image)
            u_dst_off, u_stride, u_row_bytes, u_height, u_bpp = (ch.upload(a) for a in (lay.file_off, lay.file_stride, lay.row_bytes, height, lay.bpp))
            u_status, u_detail = ch.results("unfilter", n)
        if laced:
            jobs, weave, scr_total = _pass_jobs(good, laced, lay, ch.dec_off)
            scr_ptr = ch.scratch(scr_total).data_ptr()
            j_src_off, j_src_len, j_dst_off, j_stride, j_row_bytes, j_height, j_bpp = (ch.upload(a) for a in (
                jobs["src_off"], jobs["src_len"], jobs["dst_off"], jobs["row_bytes"].astype(np.uint64), jobs["row_bytes"], jobs["height"], jobs["bpp"]))
            w_src_off, w_dst_off, w_stride, w_width, w_height, w_bits = (ch.upload(weave[f]) for f in _WEAVE.names)
            j_status, j_detail = ch.results("passes", len(jobs))
            w_status, _no_detail = ch.results("adam7", len(weave))
        if expand is not None:
            desc, pal = _expand_descriptors([i for _k, i, _z in good], lay.file_off, lay.file_stride, lay.pix_off, lay.pix_stride, _EXPAND[expand][0])
            x_desc, x_pal = ch.upload(desc), ch.upload(pal)
            x_status, x_detail = ch.results("expand", n)
        ch.decode()
        if plain:
            ctx.unfilter_many_device(ch.dec_ptr, ch.dec_off_ptr, ch.out_len_ptr, rows_ptr, u_dst_off, u_stride, u_row_bytes, u_height, u_bpp, u_status,
                                     u_detail, n, sync=False)
        if laced:
            ctx.unfilter_many_device(ch.dec_ptr, j_src_off, j_src_len, scr_ptr, j_dst_off, j_stride, j_row_bytes, j_height, j_bpp, j_status, j_detail,
                                     len(jobs), sync=False)
            ctx.adam7_many_device(scr_ptr, w_src_off, rows_ptr, w_dst_off, w_stride, w_width, w_height, w_bits, w_status, 0, len(weave), sync=False)
        if expand is not None:
            ctx.expand_many_device(rows_ptr, pix_ptr, x_pal, x_desc, x_status, x_detail, n, sync=False)
        blocks = ch.finish()
        bad_index = _bad_indices(good, lay, blocks["expand"], rows) if expand is not None else {}
        return ch.out_len(), blocks, pix.cpu().numpy() if pix is not None else None, bad_index  # (the pixels: the one copy out)


def _bad_indices(good, lay: _Layout, expansion, rows) -> dict:
    """{place in good: (row, x, the index found there) of an image the expansion refused; () where it refused for another reason}"""
    out, (xstatus, xdetail) = {}, expansion
    for j in np.flatnonzero(xstatus != _ffi.OK):
        row, x, depth = int(xdetail[j, 0]), int(xdetail[j, 1]), good[j][1].bit_depth
        if int(xstatus[j]) != _ffi.E_PALETTE:
            out[int(j)] = ()
            continue
        byte = int(rows[int(lay.file_off[j]) + row * int(lay.file_stride[j]) + x * depth // 8])  # (one byte back: the index itself)
        out[int(j)] = (row, x, (byte >> (8 - depth - x * depth % 8)) & ((1 << depth) - 1))
    return out


def _pass_errors(laced, blocks) -> dict:
    """{place in good: (pass or 0 for the deinterlacing, status, detail 0, detail 1)}: what an image's passes and its
    deinterlacing say, the first pass in pass order first."""
    if not laced:
        return {}
    out, at, (jstatus, jdetail), (astatus, _none) = {}, 0, blocks["passes"], blocks["adam7"]
    for i, (j, passes) in enumerate(laced):
        for t, (pno, _ph, _prb) in enumerate(passes):
            if j not in out and int(jstatus[at + t]) != _ffi.OK:
                out[j] = (pno, int(jstatus[at + t]), int(jdetail[at + t, 0]), int(jdetail[at + t, 1]))
        if j not in out and int(astatus[i]) != _ffi.OK:
            out[j] = (0, int(astatus[i]), 0, 0)
        at += len(passes)
    return out


def _verdict(name: str, img: PngImage, z: bytes, decode, unfilter, pass_error, bad_index, out_len: int, dec_cap: int) -> Optional[Exception]:
    """The error of one image, or None: the first of what the decode, the passes, the unfilter and the expansion say.  decode,
    unfilter: (status, its detail pair); pass_error: an entry of _pass_errors or None; bad_index: one of _bad_indices or None."""
    (st, detail), (ust, (row, ft)) = decode, unfilter
    if st == _ffi.E_OUT_TOO_SMALL:
        return _format_error("%s: too much image data" % name)
    if st != _ffi.OK:
        e = error_from_status(z, st, detail)
        return DecompressionError(e.constructor, "%s: %s" % (name, e.message), e.status, e.detail)
    if out_len != dec_cap:
        return _format_error("%s: not enough image data" % name)
    if pass_error is not None:
        pno, pst, d0, d1 = pass_error
        if pno and pst == _ffi.E_FILTER:
            return DecompressionError("FormatError", "%s: pass %d: row %d has filter type %d" % (name, pno, d0, d1), pst, (d0, d1))
        return _format_error("%s: the image's passes could not be put together" % name)
    if ust == _ffi.E_FILTER:
        return DecompressionError("FormatError", "%s: row %d has filter type %d" % (name, int(row), int(ft)), ust, (int(row), int(ft)))
    if ust != _ffi.OK:
        return _format_error("%s: not enough image data" % name)
    if bad_index is not None:
        if not bad_index:
            return _format_error("%s: the image's pixels could not be expanded" % name)
        row, x, index = bad_index
        return DecompressionError("FormatError", "%s: row %d, pixel %d: palette index %d of %d" % (name, row, x, index, len(img.palette) // 3),
                                  _ffi.E_PALETTE, (row, x))
    return None


def read_png_many(blobs_or_paths: Sequence[Union[str, os.PathLike, bytes, bytearray, memoryview]], ctx: Optional[Context] = None,
                  device_out: Optional[Tuple[int, Sequence[int], Sequence[int]]] = None, adam7: bool = False,
                  expand: Optional[str] = None) -> List[Union[PngImage, Exception]]:
    """Every image of the batch, or in its place the exception that read_png would raise for it: a bad image never disturbs its
    neighbours.  device_out = (ptr, offsets, strides): the rows of image i land at ptr + offsets[i] + r * strides[i] in device
    memory of the caller's (a torch tensor's data_ptr()), nothing is copied out and `data` is None.  adam7: Adam7-interlaced
    images are read too, deinterlaced on the device (without it each is NotImplementedError).  expand = "rgba8" | "rgb8": `data` is
    (H, W, 4 | 3) uint8 pixels for every colour type, expanded on the device (the module's docstring has the rules), and device_out's
    offsets and strides describe those rows; an image with an error may leave anything in its own rows there."""
    if expand is not None and expand not in _EXPAND:
        raise ValueError("expand: None, 'rgba8' or 'rgb8', not %r" % (expand,))
    names, results, good, laced = _collect(blobs_or_paths, adam7, expand)
    if not good:
        return results
    lay = _layout(good, laced, expand, device_out)
    out_len, blocks, pixels, bad_index = _run(ctx or default_context(), good, laced, lay, expand, int(device_out[0]) if device_out is not None else None)
    pass_error, (dstatus, ddetail) = _pass_errors(laced, blocks), blocks["decode"]
    ustatus, udetail = blocks.get("unfilter", (np.zeros(len(good), np.int32), np.zeros((len(good), 2), np.uint32)))
    for j, (k, img, z) in enumerate(good):
        results[k] = _verdict(names[k], img, z, (int(dstatus[j]), ddetail[j]), (int(ustatus[j]), udetail[j]), pass_error.get(j), bad_index.get(j),
                              int(out_len[j]), int(lay.dec_cap[j]))
        if results[k] is None:
            if pixels is not None:
                flat = pixels[int(lay.pix_off[j]):int(lay.pix_off[j]) + int(lay.pix[j])].copy()
                img.data = _shape(img, flat) if expand is None else flat.reshape(img.height, img.width, _EXPAND[expand][1])
            img.expanded = expand
            results[k] = img
    return results


def _expand_descriptors(images: Sequence[PngImage], src_off, src_stride, dst_off, dst_stride, out_format: int) -> Tuple[np.ndarray, np.ndarray]:
    """(the pzg_expand_desc of every image, the palettes one behind the other as R, G, B, A entries -- PLTE with tRNS as its alpha,
    255 where tRNS has none)."""
    desc = np.zeros(len(images), dtype=EXPAND_DESC)
    desc["src_off"], desc["src_stride"], desc["dst_off"], desc["dst_stride"] = src_off, src_stride, dst_off, dst_stride
    desc["out_format"] = out_format
    pals, at = [], 0
    for d, img in zip(desc, images):
        d["width"], d["height"], d["color_type"], d["bit_depth"] = img.width, img.height, img.color_type, img.bit_depth
        if img.color_type == 3:
            entries = np.full((len(img.palette) // 3, 4), 255, dtype=np.uint8)
            entries[:, :3] = np.frombuffer(img.palette, dtype=np.uint8).reshape(-1, 3)
            if img.trns is not None:
                entries[:len(img.trns), 3] = np.frombuffer(img.trns, dtype=np.uint8)
            d["pal_off"], d["pal_len"] = at, len(entries)
            pals.append(entries)
            at += len(entries)
        elif img.trns is not None:
            d["has_key"] = 1
            d["key"][:img.channels] = struct.unpack(">%dH" % img.channels, img.trns)
    pals.append(np.zeros((1, 4), dtype=np.uint8))  # (never empty)
    return desc, np.concatenate(pals).view("<u4").reshape(-1)


def read_png(blob_or_path, ctx: Optional[Context] = None, adam7: bool = False, expand: Optional[str] = None) -> PngImage:
    """One image.  Raises what read_png_many would put in its place."""
    r = read_png_many([blob_or_path], ctx, adam7=adam7, expand=expand)[0]
    if isinstance(r, Exception):
        raise r
    return r


def read_png_batch(blobs_or_paths, expand: str = "rgb8", adam7: bool = False, ctx: Optional[Context] = None):
    """Images that all share one size as ONE (N, H, W, C) uint8 torch tensor on the context's device, C = 4 ("rgba8") or 3 ("rgb8"):
    read_png_many(..., expand=expand) delivering straight into it.  H and W are those of the first image whose IHDR can be read.
    Returns (tensor, errors), errors = [(index, exception)]: an image of another size or with an error of its own is listed there,
    and its slab of the tensor is zero."""
    import torch
    ctx = ctx or default_context()
    channels, n = _EXPAND[expand][1], len(blobs_or_paths)
    blobs, sizes, errors = [], [], {}
    for k, src in enumerate(blobs_or_paths):
        try:
            blobs.append(load(src)[1])
        except OSError as e:
            blobs.append(b"")
            errors[k] = e
        b = blobs[-1]
        sizes.append(struct.unpack_from(">II", b, 16) if b[:8] == SIGNATURE and b[12:16] == b"IHDR" and len(b) >= 24 else None)
    size = next((s for s in sizes if s is not None and 0 < s[0] < 1 << 31 and 0 < s[1] < 1 << 31), None)
    if size is None:
        raise ValueError("read_png_batch: no image of the batch has a readable IHDR")
    w, h = size
    out = torch.zeros((n, h, w, channels), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    mine = [k for k in range(n) if k not in errors and sizes[k] in (size, None)]  # (None: read_png_many says what is wrong with it)
    for k in range(n):
        if k not in errors and k not in mine:
            errors[k] = ValueError("#%d: an image of %d x %d in a batch of %d x %d" % (k, sizes[k][0], sizes[k][1], w, h))
    slab = h * w * channels
    got = read_png_many([blobs[k] for k in mine], ctx, device_out=(out.data_ptr(), {j: k * slab for j, k in enumerate(mine)},
                                                                   {j: w * channels for j in range(len(mine))}), adam7=adam7, expand=expand)
    for k, r in zip(mine, got):
        if isinstance(r, Exception):
            errors[k] = r
            out[k].zero_()
    return out, sorted(errors.items())


def test_png_many(blobs_or_paths, ctx: Optional[Context] = None, adam7: bool = False) -> List[Tuple[Union[int, str], str]]:
    """What `pngcheck` does for a batch: [(index or path, problem)] for every image read_png would refuse."""
    out = []
    for k, (src, r) in enumerate(zip(blobs_or_paths, read_png_many(blobs_or_paths, ctx, adam7=adam7))):
        if isinstance(r, Exception):
            out.append((k if isinstance(src, (bytes, bytearray, memoryview)) else os.fspath(src), str(r)))
    return out


test_png_many.__test__ = False  # (not a pytest test, whatever imports it)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) >= 2 and argv[0] == "-t":
        adam7 = "--adam7" in argv[1:]
        files = [a for a in argv[1:] if a != "--adam7"]
        if files:
            bad = test_png_many(files, adam7=adam7)
            for name, why in bad:
                print("%s: %s" % (name, why))
            print("%d image(s): %s" % (len(files), "%d bad" % len(bad) if bad else "OK"))
            return 1 if bad else 0
    print("usage: python -m pure_zlib_amd.png -t [--adam7] A.png B.png ...", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
