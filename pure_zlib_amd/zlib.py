"""Host-side mirror of the reference module `Codec.Compression.Zlib`
(src/Codec/Compression/Zlib.hs:3-8) over the C ABI of include/pzg.h.

    decompress      :: L.ByteString   -> Either DecompressionError L.ByteString   (Zlib.hs:32)
    decompressMany  :: [L.ByteString] -> [Either DecompressionError L.ByteString]  (new, batched)

Same names, argument meaning and error behaviour as the reference: a lazy ByteString is a
`bytes` (one chunk) or a sequence of `bytes` chunks; the result is `Right(bytes)` or
`Left(DecompressionError)` whose `show` text equals the reference's.  All decoding happens in the
HIP kernels behind libpzg.so; nothing here inflates on the CPU.
"""
import ctypes as C
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _ffi
from ._batch import pack

# ---- DecompressionError (Monad.hs:87-104) -------------------------------------------------------

_SHOW_PREFIX = {
    "HuffmanTreeError": "Huffman tree manipulation error: ",
    "FormatError": "Block format error: ",
    "DecompressionError": "Decompression error: ",
    "HeaderError": "Header error: ",
    "ChecksumError": "Checksum error: ",
    # outcomes on which the reference throws a Haskell exception instead of returning Left
    # (SURVEY.md 8a a7/a16); this build reports them as a value
    "ReferenceThrows": "",
}


class DecompressionError(Exception):
    """`data DecompressionError = HuffmanTreeError String | FormatError String | DecompressionError String
    | HeaderError String | ChecksumError String  deriving (Eq)` with the reference's custom Show."""

    def __init__(self, constructor: str, message: str, status: int = -1, detail=(0, 0)):
        super().__init__(constructor, message)
        self.constructor = constructor
        self.message = message
        self.status = status
        self.detail = tuple(detail)

    def show(self) -> str:
        return _SHOW_PREFIX[self.constructor] + self.message

    __str__ = show

    def __repr__(self):
        return f"{self.constructor} {self.message!r}"

    def __eq__(self, other):
        return (isinstance(other, DecompressionError) and self.constructor == other.constructor
                and self.message == other.message)

    def __hash__(self):
        return hash((self.constructor, self.message))


def HuffmanTreeError(s):
    return DecompressionError("HuffmanTreeError", s)


def FormatError(s):
    return DecompressionError("FormatError", s)


def DecompressionError_(s):
    return DecompressionError("DecompressionError", s)


def HeaderError(s):
    return DecompressionError("HeaderError", s)


def ChecksumError(s):
    return DecompressionError("ChecksumError", s)


@dataclass(frozen=True)
class Left:
    value: DecompressionError

    def is_right(self):
        return False


@dataclass(frozen=True)
class Right:
    value: bytes

    def is_right(self):
        return True


Either = Union[Left, Right]
LazyByteString = Union[bytes, bytearray, memoryview, Sequence[bytes]]

# pzg_expand_desc (include/pzg.h) as a numpy record: one image of Context.expand_many
EXPAND_DESC = np.dtype([("src_off", "<u8"), ("src_stride", "<u8"), ("dst_off", "<u8"), ("dst_stride", "<u8"), ("width", "<u4"), ("height", "<u4"),
                        ("pal_off", "<u4"), ("pal_len", "<u2"), ("key", "<u2", (3,)), ("color_type", "u1"), ("bit_depth", "u1"), ("out_format", "u1"),
                        ("has_key", "u1"), ("reserved", "<u4", (2,))])
assert EXPAND_DESC.itemsize == 64

# pzg_unpredict_desc (include/pzg.h) as a numpy record: one strip or tile of Context.unpredict_many
UNPREDICT_DESC = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("dst_stride", "<u8"), ("src_row_bytes", "<u4"), ("rows", "<u4"), ("win_row", "<u4"),
                           ("win_rows", "<u4"), ("win_byte", "<u4"), ("win_bytes", "<u4"), ("predictor", "u1"), ("sample_bytes", "u1"), ("samples", "u1"),
                           ("big_endian", "u1"), ("reserved", "<u4", (3,))])
assert UNPREDICT_DESC.itemsize == 64

# pzg_unshuffle_desc (include/pzg.h) as a numpy record: one strip, tile or chunk of Context.unshuffle_many
UNSHUFFLE_DESC = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("dst_stride", "<u8"), ("src_row_bytes", "<u4"), ("rows", "<u4"), ("win_row", "<u4"),
                           ("win_rows", "<u4"), ("win_byte", "<u4"), ("win_bytes", "<u4"), ("elem_bytes", "u1"), ("sum_stride", "u1"), ("reverse", "u1"),
                           ("reserved0", "u1"), ("reserved", "<u4", (3,))])
assert UNSHUFFLE_DESC.itemsize == 64

_STATUS_CONSTRUCTOR = {
    _ffi.E_TRUNCATED: "DecompressionError",
    _ffi.E_HDR_FCHECK: "HeaderError",
    _ffi.E_HDR_METHOD: "HeaderError",
    _ffi.E_HDR_WINDOW: "HeaderError",
    _ffi.E_FMT_LEN_NLEN: "FormatError",
    _ffi.E_FMT_BTYPE: "FormatError",
    _ffi.E_HUFF_BUILD: "HuffmanTreeError",
    _ffi.E_HUFF_EMPTY_TREE: "HuffmanTreeError",
    _ffi.E_HUFF_EMPTY_BRANCH: "HuffmanTreeError",
    _ffi.E_CHECKSUM: "ChecksumError",
    _ffi.E_BAD_DISTANCE: "ReferenceThrows",
    _ffi.E_BAD_LITLEN_SYMBOL: "ReferenceThrows",
    _ffi.E_BAD_DIST_SYMBOL: "ReferenceThrows",
    _ffi.E_DATA_REMAINING: "DecompressionError",
    _ffi.E_GZIP_HEADER: "HeaderError",   # extension (PZG_GZIP): the reference has no gzip
    _ffi.E_GZIP_ISIZE: "ChecksumError",
    _ffi.E_DICT: "HeaderError",         # extension (preset dictionaries)
    _ffi.E_FILTER: "FormatError",       # extension (pzg_unfilter_many)
    _ffi.E_PALETTE: "FormatError",      # extension (pzg_expand_many)
    _ffi.E_LZW: "FormatError",          # extension (pzg_unlzw_many)
}


def error_from_status(stream: bytes, status: int, detail) -> DecompressionError:
    """Rebuild the reference's DecompressionError (constructor + exact message) from the ABI's
    (status, detail) pair via pzg_error_message()."""
    d = (C.c_uint32 * 2)(int(detail[0]), int(detail[1]))
    buf = C.create_string_buffer(256)
    _ffi.lib().pzg_error_message(stream, len(stream), int(status), d, buf, len(buf))
    text = buf.value.decode()
    cons = _STATUS_CONSTRUCTOR.get(int(status), "ReferenceThrows")
    prefix = _SHOW_PREFIX[cons]
    msg = text[len(prefix):] if prefix and text.startswith(prefix) else text
    return DecompressionError(cons, msg, int(status), (int(detail[0]), int(detail[1])))


# ---- context ---------------------------------------------------------------------------------------


class Context:
    """One pzg_ctx (HIP device + stream + staging arenas)."""

    def __init__(self, device: int = 0, device_mask: Optional[int] = None, devices: Optional[Sequence[int]] = None):
        """device: one HIP device.  device_mask: several devices of one node (bit d = device d, 0 = all visible):
        decompress_many then shards a host batch over them inside the library (pzg_init_mask).  devices: the same with
        the devices named one by one, one shard per entry (pzg_init_devices; a device may appear more than once)."""
        L = _ffi.lib()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            _ffi.check(L.pzg_init_devices(arr, len(devices), C.byref(h)))
        elif device_mask is None:
            _ffi.check(L.pzg_init(device, C.byref(h)))
        else:
            _ffi.check(L.pzg_init_mask(device_mask, C.byref(h)))
        self._h = h
        self._L = L
        self.device = device

    @property
    def device_count(self) -> int:
        return int(self._L.pzg_device_count(self._h))

    def close(self):
        """pzg_shutdown: drops this handle.  DecoderPools made from the context stay usable and free the device state
        when the last of them is closed (the library counts references; include/pzg.h "Lifetimes")."""
        if self._h:
            self._L.pzg_shutdown(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_stream(self, hip_stream: Optional[int]):
        """Launch on an existing hipStream_t (integer handle; 0/None = HIP's default stream)."""
        _ffi.check(self._L.pzg_set_stream(self._h, C.c_void_p(hip_stream or 0)), self._h)

    def reset_stream(self):
        _ffi.check(self._L.pzg_reset_stream(self._h), self._h)

    def set_ring_bits(self, ring_bits: int):
        """LDS near-ring size class (11..15; 15 = the whole 32 KiB window in LDS).  Results are identical."""
        _ffi.check(self._L.pzg_set_option(self._h, _ffi.OPT_RING_BITS, int(ring_bits)), self._h)

    def set_host_threads(self, n: int):
        """Helper threads of the staged host-pointer path and of the decoders' feeds (PZG_OPT_HOST_THREADS)."""
        _ffi.check(self._L.pzg_set_option(self._h, _ffi.OPT_HOST_THREADS, int(n)), self._h)

    def set_scratch_bytes(self, nbytes: int):
        """Upper bound, per device, on the scratch the library allocates for its inflate kernels (PZG_OPT_SCRATCH_BYTES; 0: no bound)."""
        _ffi.check(self._L.pzg_set_option(self._h, _ffi.OPT_SCRATCH_BYTES, int(nbytes)), self._h)

    def set_bundles(self, mode: int):
        """PZG_OPT_BUNDLES: device-pointer launches take their streams of the fixed code 64 to a wavefront, one lane per stream
        (0: never, 1: launches of 32,768 streams or more -- the default, 2: always).  Results are identical."""
        _ffi.check(self._L.pzg_set_option(self._h, _ffi.OPT_BUNDLES, int(mode)), self._h)

    def set_profile(self, on: bool):
        """PZG_OPT_PROFILE: the stream-waves' memory of where the last stream's tokens lay (default on).  Results are identical."""
        _ffi.check(self._L.pzg_set_option(self._h, _ffi.OPT_PROFILE, 1 if on else 0), self._h)

    def sync(self):
        _ffi.check(self._L.pzg_sync(self._h), self._h)

    def last_kernel_ms(self) -> float:
        return float(self._L.pzg_last_kernel_ms(self._h))

    # -- raw batched call on host memory ----------------------------------------------------------
    def decompress_many_raw(self, in_buf: np.ndarray, in_off, in_len, out_buf: np.ndarray, out_off, out_cap, gzip: bool = False,
                            dict_buf: Optional[np.ndarray] = None, dict_off=None, dict_len=None, pinned: bool = False,
                            raw: bool = False, crc32: bool = False):
        """Thin wrapper of pzg_decompress_many on host numpy buffers.
        pinned: in_buf / out_buf are page-locked arenas (pinned_array) with ascending extents -- PZG_HOST_PINNED.
        raw: the streams are bare RFC 1951 (PZG_RAW); crc32 (with raw only): adler holds the CRC-32 of what was delivered (PZG_CRC32).
        Returns (out_len u64[n], status i32[n], detail u32[n,2], in_used u64[n], adler u32[n])."""
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        out_cap = np.ascontiguousarray(out_cap, dtype=np.uint64)
        n = len(in_off)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        in_used = np.zeros(n, dtype=np.uint64)
        adler = np.zeros(n, dtype=np.uint32)
        if n == 0:
            return out_len, status, detail, in_used, adler
        container = (_ffi.GZIP if gzip else 0) | (_ffi.RAW if raw else 0) | (_ffi.CRC32 if crc32 else 0)
        if dict_buf is not None:  # extension: one preset dictionary extent per stream (length 0 = none)
            if gzip:  # (preset dictionaries are a zlib-container notion: the C ABI rejects the combination too)
                raise ValueError("gzip=True and preset dictionaries cannot be combined")
            dict_off = np.ascontiguousarray(dict_off, dtype=np.uint64)
            dict_len = np.ascontiguousarray(dict_len, dtype=np.uint64)
            rc = self._L.pzg_decompress_many_dict(
                self._h, in_buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, dict_buf.ctypes.data, dict_off.ctypes.data,
                dict_len.ctypes.data, out_buf.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                status.ctypes.data, detail.ctypes.data, in_used.ctypes.data, adler.ctypes.data, n, container)
            _ffi.check(rc, self._h)
            return out_len, status, detail, in_used, adler
        rc = self._L.pzg_decompress_many(
            self._h, in_buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, out_buf.ctypes.data,
            out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data, status.ctypes.data, detail.ctypes.data,
            in_used.ctypes.data, adler.ctypes.data, n, container | (_ffi.HOST_PINNED if pinned else 0))
        _ffi.check(rc, self._h)
        return out_len, status, detail, in_used, adler

    # -- the parallel index scan over many raw streams (host memory) -------------------------------
    def index_scan_many(self, in_buf: np.ndarray, in_off, in_len, point_off, chunk: int = 0, span: int = 0, windows: bool = True):
        """Thin wrapper of pzg_index_scan_many on a host numpy buffer: stream s is in_buf[in_off[s] : in_off[s] + in_len[s]] and owns
        the slots point_off[s] .. point_off[s + 1] (point_off: n + 1 entries, ascending).  chunk 0: 128 KiB; span 0: 1 MiB.
        Returns (points u64[slots,2], windows u8[slots,32768] or None, npoints u32[n], out_len u64[n], status i32[n], detail u32[n,2],
        in_used u64[n]); raises PzgError (rc -4 when the device has not the memory the call needs)."""
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        point_off = np.ascontiguousarray(point_off, dtype=np.uint32)
        n = len(in_off)
        if len(in_len) != n or len(point_off) != n + 1:
            raise ValueError("in_off, in_len: n entries; point_off: n + 1")
        slots = int(point_off[-1])
        points = np.zeros((max(slots, 1), 2), dtype=np.uint64)
        wins = np.zeros((max(slots, 1), 32768), dtype=np.uint8) if windows else None
        npoints = np.zeros(n, dtype=np.uint32)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        in_used = np.zeros(n, dtype=np.uint64)
        rc = self._L.pzg_index_scan_many(self._h, in_buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, n, int(chunk), int(span),
                                         points.ctypes.data, point_off.ctypes.data, npoints.ctypes.data,
                                         wins.ctypes.data if windows else None, out_len.ctypes.data, status.ctypes.data, detail.ctypes.data,
                                         in_used.ctypes.data, 0)
        _ffi.check(rc, self._h)
        return points[:slots], (wins[:slots] if windows else None), npoints, out_len, status, detail, in_used

    # -- device-pointer call (the timed path; pointers are raw integers) ----------------------------
    def decompress_many_device(self, in_base: int, in_off: int, in_len: int, out_base: int, out_off: int,
                               out_cap: int, out_len: int, status: int, detail: int, in_used: int, adler: int,
                               n: int, sync: bool = True, gzip: bool = False, lpt: bool = False, raw: bool = False, crc32: bool = False):
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC) | (_ffi.GZIP if gzip else 0) | (_ffi.LPT_ORDER if lpt else 0)
        flags |= (_ffi.RAW if raw else 0) | (_ffi.CRC32 if crc32 else 0)
        rc = self._L.pzg_decompress_many(self._h, in_base, in_off, in_len, out_base, out_off, out_cap, out_len,
                                         status, detail or None, in_used or None, adler or None, n, flags)
        _ffi.check(rc, self._h)

    # -- scanline unfiltering (pzg_unfilter_many) -----------------------------------------------------
    def unfilter_many(self, src: np.ndarray, src_off, src_len, dst: np.ndarray, dst_off, dst_stride, row_bytes, height, bpp):
        """Thin wrapper of pzg_unfilter_many on host numpy buffers: image i is height[i] rows of a filter byte and row_bytes[i]
        filtered bytes at src[src_off[i]:], delivered without the filter bytes at dst[dst_off[i] + r * dst_stride[i]:].
        Returns (status i32[n], detail u32[n,2])."""
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((src_off, np.uint64), (src_len, np.uint64), (dst_off, np.uint64),
                                                              (dst_stride, np.uint64), (row_bytes, np.uint32), (height, np.uint32), (bpp, np.uint8))]
        n = len(arrs[0])
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        rc = self._L.pzg_unfilter_many(self._h, src.ctypes.data, arrs[0].ctypes.data, arrs[1].ctypes.data, dst.ctypes.data, arrs[2].ctypes.data,
                                       arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data, arrs[6].ctypes.data, status.ctypes.data,
                                       detail.ctypes.data, n, 0)
        _ffi.check(rc, self._h)
        return status, detail

    def unfilter_many_device(self, src_base: int, src_off: int, src_len: int, dst_base: int, dst_off: int, dst_stride: int, row_bytes: int,
                             height: int, bpp: int, status: int, detail: int, n: int, sync: bool = True):
        """pzg_unfilter_many on device memory, every pointer an integer address as decompress_many_device takes them: the launch goes
        on the context's stream behind what was enqueued before it, so src_len may be the out_len array of a decode enqueued with
        sync=False, and dst_base memory of the caller's own (a torch tensor's data_ptr())."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_unfilter_many(self._h, src_base, src_off, src_len, dst_base, dst_off, dst_stride, row_bytes, height, bpp,
                                             status, detail or None, n, flags), self._h)

    # -- Adam7 deinterlacing (pzg_adam7_many) ----------------------------------------------------------
    def adam7_many(self, src: np.ndarray, src_off, dst: np.ndarray, dst_off, dst_stride, width, height, pixel_bits):
        """Thin wrapper of pzg_adam7_many on host numpy buffers: image i is its seven reduced images, unfiltered, dense and in pass
        order at src[src_off[i]:], delivered as height[i] rows at dst[dst_off[i] + y * dst_stride[i]:].
        Returns (status i32[n], detail u32[n,2])."""
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((src_off, np.uint64), (dst_off, np.uint64), (dst_stride, np.uint64),
                                                              (width, np.uint32), (height, np.uint32), (pixel_bits, np.uint8))]
        n = len(arrs[0])
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        rc = self._L.pzg_adam7_many(self._h, src.ctypes.data, arrs[0].ctypes.data, dst.ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                    arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data, status.ctypes.data, detail.ctypes.data, n, 0)
        _ffi.check(rc, self._h)
        return status, detail

    def adam7_many_device(self, src_base: int, src_off: int, dst_base: int, dst_off: int, dst_stride: int, width: int, height: int,
                          pixel_bits: int, status: int, detail: int, n: int, sync: bool = True):
        """pzg_adam7_many on device memory, every pointer an integer address as unfilter_many_device takes them: the launch goes on
        the context's stream behind what was enqueued before it, so src may be where unfilter_many_device(sync=False) delivers the
        passes, and dst_base memory of the caller's own (a torch tensor's data_ptr())."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_adam7_many(self._h, src_base, src_off, dst_base, dst_off, dst_stride, width, height, pixel_bits,
                                          status, detail or None, n, flags), self._h)

    # -- pixel expansion (pzg_expand_many) -----------------------------------------------------------------
    def expand_many(self, src: np.ndarray, dst: np.ndarray, palette: Optional[np.ndarray], desc: np.ndarray):
        """Thin wrapper of pzg_expand_many on host numpy buffers: image i is described by desc[i] (EXPAND_DESC: a structured array of
        pzg_expand_desc), its rows as PNG stores them in src, its RGBA8 / RGB8 rows delivered into dst; palette: uint32 entries whose
        bytes in memory order are R, G, B, A (None: no palette image).  Returns (status i32[n], detail u32[n,2])."""
        desc = np.ascontiguousarray(desc)
        if desc.dtype.itemsize != EXPAND_DESC.itemsize:
            raise ValueError("desc: records of %d bytes (EXPAND_DESC)" % EXPAND_DESC.itemsize)
        n = len(desc)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        pal = None if palette is None else np.ascontiguousarray(palette, dtype=np.uint32)
        rc = self._L.pzg_expand_many(self._h, src.ctypes.data, dst.ctypes.data, pal.ctypes.data if pal is not None else None, desc.ctypes.data,
                                     status.ctypes.data, detail.ctypes.data, n, 0)
        _ffi.check(rc, self._h)
        return status, detail

    def expand_many_device(self, src_base: int, dst_base: int, palette_base: int, desc: int, status: int, detail: int, n: int, sync: bool = True):
        """pzg_expand_many on device memory, every pointer an integer address as adam7_many_device takes them: the launch goes on the
        context's stream behind what was enqueued before it, so src may be where unfilter_many_device(sync=False) or
        adam7_many_device(sync=False) deliver, and dst_base memory of the caller's own (a torch tensor's data_ptr())."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_expand_many(self._h, src_base, dst_base, palette_base or None, desc, status, detail or None, n, flags), self._h)

    # -- TIFF Predictor 2 and window clipping (pzg_unpredict_many) -----------------------------------------
    def unpredict_many(self, src: np.ndarray, src_len, dst: np.ndarray, desc: np.ndarray):
        """Thin wrapper of pzg_unpredict_many on host numpy buffers: job i -- one strip or tile as it was decoded -- is described by
        desc[i] (UNPREDICT_DESC: a structured array of pzg_unpredict_desc), src_len[i] of its bytes are in src, and the window of its
        reconstructed rows is delivered into dst.  Returns (status i32[n], detail u32[n,2])."""
        desc = np.ascontiguousarray(desc)
        if desc.dtype.itemsize != UNPREDICT_DESC.itemsize:
            raise ValueError("desc: records of %d bytes (UNPREDICT_DESC)" % UNPREDICT_DESC.itemsize)
        n = len(desc)
        src_len = np.ascontiguousarray(src_len, dtype=np.uint64)
        if len(src_len) != n:
            raise ValueError("src_len: one entry per descriptor")
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        rc = self._L.pzg_unpredict_many(self._h, src.ctypes.data, src_len.ctypes.data, dst.ctypes.data, desc.ctypes.data, status.ctypes.data,
                                        detail.ctypes.data, n, 0)
        _ffi.check(rc, self._h)
        return status, detail

    def unpredict_many_device(self, src_base: int, src_len: int, dst_base: int, desc: int, status: int, detail: int, n: int, sync: bool = True):
        """pzg_unpredict_many on device memory, every pointer an integer address as unfilter_many_device takes them: the launch goes on
        the context's stream behind what was enqueued before it, so src_len may be the out_len array of a decode enqueued with
        sync=False, and dst_base memory of the caller's own (a torch tensor's data_ptr())."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_unpredict_many(self._h, src_base, src_len, dst_base, desc, status, detail or None, n, flags), self._h)

    # -- the byte-plane transpose and TIFF Predictor 3 (pzg_unshuffle_many) --------------------------------
    def unshuffle_many(self, src: np.ndarray, src_len, dst: np.ndarray, desc: np.ndarray):
        """Thin wrapper of pzg_unshuffle_many on host numpy buffers: job i -- one strip, tile or chunk as it was decoded -- is described
        by desc[i] (UNSHUFFLE_DESC: a structured array of pzg_unshuffle_desc), src_len[i] of its bytes are in src, and the window of
        its reconstructed rows is delivered into dst.  Returns (status i32[n], detail u32[n,2])."""
        desc = np.ascontiguousarray(desc)
        if desc.dtype.itemsize != UNSHUFFLE_DESC.itemsize:
            raise ValueError("desc: records of %d bytes (UNSHUFFLE_DESC)" % UNSHUFFLE_DESC.itemsize)
        n = len(desc)
        src_len = np.ascontiguousarray(src_len, dtype=np.uint64)
        if len(src_len) != n:
            raise ValueError("src_len: one entry per descriptor")
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        rc = self._L.pzg_unshuffle_many(self._h, src.ctypes.data, src_len.ctypes.data, dst.ctypes.data, desc.ctypes.data, status.ctypes.data,
                                        detail.ctypes.data, n, 0)
        _ffi.check(rc, self._h)
        return status, detail

    def unshuffle_many_device(self, src_base: int, src_len: int, dst_base: int, desc: int, status: int, detail: int, n: int, sync: bool = True):
        """pzg_unshuffle_many on device memory, every pointer an integer address as unpredict_many_device takes them: the launch goes
        on the context's stream behind what was enqueued before it, so src_len may be the out_len array of a decode enqueued with
        sync=False."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_unshuffle_many(self._h, src_base, src_len, dst_base, desc, status, detail or None, n, flags), self._h)

    # -- LZW streams: TIFF Compression 5, PDF LZWDecode (pzg_unlzw_many) ------------------------------------
    def unlzw_many(self, in_buf: np.ndarray, in_off, in_len, out: np.ndarray, out_off, out_cap, early_change: bool = True):
        """Thin wrapper of pzg_unlzw_many on host numpy buffers: stream i is in_len[i] bytes at in_buf[in_off[i]], its output goes to
        out[out_off[i]] with room for out_cap[i].  Returns (out_len u64[n], status i32[n], detail u32[n,2])."""
        in_off, in_len, out_off, out_cap = (np.ascontiguousarray(x, dtype=np.uint64) for x in (in_off, in_len, out_off, out_cap))
        n = len(in_off)
        if not (len(in_len) == len(out_off) == len(out_cap) == n):
            raise ValueError("in_off, in_len, out_off, out_cap: one entry per stream")
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.zeros((n, 2), dtype=np.uint32)
        rc = self._L.pzg_unlzw_many(self._h, in_buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, out.ctypes.data, out_off.ctypes.data,
                                    out_cap.ctypes.data, out_len.ctypes.data, status.ctypes.data, detail.ctypes.data, n,
                                    _ffi.LZW_EARLY_CHANGE if early_change else 0, 0)
        _ffi.check(rc, self._h)
        return out_len, status, detail

    def unlzw_many_device(self, in_base: int, in_off: int, in_len: int, out_base: int, out_off: int, out_cap: int, out_len: int, status: int,
                          detail: int, n: int, early_change: bool = True, sync: bool = True):
        """pzg_unlzw_many on device memory, every pointer an integer address: the launch goes on the context's stream behind what was
        enqueued before it, and out_len may be the src_len array of a stage enqueued behind it."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_unlzw_many(self._h, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, status, detail or None, n,
                                          _ffi.LZW_EARLY_CHANGE if early_change else 0, flags), self._h)

    def decompress_many_sharded(self, batches, sync: bool = True, gzip: bool = False, lpt: bool = False, raw: bool = False,
                                crc32: bool = False):
        """pzg_decompress_many_sharded: `batches` is a list of dicts (shard, n, in_base, in_off, in_len, out_base, out_off,
        out_cap, out_len, status and optionally detail, in_used, adler), every pointer an integer address of device memory
        on that shard's device.  One call enqueues them all; nothing leaves the devices."""
        arr = (_ffi.DeviceBatch * len(batches))()
        for q, b in zip(arr, batches):
            for k, _t in _ffi.DeviceBatch._fields_:
                setattr(q, k, b.get(k) or 0)
        flags = (0 if sync else _ffi.ASYNC) | (_ffi.GZIP if gzip else 0) | (_ffi.LPT_ORDER if lpt else 0)
        flags |= (_ffi.RAW if raw else 0) | (_ffi.CRC32 if crc32 else 0)
        _ffi.check(self._L.pzg_decompress_many_sharded(self._h, C.byref(arr) if len(batches) else None, len(batches), flags), self._h)

    def adler32(self, data, init: int = 1) -> int:
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        out = C.c_uint32(0)
        ptr = arr.ctypes.data if arr.size else None
        _ffi.check(self._L.pzg_adler32(self._h, ptr, arr.size, init, C.byref(out), 0), self._h)
        return out.value

    def adler32_many_device(self, base: int, off: int, length: int, out_ptr: int, n: int, sync: bool = True):
        """Adler-32 of n device buffers (one wave each): BASELINE config 2 in its batched form."""
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_adler32_many(self._h, base, off, length, out_ptr, n, flags), self._h)

    def adler32_device(self, ptr: int, nbytes: int, out_ptr: int, init: int = 1, sync: bool = True):
        flags = _ffi.DEVICE_PTRS | (0 if sync else _ffi.ASYNC)
        _ffi.check(self._L.pzg_adler32(self._h, ptr, nbytes, init, out_ptr, flags), self._h)


class PinnedArena:
    """A page-locked host buffer from pzg_host_alloc, seen as a numpy uint8 array (`.a`).  The copy engines read and write
    it directly (PZG_HOST_PINNED): what the mirrors pack their batches into, so that nothing is staged a second time."""

    def __init__(self, nbytes: int):
        self._L = _ffi.lib()
        self.nbytes = max(int(nbytes), 1)
        self._p = self._L.pzg_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError(f"pzg_host_alloc({self.nbytes}) failed: the system will not lock that much memory")
        self.a = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self._p))

    def close(self):
        if self._p:
            self.a = None
            self._L.pzg_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the mirrors' arenas: grow-only, one pair per thread (a `decompress` call is synchronous)
_arenas = threading.local()


def _arena(kind: str, nbytes: int) -> Optional[np.ndarray]:
    """A page-locked array of at least nbytes for this thread's `kind` ("in" / "out"), or None when the system refuses."""
    cur = getattr(_arenas, kind, None)
    if cur is None or cur.nbytes < nbytes:
        if cur is not None:
            cur.close()
        try:
            cur = PinnedArena(max(nbytes, 1 << 20) * 5 // 4)
        except MemoryError:
            setattr(_arenas, kind, None)
            return None
        setattr(_arenas, kind, cur)
    return cur.a


_default_ctx = None
_default_lock = threading.Lock()


def default_context() -> Context:
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            _default_ctx = Context(0)
        return _default_ctx


# ---- the reference API -------------------------------------------------------------------------------


def _to_chunks(x: LazyByteString) -> List[bytes]:
    if isinstance(x, (bytes, bytearray, memoryview)):
        b = bytes(x)
        return [b] if b else []
    return [bytes(c) for c in x if len(c)]  # a lazy ByteString never holds empty chunks


def decompress_many(streams: Sequence[LazyByteString], ctx: Optional[Context] = None,
                    size_hint: Optional[Sequence[int]] = None, gzip: bool = False,
                    zdict: Optional[Sequence[Optional[bytes]]] = None) -> List[Either]:
    """decompressMany: every stream decoded by its own wavefront in one launch.

    zlib streams do not carry their decoded size, so each stream gets a capacity (size_hint[i] or a
    guess); streams that report PZG_E_OUT_TOO_SMALL are relaunched once with the exact size the
    kernel measured.

    zdict (EXTENSION, the reference skips DICTID: Zlib.hs:68): one preset dictionary per stream (None = none); a stream
    whose header has FDICT set then decodes with it as history, as zlib.decompressobj(zdict=...) does."""
    return _decompress_many(streams, ctx, size_hint, gzip, zdict)[0]


def _decompress_many(streams, ctx, size_hint, gzip, zdict, raw=False, crc32=False):
    """The body of decompress_many and raw_decompress_many: (results, checksums) -- the library's adler[] word of every Right."""
    ctx = ctx or default_context()
    chunked = [_to_chunks(s) for s in streams]
    flat = [b"".join(c) for c in chunked]
    n = len(flat)
    results: List[Optional[Either]] = [None] * n
    sums: List[Optional[int]] = [None] * n
    # without a hint: a modest first guess (the batch is packed, so small guesses cost little); PZG_E_OUT_TOO_SMALL
    # streams come back with their exact size and are relaunched once
    caps = [int(size_hint[i]) if size_hint is not None else max(256, 4 * len(flat[i])) for i in range(n)]
    todo = list(range(n))
    for _attempt in range(2):
        if not todo:
            break
        m = len(todo)
        in_len = np.array([len(flat[i]) for i in todo], dtype=np.uint64)
        out_cap = np.array([caps[i] for i in todo], dtype=np.uint64)
        (in_off, tot_in), (out_off, tot_out) = pack(in_len), pack(out_cap)
        # packed into page-locked arenas (PZG_HOST_PINNED: the library then stages nothing a second time); preset dictionaries
        # and a system that will not lock the memory take the staged path over ordinary arrays
        in_buf = out_buf = None
        if zdict is None:
            in_buf, out_buf = _arena("in", tot_in), _arena("out", tot_out)
        pinned = in_buf is not None and out_buf is not None
        if not pinned:
            in_buf = np.zeros(tot_in, dtype=np.uint8)
            out_buf = np.zeros(tot_out, dtype=np.uint8)
        for k, i in enumerate(todo):
            in_buf[int(in_off[k]):int(in_off[k]) + len(flat[i])] = np.frombuffer(flat[i], dtype=np.uint8)
        dict_args = {}
        if zdict is not None:
            dl = np.array([len(zdict[i] or b"") for i in todo], dtype=np.uint64)
            do = np.zeros(m, dtype=np.uint64)
            do[1:] = np.cumsum(dl[:-1])
            db = np.frombuffer(b"".join((zdict[i] or b"") for i in todo) + b"\0" * 16, dtype=np.uint8)
            dict_args = dict(dict_buf=db, dict_off=do, dict_len=dl)
        out_len, status, detail, in_used, adler = ctx.decompress_many_raw(in_buf, in_off, in_len, out_buf, out_off, out_cap, gzip,
                                                                          pinned=pinned, raw=raw, crc32=crc32, **dict_args)
        retry = []
        for k, i in enumerate(todo):
            st = int(status[k])
            if st == _ffi.OK:
                data = out_buf[int(out_off[k]):int(out_off[k]) + int(out_len[k])].tobytes()
                results[i] = _apply_chunk_rule(chunked[i], int(in_used[k]), data)
                sums[i] = int(adler[k])
            elif st == _ffi.E_OUT_TOO_SMALL and _attempt == 0:
                caps[i] = int(out_len[k])
                retry.append(i)
            else:
                results[i] = Left(error_from_status(flat[i], st, detail[k]))
        todo = retry
    return results, sums


def _apply_chunk_rule(chunks: List[bytes], in_used: int, data: bytes) -> Either:
    """Zlib.hs:46-49: `Done` with whole unread chunks left is `Left "Finished with data remaining."`;
    trailing bytes inside the last chunk handed over are silently ignored."""
    cum = 0
    loaded = 0
    for c in chunks:
        if cum >= in_used:
            break
        cum += len(c)
        loaded += 1
    if loaded < len(chunks):
        return Left(DecompressionError("DecompressionError", "Finished with data remaining.", _ffi.E_DATA_REMAINING))
    return Right(data)


def decompress(ifile: LazyByteString, ctx: Optional[Context] = None, size_hint: Optional[int] = None) -> Either:
    """Codec.Compression.Zlib.decompress (Zlib.hs:32-51)."""
    return decompress_many([ifile], ctx, None if size_hint is None else [size_hint])[0]


def adler32(data: bytes, init: int = 1, ctx: Optional[Context] = None) -> int:
    """Codec.Compression.Zlib.Adler32 over one buffer, as a device-wide reduction (Adler32.hs:17-57)."""
    return (ctx or default_context()).adler32(data, init)


def gzip_decompress_many(streams: Sequence[LazyByteString], ctx: Optional[Context] = None,
                         size_hint: Optional[Sequence[int]] = None) -> List[Either]:
    """EXTENSION (the reference lists gzip as a TODO): decompress_many over RFC 1952
    members -- same DEFLATE kernel, gzip header, CRC-32 + ISIZE trailer verified on the device."""
    return decompress_many(streams, ctx, size_hint, gzip=True)


def raw_decompress_many(streams: Sequence[LazyByteString], size_hint: Optional[Sequence[int]] = None, crc32: bool = False,
                        dicts: Optional[Sequence[Optional[bytes]]] = None, ctx: Optional[Context] = None):
    """EXTENSION: decompress_many over bare RFC 1951 streams (PZG_RAW) -- what a deflated ZIP member holds, system zlib's
    wbits = -15: no header, no trailer, nothing checked.  The same capacity guess and single relaunch, the same errors, and
    "Finished with data remaining." for whole chunks behind the final block.  dicts: one dictionary per stream (None = none),
    the history in front of the stream's output as zlib.decompressobj(-15, zdict=...) has it.
    crc32=True: returns (results, crcs) -- crcs[i] is the CRC-32 (RFC 1952) of stream i's bytes, computed on the device and
    checked against nothing (None for a Left); the caller owns the expected value."""
    results, sums = _decompress_many(streams, ctx, size_hint, False, dicts, raw=True, crc32=crc32)
    return (results, sums) if crc32 else results


def raw_decompress(data: LazyByteString, ctx: Optional[Context] = None, size_hint: Optional[int] = None) -> Either:
    """decompress over one bare RFC 1951 stream (see raw_decompress_many)."""
    return raw_decompress_many([data], None if size_hint is None else [size_hint], ctx=ctx)[0]


# Haskell-cased aliases so call sites read like the reference
decompressMany = decompress_many
