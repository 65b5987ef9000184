"""pure_zlib_amd -- MI355X-native batched zlib/DEFLATE decompression behind pure-zlib's
`Codec.Compression.Zlib.decompress` API.

Only what the hot path needs lives here:
  csrc/      hand-written HIP kernels (gfx950) + the C ABI of include/pzg.h  -> libpzg.so
  zlib.py    host-side mirror of the reference module Codec.Compression.Zlib
  shard.py   host-side sharding of a batch of streams over the GPUs of a node
  incremental.py, deflate_cli.py, benchmark.py   the reference's streaming protocol, CLI and criterion harness
             over the same path; gzip members (row 4) are `gzip_decompress_many`
  zip.py     ZIP archives read and tested in one launch (raw DEFLATE members, sizes and CRC-32s from the central directory)
  indexed.py ONE large stream: an index of access points, every segment its own wavefront, reads at any offset
  gzfile.py  a gzip FILE of many members (BGZF, WARC, concatenated .gz): members found on the device, a wavefront per member
  png.py     PNG images in batches: one decode launch, one unfilter launch (pzg_unfilter_many), the pixels in one copy;
             Adam7 images with adam7=True, deinterlaced on the device (pzg_adam7_many); expand="rgba8" | "rgb8": (H, W, 4 | 3) uint8 pixels
             of every colour type, expanded on the device (pzg_expand_many); read_png_batch: one (N, H, W, C) tensor
  tiff.py    Deflate-compressed TIFF files in batches: every strip and tile of every page of every file in one decode launch, Predictor 2
             undone and tiles clipped in one more (pzg_unpredict_many); read_tiff_region decodes only what covers a rectangle;
             float_predictor=True: Predictor 3 pages (float rasters) through one pzg_unshuffle_many launch as well;
             lzw=True: LZW pages (Compression 5), their strips and tiles decoded by one pzg_unlzw_many launch
  cxx/       the same module mirror in C++ (header-only; the image stages are not mirrored)

There is no CPU fallback: importing works anywhere, computing needs libpzg.so and a gfx950 device.
"""
from . import _ffi  # noqa: F401
from .zlib import (  # noqa: F401
    ChecksumError, Context, DecompressionError, DecompressionError_, FormatError, HeaderError,
    HuffmanTreeError, Left, Right, adler32, decompress, decompress_many, decompressMany, default_context,
    gzip_decompress_many, raw_decompress, raw_decompress_many,
)
from .indexed import Index, adler32_combine, crc32_combine  # noqa: F401
from .gzfile import MemberIndex, decompress_gzip_file  # noqa: F401
from .tiff import TiffImage, TiffPage, parse_tiff, read_tiff, read_tiff_many, read_tiff_region, test_tiff_many  # noqa: F401
from .incremental import FORMATS, DecoderPool, decompress_incremental, decompressIncremental  # noqa: F401
