"""CPU: the host arithmetic of pure_zlib_amd/indexed.py -- checksum combination, the wrapper parsers, the index file -- without a
library call; and, over the host model of the segment decoder, that combining the segments' checksums catches a wrong window."""
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

import indexcheck as X
from pure_zlib_amd.indexed import Index, adler32_combine, crc32_combine, parse_gzip_header, parse_zlib_header
from pure_zlib_amd.zlib import DecompressionError


def test_combine_on_random_splits():
    rng = random.Random(5)
    big = rng.randbytes(5 << 20)
    lens = [0, 1, 65520, 65521, 65522, 2 * 65521] + [rng.choice([rng.randint(0, 300), rng.randint(0, 200000)]) for _ in range(194)]
    for k, n2 in enumerate(lens):
        n1 = rng.choice([0, 1, 65521, rng.randint(0, 100000)])
        a, b = big[:n1], big[n1:n1 + n2]
        assert adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(a + b), (k, n1, n2)
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b), (k, n1, n2)
    head, tail = big[:777], big[777:]  # a 5 MiB tail
    assert adler32_combine(zlib.adler32(head), zlib.adler32(tail), len(tail)) == zlib.adler32(big)
    assert crc32_combine(zlib.crc32(head), zlib.crc32(tail), len(tail)) == zlib.crc32(big)
    # many parts, left to right, from the checksums' initial values -- as Index.decompress folds its segments
    a, c, at = 1, 0, 0
    while at < len(big):
        n = rng.choice([0, 1, 4096, 65521, 300000])
        part = big[at:at + n]
        a, c, at = adler32_combine(a, zlib.adler32(part), len(part)), crc32_combine(c, zlib.crc32(part), len(part)), at + n
    assert (a, c) == (zlib.adler32(big), zlib.crc32(big))


def _message(fn, data):
    with pytest.raises(DecompressionError) as e:
        fn(data)
    return e.value.show()


def test_zlib_header_parser():
    assert parse_zlib_header(zlib.compress(b"abc")) == 2
    for cmf, flg in ((0x78, 0x9c), (0x78, 0x01), (0x08, 0x1d), (0x48, 0x0d)):
        assert ((cmf << 8) | flg) % 31 == 0 and parse_zlib_header(bytes([cmf, flg, 3, 0])) == 2
    # the reference's texts (Zlib.hs:55-68), in its order: FCHECK first, then CM, then CINFO
    assert _message(parse_zlib_header, b"\x78\x9d") == "Header error: Header checksum failed"
    assert _message(parse_zlib_header, b"\x79\x9c") == "Header error: Header checksum failed"
    assert _message(parse_zlib_header, bytes([0x77, 31 - (0x7700 % 31)])) == "Header error: Bad compression method: 7"
    assert _message(parse_zlib_header, bytes([0x88, 31 - (0x8800 % 31)])) == "Header error: Window size too big: 8"
    fdict = bytes([0x78, 0x20 + 31 - (0x7820 % 31)])
    assert (fdict[0] << 8 | fdict[1]) % 31 == 0 and fdict[1] & 0x20
    assert _message(parse_zlib_header, fdict + b"\0\0\0\0").startswith("Header error: preset dictionary")
    assert _message(parse_zlib_header, b"\x78") == "Decompression error: Ran out of data mid-decompression 2."


def _gz_header(extra=None, name=None, comment=None, hcrc=False):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x11\x22\x33\x44\x02\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def test_gzip_header_parser():
    body = X.raw_of(b"hello " * 50)
    assert parse_gzip_header(gzip.compress(b"x")) == 10
    for kw in (dict(), dict(extra=b"ab\x03\x00xyz"), dict(name=b"file.txt"), dict(comment=b"c"), dict(hcrc=True), dict(extra=b"", name=b"", hcrc=True),
               dict(extra=b"\0" * 300, name=b"n" * 40, comment=b"k" * 9, hcrc=True)):
        h = _gz_header(**kw)
        assert parse_gzip_header(h + body) == len(h), kw
        assert zlib.decompressobj(31).decompress(h + body + struct.pack("<II", zlib.crc32(b"hello " * 50), 300)) == b"hello " * 50  # (zlib agrees it is a header)
        for cut in range(len(h)):
            assert _message(parse_gzip_header, h[:cut]) == "Decompression error: Ran out of data mid-decompression 2.", (kw, cut)
    assert _message(parse_gzip_header, b"\x1f\x8c" + bytes(8)) == "Header error: gzip: bad magic"
    assert _message(parse_gzip_header, b"\x1f\x8b\x07" + bytes(7)) == "Header error: gzip: bad compression method: 7"
    assert _message(parse_gzip_header, b"\x1f\x8b\x08\x20" + bytes(6)) == "Header error: gzip: reserved flag bits set"
    bad = bytearray(_gz_header(name=b"abc", hcrc=True))
    bad[-1] ^= 1
    assert _message(parse_gzip_header, bytes(bad)) == "Header error: gzip: header crc mismatch"


def test_index_file_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    pts = np.array([[1234567, 1 << 20], [7654321, (2 << 20) + 17], [1 << 35, 1 << 34]], dtype=np.uint64)
    win = rng.integers(0, 256, (3, 32768), dtype=np.uint8)
    for kind in ("zlib", "gzip", "raw"):
        ix = Index(kind, 1 << 20, pts, win, (1 << 34) + 5, 2, 99999, 0xDEADBEEF, (123456, 0xCAFEF00D))
        p = tmp_path / ("a.%s.pzi" % kind)
        ix.save(p)
        assert sorted(x.name for x in tmp_path.iterdir() if kind in x.name) == [p.name]  # (no ".npz" appended)
        iy = Index.load(p)
        assert (iy.kind, iy.span, iy.out_len, iy.body_off, iy.body_len, iy.expect, iy.fingerprint) == \
            (kind, 1 << 20, (1 << 34) + 5, 2, 99999, 0xDEADBEEF, (123456, 0xCAFEF00D))
        assert np.array_equal(iy.points, pts) and np.array_equal(iy.windows, win) and iy.points.dtype == np.uint64
        assert iy.segments() == ix.segments() and len(iy.segments()) == 4 and iy.segments()[-1][3] == 0
    empty = Index("raw", 4096, np.zeros((0, 2), np.uint64), np.zeros((0, 32768), np.uint8), 10, 0, 12, 1, (12, 0))
    empty.save(tmp_path / "e.pzi")
    assert Index.load(tmp_path / "e.pzi").segments() == [(0, 12, 0, 0, 0, 10)]
    with open(tmp_path / "junk.pzi", "wb") as f:
        np.savez(f, points=pts, windows=win[:2], kind=np.array(0), lengths=np.arange(7, dtype=np.uint64))
    with pytest.raises(ValueError):
        Index.load(tmp_path / "junk.pzi")


def test_segments_agree_with_the_tests_own_cut():
    pts = [(75, 5000), (8 * 900 + 7, 9000), (8 * 4000, 9000 + 32768)]
    ix = Index("raw", 4096, np.array(pts, dtype=np.uint64), np.zeros((3, 32768), np.uint8), 50000, 0, 5000, 1, (5000, 0))
    assert ix.segments() == X.segments(pts, 5000, 50000)


def test_combined_checksums_catch_a_wrong_window():
    """A segment decoded with a zeroed window is PZG_OK with other bytes (tests/test_model_segments.py): the combination of the
    segments' Adler-32s is then not the stream's -- what Index.decompress compares with the trailer."""
    model = X.SegModel()
    name, d, data = X.big_inputs()[0]
    _r, _out, _n, pts = model.build(d, len(data), 40000)
    segs = X.segments(pts, len(d), len(data))
    for zeroed in (None, 2):
        total = 1
        for k, (off, ln, sb, eb, a, b) in enumerate(segs):
            win = data[max(0, a - X.WINDOW):a]
            r, _ = model.segment(d[off:off + ln], sb, eb, bytes(len(win)) if k == zeroed else win, b - a)
            assert (r.status, r.out_len) == (0, b - a)
            total = adler32_combine(total, r.adler, b - a)
        assert (total == zlib.adler32(data)) == (zeroed is None)
