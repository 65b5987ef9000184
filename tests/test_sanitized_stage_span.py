"""CPU: the staging arithmetic of the image stages' host-pointer form (pure_zlib_amd/csrc/pzg_stage_span.h: the spans, their places
modulo 16, the rebased offsets, the metadata block's pieces, the copy-back of the delivered rows) under AddressSanitizer and UBSan as
a stand-alone program (tests/cxx/san_stage_span.cpp), built and run the way tests/test_sanitized_cores.py runs the cores.  On the
device path none of it can be compiled without HIP, and the row count that decides how many bytes are copied into caller memory
shows only where it is wrong by a whole row; here the staged spans, the caller's destination and the block are heap blocks of exactly
the sizes this file computes, so an offset one byte outside is a report.  Every expectation is computed below from the case's
description, never by the header.  Nothing loaded into Python is sanitized."""
import struct
from dataclasses import dataclass

import numpy as np

import sancases as S

FILL = 0xCD
WILD = 1 << 60


@dataclass
class Image:
    src_off: int
    src_len: int
    dst_off: int
    stride: int
    row_bytes: int
    rows: int
    delivered: int      # what the kernel is said to have delivered: may exceed rows
    empty: bool = False


def pattern(k):
    v = (k * 31 + 7) & 0xff
    return 0x11 if v == FILL else v


def pad256(x):
    return (x + 255) // 256 * 256


def u64s(values):
    return struct.pack("<%dQ" % len(values), *values)


def case(name, images, s_mis, d_mis, takes):
    """The case's fields (tests/cxx/san_stage_span.cpp): the description, then what must come of it."""
    n = len(images)
    live = [im for im in images if not im.empty]
    reads = [im for im in live if im.src_len]
    s_lo, s_hi = (min(im.src_off for im in reads), max(im.src_off + im.src_len for im in reads)) if reads else (0, 0)
    d_lo = min((im.dst_off for im in live), default=0)
    d_hi = max((im.dst_off + (im.rows - 1) * im.stride + im.row_bytes for im in live), default=0)
    want = np.full(d_hi if live else 24, FILL, np.uint8)  # the caller's destination ends with the last extent's last byte
    for im in live:
        assert im.rows >= 1 and im.row_bytes >= 1 and im.stride >= im.row_bytes
        for r in range(min(im.delivered, im.rows)):
            at = im.dst_off + r * im.stride
            want[at:at + im.row_bytes] = [pattern(k) for k in range(at, at + im.row_bytes)]
    src_at = [im.src_off - s_lo if not im.empty and im.src_len else 0 for im in images]
    dst_at = [0 if im.empty else im.dst_off - d_lo for im in images]
    for im, sa, da in zip(images, src_at, dst_at):  # what the program's blocks hold it to
        assert im.empty or (sa + im.src_len <= s_hi - s_lo and da + (im.rows - 1) * im.stride + im.row_bytes <= d_hi - d_lo)
    offs, at = [], 0
    for size, count in takes:
        offs.append(at)
        at += pad256(size * count)
    m_in, m_all = at, at + pad256(4 * n) + pad256(8 * n)
    cols = [[getattr(im, k) for im in images] for k in ("src_off", "src_len", "dst_off", "stride", "row_bytes", "rows")]
    cols += [[int(im.empty) for im in images], [im.delivered for im in images]]
    return ([name, n] + [u64s(col) for col in cols] + [s_mis, d_mis, int(not live), s_lo, s_hi, d_lo, d_hi, (s_mis + s_lo) % 16, (d_mis + d_lo) % 16,
                                                       u64s(src_at), u64s(dst_at), want.tobytes(), u64s([v for t in takes for v in t]), u64s(offs), m_in, m_all])


def unfilter_takes(n):
    return [(8, n)] * 4 + [(4, n)] * 2 + [(1, n)]


def adam7_takes(n):
    return [(8, n)] * 3 + [(4, n)] * 2 + [(1, n)]


def expand_takes(n, palette):
    return [(64, n), (4, palette), (8, 2 * n)]


def all_cases():
    out = []
    empty = lambda: Image(WILD, 0, WILD + 5, 0, 0, 0, 7, empty=True)  # noqa: E731  (its offsets are not looked at)
    # one image: the stride equal to the row's bytes, and larger
    out.append(case("n = 1, dense rows", [Image(5, 40, 3, 9, 9, 4, 4)], 0, 0, unfilter_takes(1)))
    out.append(case("n = 1, padded rows", [Image(5, 40, 3, 14, 9, 4, 4)], 3, 9, adam7_takes(1)))
    out.append(case("n = 1, one row of one byte", [Image(0, 1, 0, 1, 1, 1, 1)], 0, 0, expand_takes(1, 0)))
    # nothing but empty images
    out.append(case("all empty", [empty(), Image(0, 0, 0, 0, 0, 0, 0, empty=True), empty()], 5, 11, expand_takes(3, 0)))
    # an empty image between two others
    out.append(case("an empty image between two", [Image(17, 30, 21, 12, 7, 3, 3), empty(), Image(60, 11, 80, 5, 5, 2, 2)], 1, 15, unfilter_takes(3)))
    # extents in descending order; spans that overlap: the rows of one image in the padding of another's, two images of one source
    out.append(case("descending order", [Image(300, 50, 400, 10, 8, 5, 5), Image(150, 60, 200, 20, 20, 3, 3), Image(7, 100, 9, 33, 30, 2, 2)], 2, 6,
                    adam7_takes(3)))
    out.append(case("overlapping spans", [Image(40, 64, 120, 40, 10, 4, 4), Image(40, 64, 100, 40, 10, 4, 4), Image(90, 30, 111, 40, 9, 5, 2),
                                          Image(20, 30, 135, 160, 3, 2, 2)], 7, 2, expand_takes(4, 300)))
    # images that read nothing: a wild offset beside images that read, and nothing read at all (the unused span is normalised)
    out.append(case("a zero-length source at a wild offset", [Image(33, 20, 50, 8, 6, 3, 3), Image(WILD, 0, 19, 8, 6, 3, 0), Image(70, 9, 90, 6, 6, 2, 1)],
                    4, 13, unfilter_takes(3)))
    out.append(case("no image reads", [Image(WILD, 0, 35, 8, 6, 3, 0), Image(WILD + 9, 0, 70, 6, 6, 2, 0)], 9, 1, unfilter_takes(2)))
    # every skew 0..15 of both spans (7 is coprime to 16), the spans' starts off the boundaries too
    for mis in range(16):
        out.append(case("skews, mis %d" % mis, [Image(13, 25, 37, 11, 7, 3, 3), Image(50, 10, 90, 4, 4, 2, 2)], mis, (7 * mis + 3) % 16,
                        expand_takes(2, 17 * mis)))
    assert {c[17] for c in out[-16:]} == set(range(16)) == {c[18] for c in out[-16:]}
    # delivered rows 0, 1, height - 1, height, and more than the height, which is clamped; dense and padded rows in turn
    h = 6
    ims = [Image(100 * i, 50, 7 + 100 * i, 9 + 5 * (i % 2), 9, h, d) for i, d in enumerate((0, 1, h - 1, h, h + 1, 0xffffffff))]
    out.append(case("delivered rows", ims, 6, 10, unfilter_takes(len(ims))))
    out.append(case("delivered rows, one row high", [Image(0, 4, 1, 4, 4, 1, 0), Image(4, 4, 9, 9, 4, 1, 1), Image(8, 4, 25, 4, 4, 1, 2)], 15, 15, adam7_takes(3)))
    # the block's pieces where a piece is an exact multiple of 256 bytes, and one element more
    for n in (32, 33, 64, 65):
        out.append(case("%d images" % n, [Image(3 * i, 3, 5 * i, 2, 2, 2, i % 3) for i in range(n)], n % 16, (n + 5) % 16,
                        (unfilter_takes, adam7_takes)[n % 2](n)))
    return out


def test_stage_span_arithmetic(tmp_path_factory):
    d = tmp_path_factory.mktemp("san_stage_span")
    exe = S.build(str(d / "san_stage_span"), ["tests/cxx/san_stage_span.cpp"])
    cases = all_cases()
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == 3 + 1 + 1 + 2 + 2 + 16 + 2 + 4
    S.run(exe, str(d / "cases.bin"), n)
