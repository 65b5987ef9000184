"""No GPU, no libpzg.so: the parts of the batch readers that are plain numpy and Python -- the packing rule of
pure_zlib_amd/_batch.py, the layout and the pass jobs of pure_zlib_amd/png.py, and the functions that turn a launch's status words
into an image's or a strip's error -- against literals worked out by hand."""
import numpy as np
import pytest

import adam7cases as A
import pngcases as PC
from pure_zlib_amd import _ffi, png, tiff
from pure_zlib_amd._batch import pack


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths, slack, offsets, total", [
    ([], 0, [], 16), ([0], 0, [0], 16), ([1], 0, [0], 32), ([16], 0, [0], 32), ([17, 0, 15, 32], 0, [0, 32, 32, 48], 96), ([12, 13], 4, [0, 16], 64)])
def test_pack(lengths, slack, offsets, total):
    off, tot = pack(lengths, slack)
    assert off.dtype == np.uint64 and off.tolist() == offsets and tot == total and isinstance(tot, int)
    assert all(o % 16 == 0 for o in off.tolist())
    ends = off.tolist()[1:] + [tot - 16]  # (16 bytes behind the last extent)
    assert all(o + n + slack <= e for o, n, e in zip(off.tolist(), lengths, ends))
    assert pack(np.array(lengths, np.uint64), slack)[0].tolist() == offsets


# ---- png._layout, png._pass_jobs -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """(good, laced) of one plain 5 x 3 RGB8 image and one interlaced 9 x 9 1-bit gray image."""
    rng = np.random.default_rng(71)
    blobs = [PC.write_png(5, 3, 2, 8, rng.integers(0, 256, size=(3, 15), dtype=np.uint8)),
             A.write_png(9, 9, 0, 1, rng.integers(0, 256, size=(9, 2), dtype=np.uint8) & np.array([0xff, 0x80], np.uint8))]
    _names, results, good, laced = png._collect(blobs, True, None)
    assert results == [None, None] and [k for k, _i, _z in good] == [0, 1] and [j for j, _ps in laced] == [1]
    return good, laced


LACED_STREAM = sum(ph * (1 + prb) for pw, ph, prb in A.pass_sizes(9, 9, 1) if pw)
LACED_DENSE = A.extent(9, 9, 1)


def test_layout_capacities_and_offsets(batch):
    good, laced = batch
    assert (LACED_STREAM, LACED_DENSE) == (42, 23) == (sum(ph * (1 + prb) for _p, ph, prb in laced[0][1]), sum(ph * prb for _p, ph, prb in laced[0][1]))
    lay = png._layout(good, laced, None, None)
    assert lay.dec_cap.tolist() == [3 * (15 + 1), 42] and lay.dec_cap.dtype == np.uint64
    assert (lay.row_bytes.tolist(), lay.height.tolist(), lay.bpp.tolist()) == ([15, 2], [3, 9], [3, 1])
    assert (lay.pix.tolist(), lay.pix_off.tolist(), lay.pix_stride.tolist(), lay.pix_total) == ([45, 18], [0, 48], [15, 2], 48 + 32 + 16)
    assert (lay.file_off.tolist(), lay.file_stride.tolist(), lay.file_total) == ([0, 48], [15, 2], None)  # the rows go straight to the pixels
    x = png._layout(good, laced, "rgb8", None)
    assert x.dec_cap.tolist() == [48, 42]
    assert (x.pix.tolist(), x.pix_off.tolist(), x.pix_stride.tolist(), x.pix_total) == ([45, 243], [0, 48], [15, 27], 48 + 256 + 16)
    assert (x.file_off.tolist(), x.file_stride.tolist(), x.file_total) == ([0, 48], [15, 2], 96)


def test_layout_with_device_out(batch):
    good, laced = batch
    lay = png._layout(good, laced, None, (0x1000, [7, 100], [20, 2]))
    assert (lay.pix_off.tolist(), lay.pix_stride.tolist(), lay.pix_total) == ([7, 100], [20, 2], None)
    assert (lay.file_off.tolist(), lay.file_stride.tolist(), lay.file_total) == ([7, 100], [20, 2], None)
    x = png._layout(good, laced, "rgb8", (0x1000, [7, 400], [15, 30]))
    assert (x.pix_off.tolist(), x.pix_stride.tolist(), x.file_off.tolist(), x.file_stride.tolist(), x.file_total) == ([7, 400], [15, 30], [0, 48], [15, 2], 96)
    for expand, strides in ((None, [14, 2]), (None, [15, 1]), ("rgb8", [15, 26]), ("rgba8", [19, 36])):
        with pytest.raises(ValueError, match="device_out: a stride below the image's row_bytes"):
            png._layout(good, laced, expand, (0x1000, [0, 400], strides))


def test_pass_jobs_abut_in_the_stream_and_are_dense_in_the_scratch(batch):
    good, laced = batch
    lay = png._layout(good, laced, None, None)
    dec_off, _total = pack(lay.dec_cap, slack=4)
    assert dec_off.tolist() == [0, 64]
    jobs, weave, scratch = png._pass_jobs(good, laced, lay, dec_off)
    assert len(jobs) == 7 == len(png._passes(good[1][1]))
    assert jobs["src_off"][0] == 64 and jobs["dst_off"][0] == 0
    assert (jobs["src_off"][1:] == jobs["src_off"][:-1] + jobs["src_len"][:-1]).all() and jobs["src_len"].sum() == 42
    assert (jobs["src_len"] == jobs["height"].astype(np.uint64) * (jobs["row_bytes"] + np.uint64(1))).all()
    assert (jobs["dst_off"][1:] == jobs["dst_off"][:-1] + jobs["height"][:-1].astype(np.uint64) * jobs["row_bytes"][:-1]).all()
    assert [(int(h), int(rb)) for h, rb in zip(jobs["height"], jobs["row_bytes"])] == [(ph, prb) for pw, ph, prb in A.pass_sizes(9, 9, 1)]
    assert (jobs["bpp"] == 1).all() and scratch == 32 + 16
    assert weave.tolist() == [(0, 48, 2, 9, 9, 1)]  # its passes from the scratch's start into the second image's rows


# ---- status words -> errors ------------------------------------------------------------------------------------------------------------
FINE = (_ffi.OK, (0, 0))


def _verdict(decode=FINE, unfilter=FINE, pass_error=None, bad_index=None, out_len=48, dec_cap=48):
    img = png.PngImage(5, 3, 3, 8, bytes(12), None, None)
    return png._verdict("x", img, b"", decode, unfilter, pass_error, bad_index, out_len, dec_cap)


def _fields(e):
    assert isinstance(e, png.DecompressionError)
    return e.constructor, e.message, e.status, e.detail


def test_png_verdict_branches():
    F = _ffi.E_FILTER
    assert _verdict() is None
    assert _fields(_verdict(decode=(_ffi.E_OUT_TOO_SMALL, (0, 0)))) == ("FormatError", "x: too much image data", F, (0, 0))
    assert _fields(_verdict(out_len=47)) == ("FormatError", "x: not enough image data", F, (0, 0))
    assert _fields(_verdict(pass_error=(3, F, 5, 7))) == ("FormatError", "x: pass 3: row 5 has filter type 7", F, (5, 7))
    for other in ((3, _ffi.E_TRUNCATED, 5, 0), (0, F, 0, 0)):  # a pass cut short; the deinterlacing itself
        assert _fields(_verdict(pass_error=other)) == ("FormatError", "x: the image's passes could not be put together", F, (0, 0))
    assert _fields(_verdict(unfilter=(F, np.array([3, 9], np.uint32)))) == ("FormatError", "x: row 3 has filter type 9", F, (3, 9))
    assert _fields(_verdict(unfilter=(_ffi.E_TRUNCATED, (1, 0)))) == ("FormatError", "x: not enough image data", F, (0, 0))
    assert _fields(_verdict(bad_index=())) == ("FormatError", "x: the image's pixels could not be expanded", F, (0, 0))
    assert _fields(_verdict(bad_index=(4, 2, 5))) == ("FormatError", "x: row 4, pixel 2: palette index 5 of 4", _ffi.E_PALETTE, (4, 2))


def test_png_verdict_precedence():
    F = _ffi.E_FILTER
    later = dict(pass_error=(3, F, 5, 7), unfilter=(F, (3, 9)), bad_index=(4, 2, 5))
    assert _verdict(decode=(_ffi.E_OUT_TOO_SMALL, (0, 0)), **later).message == "x: too much image data"
    assert _verdict(out_len=47, **later).message == "x: not enough image data"
    assert _verdict(**later).message == "x: pass 3: row 5 has filter type 7"
    del later["pass_error"]
    assert _verdict(**later).message == "x: row 3 has filter type 9"
    del later["unfilter"]
    assert _verdict(**later).message == "x: row 4, pixel 2: palette index 5 of 4"


def test_tiff_job_error():
    F = _ffi.E_FILTER
    tile = tiff._Job(0, 2, 7, True, b"", 0, 0, 12, 4, (0, 4, 0, 12), 0, 12, 2, 1, 3, False)
    strip = tiff._Job(1, 0, 4, False, b"", 0, 0, 10, 7, (0, 7, 0, 10), 0, 10, 2, 2, 1, True)
    assert tiff._job_error(tile, _ffi.OK, (0, 0), _ffi.OK) is None
    assert _fields(tiff._job_error(tile, _ffi.E_OUT_TOO_SMALL, (0, 0), _ffi.OK)) == ("FormatError", "page 2, tile 7: too much image data", F, (0, 0))
    assert _fields(tiff._job_error(strip, _ffi.OK, (0, 0), _ffi.E_TRUNCATED)) == ("FormatError", "page 0, strip 4: not enough image data", F, (0, 0))
    assert _fields(tiff._job_error(strip, _ffi.OK, (0, 0), F)) == ("FormatError", "page 0, strip 4: the rows could not be reconstructed", F, (0, 0))
    assert tiff._job_error(tile, _ffi.E_OUT_TOO_SMALL, (0, 0), _ffi.E_TRUNCATED).message == "page 2, tile 7: too much image data"  # the decode first
