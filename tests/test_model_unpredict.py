"""CPU: the Predictor 2 / window stage of pzg_unpredict_many (pure_zlib_amd/csrc/unpredict_core.h) as a host program
(tests/model/model_unpredict.cpp) against the numpy reference written from the header's rules (tests/tiffcases.py), over the cases the
device runs (tests/test_gpu_unpredict.py): destinations are prefilled and compared whole, so a write outside the window fails.  Then
the kernel's code-object notes, the ABI, parse_tiff on what the writer writes and on every prefix of two files, the writer against
PIL where PIL has libtiff, and the golden files' own consistency."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import tiffcases as T
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")


class UnpredictModel:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelunpredict.so")
        srcs = [os.path.join(d, "model_unpredict.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "unpredict_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pzu_unpredict.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        self.M.pzu_run.argtypes = [C.c_uint32, C.c_uint32]
        self.M.pzu_run.restype = C.c_uint32

    def run(self, case, i, slices=4, descending=0):
        desc, src, mis, want = T.single(case, i)
        dst = np.full(len(want), T.FILL, np.uint8)
        sd = np.zeros(3, np.int32)
        rc = self.M.pzu_unpredict(desc.ctypes.data, src.ctypes.data if len(src) else None, len(src), case.slen, mis, dst.ctypes.data, len(dst), slices,
                                  descending, sd.ctypes.data)
        assert rc == 0, (("", "written outside the destination", "the status was not written exactly once")[rc], case.name)
        return int(sd[0]), int(sd[1]) & 0xffffffff, int(sd[2]) & 0xffffffff, dst, want


@pytest.fixture(scope="module")
def model():
    return UnpredictModel()


def check(model, cases, slices=4, descending=0, shift=0):
    for i, c in enumerate(cases):
        st, d0, d1, dst, want = model.run(c, i + shift, slices, descending)
        assert (st, d0, d1) == (c.status, c.d0, c.d1), (c.name, i)
        diff = dst != want
        assert not diff.any(), (c.name, i, int(np.flatnonzero(diff)[0]))


def test_the_run_is_what_the_cases_take_it_for(model):
    for sb in T.SAMPLE_BYTES:
        for s in T.SAMPLES:
            assert model.M.pzu_run(sb, s) == T.run_bytes(sb, s) and T.run_bytes(sb, s) % 16 == 0 and T.run_bytes(sb, s) % (sb * s) == 0


def test_every_sample_width_pixel_size_byte_order_and_width(model):
    assert len(T.shape_cases()) == 4 * 4 * 2 * 11 + 4 * 11
    check(model, T.shape_cases())


def test_every_layout_meets_every_format(model):
    for shift in (1, 6):
        check(model, T.shape_cases()[::3], shift=shift)


def test_heights_windows_carries_and_long_rows(model):
    check(model, T.special_cases())
    check(model, T.special_cases(), shift=3)


def test_sources_cut_short(model):
    check(model, T.truncated_cases())


def test_empty_jobs_and_illegal_geometry(model):
    assert len(T.bad_geometry_cases()) == 20
    check(model, T.empty_cases() + T.bad_geometry_cases())


def test_any_number_of_row_slices_gives_the_same(model):
    for slices, descending in ((1, 0), (3, 1), (64, 0), (4096, 1)):
        check(model, T.shape_cases()[::7] + T.special_cases()[::3] + T.truncated_cases()[::4], slices, descending)


def test_the_cases_hold_what_their_names_say():
    by = {}
    for c in T.shape_cases():
        if c.predictor == 2:
            by.setdefault((c.sb, c.s, c.big_endian), []).append(c)
    assert len(by) == 32
    for (sb, s, _be), v in by.items():
        assert sorted(c.srb // (sb * s) for c in v) == sorted(T.WIDTHS + (T.reach_pixels(sb, s) + 1,))
    kinds = {(c.window[0] > 0, c.window[2] > 0, c.window[1] < c.rows, c.window[3] < c.srb) for c in T.shape_cases() + T.special_cases()}
    assert {(False, False, False, False), (True, True, True, True)} <= kinds and any(c.window[2] % 2 for c in T.shape_cases())
    assert any(c.window[1:] == (1, c.srb - 1, 1) for c in T.shape_cases())  # one byte in the last corner
    hs = {(c.rows, T.rows_per_wave(c.srb, c.sb, c.s)) for c in T.shape_cases() if c.predictor == 2}
    assert any(h == r + 1 for h, r in hs) and any(h == r - 1 for h, r in hs if r > 2) and any(h == 1 for h, _r in hs) and any(h == 2 for h, _r in hs)
    assert {T.layout_of(i)[0] for i in range(28)} == {0, 1, 2, 3} and any(T.layout_of(i)[1] % 4 for i in range(7))
    # the differencing of random rows comes back through the reference, sums wrapping on the way
    rng = np.random.default_rng(5)
    for sb in T.SAMPLE_BYTES:
        for be in (False, True):
            a = rng.integers(0, 256, size=(3, 24 * sb), dtype=np.uint8)
            assert np.array_equal(T.reconstruct(T.difference(a, sb, 3, be), 2, sb, 3, be), a)
    cut = T.truncated_cases()
    assert any(c.slen % c.srb for c in cut) and any(c.slen % c.srb == 0 and c.slen for c in cut) and all(c.d0 == c.slen // c.srb for c in cut)


def test_unpredict_kernel_keeps_everything_in_registers():
    """No spilled vector register, no scratch memory and no LDS in unpredict_kernel, as for the other image stages."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "unpredict_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]
    assert k[0]["group_segment_fixed_size"] == 0, k[0]


def test_abi_has_the_call():
    from pure_zlib_amd import _ffi
    assert "pzg_unpredict_many" in _ffi.SYMBOLS and hasattr(_ffi.lib(), "pzg_unpredict_many")
    assert C.sizeof(_ffi.UnpredictDesc) == 64 == T.DESC.itemsize
    for name in T.DESC.names:
        assert getattr(_ffi.UnpredictDesc, name).offset == T.DESC.fields[name][1], name
    import pure_zlib_amd.zlib as Z
    assert Z.UNPREDICT_DESC.itemsize == 64 and all(Z.UNPREDICT_DESC.fields[n][1] == T.DESC.fields[n][1] for n in T.DESC.names)
    import pure_zlib_amd as P
    assert all(hasattr(P, n) for n in ("parse_tiff", "read_tiff", "read_tiff_many", "read_tiff_region", "test_tiff_many", "TiffImage"))


# ---- the parser and the writer -----------------------------------------------------------------------------------------------------------
def _variants():
    rng = np.random.default_rng(77)
    rgb16 = rng.integers(0, 65536, size=(37, 50, 3)).astype("u2")
    gray8 = rng.integers(0, 256, size=(21, 33, 1)).astype("u1")
    for be in (False, True):
        for big in (False, True):
            yield be, big, [T.Page(rgb16, tile=(16, 16), predictor=2), T.Page(gray8, rows_per_strip=7, compression=32946),
                            T.Page(rgb16, rows_per_strip=5, planar=2, predictor=2, extra_samples=(0,)), T.Page(gray8, tile=(32, 16), orientation=3)]


def test_parse_tiff_reads_what_the_writer_writes():
    from pure_zlib_amd.tiff import parse_tiff
    for be, big, pages in _variants():
        got = parse_tiff(T.write_tiff(pages, be, big))
        assert [(p.index, p.big_endian, p.width, p.height, p.samples, p.bits, p.tiled, p.predictor, p.planar, p.compression) for p in got] == [
            (0, be, 50, 37, 3, 16, True, 2, 1, 8), (1, be, 33, 21, 1, 8, False, 1, 1, 32946), (2, be, 50, 37, 3, 16, False, 2, 2, 8),
            (3, be, 33, 21, 1, 8, True, 1, 1, 8)]
        assert [len(p.offsets) for p in got] == [4 * 3, 3, 8 * 3, 2 * 2] and (got[0].tile_width, got[0].tile_length, got[1].tile_length) == (16, 16, 7)
        assert got[2].extra_samples == (0,) and got[3].orientation == 3 and got[0].photometric == 2 and got[1].photometric == 1
        assert all(p.sample_format == 1 and p.colormap is None for p in got)


def test_every_prefix_of_a_file_is_pages_or_a_named_error():
    from pure_zlib_amd.tiff import parse_tiff
    rng = np.random.default_rng(78)
    a = rng.integers(0, 256, size=(9, 20, 3)).astype("u1")
    files = [T.write_tiff([T.Page(a, rows_per_strip=4, predictor=2), T.Page(a[..., :1])], False, False),
             T.write_tiff([T.Page(a, tile=(16, 16), predictor=2)], True, True)]
    for blob in files:
        assert len(parse_tiff(blob)) >= 1
        kinds = set()
        for n in range(len(blob)):
            try:
                parse_tiff(blob[:n])
                kinds.add("pages")
            except (ValueError, NotImplementedError) as e:
                assert "page" in str(e) or "TIFF" in str(e) or "IFD" in str(e), str(e)
                kinds.add("error")
        assert "error" in kinds


def test_broken_ifds_name_the_page_and_the_tag():
    from pure_zlib_amd.tiff import parse_tiff
    a = np.zeros((4, 4, 1), "u1")
    good = T.write_tiff([T.Page(a, rows_per_strip=4), T.Page(a)])
    first = int.from_bytes(good[4:8], "little")
    loop = bytearray(good)
    n = int.from_bytes(good[first:first + 2], "little")
    second = int.from_bytes(good[first + 2 + 12 * n:first + 6 + 12 * n], "little")
    m = int.from_bytes(good[second:second + 2], "little")
    loop[second + 2 + 12 * m:second + 6 + 12 * m] = first.to_bytes(4, "little")
    with pytest.raises(ValueError, match="page 2: the chain of IFDs comes back"):
        parse_tiff(bytes(loop))
    with pytest.raises(ValueError, match=r"page 0: tag 273 \(StripOffsets\).*past the end"):
        parse_tiff(_with_tag(good, first, 273, 1 << 30))
    with pytest.raises(ValueError, match=r"page 0: tag 257 \(ImageLength\) is missing"):
        parse_tiff(_with_tag(good, first, 257, None))
    with pytest.raises(ValueError, match=r"page 0: tag 273 \(StripOffsets\): 1 values for 2 strips"):
        parse_tiff(_with_tag(good, first, 278, 2))


def _with_tag(blob, ifd, tag, value):
    """The classic little-endian file with the inline value of a tag of its first IFD replaced (None: the tag renamed to 65000)."""
    b = bytearray(blob)
    n = int.from_bytes(b[ifd:ifd + 2], "little")
    for k in range(n):
        at = ifd + 2 + 12 * k
        if int.from_bytes(b[at:at + 2], "little") == tag:
            if value is None:
                b[at:at + 2] = (65000).to_bytes(2, "little")
            else:
                b[at + 2:at + 4] = (4).to_bytes(2, "little")
                b[at + 8:at + 12] = value.to_bytes(4, "little")
            return bytes(b)
    raise AssertionError(tag)


def test_writer_against_pil():
    """A second opinion on the writer (and so on what the device tests hold the reader to): PIL reads its files to the arrays they
    were written from.  Skipped where PIL or its libtiff is missing; the numpy reference is never skipped."""
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    rng = np.random.default_rng(79)
    rgb8 = rng.integers(0, 256, size=(37, 50, 3)).astype("u1")
    gray16 = rng.integers(0, 65536, size=(37, 50, 1)).astype("u2")
    n = 0
    for be in (False, True):
        for page in (T.Page(rgb8, rows_per_strip=7, predictor=2), T.Page(rgb8, tile=(16, 16), predictor=2), T.Page(gray16, tile=(32, 16), predictor=2),
                     T.Page(gray16, rows_per_strip=1, predictor=2, compression=32946), T.Page(rgb8, predictor=1)):
            im = Image.open(io.BytesIO(T.write_tiff([page], be)))
            got = np.asarray(im)
            assert np.array_equal(got.reshape(page.data.shape), page.data), (be, page.tile, page.rows_per_strip)
            n += 1
    assert n == 10


def test_golden_files_are_small_and_parse():
    """Files PIL's libtiff 4.7.1 wrote with Predictor 2 (8-bit RGB and 16-bit gray, as "tiff_deflate" and as "tiff_adobe_deflate"), with
    their pixels beside them: writer-independent fixtures for tests/test_gpu_tiff.py.  That PIL writes strips only, and Compression 8
    under either name: tiles and 32946 come from the writer of tests/tiffcases.py alone."""
    from pure_zlib_amd.tiff import parse_tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 4
    seen = set()
    for f in files:
        blob = open(f, "rb").read()
        px = np.load(f[:-4] + ".npy")
        assert len(blob) < 8192
        pg = parse_tiff(blob)[0]
        assert (pg.height, pg.width) == px.shape[:2] and pg.predictor == 2 and pg.compression in (8, 32946) and len(pg.offsets) > 1
        seen.add((pg.bits, pg.samples))
    assert seen == {(8, 3), (16, 1)}
