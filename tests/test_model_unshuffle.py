"""CPU: the byte-plane stage of pzg_unshuffle_many (pure_zlib_amd/csrc/unshuffle_core.h) as a host program
(tests/model/model_unshuffle.cpp) against the numpy reference written from the header's rules (tests/fpcases.py), over the cases the
device runs (tests/test_gpu_unshuffle.py): destinations are prefilled and compared whole, so a write outside the window fails.  Then
the kernel's code-object notes, the ABI, parse_tiff on the writer's Predictor 3 files, the writer against PIL where PIL has libtiff,
and the golden files' own consistency."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import fpcases as F
import tiffcases as T
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_float")


class UnshuffleModel:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelunshuffle.so")
        srcs = [os.path.join(d, "model_unshuffle.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "unshuffle_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pzs_unshuffle.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        self.M.pzs_run.restype = C.c_uint32

    def run(self, case, i, slices=4, descending=0):
        desc, src, mis, want = F.single(case, i)
        dst = np.full(len(want), F.FILL, np.uint8)
        sd = np.zeros(3, np.int32)
        rc = self.M.pzs_unshuffle(desc.ctypes.data, src.ctypes.data if len(src) else None, len(src), case.slen, mis, dst.ctypes.data, len(dst), slices,
                                  descending, sd.ctypes.data)
        assert rc == 0, (("", "written outside the destination", "the status was not written exactly once")[rc], case.name)
        return int(sd[0]), int(sd[1]) & 0xffffffff, int(sd[2]) & 0xffffffff, dst, want


@pytest.fixture(scope="module")
def model():
    return UnshuffleModel()


def check(model, cases, slices=4, descending=0, shift=0):
    for i, c in enumerate(cases):
        st, d0, d1, dst, want = model.run(c, i + shift, slices, descending)
        assert (st, d0, d1) == (c.status, c.d0, c.d1), (c.name, i)
        diff = dst != want
        assert not diff.any(), (c.name, i, int(np.flatnonzero(diff)[0]))


def test_the_run_is_what_the_cases_take_it_for(model):
    assert model.M.pzs_run() == F.RUN and F.REACH == 64 * F.RUN


def test_every_element_size_sum_stride_plane_order_and_count(model):
    assert len(F.shape_cases()) == 3 * 5 * 2 * 10
    check(model, F.shape_cases())


def test_every_layout_meets_every_format(model):
    for shift in (1, 2, 3, 6):
        check(model, F.shape_cases()[::3], shift=shift)


def test_heights_windows_carries_and_long_rows(model):
    check(model, F.special_cases())
    check(model, F.special_cases(), shift=3)


def test_sources_cut_short(model):
    check(model, F.truncated_cases())


def test_empty_jobs_and_illegal_geometry(model):
    assert len(F.empty_cases()) == 5 and len(F.bad_geometry_cases()) == 21
    check(model, F.empty_cases() + F.bad_geometry_cases())


def test_any_number_of_row_slices_gives_the_same(model):
    for slices, descending in ((1, 0), (3, 1), (64, 0), (4096, 1)):
        check(model, F.shape_cases()[::7] + F.special_cases()[::3] + F.truncated_cases()[::4], slices, descending)


def test_the_cases_hold_what_their_names_say():
    by = {}
    for c in F.shape_cases():
        by.setdefault((c.b, c.s, c.reverse), []).append(c)
    assert len(by) == 30
    for (b, s, _rev), v in by.items():
        assert sorted(c.srb // b for c in v) == sorted(F._count(n, s) for n in F.COUNTS)
        assert all(s == 0 or (c.srb // b) % s == 0 for c in v)
    cases = F.shape_cases() + F.special_cases()
    kinds = {(c.window[0] > 0, c.window[2] > 0, c.window[1] < c.rows, c.window[3] < c.srb) for c in cases}
    assert {(False, False, False, False), (True, True, True, True)} <= kinds
    assert any(c.window[2] % c.b for c in cases) and any((c.window[2] + c.window[3]) % c.b for c in cases)  # windows that start, and end, inside an element
    assert any(c.window[1:] == (1, c.srb - 1, 1) for c in cases) and any(c.window[1:] == (1, c.srb - c.b, c.b) for c in cases)
    hs = {(c.rows, F.rows_per_wave(c.srb // c.b)) for c in F.shape_cases()}
    assert any(h == r + 1 for h, r in hs) and any(h == r - 1 for h, r in hs if r > 2) and any(h == 1 for h, _r in hs) and any(h == 2 for h, _r in hs)
    assert {F.layout_of(i)[0] for i in range(28)} == {0, 1, 2, 3} and any(F.layout_of(i)[1] % 4 for i in range(7))
    # the encoding of random rows comes back through the reference, sums wrapping on the way
    rng = np.random.default_rng(5)
    for b in F.ELEM_BYTES:
        for s in F.SUM_STRIDES:
            for rev in (False, True):
                a = rng.integers(0, 256, size=(3, 24 * b), dtype=np.uint8)
                assert np.array_equal(F.reconstruct(F.encode(a, b, s, rev), b, s, rev), a)
                assert s == 0 or not np.array_equal(F.encode(a, b, s, rev), F.encode(a, b, 0, rev))
    # the transpose alone is the shuffle filter of HDF5 and Zarr: plane j holds byte j of every element
    a = np.arange(3 * 5 * 4, dtype=np.uint8).reshape(3, 20)
    assert np.array_equal(F.encode(a, 4, 0, False), a.reshape(3, 5, 4).transpose(0, 2, 1).reshape(3, 20))
    cut = F.truncated_cases()
    assert any(c.slen % c.srb for c in cut) and any(c.slen % c.srb == 0 and c.slen for c in cut) and all(c.d0 == c.slen // c.srb for c in cut)


def test_unshuffle_kernel_keeps_everything_in_registers():
    """No spilled vector register, no scratch memory and no LDS in unshuffle_kernel: the sums and the planes' carries live in
    registers (unshuffle_core.h says why LDS staging was not built), as for the other image stages."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "unshuffle_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]
    assert k[0]["group_segment_fixed_size"] == 0, k[0]


def test_abi_has_the_call():
    from pure_zlib_amd import _ffi
    assert "pzg_unshuffle_many" in _ffi.SYMBOLS and hasattr(_ffi.lib(), "pzg_unshuffle_many")
    assert C.sizeof(_ffi.UnshuffleDesc) == 64 == F.DESC.itemsize
    assert F.DESC.names == ("src_off", "dst_off", "dst_stride", "src_row_bytes", "rows", "win_row", "win_rows", "win_byte", "win_bytes", "elem_bytes",
                            "sum_stride", "reverse", "reserved0")
    assert [F.DESC.fields[n][1] for n in F.DESC.names] == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 49, 50, 51]
    for name in F.DESC.names:
        assert getattr(_ffi.UnshuffleDesc, name).offset == F.DESC.fields[name][1], name
    assert _ffi.UnshuffleDesc.reserved.offset == 52
    import pure_zlib_amd.zlib as Z
    assert Z.UNSHUFFLE_DESC.itemsize == 64 and all(Z.UNSHUFFLE_DESC.fields[n][1] == F.DESC.fields[n][1] for n in F.DESC.names)
    assert Z.UNSHUFFLE_DESC.fields["reserved"][1] == 52
    assert hasattr(Z.Context, "unshuffle_many") and hasattr(Z.Context, "unshuffle_many_device")
    assert _ffi.lib().pzg_version() == 5
    import inspect
    import pure_zlib_amd.tiff as tiff
    for fn in (tiff.read_tiff_many, tiff.read_tiff, tiff.read_tiff_region, tiff.test_tiff_many):
        assert inspect.signature(fn).parameters["float_predictor"].default is False, fn.__name__


# ---- the parser and the writer -----------------------------------------------------------------------------------------------------------
def test_parse_tiff_reads_the_writers_float_pages():
    from pure_zlib_amd.tiff import parse_tiff
    rng = np.random.default_rng(77)
    rgb32 = F.float_data(rng, (37, 50, 3), "f4")
    gray16 = F.float_data(rng, (21, 33, 1), "f2")
    gray64 = F.float_data(rng, (21, 33, 1), "f8")
    for be in (False, True):
        for big in (False, True):
            pages = [F.float_page(rgb32, be, tile=(16, 16)), F.float_page(gray16, be, rows_per_strip=7, compression=32946),
                     F.float_page(rgb32, be, rows_per_strip=5, planar=2), F.float_page(gray64, be, tile=(32, 16))]
            got = parse_tiff(T.write_tiff(pages, be, big))
            assert [(p.index, p.big_endian, p.width, p.height, p.samples, p.bits, p.tiled, p.predictor, p.planar, p.compression, p.sample_format) for p in got] == [
                (0, be, 50, 37, 3, 32, True, 3, 1, 8, 3), (1, be, 33, 21, 1, 16, False, 3, 1, 32946, 3), (2, be, 50, 37, 3, 32, False, 3, 2, 8, 3),
                (3, be, 33, 21, 1, 64, True, 3, 1, 8, 3)]
            assert [len(p.offsets) for p in got] == [4 * 3, 3, 8 * 3, 2 * 2]


def test_the_hook_stores_what_the_reference_reads():
    """The streams of a written Predictor 3 page inflate to rows that the reference turns back into the page's bytes."""
    import zlib
    from pure_zlib_amd.tiff import parse_tiff
    rng = np.random.default_rng(80)
    a = F.float_data(rng, (9, 20, 3), "f4")
    for be in (False, True):
        blob = T.write_tiff([F.float_page(a, be, rows_per_strip=4)], be)
        pg = parse_tiff(blob)[0]
        rows = [F.reconstruct(np.frombuffer(zlib.decompress(blob[o:o + n]), np.uint8).reshape(-1, 240), 4, 3, not be) for o, n in zip(pg.offsets, pg.byte_counts)]
        assert np.concatenate(rows).tobytes() == a.astype(">f4" if be else "<f4").tobytes()


def test_writer_against_pil():
    """A second opinion on the encoder (and so on what the device tests hold the reader to): PIL's libtiff reads the writer's
    little-endian float32 gray Predictor 3 files to the arrays they were written from, bit for bit.  Skipped where PIL or its libtiff
    is missing; the numpy reference is never skipped."""
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    rng = np.random.default_rng(79)
    gray = F.float_data(rng, (37, 50, 1), "<f4")
    n = 0
    for kw in (dict(rows_per_strip=1), dict(rows_per_strip=7), dict(tile=(16, 16)), dict(tile=(32, 16)), dict(rows_per_strip=7, compression=32946)):
        im = Image.open(io.BytesIO(T.write_tiff([F.float_page(gray, False, **kw)], False)))
        got = np.asarray(im)
        assert got.dtype == np.float32 and got.tobytes() == gray.tobytes(), kw
        n += 1
    assert n == 5


def test_golden_files_are_small_and_parse():
    """Files PIL's libtiff 4.7.1 wrote with Predictor 3 (float32 gray in strips of several rows, as "tiff_deflate" and as
    "tiff_adobe_deflate", at 33 x 16 and 129 x 21), with their pixels beside them: writer-independent fixtures for
    tests/test_gpu_tiff_float.py.  The reference reads them here."""
    import zlib
    from pure_zlib_amd.tiff import parse_tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 4
    seen = set()
    for f in files:
        blob = open(f, "rb").read()
        px = np.load(f[:-4] + ".npy")
        assert len(blob) < 8192 and px.dtype == np.dtype("<f4")
        pg = parse_tiff(blob)[0]
        assert (pg.height, pg.width) == px.shape[:2] and pg.predictor == 3 and pg.sample_format == 3 and pg.bits == 32 and pg.samples == 1
        assert pg.compression in (8, 32946) and len(pg.offsets) > 1 and pg.tile_length > 1 and not pg.tiled and not pg.big_endian and pg.width % 2
        rows = [F.reconstruct(np.frombuffer(zlib.decompress(blob[o:o + n]), np.uint8).reshape(-1, 4 * pg.width), 4, 1, True)
                for o, n in zip(pg.offsets, pg.byte_counts)]
        assert np.concatenate(rows).tobytes() == px.tobytes()
        seen.add((pg.width, pg.height))
    assert seen == {(33, 16), (129, 21)}
