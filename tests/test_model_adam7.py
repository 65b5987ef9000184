"""CPU: the Adam7 gather of pzg_adam7_many (pure_zlib_amd/csrc/adam7_core.h) as a host program (tests/model/model_adam7.cpp) against
the reference written from the PNG specification (tests/adam7cases.py), over the shapes the device runs (tests/test_gpu_adam7.py),
and the interlaced PNG writer against PIL where PIL is installed.  The kernel's code-object notes are checked here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adam7cases as A
import pngcases as PC
from conftest import ROOT


class Adam7Model:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodeladam7.so")
        srcs = [os.path.join(d, "model_adam7.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "adam7_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pza_adam7.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_void_p]
        self.M.pza_slices.restype = C.c_uint32
        self.M.pza_src_extent.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        self.M.pza_src_extent.restype = C.c_uint64

    def run(self, case, mis, dst_off, stride_extra, slices=A.ROW_SLICES):
        """(status, d0, d1, the destination: FILL, the image at dst_off in it, 9 bytes behind it)"""
        stride = A.stride_of(case, stride_extra)
        dst = np.full(dst_off + len(case.rows) * max(stride, 0) + 9, A.FILL, np.uint8)
        sd = np.zeros(3, np.int32)
        rc = self.M.pza_adam7(case.src, len(case.src), mis, dst.ctypes.data, len(dst), dst_off, stride, case.width, case.height, case.bits, slices,
                              sd.ctypes.data)
        assert rc == 0, ("written outside the destination", case.name)
        return int(sd[0]), int(sd[1]) & 0xffffffff, int(sd[2]) & 0xffffffff, dst


@pytest.fixture(scope="module")
def model():
    return Adam7Model()


def check(model, cases, slices=A.ROW_SLICES):
    for i, c in enumerate(cases):
        for mis, dst_off, extra in ((i % 4, (1, 7, 12, 3, 0)[i % 5], 5), ((i + 1) % 4, 16, 0)):
            st, d0, d1, dst = model.run(c, mis, dst_off, extra, slices)
            assert (st, d0, d1) == (c.status, c.d0, c.d1), (c.name, mis, dst_off)
            want = np.full(len(dst), A.FILL, np.uint8)
            for r, row in enumerate(c.rows):
                at = dst_off + r * A.stride_of(c, extra)
                want[at:at + len(row)] = np.frombuffer(row, np.uint8)
            assert np.array_equal(dst, want), (c.name, mis, dst_off, int(np.flatnonzero(dst != want)[0]))


def test_every_small_shape_of_every_depth(model):
    """1..9 x 1..9: every combination of empty passes."""
    assert len(A.small_cases()) == 729
    check(model, A.small_cases())


def test_edge_shapes_and_a_tall_narrow_image(model):
    assert model.M.pza_slices() == A.ROW_SLICES  # the tall case is taller than a round of the kernel's own number of slices
    assert len(A.edge_cases()) == 28 and A.edge_cases()[-1].height > A.ROW_SLICES
    check(model, A.edge_cases())


def test_any_number_of_row_slices_gives_the_same(model):
    """The split is no part of the result: one wave an image, three, and more waves than most images have rows."""
    for slices in (1, 3, 64):
        check(model, A.small_cases()[::13] + A.edge_cases()[::4], slices)


def test_empty_images_and_illegal_geometry(model):
    check(model, A.empty_cases() + A.bad_geometry_cases())
    c = A.small_cases()[40]
    st, d0, d1, dst = model.run(A.Case("stride", c.width, c.height, c.bits, b"", 0, 0, 0, []), 0, 4, -1)
    assert (st, d0, d1) == (A.E_FILTER, A.BAD_ARGS, c.bits) and (dst == A.FILL).all()


def test_the_source_extent_is_the_sum_of_the_passes(model):
    for c in A.all_cases()[::7]:
        assert model.M.pza_src_extent(c.width, c.height, c.bits) == len(c.src) == A.extent(c.width, c.height, c.bits), c.name


def test_the_cases_hold_what_their_names_say():
    """Every combination of empty passes occurs, random padding bits do, and 33 x 131 has the pass heights the unfilter's group boundary
    falls inside."""
    empties = {tuple(pw == 0 for pw, _ph, _prb in A.pass_sizes(c.width, c.height, c.bits)) for c in A.small_cases()}
    # pass 1 is never empty; 2, 4, 6 go with the width (w <= 4, w <= 2, w = 1), 3, 5, 7 with the height: 4 x 4 combinations
    assert len(empties) == 16 and all(not e[0] for e in empties)
    assert [ph for _pw, ph, _prb in A.pass_sizes(33, 131, 8)][5:] == [66, 65]
    assert len({(c.width, c.height, c.bits) for c in A.all_cases()}) == len(A.all_cases()) == 757
    # one pixel a row at one bit a pixel: every source byte is a pixel and seven padding bits, and the delivered rows have none set
    narrow = [c for c in A.small_cases() if c.bits == 1 and c.width == 1]
    assert any(b & 0x7f for c in narrow for b in c.src) and not any(r[0] & 0x7f for c in narrow for r in c.rows)


def test_writer_against_pil():
    """A second opinion on whole files: what the interlaced writer writes, PIL reads back as the pixels it was given."""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(4)
    for ctype, mode, depth in ((0, "L", 8), (2, "RGB", 8), (6, "RGBA", 8), (4, "LA", 8), (3, "P", 8)):
        for w, h in ((5, 3), (67, 65)):
            rb, _bpp = PC.geometry(w, ctype, depth)
            raw = rng.integers(0, 16 if ctype == 3 else 256, size=(h, rb), dtype=np.uint8)
            for filters in ((lambda ph: rng.integers(0, 5, size=ph)), "adaptive"):
                png = A.write_png(w, h, ctype, depth, raw, filters, idat=7)
                im = Image.open(io.BytesIO(png))
                im.load()
                assert im.mode == mode and im.size == (w, h) and im.info.get("interlace") == 1
                assert np.array_equal(np.asarray(im).reshape(h, rb), raw), (ctype, w, h)


def test_adam7_kernel_keeps_everything_in_registers():
    """No spilled vector register and no scratch memory in adam7_kernel, as for the unfilter (tests/test_model_unfilter.py)."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "adam7_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]


def test_abi_has_the_call():
    from pure_zlib_amd import _ffi
    assert "pzg_adam7_many" in _ffi.SYMBOLS and hasattr(_ffi.lib(), "pzg_adam7_many")
