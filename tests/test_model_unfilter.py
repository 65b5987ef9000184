"""CPU: the scanline unfilter of pzg_unfilter_many (pure_zlib_amd/csrc/unfilter_core.h) as a host program (tests/model/model_unfilter.cpp)
against the reference unfilter written from the PNG specification (tests/pngcases.py), over the shapes the device runs
(tests/test_gpu_png.py), and the PNG writer against PIL where PIL is installed.  The kernel's code-object notes are checked here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pngcases as PC
from conftest import ROOT


class UnfilterModel:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelunfilter.so")
        srcs = [os.path.join(d, "model_unfilter.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "unfilter_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pzu_unfilter.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_void_p]

    def run(self, case, mis, dst_off, stride_extra):
        """(status, d0, d1, the destination: FILL, the image at dst_off in it, 9 bytes behind it)"""
        stride = case.row_bytes + stride_extra
        dst = np.full(dst_off + case.height * stride + 9, PC.FILL, np.uint8)
        sd = np.zeros(3, np.int32)
        rc = self.M.pzu_unfilter(case.stream, len(case.stream), mis, dst.ctypes.data, len(dst), dst_off, stride, case.row_bytes, case.height,
                                 case.bpp, sd.ctypes.data)
        assert rc == 0, ("written outside the destination", case.name)
        return int(sd[0]), int(sd[1]) & 0xffffffff, int(sd[2]) & 0xffffffff, dst


@pytest.fixture(scope="module")
def model():
    return UnfilterModel()


def check(model, cases):
    for i, c in enumerate(cases):
        for mis, dst_off, extra in ((i % 4, (1, 7, 12, 3, 0)[i % 5], 5), ((i + 1) % 4, 16, 0)):
            st, d0, d1, dst = model.run(c, mis, dst_off, extra)
            assert (st, d0, d1) == (c.status, c.d0, c.d1), (c.name, mis, dst_off)
            want = np.full(len(dst), PC.FILL, np.uint8)
            for r, row in enumerate(c.rows):
                at = dst_off + r * (c.row_bytes + extra)
                want[at:at + c.row_bytes] = np.frombuffer(row, np.uint8)
            assert np.array_equal(dst, want), (c.name, mis, dst_off, int(np.flatnonzero(dst != want)[0]))


def test_every_shape_with_random_filters(model):
    check(model, PC.shape_cases())


def test_each_filter_paeth_ties_and_average_carry(model):
    check(model, PC.filter_cases())


def test_bad_filter_bytes_and_cut_inputs(model):
    check(model, PC.error_cases() + [PC.empty_case()])


def test_illegal_geometry_is_reported_not_run(model):
    c = PC.shape_cases()[0]
    for bpp in (0, 5, 7, 9, 255):
        bad = PC.Case("bpp %d" % bpp, bpp, c.row_bytes, c.height, c.stream, PC.E_FILTER, 0xffffffff, bpp, [])
        check(model, [bad])
    st, d0, _d1, dst = model.run(PC.Case("stride", 3, 9, 2, bytes(20), 0, 0, 0, []), 0, 4, -1)
    assert (st, d0) == (PC.E_FILTER, 0xffffffff) and (dst == PC.FILL).all()


def test_the_cases_hold_what_their_names_say():
    """Paeth's three tie orders and Average's ninth bit really occur in the bytes built for them."""
    seen = set()
    for c in PC.filter_cases():
        if c.name.startswith("paeth-ties"):
            rows = [np.frombuffer(r, np.uint8).astype(int) for r in c.rows]
            for y in range(1, len(rows)):
                for j in range(c.bpp, c.row_bytes):
                    a, b, cc = rows[y][j - c.bpp], rows[y - 1][j], rows[y - 1][j - c.bpp]
                    pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                    seen |= {"a=b=c"} if a == b == cc else set()
                    seen |= {"pa=pb<pc"} if pa == pb < pc else set()
                    seen |= {"pb=pc<pa"} if pb == pc < pa else set()
        if c.name.startswith("average-high"):
            rows = [np.frombuffer(r, np.uint8).astype(int) for r in c.rows]
            assert all(rows[y][j - c.bpp] + rows[y - 1][j] >= 256 for y in range(1, len(rows)) for j in range(c.bpp, c.row_bytes))
    assert seen == {"a=b=c", "pa=pb<pc", "pb=pc<pa"}
    shapes = {(c.bpp, c.row_bytes, c.height) for c in PC.shape_cases()}
    assert len(shapes) == len(PC.shape_cases()) >= 200


def test_writer_against_pil():
    """A second opinion on whole files: what the writer writes, PIL reads back as the samples it was given."""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(3)
    for ctype, mode, depth in ((0, "L", 8), (2, "RGB", 8), (6, "RGBA", 8), (4, "LA", 8), (3, "P", 8)):
        for w, h in ((5, 3), (67, 65)):
            rb, _bpp = PC.geometry(w, ctype, depth)
            raw = rng.integers(0, 16 if ctype == 3 else 256, size=(h, rb), dtype=np.uint8)
            for filters in (rng.integers(0, 5, size=h), "adaptive"):
                png = PC.write_png(w, h, ctype, depth, raw, filters, idat=7)
                im = Image.open(io.BytesIO(png))
                im.load()
                assert im.mode == mode and im.size == (w, h)
                assert np.array_equal(np.asarray(im).reshape(h, rb), raw), (ctype, w, h)


def test_unfilter_kernel_keeps_everything_in_registers():
    """No spilled vector register and no scratch memory in unfilter_kernel, as for the inflate kernels (tests/test_abi.py)."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "unfilter_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]


def test_abi_has_the_call_and_its_error_text():
    from pure_zlib_amd import _ffi
    import pure_zlib_amd.zlib as Z
    assert hasattr(_ffi.lib(), "pzg_unfilter_many") and _ffi.E_FILTER == 23
    assert Z.error_from_status(b"", 23, (64, 5)).show() == "Block format error: row 64 has filter type 5"
