"""CPU: the pixel expansion of pzg_expand_many (pure_zlib_amd/csrc/expand_core.h) as a host program (tests/model/model_expand.cpp)
against the numpy reference written from the header's rules (tests/expandcases.py), over the cases the device runs
(tests/test_gpu_expand.py); the reference itself against PIL where PIL is installed and converts the same way; the 16-bit rule
against its statement; the kernel's code-object notes."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import expandcases as X
import pngcases as PC
from conftest import ROOT


class ExpandModel:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelexpand.so")
        srcs = [os.path.join(d, "model_expand.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "expand_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pze_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                      C.c_void_p]
        self.M.pze_slices.restype = C.c_uint32
        self.M.pze_unit.restype = C.c_uint32

    def run(self, case, i, slices=X.ROW_SLICES, descending=0):
        """(status, d0, d1, the destination, what it must be, the bytes of it that may hold anything)"""
        desc, src, mis, pal, want, loose = X.single(case, i)
        dst = np.full(len(want), X.FILL, np.uint8)
        sd = np.zeros(3, np.int32)
        rc = self.M.pze_expand(desc.ctypes.data, src.ctypes.data if len(src) else None, len(src), mis, pal.ctypes.data if pal is not None else None,
                               len(pal) if pal is not None else 0, dst.ctypes.data, len(dst), slices, descending, sd.ctypes.data)
        assert rc == 0, (("", "written outside the destination", "the status was not written exactly once")[rc], case.name)
        return int(sd[0]), int(sd[1]) & 0xffffffff, int(sd[2]) & 0xffffffff, dst, want, loose


@pytest.fixture(scope="module")
def model():
    return ExpandModel()


def check(model, cases, slices=X.ROW_SLICES, descending=0, shift=0):
    for i, c in enumerate(cases):
        st, d0, d1, dst, want, loose = model.run(c, i + shift, slices, descending)
        assert (st, d0, d1) == (c.status, c.d0, c.d1), (c.name, i)
        diff = (dst != want) & ~loose
        assert not diff.any(), (c.name, i, int(np.flatnonzero(diff)[0]))


def test_every_type_format_and_width(model):
    assert model.M.pze_slices() == X.ROW_SLICES and X.HEIGHTS[-1] == X.ROW_SLICES + 1 and model.M.pze_unit() == 16
    assert len(X.shape_cases()) == 15 * 2 * 2 * 19
    check(model, X.shape_cases())


def test_every_layout_meets_every_type(model):
    """layout_of() has a period of 12 and a type's cases come 19 at a time: shifted, every case has another layout."""
    for shift in (1, 5):
        check(model, X.shape_cases()[::3], shift=shift)


def test_heights_palette_sizes_and_near_miss_keys(model):
    check(model, X.special_cases())


def test_the_first_bad_palette_index_is_named_whatever_the_order_of_the_waves(model):
    for slices, descending in ((X.ROW_SLICES, 0), (X.ROW_SLICES, 1), (1, 0), (3, 1), (64, 0)):
        check(model, X.bad_index_cases(), slices, descending)


def test_any_number_of_row_slices_gives_the_same(model):
    for slices in (1, 3, 64):
        check(model, X.shape_cases()[::11] + X.special_cases()[::5], slices, descending=slices == 3)


def test_empty_images_and_illegal_geometry(model):
    assert len(X.bad_geometry_cases()) == 17
    check(model, X.empty_cases() + X.bad_geometry_cases())


def test_the_cases_hold_what_their_names_say():
    by = {}
    for c in X.shape_cases():
        by.setdefault((c.ct, c.depth, c.fmt, c.name.split()[3]), []).append(c)
        assert (c.key is not None) == (c.name.split()[3] == "trns1" and c.ct in (0, 2)), c.name
        if c.ct == 3 and len(c.palette) > 1:
            assert (c.palette >> 24 != 255).any() == (c.name.split()[3] == "trns1"), c.name
    assert len(by) == 60 and all(sorted(c.width for c in v) == sorted(X.WIDTHS) for v in by.values())
    assert {c.height for c in X.shape_cases()} == set(X.HEIGHTS)
    # padding bits are set in the packed sources, and the reference does not show them
    c = next(c for c in X.shape_cases() if (c.ct, c.depth, c.width, c.key) == (0, 1, 3, None))
    assert (c.rows[:, -1] & 0x1f == 0x1f).all() and set(np.unique(c.out)) <= {0, 255}
    assert sorted({len(c.palette) for c in X.special_cases() if c.name.startswith("palette of")}) == list(X.PALETTE_SIZES)
    assert {X.layout_of(i)[0] for i in range(12)} == {0, 1, 2, 3} and {X.layout_of(i)[1] for i in range(12)} == set(X.DST_OFFS)
    assert {X.layout_of(i)[2] for i in range(12)} == {0, 5}


def test_sixteen_bit_samples_give_their_high_byte():
    rng = np.random.default_rng(3)
    for ct in (0, 2, 4, 6):
        ch = X.CHANNELS[ct]
        s = rng.integers(0, 65536, size=(3, 5, ch)).astype(">u2")
        out = X.expand_reference(5, 3, ct, 16, s.view(np.uint8).reshape(3, -1))
        hi = (s.astype(np.uint32) >> 8).astype(np.uint8)
        assert np.array_equal(out[..., 0], hi[..., 0]) and np.array_equal(out[..., 2], hi[..., 2 if ch >= 3 else 0])
        assert np.array_equal(out[..., 3], hi[..., ch - 1]) if ct in (4, 6) else (out[..., 3] == 255).all()


def test_reference_against_pil():
    """Whole files (tests/pngcases.py writes them): PIL's convert("RGBA") where it is defined as the header defines the expansion --
    gray 1/2/4/8, RGB 8, RGBA 8, gray+alpha 8, palette 1/2/4/8, with and without tRNS (a colour key on gray: at 1 and 8 bits)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    n = 0
    for ct, depth in [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (6, 8), (4, 8), (3, 1), (3, 2), (3, 4), (3, 8)]:
        for trns in (False, True):
            if trns and (ct in (4, 6) or (ct, depth) in ((0, 2), (0, 4))):
                continue  # (PIL scales 2- and 4-bit gray to 8 bits on loading and then holds the UNSCALED key against it: not the same rule)
            w, h = 13, 5
            entries = min(1 << depth, 16)
            rows = X._random_rows(rng, w, h, ct, depth, entries if ct == 3 else None)
            plte = rng.integers(0, 256, size=(entries, 3), dtype=np.uint8) if ct == 3 else None
            key = pal = chunk = None
            if ct == 3:
                alpha = rng.integers(0, 256, size=entries // 2 if trns else 0, dtype=np.uint8)  # shorter than PLTE
                pal = np.full((entries, 4), 255, np.uint8)
                pal[:, :3], pal[:len(alpha), 3] = plte, alpha
                chunk = alpha.tobytes() if trns else None
            elif trns:
                key = tuple(int(v) for v in X.samples_of(rows, w, ct, depth)[2, 6])
                chunk = b"".join(int(v).to_bytes(2, "big") for v in key)
            png = PC.write_png(w, h, ct, depth, rows, "adaptive", palette=plte.tobytes() if plte is not None else None, trns=chunk)
            im = Image.open(io.BytesIO(png))
            want = np.asarray(im.convert("RGBA"))
            got = X.expand_reference(w, h, ct, depth, rows, X.RGBA8, pal, key)
            assert np.array_equal(got, want), (ct, depth, trns)
            assert np.array_equal(X.expand_reference(w, h, ct, depth, rows, X.RGB8, pal, key), want[..., :3])
            n += 1
    assert n == 18


def test_expand_kernel_keeps_everything_in_registers():
    """No spilled vector register and no scratch memory in expand_kernel, as for the Adam7 kernel (tests/test_model_adam7.py); its LDS
    is the palette's 1 KiB."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "expand_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]
    assert k[0]["group_segment_fixed_size"] == 1024, k[0]


def test_abi_has_the_call():
    from pure_zlib_amd import _ffi
    assert "pzg_expand_many" in _ffi.SYMBOLS and hasattr(_ffi.lib(), "pzg_expand_many")
    assert C.sizeof(_ffi.ExpandDesc) == 64 == X.DESC.itemsize
    for name in X.DESC.names:
        assert getattr(_ffi.ExpandDesc, name).offset == X.DESC.fields[name][1], name
    import pure_zlib_amd.zlib as Z
    assert Z.EXPAND_DESC.itemsize == 64 and all(Z.EXPAND_DESC.fields[n][1] == X.DESC.fields[n][1] for n in X.DESC.names)
    assert _ffi.E_PALETTE == X.E_PALETTE == 24
    e = Z.error_from_status(b"", _ffi.E_PALETTE, (7, 9))
    assert e.constructor == "FormatError" and "row 7, pixel 9" in e.message
