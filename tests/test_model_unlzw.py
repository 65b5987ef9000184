"""CPU: the LZW decoder of pzg_unlzw_many (pure_zlib_amd/csrc/unlzw_core.h) as a host program (tests/model/model_unlzw.cpp) against the
table decoder written from the header's rules (tests/lzwcases.py), over the cases the device runs (tests/test_gpu_unlzw.py):
destinations are prefilled and compared whole, so a write outside the capacity fails; status, detail and out_len are compared.  Then
the kernel's code-object notes, the ABI, the writer against PIL's libtiff in both directions, and the golden files' own
consistency."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import lzwcases as L
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_lzw")


class UnlzwModel:
    def __init__(self):
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelunlzw.so")
        srcs = [os.path.join(d, "model_unlzw.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "unlzw_core.h"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        self.M.pzs_unlzw.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
        self.M.pzs_unlzw_starts.restype = C.c_uint32

    def run(self, c, i):
        mis, out_off, nbytes = L.layout(c, i)
        dst = np.full(nbytes, L.FILL, np.uint8)
        res = np.zeros(4, np.int64)
        rc = self.M.pzs_unlzw(c.stream, len(c.stream), mis, dst.ctypes.data, nbytes, out_off, c.cap, c.early_change, res.ctypes.data)
        assert rc == 0, ("written outside the destination", c.name)
        return tuple(int(x) for x in res), dst


@pytest.fixture(scope="module")
def model():
    return UnlzwModel()


def check(model, cases, shift=0):
    for i, c in enumerate(cases):
        res, dst = model.run(c, i + shift)
        assert res == (c.status, len(c.out), c.d0, c.d1), (c.name, i, res)
        diff = dst != L.expected_dst(c, i + shift)
        assert not diff.any(), (c.name, i, int(np.flatnonzero(diff)[0]))


def test_every_case_at_its_layout(model):
    assert model.M.pzs_unlzw_starts() == 3840
    check(model, L.all_cases())


def test_every_layout_meets_other_cases(model):
    for shift in (1, 2, 3):
        check(model, L.all_cases()[shift::3], shift=shift)


def test_the_cases_hold_what_their_names_say():
    cases = L.all_cases()
    by = {c.name: c for c in cases}
    assert len(by) == len(cases) > 200
    assert {c.status for c in cases} == {L.OK, L.E_TRUNCATED, L.E_LZW} and {c.early_change for c in cases} == {0, 1}
    assert {L.layout(c, i)[0] for i, c in enumerate(cases)} == {0, 1, 2, 3} and any(L.layout(c, i)[1] % 16 for i, c in enumerate(cases))
    # the writer's streams come back through the reference
    rnd = np.random.default_rng(1).integers(0, 256, 9000, dtype=np.uint8).tobytes()
    for data in (rnd, bytes(5000), L.text_like(9000)):
        for ec in (0, 1):
            for kw in (dict(), dict(clear_every=None), dict(clear_every=100), dict(leading_clear=False), dict(eoi=False)):
                assert L.decode(L.encode(data, ec, **kw), len(data), ec) == (L.OK, data, 0, 0), (ec, kw)
    assert L.decode(L.encode(rnd, 1), len(rnd), 0)[1] != rnd  # (the two modes part ways at the first width switch)
    # runs: every code but the first is the entry just made
    codes = L.codes_of(bytes(6000), clear_every=None)
    assert codes[:2] == [L.CLEAR, 0] and codes[2:-2] == list(range(258, 258 + len(codes) - 4))
    # random data fills the table: with no Clear it stays full, with one it is cleared
    assert L.CLEAR not in L.codes_of(rnd, clear_every=None)[1:] and len(L.codes_of(rnd, clear_every=None)) > 4200
    assert L.codes_of(rnd, clear_every=3837)[1:].count(L.CLEAR) == 2
    # a string longer than 64 bytes, and one that crosses the capacity
    assert max(len(c.out) for c in cases) >= 40000
    c = by["zeros cap 2017 (a string crosses it)"]
    assert c.status == L.OK and len(c.out) == 2017 and L.decode(c.stream, 2018)[1] == bytes(2018)
    # the failures
    assert (by["f + 1"].status, by["f + 1"].d0, by["f + 1"].d1, by["f + 1"].out) == (L.E_LZW, 260, 2, b"AB")
    assert (by["bad first code after a Clear"].status, by["bad first code after a Clear"].d0, by["bad first code after a Clear"].d1) == (L.E_LZW, 300, 2)
    assert by["f exactly"].out == b"ABBBC" and by["bad code behind the capacity"].status == L.OK
    assert by["empty input"].status == L.E_TRUNCATED and by["empty input, no room"].status == L.OK
    cuts = [c for c in cases if c.name.startswith("cut at")]
    assert len(cuts) > 60 and all(c.status == L.E_TRUNCATED for c in cuts) and len({len(c.out) for c in cuts}) > 30
    # the widths: 254 codes of 9 bits with early change, 255 without
    assert L.width_for(510, 1) == 9 and L.width_for(511, 1) == 10 and L.width_for(511, 0) == 9 and L.width_for(512, 0) == 10
    assert L.width_for(2046, 1) == 11 and L.width_for(2047, 1) == 12 and L.width_for(4096, 1) == 12 == L.width_for(4096, 0)


def test_unlzw_kernel_notes():
    """unlzw_kernel: the position array in LDS (3,840 dwords), no spilled register and no scratch memory."""
    from test_abi import _kernel_notes
    k = [v for name, v in _kernel_notes().items() if "unlzw_kernel" in name]
    assert len(k) == 1, k
    assert k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0, k[0]
    assert k[0]["group_segment_fixed_size"] == 4 * 3840, k[0]


def test_abi_has_the_call():
    from pure_zlib_amd import _ffi
    assert "pzg_unlzw_many" in _ffi.SYMBOLS and hasattr(_ffi.lib(), "pzg_unlzw_many")
    assert _ffi.E_LZW == 25 and _ffi.LZW_EARLY_CHANGE == 1
    import pure_zlib_amd.zlib as Z
    assert hasattr(Z.Context, "unlzw_many") and hasattr(Z.Context, "unlzw_many_device")
    e = Z.error_from_status(b"", 25, (300, 2))
    assert e.constructor == "FormatError" and e.message == "LZW code 300 is not in the table after 2 bytes"
    import inspect
    import pure_zlib_amd.tiff as tiff
    for fn in (tiff.read_tiff_many, tiff.read_tiff, tiff.read_tiff_region, tiff.test_tiff_many):
        assert inspect.signature(fn).parameters["lzw"].default is False, fn.__name__


# ---- the writer against libtiff --------------------------------------------------------------------------------------------------------------
def _pil():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    return Image


def test_reference_reads_what_libtiff_writes():
    """Strips written by libtiff through PIL -- text-like, random (the table fills and is cleared), all-zero and period-7 pixels --
    decode with the reference to the pixels they were written from."""
    Image = _pil()
    from pure_zlib_amd.tiff import parse_tiff
    rnd = np.random.default_rng(5).integers(0, 256, (120, 200), dtype=np.uint8)
    for a in (np.frombuffer(L.text_like(120 * 200), np.uint8).reshape(120, 200), rnd, np.zeros((120, 200), np.uint8),
              (np.arange(120 * 200) % 7).astype(np.uint8).reshape(120, 200)):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="TIFF", compression="tiff_lzw")
        blob = buf.getvalue()
        pg = parse_tiff(blob)[0]
        assert pg.compression == 5
        rows = pg.tile_length
        got = b"".join(L.decode(blob[o:o + n], min(rows, 120 - k * rows) * 200)[1] for k, (o, n) in enumerate(zip(pg.offsets, pg.byte_counts)))
        assert got == a.tobytes()


def test_libtiff_reads_what_the_writer_writes():
    Image = _pil()
    import tiffcases as T
    rng = np.random.default_rng(6)
    for a in (rng.integers(0, 256, (37, 50, 3), dtype=np.uint8), np.zeros((37, 50, 3), np.uint8)):
        for kw in (dict(rows_per_strip=7), dict(tile=(16, 16)), dict(rows_per_strip=37, predictor=2)):
            got = np.asarray(Image.open(io.BytesIO(T.write_tiff([L.lzw_page(a, **kw)], False))))
            assert got.tobytes() == a.tobytes(), kw


def test_golden_files_are_small_and_decode_with_the_reference():
    """Files PIL's libtiff wrote with Compression 5 (tests/golden/tiff_lzw/make_golden.py), their pixels beside them."""
    from pure_zlib_amd.tiff import parse_tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 5
    for f in files:
        blob = open(f, "rb").read()
        px = np.load(f[:-4] + ".npy")
        assert len(blob) < 65536
        pg = parse_tiff(blob)[0]
        assert pg.compression == 5 and (pg.height, pg.width) == px.shape[:2]
        if pg.predictor == 1 and not pg.tiled:
            row = pg.width * pg.samples * pg.bits // 8
            got = b"".join(L.decode(blob[o:o + n], min(pg.tile_length, pg.height - k * pg.tile_length) * row)[1]
                           for k, (o, n) in enumerate(zip(pg.offsets, pg.byte_counts)))
            assert got == px.tobytes()
