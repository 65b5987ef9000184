"""GPU: pure_zlib_amd/tiff.py with lzw=True against the arrays its Compression 5 files were written from, bit for bit: the writer of
tests/tiffcases.py with the LZW hook of tests/lzwcases.py over its variants (layouts x predictors x byte orders x planar), the golden
files PIL's libtiff wrote, batches that mix Deflate, LZW and Predictor 3 files with broken files among good ones, device_out, regions,
and the launches a call issues."""
import glob
import os

import numpy as np
import pytest

import fpcases as F
import lzwcases as L
import tiffcases as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_lzw")


def _same(img, a, be, planar=1):
    want = a if planar == 1 else np.moveaxis(a, 2, 0)
    file_dt = a.dtype.newbyteorder(">" if be else "<") if a.dtype.itemsize > 1 else a.dtype
    assert img.data.shape == want.shape and img.data.dtype == file_dt, (img.data.shape, img.data.dtype, want.shape, file_dt)
    assert img.data.tobytes() == np.ascontiguousarray(want).astype(file_dt).tobytes()


@pytest.fixture(scope="module")
def arrays():
    rng = np.random.default_rng(201)
    smooth = lambda shape, top: (np.cumsum(rng.integers(-3, 4, size=shape), axis=1) % top)  # noqa: E731
    return {"rgb8": smooth((37, 50, 3), 256).astype(np.uint8), "gray16": smooth((33, 65, 1), 65536).astype(np.uint16),
            "rgba8": rng.integers(0, 256, size=(21, 33, 4), dtype=np.uint8), "gray32": smooth((16, 33, 1), 1 << 32).astype(np.uint32),
            "zero8": np.zeros((40, 70, 1), np.uint8)}


def test_read_tiff_many_over_the_writers_variants(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    files, wants = [], []
    i = 0
    for name, a in arrays.items():
        for layout in ({"tile": (16, 16)}, {"tile": (32, 16)}, {"rows_per_strip": 1}, {"rows_per_strip": 7}, {}):
            for predictor in (1, 2):
                for planar in ((1, 2) if a.shape[2] > 1 else (1,)):
                    be, big = bool(i & 1), bool(i & 2)
                    files.append(T.write_tiff([L.lzw_page(a, predictor=predictor, planar=planar, **layout)], be, big, seed=i))
                    wants.append((a, be, planar, name, layout, predictor))
                    i += 1
    assert {(w[1], bool(k & 2)) for k, w in enumerate(wants)} == {(False, False), (True, False), (False, True), (True, True)}
    got = tiff.read_tiff_many(files, ctx=gpu_ctx, lzw=True)
    assert len(got) == len(files) > 60
    for g, (a, be, planar, name, layout, predictor) in zip(got, wants):
        assert isinstance(g, list) and len(g) == 1, (g, name, layout, planar, predictor)
        assert (g[0].width, g[0].height, g[0].samples, g[0].planar, g[0].tiled) == (a.shape[1], a.shape[0], a.shape[2], planar, "tile" in layout), (name, layout)
        _same(g[0], a, be, planar)
    assert tiff.test_tiff_many(files[:6], ctx=gpu_ctx, lzw=True) == []
    assert [k for k, _why in tiff.test_tiff_many(files[:6], ctx=gpu_ctx)] == list(range(6))


def test_float_predictor_and_packed_rows(gpu_ctx):
    from pure_zlib_amd import tiff
    rng = np.random.default_rng(202)
    f32, rgb16 = F.float_data(rng, (40, 50, 1), "f4"), F.float_data(rng, (17, 31, 3), "f2")
    for a, be, kw in ((f32, False, dict(tile=(16, 16))), (f32, True, dict(rows_per_strip=7)), (rgb16, False, dict(planar=2)), (rgb16, True, dict(tile=(16, 16)))):
        img = tiff.read_tiff(T.write_tiff([L.lzw_float_page(a, be, **kw)], be), ctx=gpu_ctx, lzw=True, float_predictor=True)
        _same(img, a, be, kw.get("planar", 1))
    with pytest.raises(NotImplementedError, match="Predictor 3"):
        tiff.read_tiff(T.write_tiff([L.lzw_float_page(f32, False)]), ctx=gpu_ctx, lzw=True)
    for bits in (1, 2, 4):
        w = 37
        rows = rng.integers(0, 256, size=(11, (w * bits + 7) // 8), dtype=np.uint8)
        img = tiff.read_tiff(T.write_tiff([L.lzw_page(rows, bits=bits, width=w, rows_per_strip=4)]), ctx=gpu_ctx, lzw=True)
        assert img.bits == bits and np.array_equal(img.data, rows)


def test_golden_files(gpu_ctx):
    from pure_zlib_amd import tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 5
    got = tiff.read_tiff_many(files, ctx=gpu_ctx, lzw=True)
    for f, g in zip(files, got):
        px = np.load(f[:-4] + ".npy")
        assert isinstance(g, list) and len(g) == 1, (f, g)
        assert g[0].data.reshape(px.shape).tobytes() == px.tobytes(), f
    assert tiff.main(["-t", "--lzw"] + files) == 0 and tiff.main(["-t"] + files) == 1


def test_without_the_keyword_an_lzw_page_is_not_read(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    blob = T.write_tiff([L.lzw_page(arrays["rgb8"], tile=(16, 16))])
    _same(tiff.read_tiff(blob, ctx=gpu_ctx, lzw=True), arrays["rgb8"], False)
    for call in (lambda: tiff.read_tiff(blob, ctx=gpu_ctx), lambda: tiff.read_tiff_region(blob, 0, 0, 0, 2, 2, ctx=gpu_ctx)):
        with pytest.raises(NotImplementedError, match=r"page 0: Compression 5 \(only Deflate, 8 and 32946, is read\)"):
            call()
    got = tiff.read_tiff_many([blob], ctx=gpu_ctx)
    assert isinstance(got[0], NotImplementedError) and "Compression 5" in str(got[0])


def test_a_batch_that_mixes_the_codecs_with_broken_files_among_good_ones(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    import pure_zlib_amd as P
    rng = np.random.default_rng(203)
    rgb8, g16 = arrays["rgb8"], arrays["gray16"]
    f32 = F.float_data(rng, (40, 50, 1), "f4")
    cut = lambda *ks: (lambda k, z: z[:len(z) // 2] if k in ks else z)  # noqa: E731
    bad_code = lambda k, z: L.pack([L.CLEAR, 1, 2, 400, 3]) if k == 2 else z  # noqa: E731
    old_style = lambda k, z: b"\x00\x01" + z if k == 1 else z  # noqa: E731
    ends_early = lambda k, z: L.encode(bytes(3 * 50 * 3)) if k == 1 else z  # noqa: E731  (three rows of a strip of seven, then EOI)
    blobs = [T.write_tiff([T.Page(rgb8, tile=(16, 16), predictor=2)]),                                # 0  Deflate, Predictor 2
             T.write_tiff([L.lzw_page(rgb8, tile=(16, 16), predictor=2)]),                            # 1  LZW, Predictor 2
             T.write_tiff([L.lzw_page(rgb8, tile=(16, 16), then=bad_code)]),                          # 2  a bad code in tile 2
             T.write_tiff([F.float_page(f32, False, tile=(32, 16))]),                                 # 3  Deflate, Predictor 3
             T.write_tiff([L.lzw_float_page(f32, True, rows_per_strip=7)], True),                     # 4  LZW, Predictor 3
             T.write_tiff([L.lzw_page(rgb8, rows_per_strip=7, then=cut(3))]),                         # 5  strip 3 cut in half
             T.write_tiff([L.lzw_page(g16, rows_per_strip=5, predictor=2), T.Page(rgb8, predictor=2)], True),  # 6  two pages, two codecs
             T.write_tiff([L.lzw_page(rgb8, rows_per_strip=7, then=old_style)]),                      # 7  old-style LZW
             T.write_tiff([L.lzw_page(rgb8, rows_per_strip=7, then=ends_early)]),                     # 8  strip 1 ends early with an EOI
             T.write_tiff([L.lzw_page(rgb8, rows_per_strip=7, enc=dict(eoi=False, leading_clear=False))])]  # 9  no Clear in front, no EOI: sound
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx, lzw=True, float_predictor=True)
    _same(got[0][0], rgb8, False)
    _same(got[1][0], rgb8, False)
    _same(got[3][0], f32, False)
    _same(got[4][0], f32, True)
    assert len(got[6]) == 2
    _same(got[6][0], g16, True)
    _same(got[6][1], rgb8, True)
    _same(got[9][0], rgb8, False)
    assert isinstance(got[2], P.DecompressionError) and str(got[2].message) == "#2: page 0, tile 2: LZW code 400 is not in the table after 2 bytes", got[2]
    assert got[2].status == 25 and got[2].detail == (400, 2)
    assert isinstance(got[5], P.DecompressionError) and "#5: page 0, strip 3: not enough image data" in str(got[5]), got[5]
    assert isinstance(got[7], NotImplementedError) and "page 0, strip 1: old-style LZW" in str(got[7]), got[7]
    assert isinstance(got[8], P.DecompressionError) and "#8: page 0, strip 1: not enough image data" in str(got[8]), got[8]
    assert [k for k, _why in tiff.test_tiff_many(blobs, ctx=gpu_ctx, lzw=True, float_predictor=True)] == [2, 5, 7, 8]


def test_device_out_with_a_fill_pattern_around_the_rows(gpu_ctx, arrays):
    import torch
    from pure_zlib_amd import tiff
    rgb8, g16 = arrays["rgb8"], arrays["gray16"]
    blobs = [T.write_tiff([L.lzw_page(rgb8, tile=(16, 16), predictor=2), T.Page(g16, rows_per_strip=7, predictor=2)]), b"not a tiff",
             T.write_tiff([L.lzw_page(rgb8, planar=2, rows_per_strip=4)], True)]
    shapes = [(rgb8, False, 1), (g16, False, 1), (rgb8, True, 2)]
    offs, strides, at = [], [], 3
    for k, (a, _be, planar) in enumerate(shapes):
        rb = a.shape[1] * (a.shape[2] if planar == 1 else 1) * a.dtype.itemsize
        offs.append(at)
        strides.append(rb + (5, 0, 3)[k])
        at += a.shape[0] * (1 if planar == 1 else a.shape[2]) * strides[-1] + (7, 1, 2)[k]
    t = torch.full((at + 9,), T.FILL, dtype=torch.uint8, device="cuda")
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides), lzw=True)
    assert [len(g) if isinstance(g, list) else type(g) for g in got] == [2, ValueError, 1] and all(i.data is None for g in (got[0], got[2]) for i in g)
    host = t.cpu().numpy()
    want = np.full(len(host), T.FILL, np.uint8)
    for (a, be, planar), o, s in zip(shapes, offs, strides):
        a = a if planar == 1 else np.moveaxis(a, 2, 0)
        rows = np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">" if be else "<")).view(np.uint8).reshape(a.shape[0] * (1 if planar == 1 else a.shape[1]), -1)
        for r in range(rows.shape[0]):
            want[o + r * s:o + r * s + rows.shape[1]] = rows[r]
    assert np.array_equal(host, want)


def test_regions(gpu_ctx):
    from pure_zlib_amd import tiff
    rng = np.random.default_rng(204)
    a = (np.cumsum(rng.integers(-3, 4, size=(70, 129, 3)), axis=1) % 256).astype(np.uint8)
    c = (np.cumsum(rng.integers(-3, 4, size=(70, 129, 3)), axis=1) % 65536).astype(np.uint16)
    files = [(T.write_tiff([L.lzw_page(a, tile=(16, 16), predictor=2)]), a, 1), (T.write_tiff([L.lzw_page(a, rows_per_strip=7)], True), a, 1),
             (T.write_tiff([L.lzw_page(c, tile=(32, 16), planar=2, predictor=2)], True, True), c, 2), (T.write_tiff([L.lzw_page(c, planar=2)]), c, 2)]
    rects = [(0, 0, 1, 1), (69, 128, 1, 1), (16, 16, 16, 16), (15, 15, 2, 2), (10, 30, 25, 40), (6, 0, 9, 129), (0, 0, 70, 129), (33, 47, 5, 3)]
    for blob, arr, planar in files:
        for y0, x0, rh, rw in rects:
            got = tiff.read_tiff_region(blob, 0, y0, x0, rh, rw, ctx=gpu_ctx, lzw=True)
            want = arr[y0:y0 + rh, x0:x0 + rw]
            want = want if planar == 1 else np.moveaxis(want, 2, 0)
            assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).astype(got.dtype).tobytes(), (planar, y0, x0, rh, rw)


# ---- the launches a call issues ------------------------------------------------------------------------------------------------------------
_LAUNCHES = {"decompress_many_device": ("decode", 11), "unlzw_many_device": ("unlzw", 9), "unpredict_many_device": ("unpredict", 6),
             "unshuffle_many_device": ("unshuffle", 6)}
SYNC = ("sync", None)


@pytest.fixture
def record(gpu_ctx, monkeypatch):
    """[(name, n)] of every launch and sync in order; every launch is asked not to wait."""
    calls = []
    cls = type(gpu_ctx)
    for method, (name, at) in _LAUNCHES.items():
        def wrapped(self, *a, _real=getattr(cls, method), _name=name, _at=at, **kw):
            calls.append((_name, a[_at]))
            assert kw.get("sync") is False
            return _real(self, *a, **kw)
        monkeypatch.setattr(cls, method, wrapped)
    real_sync = cls.sync
    monkeypatch.setattr(cls, "sync", lambda self: (calls.append(SYNC), real_sync(self))[1])
    return calls


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(205)
    u8 = rng.integers(0, 8, size=(7, 9, 3), dtype=np.uint8)
    f32 = F.float_data(rng, (7, 9, 1), "f4")
    return dict(u8=u8, f32=f32,
                deflate=T.write_tiff([T.Page(u8, rows_per_strip=3, predictor=2), T.Page(u8, tile=(8, 4))]),   # 3 + 4 jobs
                lzw=T.write_tiff([L.lzw_page(u8, rows_per_strip=3, predictor=2), L.lzw_page(u8, tile=(8, 4))]),  # 3 + 4
                flzw=T.write_tiff([L.lzw_float_page(f32, False, rows_per_strip=3)]),                            # 3
                fdeflate=T.write_tiff([F.float_page(f32, False, rows_per_strip=2)]))                            # 4


def test_the_launches_with_and_without_lzw_pages(gpu_ctx, record, small):
    from pure_zlib_amd import tiff
    u8, f32 = small["u8"], small["f32"]
    got = tiff.read_tiff_many([small["deflate"]], ctx=gpu_ctx, lzw=True)
    assert record == [("decode", 7), ("unpredict", 7), SYNC], record  # (what it issued before)
    _same(got[0][1], u8, False)
    del record[:]
    got = tiff.read_tiff_many([small["lzw"]], ctx=gpu_ctx, lzw=True)
    assert record == [("unlzw", 7), ("unpredict", 7), SYNC], record
    _same(got[0][0], u8, False)
    _same(got[0][1], u8, False)
    del record[:]
    got = tiff.read_tiff_many([small["lzw"], small["fdeflate"], small["deflate"], small["flzw"]], ctx=gpu_ctx, lzw=True, float_predictor=True)
    assert record == [("decode", 7), ("unlzw", 10), ("decode", 4), ("unpredict", 14), ("unshuffle", 7), SYNC], record
    for g, want in zip(got, ([u8, u8], [f32], [u8, u8], [f32])):
        assert isinstance(g, list) and len(g) == len(want), g
        for img, a in zip(g, want):
            _same(img, a, False)
    del record[:]
    got = tiff.read_tiff_region(small["lzw"], 1, 3, 3, 2, 6, ctx=gpu_ctx, lzw=True)
    assert record == [("unlzw", 4), ("unpredict", 4), SYNC], record
    assert got.tobytes() == u8[3:5, 3:9].tobytes()
