"""GPU: pure_zlib_amd/tiff.py with float_predictor=True against the arrays its Predictor 3 files were written from, bit for bit (NaN,
infinities and subnormals among them: the comparison is on bytes): the writer of tests/tiffcases.py through the hook of
tests/fpcases.py over its variants, the golden files PIL's libtiff wrote, batches that mix the three predictors with broken files
among good ones, device_out, regions, and the launches a call issues."""
import glob
import os

import numpy as np
import pytest

import fpcases as F
import tiffcases as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_float")


def _arrays():
    rng = np.random.default_rng(93)
    return {"f32": F.float_data(rng, (70, 129, 1), "f4"), "f16": F.float_data(rng, (33, 65, 1), "f2"), "f64": F.float_data(rng, (16, 33, 1), "f8"),
            "rgb32": F.float_data(rng, (40, 50, 3), "f4"), "rgba16": F.float_data(rng, (17, 31, 4), "f2"), "rgb64": F.float_data(rng, (31, 17, 3), "f8"),
            "five32": F.float_data(rng, (12, 19, 5), "f4")}


@pytest.fixture(scope="module")
def arrays():
    return _arrays()


def _same(img, a, be, planar=1):
    """The image holds the array's samples in the file's byte order, bit for bit."""
    want = a if planar == 1 else np.moveaxis(a, 2, 0)
    file_dt = a.dtype.newbyteorder(">" if be else "<")
    assert img.data.shape == want.shape and img.data.dtype == file_dt, (img.data.shape, img.data.dtype, want.shape, file_dt)
    assert img.data.tobytes() == np.ascontiguousarray(want).astype(file_dt).tobytes()


def test_read_tiff_many_over_the_writers_variants(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    files, wants = [], []
    i = 0
    for name, a in arrays.items():
        for layout in ({"tile": (16, 16)}, {"tile": (32, 16)}, {"rows_per_strip": 1}, {"rows_per_strip": 7}, {}):
            for planar in ((1, 2) if a.shape[2] > 1 else (1,)):
                if planar == 1 and a.shape[2] > 4:
                    continue
                be, big = bool(i & 1), bool(i & 2)
                page = F.float_page(a, be, planar=planar, compression=(8, 32946)[(i // 2) % 2], **layout)
                files.append(T.write_tiff([page], be, big, seed=i))
                wants.append((a, be, planar, name, layout))
                i += 1
    assert {(w[3], w[2]) for w in wants} >= {("rgb32", 2), ("five32", 2), ("rgba16", 1), ("f64", 1)}
    assert {(w[1], bool(k & 2)) for k, w in enumerate(wants)} == {(False, False), (True, False), (False, True), (True, True)}
    got = tiff.read_tiff_many(files, ctx=gpu_ctx, float_predictor=True)
    assert len(got) == len(files) > 45
    for g, (a, be, planar, name, layout) in zip(got, wants):
        assert isinstance(g, list) and len(g) == 1, (g, name, layout, planar)
        assert (g[0].width, g[0].height, g[0].samples, g[0].bits, g[0].planar, g[0].tiled, g[0].sample_format) == (
            a.shape[1], a.shape[0], a.shape[2], 8 * a.dtype.itemsize, planar, "tile" in layout, 3), (name, layout)
        _same(g[0], a, be, planar)
    assert any(np.isnan(g[0].data).any() and np.isinf(g[0].data).any() for g in got)
    assert tiff.test_tiff_many(files[:6], ctx=gpu_ctx, float_predictor=True) == []
    assert [k for k, _why in tiff.test_tiff_many(files[:6], ctx=gpu_ctx)] == list(range(6))


def test_golden_files(gpu_ctx):
    from pure_zlib_amd import tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 4
    got = tiff.read_tiff_many(files, ctx=gpu_ctx, float_predictor=True)
    for f, g in zip(files, got):
        px = np.load(f[:-4] + ".npy")
        assert isinstance(g, list) and len(g) == 1, (f, g)
        assert g[0].data.dtype == np.dtype("<f4") and g[0].data.reshape(px.shape).tobytes() == px.tobytes(), f
    assert tiff.main(["-t", "--float-predictor"] + files) == 0 and tiff.main(["-t"] + files) == 1


def test_without_the_keyword_a_float_page_is_not_read(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    blob = T.write_tiff([F.float_page(arrays["f32"], False, tile=(32, 16))])
    _same(tiff.read_tiff(blob, ctx=gpu_ctx, float_predictor=True), arrays["f32"], False)
    for call in (lambda: tiff.read_tiff(blob, ctx=gpu_ctx), lambda: tiff.read_tiff_region(blob, 0, 0, 0, 2, 2, ctx=gpu_ctx)):
        with pytest.raises(NotImplementedError, match=r"page 0: Predictor 3 \(the floating-point predictor\) is not read"):
            call()
    got = tiff.read_tiff_many([blob], ctx=gpu_ctx)
    assert isinstance(got[0], NotImplementedError) and "Predictor 3" in str(got[0])


def test_what_the_floating_point_predictor_does_not_take(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    rng = np.random.default_rng(94)
    u32 = rng.integers(0, 1 << 32, size=(9, 11, 1), dtype=np.uint32)
    u8 = rng.integers(0, 256, size=(9, 11, 1), dtype=np.uint8)
    for bad in (T.write_tiff([T.Page(u32, predictor=3)]), T.write_tiff([T.Page(u8, predictor=3, sample_format=3)]),
                T.write_tiff([T.Page(u32.view("i4"), predictor=3)], True)):
        with pytest.raises(ValueError, match=r"page 0: tag 317 \(Predictor\) 3 with tag 339 \(SampleFormat\)"):
            tiff.read_tiff(bad, ctx=gpu_ctx, float_predictor=True)
    with pytest.raises(NotImplementedError, match="Predictor 3 with 5 chunky samples"):
        tiff.read_tiff(T.write_tiff([T.Page(arrays["five32"], predictor=3)]), ctx=gpu_ctx, float_predictor=True)
    with pytest.raises(NotImplementedError, match="24 bits per sample"):
        tiff.read_tiff(T.write_tiff([T.Page(arrays["f32"][:4, :4], predictor=3, more_tags=((258, T.SHORT, (24,)),))]), ctx=gpu_ctx, float_predictor=True)


def _with_height(blob, height):
    """The classic little-endian file with ImageLength of its first IFD replaced."""
    b = bytearray(blob)
    ifd = int.from_bytes(b[4:8], "little")
    for k in range(int.from_bytes(b[ifd:ifd + 2], "little")):
        at = ifd + 2 + 12 * k
        if int.from_bytes(b[at:at + 2], "little") == 257:
            b[at + 8:at + 12] = height.to_bytes(4, "little")
            return bytes(b)
    raise AssertionError


def test_a_batch_that_mixes_the_predictors_with_broken_files_among_good_ones(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    import pure_zlib_amd as P
    rng = np.random.default_rng(95)
    f32, f16, rgb = arrays["f32"], arrays["f16"], arrays["rgb32"]
    u8 = rng.integers(0, 256, size=(37, 50, 3), dtype=np.uint8)
    u16 = rng.integers(0, 65536, size=(21, 33, 1), dtype=np.uint16)
    cut = lambda *ks: (lambda k, z: z[:len(z) // 2] if k in ks else z)  # noqa: E731
    blobs = [T.write_tiff([T.Page(u8, tile=(16, 16), predictor=2)]),                                  # 0  Predictor 2
             T.write_tiff([F.float_page(f32, False, tile=(32, 16))]),                                 # 1  Predictor 3
             T.write_tiff([F.float_page(f32, False, tile=(32, 16), then=cut(7, 11))]),                # 2  a corrupt Predictor 3 tile, and a later one
             T.write_tiff([T.Page(u16, rows_per_strip=7)], True),                                     # 3  Predictor 1
             _with_height(T.write_tiff([F.float_page(f16[:30], False, rows_per_strip=7)]), 33),       # 4  a short Predictor 3 strip
             T.write_tiff([F.float_page(rgb, True, rows_per_strip=5), T.Page(u8, predictor=2)], True),  # 5  two pages, both kinds
             # 6  its first error in file order is the float page's, which the launches take last
             T.write_tiff([F.float_page(f16, False, rows_per_strip=7, then=cut(2, 3)), T.Page(u8, rows_per_strip=9, predictor=2, edit=cut(0))]),
             T.write_tiff([F.float_page(rgb, False, planar=2, tile=(16, 16))], False, True)]          # 7  Predictor 3, planes
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx, float_predictor=True)
    _same(got[0][0], u8, False)
    _same(got[1][0], f32, False)
    _same(got[3][0], u16, True)
    assert len(got[5]) == 2
    _same(got[5][0], rgb, True)
    _same(got[5][1], u8, True)
    _same(got[7][0], rgb, False, 2)
    assert isinstance(got[2], P.DecompressionError) and str(got[2].message).startswith("#2: page 0, tile 7: ") and "Ran out of data" in str(got[2]), got[2]
    assert isinstance(got[4], P.DecompressionError) and "#4: page 0, strip 4: not enough image data" in str(got[4]), got[4]
    assert isinstance(got[6], P.DecompressionError) and str(got[6].message).startswith("#6: page 0, strip 2: "), got[6]
    assert [k for k, _why in tiff.test_tiff_many(blobs, ctx=gpu_ctx, float_predictor=True)] == [2, 4, 6]
    with pytest.raises(P.DecompressionError, match="tile 7"):
        tiff.read_tiff(blobs[2], ctx=gpu_ctx, float_predictor=True)


def test_device_out_with_a_fill_pattern_around_the_rows(gpu_ctx, arrays):
    import torch
    from pure_zlib_amd import tiff
    rng = np.random.default_rng(96)
    u8 = rng.integers(0, 256, size=(20, 31, 3), dtype=np.uint8)
    blobs = [T.write_tiff([F.float_page(arrays["f32"], False, tile=(32, 16)), T.Page(u8, rows_per_strip=7, predictor=2)]),
             b"not a tiff", T.write_tiff([F.float_page(arrays["rgba16"], True)], True), T.write_tiff([F.float_page(arrays["rgb64"], False, planar=2, rows_per_strip=4)])]
    shapes = [(arrays["f32"], False, 1), (u8, False, 1), (arrays["rgba16"], True, 1), (arrays["rgb64"], False, 2)]
    offs, strides, at = [], [], 3
    for k, (a, _be, planar) in enumerate(shapes):
        rb = a.shape[1] * (a.shape[2] if planar == 1 else 1) * a.dtype.itemsize
        offs.append(at)
        strides.append(rb + (5, 0, 1, 3)[k])
        at += a.shape[0] * (1 if planar == 1 else a.shape[2]) * strides[-1] + (7, 1, 12, 2)[k]
    t = torch.full((at + 9,), T.FILL, dtype=torch.uint8, device="cuda")
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides), float_predictor=True)
    assert [len(g) if isinstance(g, list) else type(g) for g in got] == [2, ValueError, 1, 1] and all(i.data is None for g in (got[0], got[2], got[3]) for i in g)
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
    rng = np.random.default_rng(97)
    a, c = F.float_data(rng, (70, 129, 3), "f4"), F.float_data(rng, (70, 129, 3), "f2")
    files = [(T.write_tiff([F.float_page(a, False, tile=(16, 16))]), a, 1), (T.write_tiff([F.float_page(a, True, rows_per_strip=7)], True), a, 1),
             (T.write_tiff([F.float_page(c, True, tile=(32, 16), planar=2)], True, True), c, 2), (T.write_tiff([F.float_page(c, False, planar=2)]), c, 2)]
    rects = [(0, 0, 1, 1), (69, 128, 1, 1), (16, 16, 16, 16), (15, 15, 2, 2), (10, 30, 25, 40), (6, 0, 9, 129), (0, 0, 70, 129), (33, 47, 5, 3)]
    for blob, arr, planar in files:
        for y0, x0, rh, rw in rects:
            got = tiff.read_tiff_region(blob, 0, y0, x0, rh, rw, ctx=gpu_ctx, float_predictor=True)
            want = arr[y0:y0 + rh, x0:x0 + rw]
            want = want if planar == 1 else np.moveaxis(want, 2, 0)
            assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).astype(got.dtype).tobytes(), (planar, y0, x0, rh, rw)


# ---- the launches a call issues (the recorder of tests/test_gpu_reader_launches.py, written anew) ------------------------------------------
_LAUNCHES = {"decompress_many_device": ("decode", 11), "unpredict_many_device": ("unpredict", 6), "unshuffle_many_device": ("unshuffle", 6)}
SYNC = ("sync", None)


@pytest.fixture
def record(gpu_ctx, monkeypatch):
    """(calls, syncs): [(name, n)] of every launch and sync in order, and the `sync` argument of every launch."""
    calls, syncs = [], []
    cls = type(gpu_ctx)
    for method, (name, at) in _LAUNCHES.items():
        def wrapped(self, *a, _real=getattr(cls, method), _name=name, _at=at, **kw):
            calls.append((_name, a[_at]))
            syncs.append(kw.get("sync", a[_at + 1] if len(a) > _at + 1 else True))
            return _real(self, *a, **kw)
        monkeypatch.setattr(cls, method, wrapped)
    real_sync = cls.sync
    monkeypatch.setattr(cls, "sync", lambda self: (calls.append(SYNC), real_sync(self))[1])
    return calls, syncs


def _issued(record, want):
    calls, syncs = record
    assert calls == want, calls
    assert syncs == [False] * (len(want) - 1), syncs
    del calls[:], syncs[:]


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(98)
    f32, rgb16, tiled = F.float_data(rng, (7, 9, 1), "f4"), F.float_data(rng, (9, 5, 3), "f2"), F.float_data(rng, (9, 9, 3), "f4")
    u8 = rng.integers(0, 256, size=(7, 9, 3), dtype=np.uint8)
    strips = T.write_tiff([F.float_page(f32, True, rows_per_strip=3), F.float_page(rgb16, True, rows_per_strip=4)], True)   # 3 + 3 jobs
    tiles = T.write_tiff([F.float_page(tiled, False, tile=(4, 4))])                                                          # 9
    ints = T.write_tiff([T.Page(u8, rows_per_strip=3, predictor=2), T.Page(u8, tile=(8, 4))])                                # 3 + 4
    return (strips, [f32, rgb16], True), (tiles, [tiled], False), (ints, [u8, u8], False)


def test_a_float_batch_is_a_decode_and_an_unshuffle(gpu_ctx, record, small):
    from pure_zlib_amd import tiff
    got = tiff.read_tiff_many([small[0][0], small[1][0]], ctx=gpu_ctx, float_predictor=True)
    _issued(record, [("decode", 15), ("unshuffle", 15), SYNC])
    for g, (_blob, arrays, be) in zip(got, small[:2]):
        assert isinstance(g, list) and len(g) == len(arrays), g
        for img, a in zip(g, arrays):
            _same(img, a, be)


def test_a_mixed_batch_is_a_decode_an_unpredict_and_an_unshuffle(gpu_ctx, record, small):
    from pure_zlib_amd import tiff
    got = tiff.read_tiff_many([small[1][0], small[2][0], small[0][0]], ctx=gpu_ctx, float_predictor=True)
    _issued(record, [("decode", 22), ("unpredict", 7), ("unshuffle", 15), SYNC])
    for g, (_blob, arrays, be) in zip(got, (small[1], small[2], small[0])):
        assert isinstance(g, list) and len(g) == len(arrays), g
        for img, a in zip(g, arrays):
            _same(img, a, be)
    # without float pages the keyword adds nothing
    got = tiff.read_tiff_many([small[2][0]], ctx=gpu_ctx, float_predictor=True)
    _issued(record, [("decode", 7), ("unpredict", 7), SYNC])
    _same(got[0][1], small[2][1][1], False)


def test_a_region_over_a_tile_corner_is_its_four_tiles(gpu_ctx, record, small):
    from pure_zlib_amd import tiff
    blob, (a,), _be = small[1]
    got = tiff.read_tiff_region(blob, 0, 3, 3, 2, 2, ctx=gpu_ctx, float_predictor=True)
    _issued(record, [("decode", 4), ("unshuffle", 4), SYNC])
    assert got.shape == (2, 2, 3) and got.tobytes() == a[3:5, 3:5].tobytes()
