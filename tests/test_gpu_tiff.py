"""GPU: pure_zlib_amd/tiff.py against the arrays its files were written from, bit for bit: the writer of tests/tiffcases.py over its
variants, the golden files PIL's libtiff wrote, batches with broken files among good ones, several pages, device_out, regions, and
the count of launches a call issues."""
import glob
import os

import numpy as np
import pytest

import tiffcases as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")


def _arrays():
    rng = np.random.default_rng(91)
    full = lambda shape, dt: rng.integers(0, 256, size=shape + (np.dtype(dt).itemsize,), dtype=np.uint8).view(dt).reshape(shape)  # noqa: E731
    return {"rgb8": full((70, 129, 3), "u1"), "gray16": full((33, 65, 1), "u2"), "rgba8": full((17, 31, 4), "u1"), "gray32": full((20, 40, 1), "u4"),
            "rgb16": full((40, 50, 3), "u2"), "ga64": full((9, 21, 2), "u8"), "f32": full((16, 33, 1), "u4").view("f4"), "i16x3": full((31, 17, 3), "i2"),
            "five8": full((12, 19, 5), "u1")}


@pytest.fixture(scope="module")
def arrays():
    return _arrays()


def _same(img, a, be, planar=1):
    """The image holds the array's samples in the file's byte order, bit for bit (NaNs of a float image included)."""
    want = a if planar == 1 else np.moveaxis(a, 2, 0)
    file_dt = a.dtype.newbyteorder(">" if be else "<")
    assert img.data.shape == want.shape and img.data.dtype == file_dt, (img.data.shape, img.data.dtype, want.shape, file_dt)
    assert img.data.tobytes() == want.astype(file_dt).tobytes()


def test_read_tiff_many_over_the_writers_variants(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    files, wants = [], []
    i = 0
    for name, a in arrays.items():
        for layout in ({"tile": (16, 16)}, {"tile": (32, 16)}, {"rows_per_strip": 1}, {"rows_per_strip": 7}, {}):
            for predictor in (1, 2):
                if predictor == 2 and a.shape[2] > 4:
                    continue
                be, big, planar = bool(i & 1), bool(i & 2), 2 if (i // 3) % 3 == 0 and a.shape[2] > 1 else 1
                page = T.Page(a, predictor=predictor, planar=planar, compression=(8, 32946)[(i // 2) % 2], **layout)
                files.append(T.write_tiff([page], be, big, seed=i))
                wants.append((a, be, planar, name, layout, predictor))
                i += 1
    # five chunky samples with Predictor 2 are not read, as a separate plane each they are
    files.append(T.write_tiff([T.Page(arrays["five8"], predictor=2, planar=2, tile=(16, 16))]))
    wants.append((arrays["five8"], False, 2, "five8", "planar tiles", 2))
    got = tiff.read_tiff_many(files, ctx=gpu_ctx)
    assert len(got) == len(files) > 80
    for g, (a, be, planar, name, layout, predictor) in zip(got, wants):
        assert isinstance(g, list) and len(g) == 1, (g, name, layout, predictor)
        assert (g[0].width, g[0].height, g[0].samples, g[0].bits, g[0].planar, g[0].tiled) == (a.shape[1], a.shape[0], a.shape[2], 8 * a.dtype.itemsize, planar,
                                                                                          isinstance(layout, str) or "tile" in layout)
        _same(g[0], a, be, planar)
    assert got[0][0].sample_format == 1 and [g[0].sample_format for g, w in zip(got, wants) if w[3] == "f32"][0] == 3


def test_packed_rows_below_eight_bits(gpu_ctx):
    from pure_zlib_amd import tiff
    rng = np.random.default_rng(92)
    files, wants = [], []
    for bits, w in ((1, 129), (2, 67), (4, 33)):
        rb = (w * bits + 7) // 8
        rows = rng.integers(0, 256, size=(21, rb), dtype=np.uint8)
        for layout in ({"rows_per_strip": 7}, {"tile": (32, 16)}, {}):
            files.append(T.write_tiff([T.Page(rows, bits=bits, width=w, **layout)], bits == 2))
            wants.append(rows)
    got = tiff.read_tiff_many(files, ctx=gpu_ctx)
    for g, rows in zip(got, wants):
        assert isinstance(g, list) and g[0].data.dtype == np.uint8 and np.array_equal(g[0].data, rows), g


def test_golden_files(gpu_ctx):
    from pure_zlib_amd import tiff
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))
    assert len(files) == 4
    got = tiff.read_tiff_many(files, ctx=gpu_ctx)
    for f, g in zip(files, got):
        px = np.load(f[:-4] + ".npy")
        assert isinstance(g, list) and len(g) == 1, (f, g)
        assert np.array_equal(g[0].data.reshape(px.shape), px), f
    assert tiff.test_tiff_many(files, ctx=gpu_ctx) == []


def test_a_batch_with_broken_files_among_good_ones(gpu_ctx, arrays, tmp_path):
    from pure_zlib_amd import tiff
    import pure_zlib_amd as P
    a, g16 = arrays["rgb8"], arrays["gray16"]
    good = [T.write_tiff([T.Page(a, tile=(32, 16), predictor=2)]), T.write_tiff([T.Page(g16, rows_per_strip=7, predictor=2)], True),
            T.write_tiff([T.Page(arrays["rgba8"], predictor=2)], False, True)]
    corrupt = T.write_tiff([T.Page(a, tile=(32, 16), predictor=2, edit=lambda k, z: z[:len(z) // 2] if k == 7 else z)])
    short = T.write_tiff([T.Page(g16[:30], rows_per_strip=7, predictor=2)])
    short = _with_height(short, 33)  # the last strip now has five rows in the IFD and two in its stream
    long_ = _with_height(T.write_tiff([T.Page(g16[:33], rows_per_strip=7, predictor=2)]), 30)
    lzw = T.write_tiff([T.Page(a, compression=5)])
    floatp = T.write_tiff([T.Page(arrays["f32"], predictor=3)])
    broken_ifd = good[0][:len(good[0]) - 40]
    path = tmp_path / "not_there.tif"
    blobs = [good[0], corrupt, good[1], short, lzw, good[2], broken_ifd, long_, floatp, str(path)]
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx)
    for k, (arr, be) in {0: (a, False), 2: (g16, True), 5: (arrays["rgba8"], False)}.items():
        assert isinstance(got[k], list), got[k]
        _same(got[k][0], arr, be)
    assert isinstance(got[1], P.DecompressionError) and str(got[1].message).startswith("#1: page 0, tile 7: ") and "Ran out of data" in str(got[1]), got[1]
    assert isinstance(got[3], P.DecompressionError) and "#3: page 0, strip 4: not enough image data" in str(got[3]), got[3]
    assert isinstance(got[4], NotImplementedError) and "#4: page 0: Compression 5" in str(got[4])
    assert isinstance(got[6], ValueError) and not isinstance(got[6], P.DecompressionError) and "#6: page 0" in str(got[6]), got[6]
    assert isinstance(got[7], P.DecompressionError) and "#7: page 0, strip 4: too much image data" in str(got[7]), got[7]
    assert isinstance(got[8], NotImplementedError) and "Predictor 3" in str(got[8])
    assert isinstance(got[9], OSError)
    listed = tiff.test_tiff_many(blobs, ctx=gpu_ctx)
    assert [k for k, _why in listed] == [1, 3, 4, 6, 7, 8, str(path)]
    with pytest.raises(P.DecompressionError, match="tile 7"):
        tiff.read_tiff(corrupt, ctx=gpu_ctx)
    for bad, what in ((T.write_tiff([T.Page(a, fill_order=2)]), "FillOrder"), (T.write_tiff([T.Page(arrays["five8"], predictor=2)]), "chunky samples"),
                      (T.write_tiff([T.Page(a, photometric=6, subsampling=(2, 2))]), "subsampling"),
                      (T.write_tiff([T.Page(a, more_tags=((258, T.SHORT, (8, 8, 5)),))]), "unequal")):
        with pytest.raises(NotImplementedError, match=what):
            tiff.read_tiff(bad, ctx=gpu_ctx)


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


def test_pages_of_one_file_and_of_many(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    order = ["rgb8", "gray16", "rgb16", "ga64"]
    pages = [T.Page(arrays[n], predictor=2, **lay) for n, lay in zip(order, ({"tile": (16, 16)}, {"rows_per_strip": 7}, {"tile": (32, 16), "planar": 2}, {}))]
    for be, big in ((False, False), (True, True)):
        blob = T.write_tiff(pages, be, big)
        got = tiff.read_tiff_many([blob, T.write_tiff(pages[1:2], be)], ctx=gpu_ctx)
        assert [len(g) for g in got] == [4, 1]
        for img, n, pg in zip(got[0], order, pages):
            _same(img, arrays[n], be, pg.planar)
        _same(got[1][0], arrays["gray16"], be)
        _same(tiff.read_tiff(blob, page=2, ctx=gpu_ctx), arrays["rgb16"], be, 2)
    with pytest.raises(ValueError, match="page 4"):
        tiff.read_tiff(blob, page=4, ctx=gpu_ctx)


def test_device_out_with_a_fill_pattern_around_the_rows(gpu_ctx, arrays):
    import torch
    from pure_zlib_amd import tiff
    blobs = [T.write_tiff([T.Page(arrays["rgb8"], tile=(32, 16), predictor=2), T.Page(arrays["gray16"], rows_per_strip=7, predictor=2)]),
             b"not a tiff", T.write_tiff([T.Page(arrays["rgba8"], predictor=2)], True)]
    shapes = [arrays["rgb8"], arrays["gray16"], arrays["rgba8"]]
    offs, strides, at = [], [], 3
    for k, a in enumerate(shapes):
        rb = a.shape[1] * a.shape[2] * a.dtype.itemsize
        offs.append(at)
        strides.append(rb + (5, 0, 1)[k])
        at += a.shape[0] * strides[-1] + (7, 1, 12)[k]
    t = torch.full((at + 9,), T.FILL, dtype=torch.uint8, device="cuda")
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides))
    assert [len(g) if isinstance(g, list) else type(g) for g in got] == [2, ValueError, 1] and all(i.data is None for g in (got[0], got[2]) for i in g)
    host = t.cpu().numpy()
    want = np.full(len(host), T.FILL, np.uint8)
    for k, (a, o, s) in enumerate(zip(shapes, offs, strides)):
        rows = a.astype(a.dtype.newbyteorder(">" if k == 2 else "<")).view(np.uint8).reshape(a.shape[0], -1)
        for r in range(a.shape[0]):
            want[o + r * s:o + r * s + rows.shape[1]] = rows[r]
    assert np.array_equal(host, want)


def test_regions(gpu_ctx, arrays):
    from pure_zlib_amd import tiff
    a, c = arrays["rgb8"], arrays["rgb16"]
    files = [(T.write_tiff([T.Page(a, tile=(16, 16), predictor=2)]), a, 1), (T.write_tiff([T.Page(a, rows_per_strip=7, predictor=2)], True), a, 1),
             (T.write_tiff([T.Page(c, tile=(32, 16), predictor=2, planar=2)], True, True), c, 2), (T.write_tiff([T.Page(c, predictor=1)]), c, 1)]
    rects = [(0, 0, 1, 1), (69, 128, 1, 1), (16, 16, 16, 16), (15, 15, 2, 2), (10, 30, 25, 40), (6, 0, 9, 129), (0, 0, 70, 129), (33, 47, 5, 3)]
    for blob, arr, planar in files:
        h, w = arr.shape[:2]
        for y0, x0, rh, rw in rects:
            y0, x0 = min(y0, h - 1), min(x0, w - 1)
            rh, rw = min(rh, h - y0), min(rw, w - x0)
            got = tiff.read_tiff_region(blob, 0, y0, x0, rh, rw, ctx=gpu_ctx)
            want = arr[y0:y0 + rh, x0:x0 + rw]
            want = want if planar == 1 else np.moveaxis(want, 2, 0)
            assert got.shape == want.shape and got.tobytes() == want.astype(got.dtype).tobytes(), (planar, y0, x0, rh, rw)
    whole = tiff.read_tiff(files[0][0], ctx=gpu_ctx).data
    assert np.array_equal(tiff.read_tiff_region(files[0][0], 0, 5, 7, 40, 100, ctx=gpu_ctx), whole[5:45, 7:107])
    for bad in ((0, 0, 71, 1), (0, 129, 1, 1), (-1, 0, 2, 2), (0, 0, 0, 5), (69, 128, 1, 2)):
        with pytest.raises(ValueError, match="outside the image"):
            tiff.read_tiff_region(files[0][0], 0, *bad, ctx=gpu_ctx)


def test_one_decode_and_one_unpredict_launch_however_many_files(gpu_ctx, arrays, monkeypatch):
    from pure_zlib_amd import tiff
    calls = []
    cls = type(gpu_ctx)
    real_d, real_u = cls.decompress_many_device, cls.unpredict_many_device
    monkeypatch.setattr(cls, "decompress_many_device", lambda self, *a, **kw: (calls.append(("decode", a[11])), real_d(self, *a, **kw))[1])
    monkeypatch.setattr(cls, "unpredict_many_device", lambda self, *a, **kw: (calls.append(("unpredict", a[6])), real_u(self, *a, **kw))[1])
    blobs = [T.write_tiff([T.Page(arrays["rgb8"], tile=(16, 16), predictor=2), T.Page(arrays["gray16"], rows_per_strip=7)], seed=k) for k in range(5)]
    got = tiff.read_tiff_many(blobs, ctx=gpu_ctx)
    assert all(isinstance(g, list) and len(g) == 2 for g in got)
    jobs = 5 * (5 * 9 + 5)
    assert calls == [("decode", jobs), ("unpredict", jobs)]
    assert gpu_ctx.last_kernel_ms() > 0.0
    del calls[:]
    tiff.read_tiff_region(blobs[0], 0, 16, 16, 16, 16, ctx=gpu_ctx)
    assert calls == [("decode", 1), ("unpredict", 1)]  # the one tile that covers the rectangle
