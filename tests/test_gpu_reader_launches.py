"""GPU: the launch sequence of the image readers as a whole.  Every *_many_device method the readers of pure_zlib_amd/png.py and
pure_zlib_amd/tiff.py call, and Context.sync, is wrapped on the context's class with a recorder; a call must issue exactly the list
of (launch, jobs) stated here, every launch with sync=False and one sync behind the last -- and deliver what the references of
pngcases.py, adam7cases.py, expandcases.py and tiffcases.py give.  Images of at most 9 x 9 pixels: the order and the job counts
depend on which kinds of image a batch holds, not on their size."""
import zlib

import numpy as np
import pytest

import adam7cases as A
import expandcases as X
import pngcases as PC
import tiffcases as T

pytestmark = pytest.mark.gpu

# method -> (its name in the record, where n stands among its positional arguments)
_LAUNCHES = {"decompress_many_device": ("decode", 11), "unfilter_many_device": ("unfilter", 11), "adam7_many_device": ("adam7", 10),
             "expand_many_device": ("expand", 6), "unpredict_many_device": ("unpredict", 6)}
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


# ---- PNG ---------------------------------------------------------------------------------------------------------------------------
PLTE = bytes([10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120])
TRNS = bytes([0, 128])
# (width, height, colour type, depth, interlaced): three plain images, two interlaced ones; the last is a palette image with tRNS
SPECS = ((1, 1, 0, 8, False), (5, 3, 2, 8, False), (9, 2, 0, 1, False), (1, 1, 0, 8, True), (9, 9, 3, 2, True))
PASSES = sum(1 for w, h, ct, d, laced in SPECS if laced for pw, _ph, _prb in A.pass_sizes(w, h, PC.CHANNELS[ct] * d) if pw)


def _rows(rng, w, h, ct, depth):
    rb, _ = PC.geometry(w, ct, depth)
    raw = rng.integers(0, 256, size=(h, rb), dtype=np.uint8)
    if depth < 8 and (w * depth) % 8:
        raw[:, -1] &= (0xff << (8 - (w * depth) % 8)) & 0xff  # (the padding bits of a packed row)
    return raw


def _write(spec, raw, filters, **kw):
    w, h, ct, depth, laced = spec
    extra = dict(palette=PLTE, trns=TRNS) if ct == 3 else {}
    return (A.write_png if laced else PC.write_png)(w, h, ct, depth, raw, filters, **extra, **kw)


def _reference_rows(blob, spec) -> bytes:
    """The image's rows by the reference unfilter and, for an interlaced file, the reference weave, from the file itself."""
    from pure_zlib_amd import png
    w, h, ct, depth, laced = spec
    stream = zlib.decompress(png._parse("", blob, True)[1])
    (rb, bpp), bits = PC.geometry(w, ct, depth), PC.CHANNELS[ct] * depth
    if not laced:
        return b"".join(PC.unfilter(stream, rb, h, bpp))
    dense, at = b"", 0
    for pw, ph, prb in A.pass_sizes(w, h, bits):
        if pw:
            dense += b"".join(PC.unfilter(stream[at:at + ph * (1 + prb)], prb, ph, bpp))
            at += ph * (1 + prb)
    assert at == len(stream)
    return A.weave(dense, w, h, bits).tobytes()


def _reference_rgba(raw, spec) -> np.ndarray:
    w, h, ct, depth, _laced = spec
    pal = None
    if ct == 3:
        pal = np.full((len(PLTE) // 3, 4), 255, np.uint8)
        pal[:, :3] = np.frombuffer(PLTE, np.uint8).reshape(-1, 3)
        pal[:len(TRNS), 3] = np.frombuffer(TRNS, np.uint8)
    return X.expand_reference(w, h, ct, depth, raw, X.RGBA8, pal, None)


@pytest.fixture(scope="module")
def images():
    """[(spec, rows, blob, the rows the references give)] of SPECS, computed once."""
    rng = np.random.default_rng(61)
    out = []
    for spec in SPECS:
        raw = _rows(rng, *spec[:4])
        blob = _write(spec, raw, (lambda ph: rng.integers(0, 5, size=ph)) if spec[4] else rng.integers(0, 5, size=spec[1]))
        want = _reference_rows(blob, spec)
        assert want == raw.tobytes(), spec  # the writers and the references agree
        out.append((spec, raw, blob, want))
    return out


def _same(got, images):
    from pure_zlib_amd import png
    for g, (spec, _raw, _blob, want) in zip(got, images):
        assert isinstance(g, png.PngImage) and (g.width, g.height, g.color_type, g.bit_depth) == spec[:4], (g, spec)
        assert g.expanded is None and g.data.tobytes() == want, spec


MIXED = [("decode", 5), ("unfilter", 5), ("unfilter", PASSES), ("adam7", 2), SYNC]


def test_the_passes_of_the_interlaced_images(images):
    from pure_zlib_amd import png
    assert PASSES == 1 + 7 == sum(len(png._passes(png._parse("", blob, True)[0])) for spec, _r, blob, _w in images if spec[4])


def test_plain_images_are_a_decode_and_an_unfilter(gpu_ctx, record, images):
    from pure_zlib_amd import png
    got = png.read_png_many([i[2] for i in images[:3]], ctx=gpu_ctx)
    _issued(record, [("decode", 3), ("unfilter", 3), SYNC])
    _same(got, images[:3])
    got = png.read_png_many([i[2] for i in images[:3]], ctx=gpu_ctx, adam7=True)  # (adam7 alone adds nothing)
    _issued(record, [("decode", 3), ("unfilter", 3), SYNC])
    _same(got, images[:3])


def test_a_mixed_batch_adds_the_pass_jobs_and_the_weave(gpu_ctx, record, images):
    from pure_zlib_amd import png
    got = png.read_png_many([i[2] for i in images], ctx=gpu_ctx, adam7=True)
    _issued(record, MIXED)
    _same(got, images)


def test_interlaced_images_alone_skip_the_first_unfilter(gpu_ctx, record, images):
    from pure_zlib_amd import png
    got = png.read_png_many([i[2] for i in images[3:]], ctx=gpu_ctx, adam7=True)
    _issued(record, [("decode", 2), ("unfilter", PASSES), ("adam7", 2), SYNC])
    _same(got, images[3:])


def test_expansion_is_one_more_launch_before_the_sync(gpu_ctx, record, images):
    from pure_zlib_amd import png
    got = png.read_png_many([i[2] for i in images], ctx=gpu_ctx, adam7=True, expand="rgba8")
    _issued(record, MIXED[:-1] + [("expand", 5), SYNC])
    for g, (spec, raw, _blob, _want) in zip(got, images):
        assert isinstance(g, png.PngImage) and g.expanded == "rgba8", (g, spec)
        assert np.array_equal(g.data, _reference_rgba(raw, spec)), spec
    assert (got[4].data[..., 3] != 255).any()  # the palette's tRNS reached the pixels


def test_a_bad_blob_and_a_cut_stream_in_the_middle(gpu_ctx, record, images):
    """The unparsable blob is in no launch; the image whose stream lacks its last byte is in all of them and an error of its own."""
    from pure_zlib_amd import png
    import pure_zlib_amd as P
    spec, raw = images[1][0], images[1][1]
    cut = _write(spec, raw, 2, stream_edit=lambda s: ("z", lambda z: z[:-1]))
    blobs = [i[2] for i in images]
    blobs[2:2] = [b"not a png", cut]
    got = png.read_png_many(blobs, ctx=gpu_ctx, adam7=True)
    _issued(record, [("decode", 6), ("unfilter", 6), ("unfilter", PASSES), ("adam7", 2), SYNC])
    assert isinstance(got[2], ValueError) and not isinstance(got[2], P.DecompressionError) and "#2: not a PNG file" in str(got[2]), got[2]
    assert isinstance(got[3], P.DecompressionError) and "#3: " in str(got[3]), got[3]
    _same(got[:2] + got[4:], images)


def test_device_out_issues_the_same_and_leaves_the_gaps_alone(gpu_ctx, record, images):
    import torch
    from pure_zlib_amd import png
    offs, strides, at = [], [], 3
    for k, (spec, raw, _blob, _want) in enumerate(images):
        offs.append(at)
        strides.append(raw.shape[1] + (0, 5, 0, 1, 2)[k])
        at += spec[1] * strides[-1] + (1, 7, 12, 0, 3)[k]
    t = torch.full((at + 9,), PC.FILL, dtype=torch.uint8, device="cuda")
    got = png.read_png_many([i[2] for i in images], ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides), adam7=True)
    _issued(record, MIXED)
    assert all(isinstance(g, png.PngImage) and g.data is None for g in got), got
    want = np.full(at + 9, PC.FILL, np.uint8)
    for (spec, raw, _blob, rows), o, s in zip(images, offs, strides):
        rows = np.frombuffer(rows, np.uint8).reshape(raw.shape)
        for r in range(spec[1]):
            want[o + r * s:o + r * s + raw.shape[1]] = rows[r]
    assert np.array_equal(t.cpu().numpy(), want)


# ---- TIFF --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiffs():
    rng = np.random.default_rng(62)
    full = lambda shape, dt: rng.integers(0, 256, size=shape + (np.dtype(dt).itemsize,), dtype=np.uint8).view(dt).reshape(shape)  # noqa: E731
    rgb8, gray16, tiled = full((7, 9, 3), "u1"), full((9, 5, 1), "u2"), full((9, 9, 3), "u1")
    strips = T.write_tiff([T.Page(rgb8, rows_per_strip=3, predictor=2), T.Page(gray16, rows_per_strip=4, predictor=2)], True)
    tiles = T.write_tiff([T.Page(tiled, tile=(4, 4), predictor=2)])
    return (strips, [rgb8, gray16], True), (tiles, [tiled], False)


def _same_tiff(img, a, be):
    file_dt = a.dtype.newbyteorder(">" if be else "<")
    assert img.data.shape == a.shape and img.data.dtype == file_dt and img.data.tobytes() == a.astype(file_dt).tobytes()


def test_tiff_strips_and_tiles_are_one_decode_and_one_unpredict(gpu_ctx, record, tiffs):
    from pure_zlib_amd import tiff
    jobs = sum(len(pg.offsets) for blob, _a, _be in tiffs for pg in tiff.parse_tiff(blob))
    assert jobs == 3 + 3 + 9
    got = tiff.read_tiff_many([blob for blob, _a, _be in tiffs], ctx=gpu_ctx)
    _issued(record, [("decode", jobs), ("unpredict", jobs), SYNC])
    for g, (_blob, arrays, be) in zip(got, tiffs):
        assert isinstance(g, list) and len(g) == len(arrays), g
        for img, a in zip(g, arrays):
            _same_tiff(img, a, be)


def test_a_region_over_a_tile_corner_is_its_four_tiles(gpu_ctx, record, tiffs):
    from pure_zlib_amd import tiff
    blob, (a,), _be = tiffs[1]
    got = tiff.read_tiff_region(blob, 0, 3, 3, 2, 2, ctx=gpu_ctx)
    _issued(record, [("decode", 4), ("unpredict", 4), SYNC])
    assert got.shape == (2, 2, 3) and got.tobytes() == a[3:5, 3:5].tobytes()
