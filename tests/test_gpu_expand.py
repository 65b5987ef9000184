"""GPU: pzg_expand_many and the expand= path of pure_zlib_amd/png.py against the numpy reference of tests/expandcases.py, byte for
byte: the cases the CPU model runs (tests/test_model_expand.py), laid out with the sources at every misalignment, the destinations
off the 16-byte boundaries and padded strides over a 0xCD prefill that is checked everywhere nothing is delivered."""
import zlib

import numpy as np
import pytest

import adam7cases as A
import expandcases as X
import pngcases as PC

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(torch.device("cuda", 0))


def run_host(ctx, b):
    dst = np.full(len(b.dst_want), X.FILL, np.uint8)
    status, detail = ctx.expand_many(b.src, dst, b.palette, b.desc)
    return dst, status, detail


def run_device(ctx, b, sync=True):
    import torch
    n = len(b.cases)
    t = [_up(a) for a in (b.src, b.palette, b.desc)]
    d_dst = torch.full((len(b.dst_want),), X.FILL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.expand_many_device(t[0].data_ptr(), d_dst.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), n, sync=sync)
    if not sync:
        ctx.sync()
    return d_dst.cpu().numpy(), d_status.cpu().numpy(), d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)


def check(b, got):
    dst, status, detail = got
    for i, c in enumerate(b.cases):
        assert (int(status[i]), int(detail[i, 0]), int(detail[i, 1])) == (c.status, c.d0, c.d1), c.name
    assert X.first_difference(dst, b) is None, X.first_difference(dst, b)


def test_every_case_on_device_pointers(gpu_ctx):
    """Every type, format, width, key and palette; the bad indices, the empty images and the illegal geometries among good neighbours;
    in one launch, and again with every image at another layout."""
    cases = X.all_cases()
    assert len(cases) == 1304
    for shift in (0, 5):
        b = X.batch(cases, shift)
        check(b, run_device(gpu_ctx, b))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_both_pointer_forms_give_the_same(gpu_ctx):
    """The host-pointer form refuses illegal geometry with its return value (test_bad_arguments): here it gets everything else."""
    cases = X.shape_cases()[::5] + X.special_cases() + X.bad_index_cases() + X.empty_cases()
    b = X.batch(cases, 1)
    host, device = run_host(gpu_ctx, b), run_device(gpu_ctx, b, sync=False)
    check(b, host)
    check(b, device)
    assert np.array_equal(host[1], device[1]) and np.array_equal(host[2], device[2])
    assert np.array_equal(host[0][~b.loose], device[0][~b.loose])
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_a_batch_of_one_image_and_a_bad_index_alone(gpu_ctx):
    for c in (X.shape_cases()[700], X.bad_index_cases()[2], X.empty_cases()[0]):
        b = X.batch([c], 3)
        check(b, run_device(gpu_ctx, b))
        check(b, run_host(gpu_ctx, b))


def test_bad_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    good = [X.shape_cases()[3], X.shape_cases()[900], X.shape_cases()[500]]
    L, h = _ffi.lib(), gpu_ctx.handle
    b = X.batch(good)
    dst = np.full(len(b.dst_want), X.FILL, np.uint8)
    status, detail = np.zeros(3, np.int32), np.zeros(6, np.uint32)

    def call(bb=b, n=3, flags=0, desc=True, pal=True):
        return L.pzg_expand_many(h, bb.src.ctypes.data, dst.ctypes.data, bb.palette.ctypes.data if pal else None, bb.desc.ctypes.data if desc else None,
                                 status.ctypes.data, detail.ctypes.data, n, flags)
    assert call(n=0) == _ffi.RC_BAD_ARG and call(flags=_ffi.GZIP) == _ffi.RC_BAD_ARG and call(flags=_ffi.ASYNC) == _ffi.RC_BAD_ARG
    assert call(desc=False) == _ffi.RC_BAD_ARG
    for bad in X.bad_geometry_cases():  # every illegal geometry, between two good images
        assert call(bb=X.batch([good[0], bad, good[2]])) == _ffi.RC_BAD_ARG, bad.name
    pal_image = next(c for c in X.shape_cases() if c.ct == 3)
    assert call(bb=X.batch([good[0], pal_image, good[2]]), pal=False) == _ffi.RC_BAD_ARG  # a palette image and no palette
    assert (dst == X.FILL).all()
    assert all(c.ct != 3 for c in good) and call(pal=False) == _ffi.RC_OK  # no palette image: palette_base may be null
    assert X.first_difference(dst, b) is None and (status == 0).all() and (detail == 0).all()


# ---- the chains ------------------------------------------------------------------------------------------------------------------------
def _chain_cases():
    pick = [c for c in X.shape_cases() if c.width in (5, 33, 65) and c.fmt == X.RGBA8][::3] + [c for c in X.shape_cases() if c.width == 17 and c.fmt == X.RGB8][::4]
    return pick + X.bad_index_cases()[2:4]


def test_async_chain_decode_unfilter_expand(gpu_ctx):
    """decompress_many_device, unfilter_many_device, expand_many_device, one sync: what the three synchronous calls give, and what
    the reference gives."""
    import torch
    rng = np.random.default_rng(41)
    cases = _chain_cases()
    b = X.batch(cases)  # (the rows are not taken from b.src: the unfilter delivers them where b.src has them, at b.desc's strides)
    n = len(cases)
    streams = [PC.filter_stream(c.rows, max(1, X.CHANNELS[c.ct] * c.depth // 8), rng.integers(0, 5, size=c.height)) for c in cases]
    zs = [zlib.compress(s, 6) for s in streams]
    pad = lambda a: (a + np.uint64(15)) & ~np.uint64(15)  # noqa: E731
    in_len, cap = np.array([len(z) for z in zs], np.uint64), np.array([len(s) for s in streams], np.uint64)
    in_off, dec_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    in_off[1:], dec_off[1:] = np.cumsum(pad(in_len))[:-1], np.cumsum(pad(cap + np.uint64(4)))[:-1]
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    t = [_up(a) for a in (h_in, in_off, in_len, dec_off, cap, b.desc["src_off"], b.desc["src_stride"], np.array([c.srb for c in cases], np.uint32),
                          np.array([c.height for c in cases], np.uint32), np.array([max(1, X.CHANNELS[c.ct] * c.depth // 8) for c in cases], np.uint8),
                          b.palette, b.desc)]
    p = [x.data_ptr() for x in t]
    results = []
    for sync in (False, True):
        d_dec = torch.full((int(dec_off[-1] + cap[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        d_file = torch.full((len(b.src),), 0xEE, dtype=torch.uint8, device="cuda")
        d_dst = torch.full((len(b.dst_want),), X.FILL, dtype=torch.uint8, device="cuda")
        d_out_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_st = torch.full((3 * n,), -1, dtype=torch.int32, device="cuda")  # the decode's, the unfilter's, the expansion's
        d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.decompress_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_out_len.data_ptr(), d_st.data_ptr(), 0, 0, 0, n, sync=sync)
        gpu_ctx.unfilter_many_device(d_dec.data_ptr(), p[3], d_out_len.data_ptr(), d_file.data_ptr(), p[5], p[6], p[7], p[8], p[9], d_st.data_ptr() + 4 * n,
                                     0, n, sync=sync)
        gpu_ctx.expand_many_device(d_file.data_ptr(), d_dst.data_ptr(), p[10], p[11], d_st.data_ptr() + 8 * n, d_detail.data_ptr(), n, sync=sync)
        if not sync:
            gpu_ctx.sync()
        st = d_st.cpu().numpy()
        assert (st[:2 * n] == 0).all() and np.array_equal(d_out_len.cpu().numpy().view(np.uint64), cap)
        results.append((d_dst.cpu().numpy(), st[2 * n:], d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)))
    check(b, results[0])
    check(b, results[1])


def test_async_chain_decode_unfilter_adam7_expand(gpu_ctx):
    """The same with interlaced streams: the pass jobs of the unfilter into dense passes, the weave into the file's rows, the expansion."""
    import torch
    from test_gpu_adam7 import _pass_streams
    rng = np.random.default_rng(42)
    cases = _chain_cases()
    b = X.batch(cases)
    n = len(cases)
    bits = [X.CHANNELS[c.ct] * c.depth for c in cases]
    acases = [A.Case(c.name, c.width, c.height, bits[i], b"", 0, 0, 0, [r.tobytes() for r in c.rows]) for i, c in enumerate(cases)]
    streams, jobs = _pass_streams(rng, acases)
    zs = [zlib.compress(s, 6) for s in streams]
    pad = lambda a: (a + np.uint64(15)) & ~np.uint64(15)  # noqa: E731
    in_len, cap = np.array([len(z) for z in zs], np.uint64), np.array([len(s) for s in streams], np.uint64)
    in_off, dec_off, scr_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    in_off[1:], dec_off[1:] = np.cumsum(pad(in_len))[:-1], np.cumsum(pad(cap + np.uint64(4)))[:-1]
    scr_off[1:] = np.cumsum(pad(np.array([A.extent(c.width, c.height, bits[i]) for i, c in enumerate(cases)], np.uint64)))[:-1]
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    flat = [(int(dec_off[i]) + so, sl, int(scr_off[i]) + do, prb, ph, max(1, bits[i] // 8)) for i in range(n) for so, sl, do, prb, ph in jobs[i]]
    m = len(flat)
    col = lambda k, ty: np.array([f[k] for f in flat], ty)  # noqa: E731
    t = [_up(a) for a in (h_in, in_off, in_len, dec_off, cap, col(0, np.uint64), col(1, np.uint64), col(2, np.uint64), col(3, np.uint64),
                          col(3, np.uint32), col(4, np.uint32), col(5, np.uint8), scr_off, b.desc["src_off"], b.desc["src_stride"],
                          np.array([c.width for c in cases], np.uint32), np.array([c.height for c in cases], np.uint32), np.array(bits, np.uint8),
                          b.palette, b.desc)]
    p = [x.data_ptr() for x in t]
    d_dec = torch.full((int(dec_off[-1] + cap[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    d_scr = torch.full((int(scr_off[-1]) + A.extent(cases[-1].width, cases[-1].height, bits[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    d_file = torch.full((len(b.src),), 0xEE, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((len(b.dst_want),), X.FILL, dtype=torch.uint8, device="cuda")
    d_out_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.full((3 * n + m,), -1, dtype=torch.int32, device="cuda")  # the decode's, the deinterlacing's, the expansion's, the pass jobs'
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.decompress_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_out_len.data_ptr(), d_st.data_ptr(), 0, 0, 0, n, sync=False)
    gpu_ctx.unfilter_many_device(d_dec.data_ptr(), p[5], p[6], d_scr.data_ptr(), p[7], p[8], p[9], p[10], p[11], d_st.data_ptr() + 12 * n, 0, m, sync=False)
    gpu_ctx.adam7_many_device(d_scr.data_ptr(), p[12], d_file.data_ptr(), p[13], p[14], p[15], p[16], p[17], d_st.data_ptr() + 4 * n, 0, n, sync=False)
    gpu_ctx.expand_many_device(d_file.data_ptr(), d_dst.data_ptr(), p[18], p[19], d_st.data_ptr() + 8 * n, d_detail.data_ptr(), n, sync=False)
    gpu_ctx.sync()
    st = d_st.cpu().numpy()
    assert (st[:2 * n] == 0).all() and (st[3 * n:] == 0).all() and np.array_equal(d_out_len.cpu().numpy().view(np.uint64), cap)
    check(b, (d_dst.cpu().numpy(), st[2 * n:3 * n], d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)))


# ---- through png.py ----------------------------------------------------------------------------------------------------------------
def _files(rng, sizes=((5, 3), (67, 65))):
    """Files of every type, plain and interlaced, with and without tRNS (a palette's shorter than its PLTE): (blob, reference RGBA)."""
    out = []
    for ct, depth in X.TYPES:
        for k, (w, h) in enumerate(sizes):
            for trns in (False, True):
                entries = min(1 << depth, 48)
                rows = X._random_rows(rng, w, h, ct, depth, entries if ct == 3 else None)
                plte = rng.integers(0, 256, size=(entries, 3), dtype=np.uint8) if ct == 3 else None
                key = pal = chunk = None
                if ct == 3:
                    alpha = rng.integers(0, 255, size=(entries + 1) // 2 if trns else 0, dtype=np.uint8)
                    pal = np.full((entries, 4), 255, np.uint8)
                    pal[:, :3], pal[:len(alpha), 3] = plte, alpha
                    chunk = alpha.tobytes() if trns else None
                elif trns and ct in (0, 2):
                    key = tuple(int(v) for v in X.samples_of(rows, w, ct, depth)[h // 2, w // 2])
                    chunk = b"".join(v.to_bytes(2, "big") for v in key)
                elif trns:
                    continue
                writer = A.write_png if (k + trns) % 2 else PC.write_png
                blob = writer(w, h, ct, depth, rows, "adaptive", palette=plte.tobytes() if plte is not None else None, trns=chunk)
                out.append((blob, X.expand_reference(w, h, ct, depth, rows, X.RGBA8, pal, key)))
    return out


def test_read_png_many_expands_every_type_beside_broken_images(gpu_ctx):
    from pure_zlib_amd import png
    import pure_zlib_amd as P
    rng = np.random.default_rng(51)
    files = _files(rng)
    assert len(files) == 15 * 2 + 11 * 2
    raw = rng.integers(0, 4, size=(9, 33), dtype=np.uint8)
    pal12 = bytes(range(12))
    broken = PC.write_png(33, 9, 3, 8, raw, 1, palette=pal12, stream_edit=lambda s: ("z", lambda z: z[:len(z) // 2]))
    bad_filter = PC.write_png(33, 9, 3, 8, raw, 1, palette=pal12, stream_edit=lambda s: s[:3 * 34] + b"\x09" + s[3 * 34 + 1:])
    raw_bad = raw.copy()
    raw_bad[7, 30], raw_bad[4, 11], raw_bad[4, 2] = 200, 4, 5
    bad_index = PC.write_png(33, 9, 3, 8, raw_bad, "adaptive", palette=pal12, trns=b"\x07")
    bad_index_laced = A.write_png(33, 9, 3, 8, raw_bad, "adaptive", palette=pal12)
    blobs = [f[0] for f in files]
    for at, blob in ((3, broken), (10, bad_filter), (20, bad_index), (31, bad_index_laced)):
        blobs.insert(at, blob)
    for expand, ch in (("rgba8", 4), ("rgb8", 3)):
        got = png.read_png_many(blobs, ctx=gpu_ctx, adam7=True, expand=expand)
        errors = {k: g for k, g in enumerate(got) if isinstance(g, Exception)}
        assert sorted(errors) == [3, 10, 20, 31], errors
        assert all(isinstance(e, P.DecompressionError) for e in errors.values())
        assert "#3: " in str(errors[3]) and "Ran out of data" in str(errors[3])
        assert "#10: row 3 has filter type 9" in str(errors[10])
        for k in (20, 31):
            assert "#%d: row 4, pixel 2: palette index 5 of 4" % k in str(errors[k]) and errors[k].status == 24 and errors[k].detail == (4, 2), errors[k]
        good = [g for g in got if not isinstance(g, Exception)]
        for g, (_blob, want) in zip(good, files):
            assert g.expanded == expand and g.data.dtype == np.uint8 and g.data.shape == want.shape[:2] + (ch,)
            assert np.array_equal(g.data, want[..., :ch]), (g.color_type, g.bit_depth, g.width)
    one = png.read_png(files[17][0], ctx=gpu_ctx, adam7=True, expand="rgba8")
    assert np.array_equal(one.data, files[17][1]) and one.expanded == "rgba8"
    with pytest.raises(P.DecompressionError, match="palette index 5 of 4"):
        png.read_png(bad_index, ctx=gpu_ctx, expand="rgb8")
    with pytest.raises(ValueError, match="expand"):
        png.read_png_many(blobs[:1], ctx=gpu_ctx, expand="bgr8")


def test_trns_is_held_to_its_colour_type_only_with_expand(gpu_ctx):
    from pure_zlib_amd import png
    rng = np.random.default_rng(52)
    mk = lambda ct, depth, trns, **kw: PC.write_png(5, 3, ct, depth, X._random_rows(rng, 5, 3, ct, depth, 2 if ct == 3 else None), 0, trns=trns, **kw)  # noqa: E731
    odd = [mk(0, 8, b"\x00"), mk(2, 8, b"\x00\x01\x00\x02"), mk(2, 16, b"\x00" * 7), mk(6, 8, b"\x00\x01"), mk(4, 16, b"\x00\x01"),
           mk(3, 4, b"\x01\x02\x03", palette=bytes(6)), mk(3, 8, b"", palette=bytes(6))]
    plain = png.read_png_many(odd, ctx=gpu_ctx)
    assert all(isinstance(r, png.PngImage) and r.expanded is None for r in plain), plain  # as before: tRNS is passed on as it stands
    got = png.read_png_many(odd + [mk(0, 8, b"\x00\x07")], ctx=gpu_ctx, expand="rgba8")
    assert all(isinstance(r, ValueError) and "tRNS" in str(r) for r in got[:-1]), got
    assert isinstance(got[-1], png.PngImage) and got[-1].data.shape == (3, 5, 4)


def test_device_out_with_odd_offsets_and_guard_bytes(gpu_ctx):
    import torch
    from pure_zlib_amd import png
    rng = np.random.default_rng(53)
    files = [f for f in _files(rng, sizes=((13, 7),)) if True][::4]
    ch = 3
    offs, strides, at = [], [], 3
    for k, (_b, want) in enumerate(files):
        offs.append(at)
        strides.append(13 * ch + (0, 5, 1)[k % 3])
        at += 7 * strides[-1] + (1, 7, 12)[k % 3]
    t = torch.full((at + 9,), PC.FILL, dtype=torch.uint8, device="cuda")
    got = png.read_png_many([f[0] for f in files], ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides), adam7=True, expand="rgb8")
    assert all(isinstance(g, png.PngImage) and g.data is None and g.expanded == "rgb8" for g in got), got
    host = t.cpu().numpy()
    want = np.full(len(host), PC.FILL, np.uint8)
    for (_b, ref), o, s in zip(files, offs, strides):
        for r in range(7):
            want[o + r * s:o + r * s + 13 * ch] = ref[r, :, :ch].reshape(-1)
    assert np.array_equal(host, want)
    with pytest.raises(ValueError, match="stride"):
        png.read_png_many([files[0][0]], ctx=gpu_ctx, device_out=(t.data_ptr(), [0], [13 * ch - 1]), adam7=True, expand="rgb8")


def test_read_png_batch_with_one_image_of_another_size(gpu_ctx):
    from pure_zlib_amd import png
    rng = np.random.default_rng(54)
    same = [f for f in _files(rng, sizes=((13, 7),))][::5]
    other = _files(rng, sizes=((5, 3),))[8]
    blobs = [f[0] for f in same]
    blobs.insert(2, other[0])
    blobs.insert(4, b"not a png")
    for expand, ch in (("rgb8", 3), ("rgba8", 4)):
        t, errors = png.read_png_batch(blobs, expand=expand, adam7=True, ctx=gpu_ctx)
        assert tuple(t.shape) == (len(blobs), 7, 13, ch) and t.is_cuda and [k for k, _e in errors] == [2, 4]
        assert "5 x 3" in str(errors[0][1]) and "signature" in str(errors[1][1])
        host = t.cpu().numpy()
        assert not host[2].any() and not host[4].any()
        refs = iter(same)
        for k in range(len(blobs)):
            if k not in (2, 4):
                assert np.array_equal(host[k], next(refs)[1][..., :ch]), k
    t, errors = png.read_png_batch(blobs[:1], ctx=gpu_ctx)
    assert tuple(t.shape) == (1, 7, 13, 3) and errors == [] and np.array_equal(t.cpu().numpy()[0], same[0][1][..., :3])


def test_without_expand_nothing_changes_and_no_expansion_is_launched(gpu_ctx, monkeypatch):
    from pure_zlib_amd import png
    rng = np.random.default_rng(55)
    blobs = [f[0] for f in _files(rng)]
    calls = []
    real = type(gpu_ctx).expand_many_device
    monkeypatch.setattr(type(gpu_ctx), "expand_many_device", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])
    first = png.read_png_many(blobs, ctx=gpu_ctx, adam7=True)
    second = png.read_png_many(blobs, ctx=gpu_ctx, adam7=True, expand=None)
    assert calls == []
    for a, b in zip(first, second):
        assert isinstance(a, png.PngImage) and a.expanded is None and a.data.dtype == b.data.dtype and a.data.shape == b.data.shape
        assert a.data.tobytes() == b.data.tobytes()
        if a.bit_depth < 8:
            assert a.data.shape == (a.height, a.row_bytes)  # the file's packed rows, as ever
    png.read_png_many(blobs[:2], ctx=gpu_ctx, adam7=True, expand="rgba8")
    assert calls == [1]
