"""GPU: pzg_unfilter_many and pure_zlib_amd/png.py against the reference unfilter of tests/pngcases.py, byte for byte: the cases the CPU
model runs (tests/test_model_unfilter.py), laid out with src_off at every misalignment, dst_off off the 16-byte boundaries and
dst_stride = row_bytes + 5 over a 0xCD prefill that is checked everywhere nothing is delivered."""
import numpy as np
import pytest

import pngcases as PC

pytestmark = pytest.mark.gpu


def run_host(ctx, b):
    dst = np.full(len(b.dst_want), PC.FILL, np.uint8)
    status, detail = ctx.unfilter_many(b.src, b.src_off, b.src_len, dst, b.dst_off, b.stride, b.row_bytes, b.height, b.bpp)
    return dst, status, detail


def run_device(ctx, b, src_len_ptr=None, sync=True):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
    n = len(b.cases)
    t = [up(a) for a in (b.src, b.src_off, b.src_len, b.dst_off, b.stride, b.row_bytes, b.height, b.bpp)]
    d_dst = torch.full((len(b.dst_want),), PC.FILL, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_detail = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.unfilter_many_device(t[0].data_ptr(), t[1].data_ptr(), src_len_ptr or t[2].data_ptr(), d_dst.data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                             t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), n, sync=sync)
    if not sync:
        ctx.sync()
    return d_dst.cpu().numpy(), d_status.cpu().numpy(), d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)


def check(b, got):
    dst, status, detail = got
    for i, c in enumerate(b.cases):
        assert (int(status[i]), int(detail[i, 0]), int(detail[i, 1])) == (c.status, c.d0, c.d1), c.name
    assert PC.first_difference(dst, b) is None, PC.first_difference(dst, b)


def test_every_shape_in_batches_of_1_64_and_200(gpu_ctx):
    """Every bpp x row_bytes x height, each image of another shape, a seeded random filter per row; an empty image in the middle."""
    cases = PC.shape_cases()
    for part in (cases[:1], cases[1:33] + [PC.empty_case()] + cases[33:64], cases[-200:]):
        assert len(part) in (1, 64, 200)
        b = PC.batch(part)
        check(b, run_device(gpu_ctx, b))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_each_filter_paeth_ties_and_average_carry(gpu_ctx):
    b = PC.batch(PC.filter_cases())
    check(b, run_device(gpu_ctx, b))


def test_bad_filter_bytes_and_cut_inputs(gpu_ctx):
    b = PC.batch(PC.error_cases())
    check(b, run_device(gpu_ctx, b))


def test_both_pointer_forms_give_the_same(gpu_ctx):
    cases = PC.shape_cases()[::7] + PC.error_cases()[::5] + [PC.empty_case()] + PC.filter_cases()[::31]
    for extra in (5, 0):
        b = PC.batch(cases, stride_extra=extra)
        host, device = run_host(gpu_ctx, b), run_device(gpu_ctx, b)
        check(b, host)
        check(b, device)
        for h, d in zip(host, device):
            assert np.array_equal(h, d)
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_bad_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    b = PC.batch(PC.shape_cases()[:3])
    L, h = _ffi.lib(), gpu_ctx.handle
    dst = np.full(len(b.dst_want), PC.FILL, np.uint8)
    status, detail = np.zeros(3, np.int32), np.zeros(6, np.uint32)

    def call(n=3, flags=0, bpp=b.bpp, stride=b.stride):
        return L.pzg_unfilter_many(h, b.src.ctypes.data, b.src_off.ctypes.data, b.src_len.ctypes.data, dst.ctypes.data, b.dst_off.ctypes.data,
                                   stride.ctypes.data, b.row_bytes.ctypes.data, b.height.ctypes.data, bpp.ctypes.data, status.ctypes.data,
                                   detail.ctypes.data, n, flags)
    assert call(n=0) == _ffi.RC_BAD_ARG and call(flags=_ffi.GZIP) == _ffi.RC_BAD_ARG and call(flags=_ffi.ASYNC) == _ffi.RC_BAD_ARG
    assert call(bpp=np.array([1, 5, 1], np.uint8)) == _ffi.RC_BAD_ARG
    assert call(stride=b.row_bytes.astype(np.uint64) - np.uint64(1)) == _ffi.RC_BAD_ARG
    assert (dst == PC.FILL).all()
    assert call() == _ffi.RC_OK and PC.first_difference(dst, b) is None
    # device arrays are not read by the host: the image is refused on the device, its neighbours are delivered
    c = PC.shape_cases()
    bad = PC.Case("bpp 5", 5, c[9].row_bytes, c[9].height, c[9].stream, PC.E_FILTER, 0xffffffff, 5, [])
    bd = PC.batch([c[8], bad, c[10]])
    check(bd, run_device(gpu_ctx, bd))


def test_async_chain_takes_the_decodes_out_len(gpu_ctx):
    """decompress_many_device, then the unfilter with src_len = the decode's out_len array, one sync: what the two synchronous calls give."""
    import torch
    import zlib
    cases = PC.shape_cases()[5::11] + PC.error_cases()[3::9]
    b = PC.batch(cases)
    n = len(cases)
    zs = [zlib.compress(c.stream, 6) for c in cases]
    in_len = np.array([len(z) for z in zs], np.uint64)
    in_off = np.zeros(n, np.uint64)
    in_off[1:] = np.cumsum((in_len + np.uint64(15)) & ~np.uint64(15))[:-1]
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
    # the decode delivers each stream where the batch has it in src: the unfilter reads it there
    t = [up(a) for a in (h_in, in_off, in_len, b.src_off, b.src_len, b.dst_off, b.stride, b.row_bytes, b.height, b.bpp)]
    results = []
    for sync in (False, True):
        d_dec = torch.full((len(b.src),), 0xEE, dtype=torch.uint8, device=dev)
        d_dst = torch.full((len(b.dst_want),), PC.FILL, dtype=torch.uint8, device=dev)
        d_out_len = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.full((2 * n,), -1, dtype=torch.int32, device=dev)
        d_detail = torch.zeros(4 * n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        gpu_ctx.decompress_many_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d_dec.data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                       d_out_len.data_ptr(), d_st.data_ptr(), d_detail.data_ptr(), 0, 0, n, sync=sync)
        gpu_ctx.unfilter_many_device(d_dec.data_ptr(), t[3].data_ptr(), d_out_len.data_ptr(), d_dst.data_ptr(), t[5].data_ptr(), t[6].data_ptr(),
                                     t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr(), d_st.data_ptr() + 4 * n, d_detail.data_ptr() + 8 * n, n,
                                     sync=sync)
        if not sync:
            gpu_ctx.sync()
        st = d_st.cpu().numpy()
        assert (st[:n] == 0).all() and np.array_equal(d_out_len.cpu().numpy().view(np.uint64), b.src_len)
        results.append((d_dst.cpu().numpy(), st[n:], d_detail.cpu().numpy().view(np.uint32)[2 * n:].reshape(n, 2)))
    check(b, results[0])
    for x, y in zip(*results):
        assert np.array_equal(x, y)


# ---- through png.py ----------------------------------------------------------------------------------------------------------------
def _raw(rng, w, h, ctype, depth):
    rb, _ = PC.geometry(w, ctype, depth)
    raw = rng.integers(0, 256, size=(h, rb), dtype=np.uint8)
    if depth < 8 and (w * PC.CHANNELS[ctype] * depth) % 8:
        raw[:, -1] &= (0xff << (8 - (w * depth) % 8)) & 0xff  # (the padding bits of a packed row)
    return raw


def test_every_colour_type_and_depth(gpu_ctx):
    from pure_zlib_amd import png
    rng = np.random.default_rng(11)
    blobs, want = [], []
    for ctype, depths in PC.DEPTHS.items():
        for depth in depths:
            for (w, h), idat in (((5, 3), 1), ((67, 65), None)):  # IDAT cut into 1-byte chunks, and one chunk
                raw = _raw(rng, w, h, ctype, depth)
                blobs.append(PC.write_png(w, h, ctype, depth, raw, rng.integers(0, 5, size=h), idat=idat, trns=b"\x01\x02" if ctype == 3 else None))
                want.append((w, h, ctype, depth, raw))
    got = png.read_png_many(blobs, ctx=gpu_ctx)
    assert len(got) == 30
    for g, (w, h, ctype, depth, raw) in zip(got, want):
        assert isinstance(g, png.PngImage), g
        assert (g.width, g.height, g.color_type, g.bit_depth) == (w, h, ctype, depth)
        assert (g.palette is not None) == (ctype == 3) and g.trns == (b"\x01\x02" if ctype == 3 else None)
        ch = PC.CHANNELS[ctype]
        assert g.data.shape == ((h, w, ch) if depth >= 8 else (h, raw.shape[1])) and g.data.dtype == (np.dtype(">u2") if depth == 16 else np.uint8)
        assert g.data.tobytes() == raw.tobytes(), (ctype, depth, w, h)
    assert png.read_png(blobs[7], ctx=gpu_ctx).data.tobytes() == want[7][4].tobytes()


def test_bad_images_beside_good_ones(gpu_ctx):
    from pure_zlib_amd import png
    import pure_zlib_amd as P
    rng = np.random.default_rng(12)
    raw = _raw(rng, 67, 65, 2, 8)
    good = PC.write_png(67, 65, 2, 8, raw, "adaptive")
    more = np.vstack([raw, raw[:1]])
    bad = {
        "crc": PC.write_png(67, 65, 2, 8, raw, 4, idat=100, bad_crc=b"IDAT"),
        "short": PC.write_png(67, 65, 2, 8, raw, 4, stream_edit=lambda s: ("z", lambda z: z[:len(z) // 2])),
        "extra row": PC.write_png(67, 65, 2, 8, more, 4),
        "row short": PC.write_png(67, 65, 2, 8, raw[:-1], 4),
        "filter byte": PC.write_png(67, 65, 2, 8, raw, 1, stream_edit=lambda s: s[:64 * 202] + b"\x07" + s[64 * 202 + 1:]),
        "interlaced": PC.write_png(67, 65, 2, 8, raw, 0, interlace=1),
    }
    for name, blob in bad.items():
        got = png.read_png_many([good, blob, good], ctx=gpu_ctx)
        for g in (got[0], got[2]):
            assert isinstance(g, png.PngImage) and g.data.tobytes() == raw.tobytes(), name
        e = got[1]
        assert isinstance(e, Exception) and str(e).find("#1: ") >= 0, (name, e)
        if name == "crc":
            assert isinstance(e, ValueError) and "IDAT: checksum mismatch" in str(e)
        elif name == "short":
            assert isinstance(e, P.DecompressionError) and e.show() == "Decompression error: #1: Ran out of data mid-decompression 2."
        elif name == "extra row":
            assert isinstance(e, P.DecompressionError) and "too much image data" in str(e)
        elif name == "row short":
            assert isinstance(e, P.DecompressionError) and "not enough image data" in str(e)
        elif name == "filter byte":
            assert isinstance(e, P.DecompressionError) and "row 64 has filter type 7" in str(e) and e.status == 23
        else:
            assert isinstance(e, NotImplementedError) and "interlaced" in str(e)
    with pytest.raises(NotImplementedError):
        png.read_png(bad["interlaced"], ctx=gpu_ctx)
    assert [k for k, _why in png.test_png_many([good, bad["crc"], good, bad["short"]], ctx=gpu_ctx)] == [1, 3]


def test_device_out_lands_the_rows_in_the_callers_tensor(gpu_ctx):
    import torch
    from pure_zlib_amd import png
    rng = np.random.default_rng(13)
    raws = [_raw(rng, 67, 65, 6, 8), _raw(rng, 5, 3, 0, 16)]
    blobs = [PC.write_png(67, 65, 6, 8, raws[0], "adaptive"), PC.write_png(5, 3, 0, 16, raws[1], 3)]
    t = torch.full((65 * 300 + 64 + 3 * 16,), PC.FILL, dtype=torch.uint8, device="cuda")
    offs, strides = [0, 65 * 300 + 64], [300, 16]
    got = png.read_png_many(blobs, ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides))
    assert all(isinstance(g, png.PngImage) and g.data is None for g in got)
    host = t.cpu().numpy()
    want = np.full(len(host), PC.FILL, np.uint8)
    for raw, o, s in zip(raws, offs, strides):
        for r in range(raw.shape[0]):
            want[o + r * s:o + r * s + raw.shape[1]] = raw[r]
    assert np.array_equal(host, want)
