"""GPU: pzg_adam7_many and the adam7=True path of pure_zlib_amd/png.py against the Adam7 reference of tests/adam7cases.py, byte for
byte: the cases the CPU model runs (tests/test_model_adam7.py), laid out with src_off at every misalignment, dst_off off the 16-byte
boundaries and dst_stride = row_bytes + 5 (and + 0) over a 0xCD prefill that is checked everywhere nothing is delivered."""
import zlib

import numpy as np
import pytest

import adam7cases as A
import pngcases as PC

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(torch.device("cuda", 0))


def run_host(ctx, b):
    dst = np.full(len(b.dst_want), A.FILL, np.uint8)
    status, detail = ctx.adam7_many(b.src, b.src_off, dst, b.dst_off, b.stride, b.width, b.height, b.bits)
    return dst, status, detail


def run_device(ctx, b, sync=True):
    import torch
    n = len(b.cases)
    t = [_up(a) for a in (b.src, b.src_off, b.dst_off, b.stride, b.width, b.height, b.bits)]
    d_dst = torch.full((len(b.dst_want),), A.FILL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.adam7_many_device(t[0].data_ptr(), t[1].data_ptr(), d_dst.data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
                          t[6].data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), n, sync=sync)
    if not sync:
        ctx.sync()
    return d_dst.cpu().numpy(), d_status.cpu().numpy(), d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)


def check(b, got):
    dst, status, detail = got
    for i, c in enumerate(b.cases):
        assert (int(status[i]), int(detail[i, 0]), int(detail[i, 1])) == (c.status, c.d0, c.d1), c.name
    assert A.first_difference(dst, b) is None, A.first_difference(dst, b)


def test_every_case_in_batches_of_1_64_and_the_rest(gpu_ctx):
    """Every pixel_bits at every (w, h) in 1..9 x 1..9 and at the edge shapes; empty images among the rest."""
    cases = A.all_cases()
    rest = cases[65:400] + A.empty_cases() + cases[400:]
    for part, extra in ((cases[:1], 5), (cases[1:65], 5), (rest, 5), (rest, 0)):
        assert len(part) in (1, 64, 757 - 65 + 2)
        b = A.batch(part, stride_extra=extra)
        check(b, run_device(gpu_ctx, b))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_both_pointer_forms_give_the_same(gpu_ctx):
    cases = A.small_cases()[::7] + A.empty_cases() + A.edge_cases()[::3]
    for extra in (5, 0):
        b = A.batch(cases, stride_extra=extra)
        host, device = run_host(gpu_ctx, b), run_device(gpu_ctx, b)
        check(b, host)
        check(b, device)
        for h, d in zip(host, device):
            assert np.array_equal(h, d)
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_bad_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    b = A.batch(A.edge_cases()[:3])
    L, h = _ffi.lib(), gpu_ctx.handle
    dst = np.full(len(b.dst_want), A.FILL, np.uint8)
    status, detail = np.zeros(3, np.int32), np.zeros(6, np.uint32)

    def call(n=3, flags=0, bits=b.bits, stride=b.stride, width=b.width, height=b.height, src_off=b.src_off):
        return L.pzg_adam7_many(h, b.src.ctypes.data, src_off.ctypes.data if src_off is not None else None, dst.ctypes.data, b.dst_off.ctypes.data,
                                stride.ctypes.data, width.ctypes.data, height.ctypes.data, bits.ctypes.data, status.ctypes.data, detail.ctypes.data,
                                n, flags)
    assert call(n=0) == _ffi.RC_BAD_ARG and call(flags=_ffi.GZIP) == _ffi.RC_BAD_ARG and call(flags=_ffi.ASYNC) == _ffi.RC_BAD_ARG
    assert call(src_off=None) == _ffi.RC_BAD_ARG
    for bad in (0, 3, 12, 65):
        assert call(bits=np.array([b.bits[0], bad, b.bits[2]], np.uint8)) == _ffi.RC_BAD_ARG
    short = b.stride.copy()
    short[2] = A.row_bytes_of(int(b.width[2]), int(b.bits[2])) - 1
    assert call(stride=short) == _ffi.RC_BAD_ARG
    assert call(width=np.array([b.width[0], 1 << 31, b.width[2]], np.uint32)) == _ffi.RC_BAD_ARG
    assert call(height=np.array([1 << 31, b.height[1], b.height[2]], np.uint32)) == _ffi.RC_BAD_ARG
    assert (dst == A.FILL).all()
    assert call() == _ffi.RC_OK and A.first_difference(dst, b) is None and (status == 0).all() and (detail == 0).all()


def test_bad_geometry_is_refused_on_the_device_between_good_neighbours(gpu_ctx):
    """Device arrays are not read by the host: the image gets PZG_E_FILTER with (0xffffffff, pixel_bits), nothing of it is written, its
    neighbours are delivered."""
    good = A.edge_cases()
    for k, bad in enumerate(A.bad_geometry_cases()):
        b = A.batch([good[k], bad, good[k + 9]])
        check(b, run_device(gpu_ctx, b))
    # a stride one below the row's bytes
    c = good[4]
    b = A.batch([good[3], A.Case("stride", c.width, c.height, c.bits, c.src, A.E_FILTER, A.BAD_ARGS, c.bits, []), good[5]])
    b.stride[1] = c.row_bytes - 1
    check(b, run_device(gpu_ctx, b))


def _pass_streams(rng, cases):
    """Per case: its filtered stream (every pass filtered on its own, a random filter per row) and the unfilter jobs of its passes
    as (offset in the stream, length, offset in the dense passes, row bytes, rows)."""
    streams, jobs = [], []
    for c in cases:
        raw = np.frombuffer(b"".join(c.rows), np.uint8).reshape(c.height, c.row_bytes)
        s, at, dense, mine = b"", 0, 0, []
        for p in A.interlace(raw, c.width, c.bits):
            if p is not None:
                ph, prb = p.shape
                s += PC.filter_stream(p, max(1, c.bits // 8), rng.integers(0, 5, size=ph))
                mine.append((at, ph * (1 + prb), dense, prb, ph))
                at += ph * (1 + prb)
                dense += ph * prb
        assert at == len(s) == A.filtered_pass_offsets(c.width, c.height, c.bits)[1]
        streams.append(s)
        jobs.append(mine)
    return streams, jobs


def test_async_chain_decode_unfilter_adam7(gpu_ctx):
    """decompress_many_device, unfilter_many_device over the pass jobs, adam7_many_device, one sync: what the three synchronous calls
    give, and what the reference gives."""
    import torch
    rng = np.random.default_rng(21)
    cases = A.small_cases()[3::41] + A.edge_cases()[1::5]
    b = A.batch(cases)  # (the passes are not taken from b.src: the unfilter delivers them where b.src has them)
    n = len(cases)
    streams, jobs = _pass_streams(rng, cases)
    zs = [zlib.compress(s, 6) for s in streams]
    pad = lambda a: (a + np.uint64(15)) & ~np.uint64(15)  # noqa: E731
    in_len, cap = np.array([len(z) for z in zs], np.uint64), np.array([len(s) for s in streams], np.uint64)
    in_off, dec_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    in_off[1:], dec_off[1:] = np.cumsum(pad(in_len))[:-1], np.cumsum(pad(cap + np.uint64(4)))[:-1]
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    flat = [(int(dec_off[i]) + so, sl, int(b.src_off[i]) + do, prb, ph, max(1, c.bits // 8)) for i, c in enumerate(cases) for so, sl, do, prb, ph in jobs[i]]
    m = len(flat)
    col = lambda k, t: np.array([f[k] for f in flat], t)  # noqa: E731
    t = [_up(a) for a in (h_in, in_off, in_len, dec_off, cap, col(0, np.uint64), col(1, np.uint64), col(2, np.uint64), col(3, np.uint64),
                          col(3, np.uint32), col(4, np.uint32), col(5, np.uint8), b.src_off, b.dst_off, b.stride, b.width, b.height, b.bits)]
    p = [x.data_ptr() for x in t]
    results = []
    for sync in (False, True):
        d_dec = torch.full((int(dec_off[-1] + cap[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        d_scr = torch.full((len(b.src),), 0xEE, dtype=torch.uint8, device="cuda")
        d_dst = torch.full((len(b.dst_want),), A.FILL, dtype=torch.uint8, device="cuda")
        d_out_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_st = torch.full((2 * n + m,), -1, dtype=torch.int32, device="cuda")  # the decode's, the deinterlacing's, the pass jobs'
        d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.decompress_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_out_len.data_ptr(), d_st.data_ptr(), 0, 0, 0, n, sync=sync)
        gpu_ctx.unfilter_many_device(d_dec.data_ptr(), p[5], p[6], d_scr.data_ptr(), p[7], p[8], p[9], p[10], p[11], d_st.data_ptr() + 8 * n, 0, m,
                                     sync=sync)
        gpu_ctx.adam7_many_device(d_scr.data_ptr(), p[12], d_dst.data_ptr(), p[13], p[14], p[15], p[16], p[17], d_st.data_ptr() + 4 * n,
                                  d_detail.data_ptr(), n, sync=sync)
        if not sync:
            gpu_ctx.sync()
        st = d_st.cpu().numpy()
        assert (st[:n] == 0).all() and (st[2 * n:] == 0).all() and np.array_equal(d_out_len.cpu().numpy().view(np.uint64), cap)
        results.append((d_dst.cpu().numpy(), st[n:2 * n], d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)))
    check(b, results[0])
    for x, y in zip(*results):
        assert np.array_equal(x, y)


# ---- through png.py ----------------------------------------------------------------------------------------------------------------
def _raw(rng, w, h, ctype, depth):
    rb, _ = PC.geometry(w, ctype, depth)
    raw = rng.integers(0, 256, size=(h, rb), dtype=np.uint8)
    if depth < 8 and (w * depth) % 8:
        raw[:, -1] &= (0xff << (8 - (w * depth) % 8)) & 0xff  # (the padding bits of a packed row)
    return raw


def _random_filters(rng):
    return lambda ph: rng.integers(0, 5, size=ph)


def test_every_colour_type_and_depth_interlaced(gpu_ctx):
    """`data` is byte for byte what read_png_many gives for the same pixels written non-interlaced."""
    from pure_zlib_amd import png
    rng = np.random.default_rng(31)
    laced, plain, want = [], [], []
    for ctype, depths in PC.DEPTHS.items():
        for depth in depths:
            for (w, h), idat in (((5, 3), 1), ((67, 65), None)):  # IDAT cut into 1-byte chunks, and one chunk
                raw = _raw(rng, w, h, ctype, depth)
                trns = b"\x01\x02" if ctype == 3 else None
                laced.append(A.write_png(w, h, ctype, depth, raw, _random_filters(rng), idat=idat, trns=trns))
                plain.append(PC.write_png(w, h, ctype, depth, raw, rng.integers(0, 5, size=h), trns=trns))
                want.append((w, h, ctype, depth, raw))
    got, ref = png.read_png_many(laced, ctx=gpu_ctx, adam7=True), png.read_png_many(plain, ctx=gpu_ctx)
    assert len(got) == 30
    for g, r, (w, h, ctype, depth, raw) in zip(got, ref, want):
        assert isinstance(g, png.PngImage) and isinstance(r, png.PngImage), (g, r)
        assert (g.width, g.height, g.color_type, g.bit_depth, g.palette, g.trns) == (r.width, r.height, r.color_type, r.bit_depth, r.palette, r.trns)
        assert g.data.shape == r.data.shape and g.data.dtype == r.data.dtype
        assert g.data.tobytes() == r.data.tobytes() == raw.tobytes(), (ctype, depth, w, h)
    assert png.read_png(laced[7], ctx=gpu_ctx, adam7=True).data.tobytes() == want[7][4].tobytes()


def test_interlaced_and_plain_images_in_one_batch(gpu_ctx):
    from pure_zlib_amd import png
    rng = np.random.default_rng(32)
    raws = [_raw(rng, 67, 65, 2, 8), _raw(rng, 5, 3, 0, 1), _raw(rng, 33, 131, 6, 16), _raw(rng, 9, 9, 3, 2)]
    geo = [(67, 65, 2, 8), (5, 3, 0, 1), (33, 131, 6, 16), (9, 9, 3, 2)]
    blobs = []
    for k, (raw, (w, h, ctype, depth)) in enumerate(zip(raws, geo)):
        blobs.append(A.write_png(w, h, ctype, depth, raw, "adaptive"))
        blobs.append(PC.write_png(w, h, ctype, depth, raw, "adaptive"))
    got = png.read_png_many(blobs, ctx=gpu_ctx, adam7=True)
    for k, g in enumerate(got):
        assert isinstance(g, png.PngImage) and g.data.tobytes() == raws[k // 2].tobytes(), k
    assert png.test_png_many(blobs, ctx=gpu_ctx, adam7=True) == [] and [k for k, _why in png.test_png_many(blobs, ctx=gpu_ctx)] == [0, 2, 4, 6]


def test_device_out_with_padded_strides(gpu_ctx):
    import torch
    from pure_zlib_amd import png
    rng = np.random.default_rng(33)
    raws = [_raw(rng, 67, 65, 6, 8), _raw(rng, 5, 3, 0, 16), _raw(rng, 13, 7, 0, 4)]
    blobs = [A.write_png(67, 65, 6, 8, raws[0], "adaptive"), PC.write_png(5, 3, 0, 16, raws[1], 3), A.write_png(13, 7, 0, 4, raws[2], 4)]
    offs, strides = [3, 65 * 300 + 64, 65 * 300 + 64 + 3 * 16 + 5], [300, 16, 7]
    t = torch.full((offs[2] + 7 * 7 + 9,), PC.FILL, dtype=torch.uint8, device="cuda")
    got = png.read_png_many(blobs, ctx=gpu_ctx, device_out=(t.data_ptr(), offs, strides), adam7=True)
    assert all(isinstance(g, png.PngImage) and g.data is None for g in got), got
    host = t.cpu().numpy()
    want = np.full(len(host), PC.FILL, np.uint8)
    for raw, o, s in zip(raws, offs, strides):
        for r in range(raw.shape[0]):
            want[o + r * s:o + r * s + raw.shape[1]] = raw[r]
    assert np.array_equal(host, want)


def test_bad_interlaced_images_beside_good_ones(gpu_ctx):
    from pure_zlib_amd import png
    import pure_zlib_amd as P
    rng = np.random.default_rng(34)
    raw = _raw(rng, 67, 65, 2, 8)
    good = A.write_png(67, 65, 2, 8, raw, "adaptive")
    offs, total = A.filtered_pass_offsets(67, 65, 24)
    _pw, _ph, prb3 = A.pass_sizes(67, 65, 24)[2]
    at3 = offs[2] + 5 * (1 + prb3)  # row 5 of pass 3 (it has 8)
    at5 = offs[4] + 2 * (1 + A.pass_sizes(67, 65, 24)[4][2])
    edit = lambda where: (lambda s: s[:where] + b"\x07" + s[where + 1:])  # noqa: E731
    not_interlaced = PC.write_png(67, 65, 2, 8, raw, 0, interlace=1)  # the existing suite's blob: 13130 bytes where Adam7 needs 13189
    assert total == 13189
    bad = {
        "filter byte": A.write_png(67, 65, 2, 8, raw, 1, stream_edit=edit(at3)),
        "two filter bytes": A.write_png(67, 65, 2, 8, raw, 1, stream_edit=lambda s: edit(at3)(edit(at5)(s))),
        "short": A.write_png(67, 65, 2, 8, raw, 4, stream_edit=lambda s: ("z", lambda z: z[:len(z) // 2])),
        "not interlaced": not_interlaced,
        "too much": A.write_png(67, 65, 2, 8, raw, 0, stream_edit=lambda s: s + b"\x00"),
    }
    for name, blob in bad.items():
        got = png.read_png_many([good, blob, good], ctx=gpu_ctx, adam7=True)
        for g in (got[0], got[2]):
            assert isinstance(g, png.PngImage) and g.data.tobytes() == raw.tobytes(), name
        e = got[1]
        assert isinstance(e, P.DecompressionError) and str(e).find("#1: ") >= 0, (name, e)
        if name in ("filter byte", "two filter bytes"):
            assert "#1: pass 3: row 5 has filter type 7" in str(e) and e.status == 23, e
        elif name == "short":  # the reference's text for the cut stream, behind the image's name
            from oracle import oracle as O
            text = O.decompress(png._parse("", blob, True)[1])[0].message.decode()
            kind, _, what = text.partition(": ")
            assert "Ran out of data" in what and e.show() == "%s: #1: %s" % (kind, what), (e.show(), text)
        elif name == "not interlaced":
            assert "not enough image data" in str(e)
        else:
            assert "too much image data" in str(e)
    e = png.read_png_many([good, not_interlaced, good], ctx=gpu_ctx)
    assert all(isinstance(x, NotImplementedError) and "interlaced" in str(x) for x in e), e
    with pytest.raises(NotImplementedError):
        png.read_png(not_interlaced, ctx=gpu_ctx)
