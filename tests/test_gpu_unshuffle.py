"""GPU: pzg_unshuffle_many against the numpy reference of tests/fpcases.py, byte for byte: the cases the CPU model runs
(tests/test_model_unshuffle.py), laid out with the sources at every misalignment, the destinations off the dword and 16-byte boundaries
and padded strides over a 0xCD prefill that is checked everywhere nothing is delivered -- through host pointers, device pointers and
the async chain behind a decode."""
import zlib

import numpy as np
import pytest

import fpcases as F

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(torch.device("cuda", 0))


def run_host(ctx, b):
    dst = np.full(len(b.dst_want), F.FILL, np.uint8)
    status, detail = ctx.unshuffle_many(b.src, b.src_len, dst, b.desc)
    return dst, status, detail


def run_device(ctx, b, sync=True):
    import torch
    n = len(b.cases)
    t = [_up(a) for a in (b.src, b.src_len, b.desc)]
    d_dst = torch.full((len(b.dst_want),), F.FILL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.unshuffle_many_device(t[0].data_ptr(), t[1].data_ptr(), d_dst.data_ptr(), t[2].data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), n, sync=sync)
    if not sync:
        ctx.sync()
    return d_dst.cpu().numpy(), d_status.cpu().numpy(), d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)


def check(b, got):
    dst, status, detail = got
    for i, c in enumerate(b.cases):
        assert (int(status[i]), int(detail[i, 0]), int(detail[i, 1])) == (c.status, c.d0, c.d1), c.name
    assert F.first_difference(dst, b) is None, F.first_difference(dst, b)


def test_every_case_on_device_pointers(gpu_ctx):
    """Every element size, sum stride, plane order, count, height and window; the sources cut short, the empty jobs and the illegal
    geometries among good neighbours; in one launch, and again with every job at another layout."""
    cases = F.all_cases()
    assert 500 < len(cases) < 700 and max(c.stored.size for c in cases) < 64 * 1024
    for shift in (0, 5):
        b = F.batch(cases, shift)
        check(b, run_device(gpu_ctx, b))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_both_pointer_forms_give_the_same(gpu_ctx):
    """The host-pointer form refuses illegal geometry with its return value (test_bad_arguments): here it gets everything else."""
    cases = F.shape_cases() + F.special_cases() + F.truncated_cases() + F.empty_cases()
    b = F.batch(cases, 1)
    host, device = run_host(gpu_ctx, b), run_device(gpu_ctx, b, sync=False)
    check(b, host)
    check(b, device)
    assert np.array_equal(host[0], device[0]) and np.array_equal(host[1], device[1]) and np.array_equal(host[2], device[2])
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_a_batch_of_one_job_and_many_slices(gpu_ctx):
    """One job alone gets the most row slices a launch gives; a few thousand get the fewest."""
    for c in (F.shape_cases()[100], F.special_cases()[-3], F.truncated_cases()[5], F.empty_cases()[0]):
        b = F.batch([c], 3)
        check(b, run_device(gpu_ctx, b))
        check(b, run_host(gpu_ctx, b))
    many = (F.shape_cases()[::4] + F.truncated_cases()) * 70
    assert len(many) > 8192
    b = F.batch(many, 2)
    check(b, run_device(gpu_ctx, b))


def test_bad_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    good = [F.shape_cases()[3], F.shape_cases()[200], F.shape_cases()[290]]
    L, h = _ffi.lib(), gpu_ctx.handle
    b = F.batch(good)
    dst = np.full(len(b.dst_want), F.FILL, np.uint8)
    status, detail = np.zeros(3, np.int32), np.zeros(6, np.uint32)

    def call(bb=b, n=3, flags=0, desc=True, slen=True, src=True):
        return L.pzg_unshuffle_many(h, bb.src.ctypes.data if src else None, bb.src_len.ctypes.data if slen else None, dst.ctypes.data,
                                    bb.desc.ctypes.data if desc else None, status.ctypes.data, detail.ctypes.data, n, flags)
    assert call(n=0) == _ffi.RC_BAD_ARG and call(flags=_ffi.GZIP) == _ffi.RC_BAD_ARG and call(flags=_ffi.ASYNC) == _ffi.RC_BAD_ARG
    assert call(desc=False) == _ffi.RC_BAD_ARG and call(slen=False) == _ffi.RC_BAD_ARG and call(src=False) == _ffi.RC_BAD_ARG
    for bad in F.bad_geometry_cases():  # every illegal geometry, between two good jobs
        assert call(bb=F.batch([good[0], bad, good[2]])) == _ffi.RC_BAD_ARG, bad.name
    assert (dst == F.FILL).all()
    assert call() == _ffi.RC_OK
    assert F.first_difference(dst, b) is None and (status == 0).all() and (detail == 0).all()


def test_async_chain_behind_a_decode_with_a_stream_that_decodes_short(gpu_ctx):
    """pzg_decompress_many -> pzg_unshuffle_many -> pzg_sync with the decode's out_len as src_len.  One stream of the batch holds
    fewer rows than its job says: that job is PZG_E_TRUNCATED with the rows it has, and its neighbours are untouched."""
    import torch
    cases = [c for c in F.shape_cases() if c.srb // c.b in (8, 9, 512, 513)][::2] + F.special_cases()[-9:-3]
    keep = 2
    short_at = next(i for i, c in enumerate(cases) if i and c.rows > keep + 1 and c.window[0] == 0 and c.window[1] > keep and c.s)
    assert 0 < short_at < len(cases) - 1
    n = len(cases)
    streams = [c.stored.tobytes() for c in cases]
    streams[short_at] = streams[short_at][:keep * cases[short_at].srb + 5]  # two rows and five bytes
    c0 = cases[short_at]
    cases[short_at] = F.Case(c0.name + " decoded short", c0.b, c0.s, c0.reverse, c0.stored, c0.rows, c0.srb, c0.window,
                             src_len=len(streams[short_at]), status=F.E_TRUNCATED, d0=keep)
    b = F.batch(cases)
    zs = [zlib.compress(s, 6) for s in streams]
    pad = lambda a: (a + np.uint64(15)) & ~np.uint64(15)  # noqa: E731
    in_len, cap = np.array([len(z) for z in zs], np.uint64), np.array([c.rows * c.srb for c in cases], np.uint64)
    in_off = np.zeros(n, np.uint64)
    in_off[1:] = np.cumsum(pad(in_len))[:-1]
    dec_off = b.desc["src_off"].astype(np.uint64)  # the decode delivers where the batch has its sources, at every misalignment
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    t = [_up(a) for a in (h_in, in_off, in_len, dec_off, cap, b.desc)]
    p = [x.data_ptr() for x in t]
    d_dec = torch.full((len(b.src) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((len(b.dst_want),), F.FILL, dtype=torch.uint8, device="cuda")
    d_out_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.decompress_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_out_len.data_ptr(), d_st.data_ptr(), 0, 0, 0, n, sync=False)
    gpu_ctx.unshuffle_many_device(d_dec.data_ptr(), d_out_len.data_ptr(), d_dst.data_ptr(), p[5], d_st.data_ptr() + 4 * n, d_detail.data_ptr(), n, sync=False)
    gpu_ctx.sync()
    st = d_st.cpu().numpy()
    assert (st[:n] == 0).all()
    assert np.array_equal(d_out_len.cpu().numpy().view(np.uint64), np.array([len(s) for s in streams], np.uint64))
    check(b, (d_dst.cpu().numpy(), st[n:], d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)))
    assert int(st[n + short_at]) == F.E_TRUNCATED and gpu_ctx.last_kernel_ms() > 0.0
