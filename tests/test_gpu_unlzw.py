"""GPU: pzg_unlzw_many against the table decoder of tests/lzwcases.py, byte for byte: the cases the CPU model runs
(tests/test_model_unlzw.py), laid out with the streams at every input alignment and the outputs off the 16-byte boundaries over a 0xCD
prefill that is checked everywhere nothing is delivered -- through host pointers and device pointers, in one batch and alone, and as
the decode in front of a stage."""
import numpy as np
import pytest

import lzwcases as L

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(torch.device("cuda", 0))


def run_host(ctx, b, ec):
    in_buf, in_off, in_len, nout, out_off, out_cap = b[:6]
    out = np.full(nout, L.FILL, np.uint8)
    out_len, status, detail = ctx.unlzw_many(in_buf, in_off, in_len, out, out_off, out_cap, early_change=bool(ec))
    return out, out_len, status, detail


def run_device(ctx, b, ec, sync=True):
    import torch
    in_buf, in_off, in_len, nout, out_off, out_cap = b[:6]
    n = len(in_off)
    t = [_up(a) for a in (in_buf, in_off, in_len, out_off, out_cap)]
    d_out = torch.full((nout,), L.FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.unlzw_many_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d_out.data_ptr(), t[3].data_ptr(), t[4].data_ptr(), d_len.data_ptr(),
                          d_status.data_ptr(), d_detail.data_ptr(), n, early_change=bool(ec), sync=sync)
    if not sync:
        ctx.sync()
    return d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint64), d_status.cpu().numpy(), d_detail.cpu().numpy().view(np.uint32).reshape(n, 2)


def check(cases, b, got):
    out, out_len, status, detail = got
    want_out, want_len, want_status, want_detail = b[6:]
    for i, c in enumerate(cases):
        assert (int(status[i]), int(out_len[i]), int(detail[i, 0]), int(detail[i, 1])) == (c.status, len(c.out), c.d0, c.d1), c.name
    diff = np.flatnonzero(out != want_out)
    assert len(diff) == 0, (int(diff[0]), [c.name for c, o in zip(cases, b[4]) if int(o) <= int(diff[0])][-1])


def _by_mode():
    return [(ec, [c for c in L.all_cases() if c.early_change == ec]) for ec in (1, 0)]


def test_every_case_on_device_pointers(gpu_ctx):
    for ec, cases in _by_mode():
        assert len(cases) > 30
        for order in (cases, cases[::-1]):  # (every case at another layout)
            b = L.batch(order)
            check(order, b, run_device(gpu_ctx, b, ec))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_both_pointer_forms_give_the_same(gpu_ctx):
    for ec, cases in _by_mode():
        b = L.batch(cases)
        host, device = run_host(gpu_ctx, b, ec), run_device(gpu_ctx, b, ec, sync=False)
        check(cases, b, host)
        check(cases, b, device)
        assert all(np.array_equal(x, y) for x, y in zip(host, device))
    assert gpu_ctx.last_kernel_ms() > 0.0


def test_streams_alone(gpu_ctx):
    by = {c.name: c for c in L.all_cases()}
    for name in ("zeros 40000", "random cleared ec 1", "text table stays full", "f + 1", "cut at 17", "empty input", "empty input, no room",
                 "zeros cap 2017 (a string crosses it)", "garbage behind the capacity", "clear every 127 (zeros)"):
        c = by[name]
        b = L.batch([c])
        check([c], b, run_device(gpu_ctx, b, c.early_change))
        check([c], b, run_host(gpu_ctx, b, c.early_change))


def test_many_streams_in_one_launch(gpu_ctx):
    cases = [c for c in L.all_cases() if c.early_change == 1 and c.cap <= 3000] * 40
    assert len(cases) > 4096
    b = L.batch(cases)
    check(cases, b, run_device(gpu_ctx, b, 1))


def test_bad_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    cases = [c for c in L.all_cases() if c.name in ("text cap 700", "f + 1", "period 3 ec 1")]
    assert len(cases) == 3
    b = L.batch(cases)
    Lb, h = _ffi.lib(), gpu_ctx.handle
    out = np.full(b[3], L.FILL, np.uint8)
    out_len, status, detail = np.zeros(3, np.uint64), np.zeros(3, np.int32), np.zeros(6, np.uint32)

    def call(n=3, mode=1, flags=0, in_off=True, in_len=True, out_off=True, out_cap=b[5], ol=True, st=True):
        p = lambda a, on=True: a.ctypes.data if on else None  # noqa: E731
        return Lb.pzg_unlzw_many(h, p(b[0]), p(b[1], in_off), p(b[2], in_len), p(out), p(b[4], out_off), p(out_cap), p(out_len, ol), p(status, st),
                                 p(detail), n, mode, flags)
    assert call(n=0) == _ffi.RC_BAD_ARG and call(flags=_ffi.GZIP) == _ffi.RC_BAD_ARG and call(flags=_ffi.ASYNC) == _ffi.RC_BAD_ARG
    assert call(mode=2) == _ffi.RC_BAD_ARG and call(mode=3) == _ffi.RC_BAD_ARG
    for kw in ("in_off", "in_len", "out_off", "ol", "st"):
        assert call(**{kw: False}) == _ffi.RC_BAD_ARG, kw
    big = b[5].copy()
    big[1] = 1 << 32
    assert call(out_cap=big) == _ffi.RC_BAD_ARG  # (positions are 32-bit)
    assert (out == L.FILL).all()
    assert call() == _ffi.RC_OK
    assert np.array_equal(out, b[6]) and np.array_equal(status, b[8]) and np.array_equal(out_len, b[7]) and np.array_equal(detail.reshape(3, 2), b[9])


def test_async_chain_in_front_of_a_stage(gpu_ctx):
    """pzg_unlzw_many -> pzg_unpredict_many -> pzg_sync with the LZW call's out_len as the stage's src_len: one stream ends (EOI) two
    rows early, and that job alone is PZG_E_TRUNCATED with the rows it has."""
    import torch
    from pure_zlib_amd.zlib import UNPREDICT_DESC
    rng = np.random.default_rng(5)
    rows, srb, n = 9, 40, 6
    tiles = [rng.integers(0, 4, size=(rows, srb), dtype=np.uint8) for _ in range(n)]
    streams = [L.encode(t.tobytes() if i != 2 else t[:7].tobytes()) for i, t in enumerate(tiles)]
    in_len = np.array([len(s) for s in streams], np.uint64)
    in_off = np.zeros(n, np.uint64)
    in_off[1:] = np.cumsum((in_len + np.uint64(15)) & ~np.uint64(15))[:-1]
    h_in = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for o, s in zip(in_off.tolist(), streams):
        h_in[o:o + len(s)] = np.frombuffer(s, np.uint8)
    cap = np.full(n, rows * srb, np.uint64)
    dec_off = np.arange(n, dtype=np.uint64) * np.uint64(rows * srb + 24) + np.uint64(3)
    desc = np.zeros(n, UNPREDICT_DESC)
    desc["src_off"], desc["dst_off"], desc["dst_stride"], desc["src_row_bytes"], desc["rows"] = dec_off, np.arange(n) * rows * srb, srb, srb, rows
    desc["win_rows"], desc["win_bytes"], desc["predictor"], desc["sample_bytes"], desc["samples"] = rows, srb, 1, 1, 1
    t = [_up(a) for a in (h_in, in_off, in_len, dec_off, cap, desc)]
    p = [x.data_ptr() for x in t]
    d_dec = torch.full((n * (rows * srb + 24) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((n * rows * srb,), L.FILL, dtype=torch.uint8, device="cuda")
    d_out_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_st = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    d_detail = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.unlzw_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_out_len.data_ptr(), d_st.data_ptr(), 0, n, sync=False)
    gpu_ctx.unpredict_many_device(d_dec.data_ptr(), d_out_len.data_ptr(), d_dst.data_ptr(), p[5], d_st.data_ptr() + 4 * n, d_detail.data_ptr(), n, sync=False)
    gpu_ctx.sync()
    st = d_st.cpu().numpy()
    assert (st[:n] == 0).all() and d_out_len.cpu().numpy().tolist() == [rows * srb if i != 2 else 7 * srb for i in range(n)]
    assert st[n:].tolist() == [0, 0, L.E_TRUNCATED, 0, 0, 0]
    got = d_dst.cpu().numpy().reshape(n, rows, srb)
    for i, tile in enumerate(tiles):
        if i != 2:
            assert np.array_equal(got[i], tile), i
        else:
            assert np.array_equal(got[i][:7], tile[:7]) and (got[i][7:] == L.FILL).all()
