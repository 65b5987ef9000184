"""GPU: what the host launcher's one-lane calls (pure_zlib_amd/csrc/pzg_api.cpp: LaneCall, copy_back_windows, extents_ok /
dict_extents_ok) owe their callers beside the decoded bytes, which the other GPU tests check: a kernel span after every call
(pzg_last_kernel_ms -- the benches under tests/tools/ read it), the front of a short window's slot left alone, and refusals that
touch nothing.  Expected bytes come from system zlib and the host models, never from the library."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest

import corpus
import indexcheck as X
import memberscheck as M
import scancheck as S
from test_gpu_indexed import index_build
from test_gpu_members import _arrays, find_members, gzip_layout
from test_gpu_scan import index_scan

pytestmark = pytest.mark.gpu

W = X.WINDOW
SPAN = 4096  # the smallest span of tests/test_gpu_indexed.py
DEVICE_PTRS, RAW = 1, 32


def many(ctx, segments, device, z, zdict, cap):
    """One stream with host or device pointers: through pzg_decompress_many_dict (a zlib stream and its preset dictionary), or through
    pzg_decompress_many_segments (a raw stream as ONE segment: start bit 0, to the final block).  -> (rc, status, out_len, the bytes)"""
    from pure_zlib_amd import _ffi
    u64 = lambda v: np.array([v], dtype=np.uint64)  # noqa: E731
    host = [np.frombuffer(z + bytes(16), dtype=np.uint8).copy(), u64(0), u64(len(z)), np.zeros(1, np.uint8), u64(0),
            np.frombuffer(zdict + bytes(16), dtype=np.uint8).copy(), u64(0), u64(len(zdict)), np.full(cap + 64, 0xCD, np.uint8), u64(0), u64(cap),
            u64(0), np.full(1, -1, np.int32), np.zeros(2, np.uint32), u64(0), np.zeros(1, np.uint32)]
    p, fetch = _arrays(device, host)
    flags = DEVICE_PTRS if device else 0
    if segments:
        rc = _ffi.lib().pzg_decompress_many_segments(ctx.handle, *p, 1, flags)
    else:
        rc = _ffi.lib().pzg_decompress_many_dict(ctx.handle, p[0], p[1], p[2], *p[5:], 1, flags)
    got = fetch()
    assert (got[8][cap:] == 0xCD).all(), "written past the capacity"
    return rc, int(got[12][0]), int(got[11][0]), got[8][:cap].tobytes()


def device_many(ctx, z, cap):
    """One zlib stream through a device-pointer pzg_decompress_many -> (status, out_len)"""
    import torch
    dev = torch.device("cuda", 0)
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    t_in = torch.from_numpy(np.frombuffer(z + bytes(16), dtype=np.uint8).copy()).to(dev)
    t_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    in_off, in_len, out_off, out_cap, out_len, in_used = i64(0), i64(len(z)), i64(0), i64(cap), i64(0), i64(0)
    status, adler, detail = (torch.full((k,), -1, dtype=torch.int32, device=dev) for k in (1, 1, 2))
    torch.cuda.synchronize()
    ctx.decompress_many_device(t_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), t_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(),
                               out_len.data_ptr(), status.data_ptr(), detail.data_ptr(), in_used.data_ptr(), adler.data_ptr(), 1, sync=True)
    return int(status.cpu()[0]), int(out_len.cpu()[0])


@pytest.fixture(scope="module")
def inputs():
    """One stream of a few hundred KiB -- raw, and as a zlib stream with a preset dictionary -- and a gzip file of four small members."""
    text = corpus.zipf_text(300 << 10, 21)
    zdict = corpus.zipf_text(20000, 22)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict)
    members = b"".join(M.gz(corpus.zipf_text(3000 + 700 * k, 30 + k)) for k in range(4))
    return dict(text=text, raw=X.raw_of(text), zdict=zdict, with_dict=co.compress(text) + co.flush(), members=members,
                found=M.MembersModel().find(members, 256))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("call", ["index_build", "index_scan", "find_members", "layout", "dict", "segments"])
def test_kernel_span_after_every_call(gpu_ctx, inputs, call, device):
    """A context that has launched nothing reports -1; after ONE call it reports that call's kernel span, finite and above zero (no
    bound on the value: the benches only need it to be there); after a device-pointer pzg_decompress_many, that launch's."""
    import pure_zlib_amd as P
    text, raw = inputs["text"], inputs["raw"]
    n, starts, _bsize = inputs["found"]
    assert n == 4
    with P.Context(0) as ctx:
        assert ctx.last_kernel_ms() == -1.0
        if call == "index_build":
            st, out_len, _used, adler, _n, _out, _pts, _win = index_build(ctx, raw, len(text), 65536, 16, device)
            assert (st, out_len, adler) == (0, len(text), zlib.adler32(text))
        elif call == "index_scan":
            rc, st, _det, out_len, _used, _n, _pts, _win = index_scan(ctx, raw, 16384, 65536, 16, device)
            assert (rc, st, out_len) == (0, 0, len(text))
        elif call == "find_members":
            rc, got_n, got_starts, _b = find_members(ctx, inputs["members"], 0, 8, device)
            assert (rc, got_n) == (0, 4) and got_starts[:4].tolist() == starts
        elif call == "layout":
            rc, total, _rows = gzip_layout(ctx, inputs["members"], starts, 0, device)
            assert (rc, total) == (0, M.MembersModel().layout(inputs["members"], starts, 0)[4])
        elif call == "dict":
            assert many(ctx, False, device, inputs["with_dict"], inputs["zdict"], len(text)) == (0, 0, len(text), text)
        else:
            assert many(ctx, True, device, raw, b"", len(text)) == (0, 0, len(text), text)
        ms = ctx.last_kernel_ms()
        assert math.isfinite(ms) and ms > 0.0, (call, device, ms)
        assert device_many(ctx, zlib.compress(text, 6), len(text)) == (0, len(text))
        ms = ctx.last_kernel_ms()
        assert math.isfinite(ms) and ms > 0.0, (call, device, "device-pointer launch", ms)


@pytest.fixture(scope="module")
def blocks():
    """(raw stream, data): some 140 KiB in 400 small blocks -- at span 4096 several points below 32768 and many above.  The data is
    system zlib's reading of the stream."""
    data, d = X.tiny_blocks()
    assert zlib.decompressobj(-15).decompress(d) == data and 100 << 10 < len(data) < 200 << 10
    return d, data


@pytest.mark.parametrize("which", ["index_build", "index_scan"])
def test_short_windows_leave_the_front_of_their_slot_alone(gpu_ctx, blocks, which):
    """Host pointers, the windows buffer pre-filled with a pattern: a point below 32768 gets out_pos bytes at the END of its slot and the
    front keeps the pattern; the slots from 32768 on are the 32 KiB before their point; the slot behind the last one keeps the pattern.
    The points are the host model's (tests/model/model_seg.cpp, model_scan.cpp), the bytes system zlib's."""
    L = gpu_ctx._L
    d, data = blocks
    if which == "index_build":
        r, _out, n, want = X.SegModel().build(d, len(data), SPAN)
        assert r.status == 0 and n == len(want)
    else:
        res = S.ScanModel().scan(d, 1024, SPAN, 256)
        assert res["status"] == 0
        n, want = res["npoints"], res["points"]
    short = [k for k, (_bit, pos) in enumerate(want) if pos < W]
    assert len(short) >= 1 and n - len(short) >= 2 and short == list(range(len(short)))
    pattern = (np.arange((n + 1) * W) % 251).astype(np.uint8)
    win, pts = pattern.copy(), np.zeros((n, 2), dtype=np.uint64)
    buf = np.frombuffer(d, dtype=np.uint8).copy()
    npoints, status, out_len = C.c_uint32(0), C.c_int32(-1), C.c_uint64(0)
    if which == "index_build":
        out = np.zeros(len(data), dtype=np.uint8)
        rc = L.pzg_index_build(gpu_ctx.handle, buf.ctypes.data, len(d), out.ctypes.data, len(data), SPAN, pts.ctypes.data, n, C.byref(npoints),
                               win.ctypes.data, C.byref(out_len), C.byref(status), None, None, None, 0)
    else:
        rc = L.pzg_index_scan(gpu_ctx.handle, buf.ctypes.data, len(d), 1024, SPAN, pts.ctypes.data, n, C.byref(npoints), win.ctypes.data,
                              C.byref(out_len), C.byref(status), None, None, 0)
    assert (rc, status.value, out_len.value, npoints.value) == (0, 0, len(data), n)
    assert [tuple(int(x) for x in p) for p in pts] == want
    for k, (_bit, pos) in enumerate(want):
        slot, w = win[k * W:(k + 1) * W], min(pos, W)
        assert (slot[:W - w] == pattern[k * W:(k + 1) * W - w]).all(), (k, pos, "front of the slot")
        assert slot[W - w:].tobytes() == data[pos - w:pos], (k, pos)
    assert (win[n * W:] == pattern[n * W:]).all(), "behind the last slot"


def test_refused_extents_touch_nothing(gpu_ctx):
    """Each refusal of extents_ok / dict_extents_ok, through pzg_decompress_many_dict and through pzg_decompress_many_segments, host
    pointers: PZG_RC_BAD_ARG, and the output and result arrays as they were.  (tests/test_gpu_api.py test_argument_validation has the
    wrapped input extent and the missing output pointer through pzg_decompress_many, by their return codes alone.)"""
    from pure_zlib_amd import _ffi
    L = gpu_ctx._L
    data = b"abc" * 100
    u64 = lambda v: np.array([v], dtype=np.uint64)  # noqa: E731
    refusals = {"in_off + in_len wraps": dict(in_off=u64(2**64 - 8), in_len=u64(64)),
                "out_cap has bit 40": dict(out_cap=u64(1 << 40)),
                "dict_off + dict_len wraps": dict(dict_off=u64(2**64 - 8), dict_len=u64(64)),
                "dict_len has bit 32": dict(dict_len=u64(1 << 32)),
                "out_cap without out_base": dict(out=None)}
    for segments in (False, True):
        z = X.raw_of(data) if segments else zlib.compress(data)
        buf = np.frombuffer(z + bytes(16), dtype=np.uint8).copy()

        def call(**change):
            a = dict(in_off=u64(0), in_len=u64(len(z)), dict_off=u64(0), dict_len=u64(0), out=np.full(512, 0xCD, np.uint8), out_cap=u64(300))
            a.update(change)
            res = [u64(0xCDCD), np.full(1, -1, np.int32), np.full(2, 0xCDCD, np.uint32), u64(0xCDCD), np.full(1, 0xCDCD, np.uint32)]
            before = [r.copy() for r in res]
            p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
            start_bit, end_bit, out_off = np.zeros(1, np.uint8), u64(0), u64(0)
            seg = [p(start_bit), p(end_bit)] if segments else []
            tail = [p(buf), p(a["dict_off"]), p(a["dict_len"]), p(a["out"]), p(out_off), p(a["out_cap"])] + [p(r) for r in res] + [1, 0]
            rc = (L.pzg_decompress_many_segments if segments else L.pzg_decompress_many_dict)(gpu_ctx.handle, p(buf), p(a["in_off"]), p(a["in_len"]), *seg, *tail)
            untouched = all((r == b).all() for r, b in zip(res, before)) and (a["out"] is None or (a["out"] == 0xCD).all())
            return rc, untouched, res, a["out"]
        rc, _untouched, res, out = call()
        assert rc == 0 and res[1][0] == 0 and res[0][0] == 300 and out[:300].tobytes() == data and (out[300:] == 0xCD).all(), segments
        for what, change in refusals.items():
            rc, untouched, _res, _out = call(**change)
            assert rc == _ffi.RC_BAD_ARG and untouched, (what, "segments" if segments else "dict", rc)
