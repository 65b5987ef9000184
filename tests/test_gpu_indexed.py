"""GPU: one large stream, indexed -- pzg_index_build and pzg_decompress_many_segments (include/pzg.h) and their mirror
(pure_zlib_amd/indexed.py).  The index the device builds must be the host model's (tests/model/model_seg.cpp), which the CPU suite
checks against system zlib alone (tests/test_model_segments.py); every segment must decode to its slice of zlib's output."""
import ctypes as C
import gzip
import random
import zlib

import numpy as np
import pytest

import indexcheck as X

pytestmark = pytest.mark.gpu

W = X.WINDOW
SPANS = [4096, 65536]
DEVICE_PTRS, ASYNC, LPT_ORDER, CRC32 = 1, 2, 8, 64


@pytest.fixture(scope="module")
def ins():
    return X.big_inputs()


@pytest.fixture(scope="module")
def model_points(ins):
    """(name, span) -> the host model's points."""
    m = X.SegModel()
    got = {}
    for name, d, data in ins:
        for span in SPANS:
            r, _out, n, pts = m.build(d, len(data), span)
            assert r.status == 0 and n == len(pts)
            got[name, span] = pts
    assert all(len(got[name, 4096]) >= 3 for name, _d, _x in ins)
    return got


def index_build(ctx, d, cap, span, max_points, device):
    """pzg_index_build with host or device pointers: 0xCD guards behind the output's capacity, a guard slot behind the points and the
    windows.  -> (status, out_len, in_used, adler, npoints, out bytes incl. guard, points incl. guard slot, windows incl. guard slot)"""
    import torch
    from pure_zlib_amd import _ffi
    h_in = np.frombuffer(d, dtype=np.uint8).copy()
    h_out = np.full(cap + 64, 0xCD, dtype=np.uint8)
    h_pts = np.full((max_points + 1, 2), 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
    h_win = np.full((max_points + 1, W), 0xCD, dtype=np.uint8)
    if device:
        dev = torch.device("cuda", 0)
        t_in, t_out = torch.from_numpy(h_in).to(dev), torch.from_numpy(h_out).to(dev)
        t_pts, t_win = torch.from_numpy(h_pts.view(np.int64)).to(dev), torch.from_numpy(h_win).to(dev)
        torch.cuda.synchronize()
        ptrs = (t_in.data_ptr(), t_out.data_ptr(), t_pts.data_ptr(), t_win.data_ptr())
    else:
        ptrs = (h_in.ctypes.data, h_out.ctypes.data, h_pts.ctypes.data, h_win.ctypes.data)
    npoints, status, adler, out_len, in_used = C.c_uint32(0), C.c_int32(-1), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    detail = (C.c_uint32 * 2)(0, 0)
    _ffi.check(_ffi.lib().pzg_index_build(ctx.handle, ptrs[0], len(d), ptrs[1], cap, span, ptrs[2], max_points, C.byref(npoints), ptrs[3],
                                          C.byref(out_len), C.byref(status), detail, C.byref(in_used), C.byref(adler), DEVICE_PTRS if device else 0),
               ctx.handle)
    if device:
        torch.cuda.synchronize()
        h_out, h_pts, h_win = t_out.cpu().numpy(), t_pts.cpu().numpy().view(np.uint64), t_win.cpu().numpy()
    return status.value, out_len.value, in_used.value, adler.value, npoints.value, h_out, h_pts, h_win


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_build_on_the_device(gpu_ctx, ins, model_points, device):
    import pure_zlib_amd as P
    for name, d, data in ins:
        (today,), (crc,) = P.raw_decompress_many([d], [len(data)], crc32=True, ctx=gpu_ctx)  # what PZG_RAW gives today
        assert today.is_right() and today.value == data and crc == zlib.crc32(data)
        for span in SPANS:
            want = model_points[name, span]
            st, out_len, in_used, adler, n, out, pts, win = index_build(gpu_ctx, d, len(data), span, len(want) + 5, device)
            what = (name, span, device)
            assert (st, out_len, in_used, adler) == (0, len(data), len(d), zlib.adler32(data)), what
            assert out[:len(data)].tobytes() == today.value and (out[len(data):] == 0xCD).all(), what
            assert n == len(want) and [tuple(int(x) for x in p) for p in pts[:n]] == want, what  # EQUAL to the host model's
            assert (pts[n:] == 0xCDCDCDCDCDCDCDCD).all() and (win[n:] == 0xCD).all(), what
            for k, (_bit, pos) in enumerate(want):
                w = min(pos, W)
                assert win[k, W - w:].tobytes() == data[pos - w:pos], what + (k,)
                assert (win[k, :W - w] == 0xCD).all(), what + (k, "front of the slot")
        # more points than room: the full count, the first three stored, nothing behind them touched
        want = model_points[name, 4096]
        room = 3 if len(want) > 3 else len(want) - 1  # (two of the text streams are three blocks and a final one: room for 2 there)
        st, out_len, _used, _adler, n, out, pts, win = index_build(gpu_ctx, d, len(data), 4096, room, device)
        assert (st, out_len, n) == (0, len(data), len(want)) and n > room, (name, device)
        assert [tuple(int(x) for x in p) for p in pts[:room]] == want[:room] and (pts[room:] == 0xCDCDCDCDCDCDCDCD).all() and (win[room:] == 0xCD).all()
        assert all(win[k, W - min(p, W):].tobytes() == data[p - min(p, W):p] for k, (_b, p) in enumerate(want[:room]))
        # too little room for the output: the size needed, nothing past the capacity
        st, out_len, _used, _adler, n, out, pts, win = index_build(gpu_ctx, d, len(data) - 1, 4096, 8, device)
        assert (st, out_len) == (14, len(data)) and (out[len(data) - 1:] == 0xCD).all(), (name, device)


class SegBatch:
    """One device-pointer pzg_decompress_many_segments launch.  items: (input bytes, start_bit, end_bit, window, capacity); the outputs lie
    back to back in the items' order -- one contiguous buffer -- between two 64-byte margins of 0xCD."""
    MARGIN = 64

    def __init__(self, items):
        import torch
        self.torch, self.n = torch, len(items)
        dev = torch.device("cuda", 0)
        in_len = np.array([len(it[0]) for it in items], dtype=np.int64)
        d_len = np.array([len(it[3]) for it in items], dtype=np.int64)
        self.cap = np.array([it[4] for it in items], dtype=np.int64)
        in_off = np.concatenate(([0], np.cumsum(in_len[:-1])))
        d_off = np.concatenate(([0], np.cumsum(d_len[:-1])))
        self.out_off = self.MARGIN + np.concatenate(([0], np.cumsum(self.cap[:-1])))
        self.total = int(self.cap.sum())
        as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.t = dict(
            inp=as_dev(np.frombuffer(b"".join(it[0] for it in items) + bytes(16), dtype=np.uint8).copy()), in_off=as_dev(in_off), in_len=as_dev(in_len),
            start=as_dev(np.array([it[1] for it in items], dtype=np.uint8)), end=as_dev(np.array([it[2] for it in items], dtype=np.int64)),
            dic=as_dev(np.frombuffer(b"".join(it[3] for it in items) + bytes(16), dtype=np.uint8).copy()), d_off=as_dev(d_off), d_len=as_dev(d_len),
            out=torch.full((self.total + 2 * self.MARGIN,), 0xCD, dtype=torch.uint8, device=dev), out_off=as_dev(self.out_off), cap=as_dev(self.cap),
            out_len=torch.zeros(self.n, dtype=torch.int64, device=dev), status=torch.full((self.n,), -1, dtype=torch.int32, device=dev),
            detail=torch.zeros(2 * self.n, dtype=torch.int32, device=dev), in_used=torch.zeros(self.n, dtype=torch.int64, device=dev),
            sums=torch.zeros(self.n, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()

    def run(self, ctx, flags=0, sync=True):
        from pure_zlib_amd import _ffi
        t = self.t
        t["out"].fill_(0xCD)
        t["status"].fill_(-1)
        self.torch.cuda.synchronize()
        p = lambda k: t[k].data_ptr()  # noqa: E731
        _ffi.check(_ffi.lib().pzg_decompress_many_segments(
            ctx.handle, p("inp"), p("in_off"), p("in_len"), p("start"), p("end"), p("dic"), p("d_off"), p("d_len"), p("out"), p("out_off"), p("cap"),
            p("out_len"), p("status"), p("detail"), p("in_used"), p("sums"), self.n, DEVICE_PTRS | flags | (0 if sync else ASYNC)), ctx.handle)
        if not sync:
            ctx.sync()
        self.torch.cuda.synchronize()
        out = t["out"].cpu().numpy()
        assert (out[:self.MARGIN] == 0xCD).all() and (out[self.MARGIN + self.total:] == 0xCD).all(), "written outside the buffer"
        return (out[self.MARGIN:self.MARGIN + self.total], t["status"].cpu().numpy(), t["out_len"].cpu().numpy(), t["in_used"].cpu().numpy(),
                t["sums"].cpu().numpy().view(np.uint32), t["detail"].cpu().numpy().view(np.uint32).reshape(-1, 2))


def seg_items(d, data, pts):
    return [(d[off:off + ln], sb, eb, data[max(0, a - W):a], b - a) for off, ln, sb, eb, a, b in X.segments(pts, len(d), len(data))]


def test_all_segments_in_one_launch(gpu_ctx, ins, model_points):
    from pure_zlib_amd.indexed import adler32_combine, crc32_combine
    try:
        for name, d, data in ins:
            items = seg_items(d, data, model_points[name, 4096])
            fwd, rev = SegBatch(items), SegBatch(items[::-1])
            for rb in (11, 15):
                gpu_ctx.set_ring_bits(rb)
                for flags, sync in ((0, True), (CRC32, True), (LPT_ORDER, False), (LPT_ORDER | CRC32, True)):
                    out, st, out_len, in_used, sums, _det = fwd.run(gpu_ctx, flags, sync)
                    what = (name, rb, flags)
                    assert (st == 0).all() and (out_len == fwd.cap).all() and (in_used == [len(it[0]) for it in items]).all(), what
                    assert out.tobytes() == data, what  # one contiguous buffer: the whole stream
                    total = 0 if flags & CRC32 else 1
                    for k, it in enumerate(items):
                        total = (crc32_combine if flags & CRC32 else adler32_combine)(total, int(sums[k]), it[4])
                    assert total == (zlib.crc32(data) if flags & CRC32 else zlib.adler32(data)), what
                out, st, out_len, _used, sums, _det = rev.run(gpu_ctx, 0)
                assert (st == 0).all() and (out_len == rev.cap).all(), (name, rb, "reversed")
                at = 0
                for k, (off, ln, sb, eb, a, b) in enumerate(X.segments(model_points[name, 4096], len(d), len(data))[::-1]):
                    assert out[at:at + b - a].tobytes() == data[a:b] and int(sums[k]) == zlib.adler32(data[a:b]), (name, rb, "reversed", k)
                    at += b - a
    finally:
        gpu_ctx.set_ring_bits(11)


def test_one_mixed_launch(gpu_ctx, ins, model_points):
    """Segments of all six streams in one launch, more of them than the chip holds stream-waves of the 32 KiB ring (1,024): the work
    counter wraps onto waves that have already decoded a segment with another dictionary, another code, another start bit."""
    once = []
    for name, d, data in ins:
        once += [(it, data[a:b]) for it, (_o, _l, _s, _e, a, b) in zip(seg_items(d, data, model_points[name, 4096]),
                                                                      X.segments(model_points[name, 4096], len(d), len(data)))]
    reps = -(-1100 // len(once))
    order = list(range(len(once))) * reps
    random.Random(4).shuffle(order)
    assert len(order) >= 1100 and len({once[k][0][1] for k in order}) == 8  # every start bit
    batch = SegBatch([once[k][0] for k in order])
    out, st, out_len, _used, sums, _det = batch.run(gpu_ctx, LPT_ORDER)
    assert (st == 0).all() and (out_len == batch.cap).all()
    assert out.tobytes() == b"".join(once[k][1] for k in order)
    adlers = {k: zlib.adler32(once[k][1]) for k in set(order)}
    assert [int(s) for s in sums] == [adlers[k] for k in order]


def test_errors_beside_good_segments(gpu_ctx, ins, model_points):
    """The error cases of the CPU suite (tests/indexcheck.py error_cases) in one batch with the stream's good segments: each as the host
    model has it, the good ones unaffected, nothing written outside an extent that the neighbours' bytes would not show."""
    m = X.SegModel()
    for name, d, data in ins:
        pts = model_points[name, 4096]
        cases, (a, b, la, lb) = X.error_cases(d, data, pts)
        good = seg_items(d, data, pts)
        segs = X.segments(pts, len(d), len(data))
        items, kinds = [], []
        for k, g in enumerate(good):  # the error cases between the good segments
            items.append(g)
            kinds.append(("good", k))
            for c in range(k, len(cases), len(good)):
                what, inp, sb, eb, win, cap, ok = cases[c]
                items.append((inp, sb, eb, win, cap))
                kinds.append(("bad", c))
        assert sum(1 for kd in kinds if kd[0] == "bad") == len(cases) == 6
        out, st, out_len, _used, sums, det = SegBatch(items).run(gpu_ctx, 0)
        at = 0
        for j, ((kind, k), it) in enumerate(zip(kinds, items)):
            mine = out[at:at + it[4]].tobytes()
            at += it[4]
            if kind == "good":
                _o, _l, _s, _e, ga, gb = segs[k]
                assert (int(st[j]), int(out_len[j]), int(sums[j])) == (0, gb - ga, zlib.adler32(data[ga:gb])) and mine == data[ga:gb], (name, "good", k)
                continue
            what, inp, sb, eb, win, cap, ok = cases[k]
            assert st[j] != 0 and ok(int(st[j]), int(det[j, 0]), int(out_len[j])), (name, what, int(st[j]), det[j].tolist(), int(out_len[j]))
            r, mout = m.segment(inp, sb, eb, win, cap)
            assert (int(st[j]), int(out_len[j]), int(sums[j])) == (r.status, r.out_len, r.adler), (name, what, int(st[j]), r.status)
            assert (int(det[j, 0]), int(det[j, 1])) == (r.detail0, r.detail1), (name, what)
            n = min(r.out_len, cap)
            base = la if what == "beyond the final block" else a
            if r.status != X.E_OUT_TOO_SMALL:
                assert mine[:n] == mout == data[base:base + n], (name, what)


def test_rejected_arguments(gpu_ctx):
    from pure_zlib_amd import _ffi
    L = _ffi.lib()
    d = X.raw_of(b"abc" * 100)
    buf = np.frombuffer(d, dtype=np.uint8).copy()
    out = np.zeros(512, dtype=np.uint8)
    u64 = lambda v: np.array([v], dtype=np.uint64)  # noqa: E731
    res = dict(out_len=u64(0), status=np.zeros(1, np.int32), detail=np.zeros(2, np.uint32), in_used=u64(0), adler=np.zeros(1, np.uint32))

    def call(start, end, flags, in_len=len(d)):
        sb = np.array([start], dtype=np.uint8)
        a = [buf, u64(0), u64(in_len), sb, u64(end), buf, u64(0), u64(0), out, u64(0), u64(300)] + list(res.values())
        return L.pzg_decompress_many_segments(gpu_ctx.handle, *[x.ctypes.data for x in a], 1, flags)
    assert call(0, 0, 0) == 0 and res["status"][0] == 0 and out[:300].tobytes() == b"abc" * 100
    assert call(8, 0, 0) == _ffi.RC_BAD_ARG and call(0, 8 * len(d) + 1, 0) == _ffi.RC_BAD_ARG
    assert call(0, 0, _ffi.GZIP) == _ffi.RC_BAD_ARG and call(0, 0, _ffi.HOST_PINNED) == _ffi.RC_BAD_ARG and call(0, 0, ASYNC) == _ffi.RC_BAD_ARG
    n, st, ol = C.c_uint32(0), C.c_int32(-1), C.c_uint64(0)
    for flags in (_ffi.GZIP, _ffi.HOST_PINNED, ASYNC, CRC32):
        assert L.pzg_index_build(gpu_ctx.handle, buf.ctypes.data, len(d), out.ctypes.data, 300, 0, None, 0, C.byref(n), None, C.byref(ol), C.byref(st),
                                 None, None, None, flags) == _ffi.RC_BAD_ARG
    assert L.pzg_index_build(gpu_ctx.handle, buf.ctypes.data, len(d), out.ctypes.data, 300, 0, None, 0, C.byref(n), None, C.byref(ol), C.byref(st),
                             None, None, None, 0) == 0 and (st.value, ol.value, n.value) == (0, 300, 0)
    buf2 = L.pzg_error_message(None, 0, 21, None, C.create_string_buffer(8), 0)
    msg = C.create_string_buffer(128)
    L.pzg_error_message(None, 0, 21, (C.c_uint32 * 2)(2, 77), msg, 128)
    assert buf2 == 0 and msg.value == b"Format error: segment does not end on its block boundary" == L.pzg_strerror(21)


def wrap(kind, d, data):
    if kind == "zlib":
        return b"\x78\x9c" + d + zlib.adler32(data).to_bytes(4, "big")
    if kind == "gzip":
        return b"\x1f\x8b\x08\x08" + bytes(6) + b"name\0" + d + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xffffffff).to_bytes(4, "little")
    return d


@pytest.mark.parametrize("kind", ["zlib", "gzip", "raw"])
def test_through_the_mirror(gpu_ctx, ins, model_points, kind, tmp_path):
    from pure_zlib_amd.indexed import Index
    from pure_zlib_amd.zlib import DecompressionError
    rng = random.Random(8)
    for name, d, data in (ins[0], ins[4]) if kind != "zlib" else ins:
        z = wrap(kind, d, data)
        if kind == "gzip":
            assert gzip.decompress(z) == data
        ix, r = Index.build(z, kind, span=4096, ctx=gpu_ctx)
        assert r.is_right() and r.value == data and [tuple(int(x) for x in p) for p in ix.points] == model_points[name, 4096], (kind, name)
        ix.save(tmp_path / "a.pzi")
        ix = Index.load(tmp_path / "a.pzi")
        r = ix.decompress(z, ctx=gpu_ctx)
        assert r.is_right() and r.value == data, (kind, name)
        ranges = [(0, 1), (0, len(data)), (len(data) - 77, 77), (len(data) - 1, 1), (5000, 0), (len(data), 10), (int(ix.points[2, 1]) + 3, 50),
                  (int(ix.points[1, 1]), int(ix.points[2, 1] - ix.points[1, 1])), (int(ix.points[0, 1]) - 1, 2)]
        ranges += [(rng.randrange(len(data)), rng.choice([1, 100, 5000, 70000])) for _ in range(11)]
        assert len(ranges) == 20
        for off, ln in ranges:
            assert ix.read(z, off, ln, ctx=gpu_ctx) == data[off:off + ln], (kind, name, off, ln)
        # a flipped trailer byte: the reference's ChecksumError text, from the build pass (zlib) and from decompress()
        if kind != "raw":
            bad = z[:-8 if kind == "gzip" else -4] + bytes([z[-8 if kind == "gzip" else -4] ^ 0x40]) + z[-7 if kind == "gzip" else -3:]
            theirs = int.from_bytes(bad[-4:], "big") if kind == "zlib" else int.from_bytes(bad[-8:-4], "little")
            ours = zlib.adler32(data) if kind == "zlib" else zlib.crc32(data)
            text = "Checksum error: checksum mismatch: %x != %x" % (theirs, ours)
            r = ix.decompress(bad, ctx=gpu_ctx)
            assert not r.is_right() and r.value.constructor == "ChecksumError" and r.value.show() == text, (kind, name, r)
            if kind == "zlib":
                none, r = Index.build(bad, kind, span=4096, ctx=gpu_ctx)
                assert none is None and not r.is_right() and r.value.show() == text
        # a zeroed window: the segment decodes, to other bytes -- the combined checksum says so
        iz = Index.load(tmp_path / "a.pzi")
        if name in ("text6", "text1", "fixed", "tiny400"):  # (streams whose segments do reach back into their windows)
            assert iz.windows[1].any()
            iz.windows[1] = 0
            r = iz.decompress(z, ctx=gpu_ctx)
            assert not r.is_right() and r.value.constructor == "ChecksumError" and r.value.show().startswith("Checksum error: checksum mismatch: "), (kind, name, r)
        # points shifted by one bit: an error, never wrong bytes as a Right
        for delta in (1, -1):
            iy = Index.load(tmp_path / "a.pzi")
            iy.points[:, 0] = (iy.points[:, 0].astype(np.int64) + delta).astype(np.uint64)
            r = iy.decompress(z, ctx=gpu_ctx)
            assert not r.is_right(), (kind, name, delta)
            with pytest.raises(DecompressionError):
                iy.read(z, int(iy.points[1, 1]) + 1, 10, ctx=gpu_ctx)
        # the index of another file
        other = wrap(kind, d[:-1] + bytes([d[-1] ^ 1]), data)
        r = ix.decompress(other, ctx=gpu_ctx)
        assert not r.is_right() and r.value.show() == "Decompression error: index does not match the stream"
    if kind == "gzip":  # a second member is refused
        name, d, data = ins[0]
        z = wrap(kind, d, data)
        none, r = Index.build(z + z, kind, span=4096, ctx=gpu_ctx)
        assert none is None and not r.is_right() and "second member" in r.value.show()


def test_cli_index_round_trip(gpu_ctx, ins, tmp_path, capsysbinary, monkeypatch):
    """deflate --index / --use-index [--range] in this process, on the default context."""
    from pure_zlib_amd import deflate_cli
    name, d, data = ins[0]
    (tmp_path / "big.z").write_bytes(wrap("zlib", d, data))
    monkeypatch.chdir(tmp_path)
    assert deflate_cli.main(["--index", "big.pzi", "big.z"]) == 0 and (tmp_path / "big").read_bytes() == data
    (tmp_path / "big").unlink()
    assert deflate_cli.main(["--use-index", "big.pzi", "big.z"]) == 0 and (tmp_path / "big").read_bytes() == data
    capsysbinary.readouterr()
    assert deflate_cli.main(["--use-index", "big.pzi", "--range", "100000:300", "big.z"]) == 0
    assert capsysbinary.readouterr().out == data[100000:100300]
