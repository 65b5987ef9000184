"""GPU: pzg_index_scan_many (include/pzg.h; pure_zlib_amd/csrc/scan_core.h ScanMany) -- many raw streams scanned in one call, a
wavefront per chunk over all of them.  The contract is per stream: every stream's results, points and windows are what the host model
of the one-stream scan (tests/model/model_scan.cpp, which the CPU suite checks against a plain-Python finder and system zlib) gives for
that stream alone, and nothing outside a stream's own slots is written."""
import ctypes as C

import numpy as np
import pytest

import indexcheck as X
import scancheck as S
import scanmanycheck as SM

pytestmark = pytest.mark.gpu

W = SM.W
CHUNKS = [1024, 16384]
SPAN = 4096
DEVICE_PTRS = 1


@pytest.fixture(scope="module")
def batch():
    sound = X.big_inputs()
    return SM.Batch([(name, d, None) for name, d, _data in sound] + SM.extra_cases(sound, CHUNKS))


@pytest.fixture(scope="module")
def refs(batch):
    """chunk -> [the host model's scan of every stream alone]"""
    m = S.ScanModel()
    return {chunk: SM.reference(m, batch, chunk, SPAN) for chunk in CHUNKS}


def scan_many(ctx, packed, in_off, in_len, point_off, chunk, span, device, flags=0, guard=1):
    """pzg_index_scan_many with host or device pointers; `guard` more slots behind the last stream's, 0xCD everywhere.
    -> (rc, results [dict], points incl. guard slots, windows incl. guard slots)"""
    import torch
    from pure_zlib_amd import _ffi
    n = len(in_off)
    in_off, in_len = np.ascontiguousarray(in_off, dtype=np.uint64), np.ascontiguousarray(in_len, dtype=np.uint64)
    point_off = np.ascontiguousarray(point_off, dtype=np.uint32)
    slots = int(point_off[-1]) + guard
    h_in = np.frombuffer(packed, dtype=np.uint8).copy()
    h_pts = np.full((slots, 2), SM.FILL64, dtype=np.uint64)
    h_win = np.full((slots, W), SM.FILL, dtype=np.uint8)
    if device:
        dev = torch.device("cuda", 0)
        t_in, t_pts, t_win = torch.from_numpy(h_in).to(dev), torch.from_numpy(h_pts.view(np.int64)).to(dev), torch.from_numpy(h_win).to(dev)
        torch.cuda.synchronize()
        ptrs = (t_in.data_ptr(), t_pts.data_ptr(), t_win.data_ptr())
    else:
        ptrs = (h_in.ctypes.data, h_pts.ctypes.data, h_win.ctypes.data)
    npoints, status = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    out_len, in_used = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    detail = np.zeros((n, 2), dtype=np.uint32)
    rc = _ffi.lib().pzg_index_scan_many(ctx.handle, ptrs[0], in_off.ctypes.data, in_len.ctypes.data, n, chunk, span, ptrs[1], point_off.ctypes.data,
                                        npoints.ctypes.data, ptrs[2], out_len.ctypes.data, status.ctypes.data, detail.ctypes.data,
                                        in_used.ctypes.data, (DEVICE_PTRS if device else 0) | flags)
    if device:
        torch.cuda.synchronize()
        h_pts, h_win = t_pts.cpu().numpy().view(np.uint64), t_win.cpu().numpy()
    results = [dict(status=int(status[i]), d0=int(detail[i, 0]), d1=int(detail[i, 1]), npoints=int(npoints[i]), out_len=int(out_len[i]),
                    in_used=int(in_used[i])) for i in range(n)]
    return rc, results, h_pts, h_win


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_stream_is_its_own_scan(gpu_ctx, batch, refs, device):
    for chunk in CHUNKS:
        want = refs[chunk]
        point_off = batch.point_off(want)
        rc, results, pts, win = scan_many(gpu_ctx, batch.packed, batch.in_off, batch.in_len, point_off, chunk, SPAN, device)
        assert rc == 0, (chunk, device)
        failed = 0
        for i, ref in enumerate(want):
            lo, hi = int(point_off[i]), int(point_off[i + 1])
            what = (batch.names[i], chunk, device)
            if ref["status"] != 0:  # its result block; with host pointers a failed stream's slots are left alone, as pzg_index_scan leaves them
                failed += 1
                assert {f: results[i][f] for f in SM.RESULT_FIELDS} == {f: ref[f] for f in SM.RESULT_FIELDS}, what
                if not device:
                    SM.check_stream(what, ref, results[i], pts[lo:hi], win[lo:hi], stored=False)
                continue
            SM.check_stream(what, ref, results[i], pts[lo:hi], win[lo:hi])
        assert (pts[int(point_off[-1]):] == SM.FILL64).all() and (win[int(point_off[-1]):] == SM.FILL).all(), (chunk, device)
        at = {name: i for i, name in enumerate(batch.names)}
        assert failed == 2 and want[at["cut"]]["d0"] == S.E_TRUNCATED  # (the empty stream and the truncated one)
        assert want[at["two_slots"]]["npoints"] > 2 or chunk != 1024


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_stream_is_pzg_index_scan(gpu_ctx, batch, device):
    from test_gpu_scan import index_scan
    for name in ("text6", "tiny400", "cut"):
        d = batch.streams[batch.names.index(name)]
        for chunk in CHUNKS:
            rc1, st, det, out_len, in_used, n, pts1, win1 = index_scan(gpu_ctx, d, chunk, SPAN, 40, device)
            rc, res, pts, win = scan_many(gpu_ctx, d, [0], [len(d)], [0, 40], chunk, SPAN, device)
            assert (rc, rc1) == (0, 0) and res[0] == dict(status=st, d0=det[0], d1=det[1], npoints=n, out_len=out_len, in_used=in_used), (name, chunk)
            assert (pts == pts1).all() and (win == win1).all(), (name, chunk, device)
            assert (st == 0) == (name != "cut")


def test_seventy_streams(gpu_ctx, batch, refs):
    """More streams than a wave has lanes: the binary search and the per-stream walk past the 64th."""
    order = [i % batch.n for i in range(70)]
    many = SM.Batch([(batch.names[i] + "_%d" % k, batch.streams[i], batch.rooms[i]) for k, i in enumerate(order)])
    want = SM.reference(S.ScanModel(), many, 1024, SPAN)
    point_off = many.point_off(want)
    rc, results, pts, win = scan_many(gpu_ctx, many.packed, many.in_off, many.in_len, point_off, 1024, SPAN, True)
    assert rc == 0 and many.n == 70
    for i, ref in enumerate(want):
        lo, hi = int(point_off[i]), int(point_off[i + 1])
        if ref["status"] == 0:
            SM.check_stream((many.names[i],), ref, results[i], pts[lo:hi], win[lo:hi])
        else:
            assert {f: results[i][f] for f in SM.RESULT_FIELDS} == {f: ref[f] for f in SM.RESULT_FIELDS}, many.names[i]
    assert sum(r["status"] == 0 for r in want[64:]) >= 4


def test_context_wrapper(gpu_ctx, batch, refs):
    want = refs[1024]
    point_off = batch.point_off(want)
    buf = np.frombuffer(batch.packed, dtype=np.uint8)
    pts, win, npoints, out_len, status, detail, in_used = gpu_ctx.index_scan_many(buf, batch.in_off, batch.in_len, point_off, 1024, SPAN)
    for i, ref in enumerate(want):
        got = (int(status[i]), int(detail[i, 0]), int(detail[i, 1]), int(npoints[i]), int(out_len[i]), int(in_used[i]))
        assert got == tuple(ref[f] for f in SM.RESULT_FIELDS), batch.names[i]
        if ref["status"] == 0:
            lo = int(point_off[i])
            assert [tuple(int(x) for x in p) for p in pts[lo:lo + len(ref["points"])]] == ref["points"], batch.names[i]


def test_rejected_arguments(gpu_ctx, batch):
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    d = batch.streams[0]
    two_off, two_len = [0, 0], [len(d), len(d)]
    run = lambda ctx=gpu_ctx, off=two_off, ln=two_len, po=(0, 8, 16), chunk=1024, flags=0, packed=d: \
        scan_many(ctx, packed, off, ln, list(po), chunk, SPAN, False, flags)[0]
    assert run() == 0 and run(chunk=0) == 0 and run(chunk=256) == 0 and run(flags=_ffi.RAW) == 0
    assert run(off=[], ln=[], po=(0,)) == _ffi.RC_BAD_ARG  # n == 0
    for flags in (_ffi.GZIP, _ffi.HOST_PINNED, _ffi.ASYNC, _ffi.CRC32, _ffi.LPT_ORDER):
        assert run(flags=flags) == _ffi.RC_BAD_ARG, flags
    two = P.Context(devices=[0, 0])
    try:
        assert run(ctx=two) == _ffi.RC_BAD_ARG
    finally:
        two.close()
    assert run(chunk=255) == _ffi.RC_BAD_ARG
    assert run(ln=[len(d), 1 << 34]) == _ffi.RC_BAD_ARG  # (rejected before anything is read)
    assert run(po=(0, 8, 7)) == _ffi.RC_BAD_ARG and run(po=(9, 8, 16)) == _ffi.RC_BAD_ARG
    # 70 streams of 2^34 - 1 bytes at chunk 256: 70 x 2^26 chunks
    assert run(off=[0] * 70, ln=[(1 << 34) - 1] * 70, po=range(71), chunk=256) == _ffi.RC_BAD_ARG
