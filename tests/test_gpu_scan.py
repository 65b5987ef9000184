"""GPU: the parallel index scan -- pzg_index_scan (include/pzg.h; pure_zlib_amd/csrc/scan_core.h) and Index.build_parallel.  What the
device finds must be the host model's (tests/model/model_scan.cpp) bit for bit, which the CPU suite checks against a plain-Python
finder and system zlib (tests/test_model_scan.py); the mirror must return what Index.build returns."""
import ctypes as C
import zlib

import numpy as np
import pytest

import indexcheck as X
import scancheck as S

pytestmark = pytest.mark.gpu

W = X.WINDOW
CHUNKS = [1024, 16384]
SPAN = 4096
DEVICE_PTRS = 1


@pytest.fixture(scope="module")
def ins():
    body, data, _bit = S.false_candidate_stream(1024)
    return X.big_inputs() + [("false_candidate", body, data)]


@pytest.fixture(scope="module")
def model(ins):
    """(name, chunk) -> the host model's scan."""
    m = S.ScanModel()
    return {(name, chunk): m.scan(d, chunk, SPAN, 256) for name, d, _data in ins for chunk in CHUNKS}


def index_scan(ctx, d, chunk, span, max_points, device, flags=0):
    """pzg_index_scan with host or device pointers, a guard slot behind the points and the windows, 0xCD everywhere.
    -> (rc, status, detail, out_len, in_used, npoints, points incl. guard slot, windows incl. guard slot)"""
    import torch
    from pure_zlib_amd import _ffi
    h_in = np.frombuffer(d, dtype=np.uint8).copy()
    h_pts = np.full((max_points + 1, 2), 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
    h_win = np.full((max_points + 1, W), 0xCD, dtype=np.uint8)
    if device:
        dev = torch.device("cuda", 0)
        t_in, t_pts, t_win = torch.from_numpy(h_in).to(dev), torch.from_numpy(h_pts.view(np.int64)).to(dev), torch.from_numpy(h_win).to(dev)
        torch.cuda.synchronize()
        ptrs = (t_in.data_ptr(), t_pts.data_ptr(), t_win.data_ptr())
    else:
        ptrs = (h_in.ctypes.data, h_pts.ctypes.data, h_win.ctypes.data)
    npoints, status, out_len, in_used = C.c_uint32(0), C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
    detail = (C.c_uint32 * 2)(0, 0)
    rc = _ffi.lib().pzg_index_scan(ctx.handle, ptrs[0], len(d), chunk, span, ptrs[1], max_points, C.byref(npoints), ptrs[2], C.byref(out_len),
                                   C.byref(status), detail, C.byref(in_used), (DEVICE_PTRS if device else 0) | flags)
    if device:
        torch.cuda.synchronize()
        h_pts, h_win = t_pts.cpu().numpy().view(np.uint64), t_win.cpu().numpy()
    return rc, status.value, (detail[0], detail[1]), out_len.value, in_used.value, npoints.value, h_pts, h_win


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_scan_on_the_device(gpu_ctx, ins, model, device):
    for name, d, data in ins:
        for chunk in CHUNKS:
            want = model[name, chunk]
            assert (want["status"], want["out_len"], want["in_used"]) == (0, len(data), len(d)), (name, chunk)
            n = want["npoints"]
            rc, st, _det, out_len, in_used, got_n, pts, win = index_scan(gpu_ctx, d, chunk, SPAN, n + 2, device)
            what = (name, chunk, device)
            assert (rc, st, out_len, in_used, got_n) == (0, 0, len(data), len(d), n), what
            assert [tuple(int(x) for x in p) for p in pts[:n]] == want["points"], what  # EQUAL to the host model's
            assert (pts[n:] == 0xCDCDCDCDCDCDCDCD).all() and (win[n:] == 0xCD).all(), what
            for k, (_bit, pos) in enumerate(want["points"]):
                w = min(pos, W)
                assert win[k, W - w:].tobytes() == want["windows"][k][W - w:].tobytes() == data[pos - w:pos], what + (k,)
                assert (win[k, :W - w] == 0xCD).all(), what + (k, "front of the slot")
        # more points than room: the full count, the first two stored, nothing behind them touched
        want = model[name, 1024]
        if want["npoints"] > 2:
            rc, st, _det, out_len, _used, got_n, pts, win = index_scan(gpu_ctx, d, 1024, SPAN, 2, device)
            assert (rc, st, out_len, got_n) == (0, 0, len(data), want["npoints"]), (name, device)
            assert [tuple(int(x) for x in p) for p in pts[:2]] == want["points"][:2] and (pts[2:] == 0xCDCDCDCDCDCDCDCD).all() and (win[2:] == 0xCD).all()
    assert any(model[name, 1024]["npoints"] > 2 for name, _d, _x in ins)  # (the over-capacity case ran)


def test_false_candidate_is_found_and_skipped(gpu_ctx, ins, model):
    name, d, data = ins[-1]
    want = model[name, 1024]
    assert want["cand"][1] == 8 * 1024 and want["next"][1] & S.NEXT_FAIL and all(b != 8 * 1024 for b, _p in want["points"])


def wrap(kind, d, data):
    if kind == "zlib":
        return b"\x78\x9c" + d + zlib.adler32(data).to_bytes(4, "big")
    if kind == "gzip":
        return b"\x1f\x8b\x08\x08" + bytes(6) + b"name\0" + d + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xffffffff).to_bytes(4, "little")
    return d


@pytest.mark.parametrize("kind", ["zlib", "gzip", "raw"])
def test_build_parallel(gpu_ctx, ins, model, kind, tmp_path, monkeypatch):
    from pure_zlib_amd.indexed import Index

    def no_fallback(*a, **k):
        raise AssertionError("build_parallel fell back to the sequential build on a sound stream")
    for name, d, data in (ins[0], ins[4], ins[6]) if kind != "zlib" else ins:
        z = wrap(kind, d, data)
        seq_ix, seq = Index.build(z, kind, span=SPAN, ctx=gpu_ctx)
        for chunk in CHUNKS:
            with monkeypatch.context() as mp:  # the parallel path itself: the sequential build is out of reach while it runs
                mp.setattr(Index, "build", staticmethod(no_fallback))
                ix, r = Index.build_parallel(z, kind, span=SPAN, chunk=chunk, ctx=gpu_ctx)
            assert r.is_right() and seq.is_right() and r.value == seq.value == data, (kind, name, chunk)
            # its points are the scan's -- the host model's for this chunk, in general not build()'s
            assert [tuple(int(x) for x in p) for p in ix.points] == model[name, chunk]["points"], (kind, name, chunk)
            assert (ix.out_len, ix.body_off, ix.body_len, ix.expect, ix.fingerprint) == (seq_ix.out_len, seq_ix.body_off, seq_ix.body_len,
                                                                                         seq_ix.expect, seq_ix.fingerprint), (kind, name, chunk)
            pts = [tuple(int(x) for x in p) for p in ix.points]
            assert all(b - a >= SPAN for a, b in zip([0] + [p for _b, p in pts], [p for _b, p in pts])), (kind, name, chunk)
            for off, ln in ((0, 10), (len(data) // 2 - 5, 70000), (len(data) - 33, 100), (4095, 2)):
                assert ix.read(z, off, ln, ctx=gpu_ctx) == data[off:off + ln], (kind, name, chunk, off)
        ix.save(tmp_path / "a.pzi")
        ix = Index.load(tmp_path / "a.pzi")
        r = ix.decompress(z, ctx=gpu_ctx)
        assert r.is_right() and r.value == data, (kind, name)


def test_broken_streams_report_what_build_reports(gpu_ctx, ins):
    from pure_zlib_amd.indexed import Index
    name, d, data = ins[0]
    z = wrap("zlib", d, data)
    flipped = z[:-1] + bytes([z[-1] ^ 1])
    cases = [("truncated", z[:len(z) * 2 // 3]), ("flipped trailer", flipped), ("no trailer", z[:-4])]
    for what, bad in cases:
        ix, r = Index.build_parallel(bad, "zlib", span=SPAN, chunk=1024, ctx=gpu_ctx)
        six, s = Index.build(bad, "zlib", span=SPAN, ctx=gpu_ctx)
        assert ix is None and six is None and not r.is_right() and not s.is_right(), what
        assert type(r.value) is type(s.value) and r.value.show() == s.value.show(), (what, r.value.show(), s.value.show())
    # the scan itself on the truncated body: PZG_E_SCAN, d0 = PZG_E_TRUNCATED, d1 = the start bit of a segment the model has too
    cut = d[:len(d) * 2 // 3]
    want = S.ScanModel().scan(cut, 1024, SPAN, 64)
    for device in (False, True):
        rc, st, det, _ol, _used, _n, _pts, _win = index_scan(gpu_ctx, cut, 1024, SPAN, 64, device)
        assert (rc, st, det) == (0, S.E_SCAN, (S.E_TRUNCATED, want["d1"])) and want["status"] == S.E_SCAN, (device, st, det)


def test_cli_parallel_round_trip(gpu_ctx, ins, tmp_path, capsysbinary, monkeypatch):
    """deflate --index FILE --parallel NAME, then --use-index [--range], in this process, on the default context."""
    from pure_zlib_amd import deflate_cli
    from pure_zlib_amd.indexed import Index
    name, d, data = ins[0]
    (tmp_path / "big.z").write_bytes(wrap("zlib", d, data))
    monkeypatch.chdir(tmp_path)
    def no_fallback(*a, **k):
        raise AssertionError("--parallel went through the sequential build")
    with monkeypatch.context() as mp:  # (--parallel is build_parallel, and that does not fall back on a sound file)
        mp.setattr(Index, "build", staticmethod(no_fallback))
        assert deflate_cli.main(["--index", "big.pzi", "--parallel", "big.z"]) == 0 and (tmp_path / "big").read_bytes() == data
    (tmp_path / "big").unlink()
    assert deflate_cli.main(["--use-index", "big.pzi", "big.z"]) == 0 and (tmp_path / "big").read_bytes() == data
    capsysbinary.readouterr()
    assert deflate_cli.main(["--use-index", "big.pzi", "--range", "100000:300", "big.z"]) == 0
    assert capsysbinary.readouterr().out == data[100000:100300]


def test_rejected_arguments(gpu_ctx, ins):
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    name, d, data = ins[0]
    ok = index_scan(gpu_ctx, d, 0, 0, 8, False)  # chunk 0: 128 KiB, span 0: 1 MiB -- one segment, no points
    assert ok[:6] == (0, 0, (0, 0), len(data), len(d), 0)
    assert index_scan(gpu_ctx, d, 256, SPAN, 64, False)[:2] == (0, 0)
    assert index_scan(gpu_ctx, d, 255, SPAN, 8, False)[0] == _ffi.RC_BAD_ARG
    for flags in (_ffi.GZIP, _ffi.HOST_PINNED, 2, _ffi.CRC32):
        assert index_scan(gpu_ctx, d, 1024, SPAN, 8, False, flags)[0] == _ffi.RC_BAD_ARG, flags
    two = P.Context(devices=[0, 0])
    try:
        assert index_scan(two, d, 1024, SPAN, 8, False)[0] == _ffi.RC_BAD_ARG
    finally:
        two.close()
    msg = C.create_string_buffer(128)
    _ffi.lib().pzg_error_message(None, 0, S.E_SCAN, (C.c_uint32 * 2)(1, 0), msg, 128)
    assert msg.value == b"Format error: the chain of blocks did not reach the final block"
