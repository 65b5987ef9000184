"""GPU: a gzip file of many members -- pzg_gzip_find_members / pzg_gzip_layout (include/pzg.h; pure_zlib_amd/csrc/member_core.h) and
the mirror pure_zlib_amd/gzfile.py.  What the device finds and lays out must be the host model's (tests/model/model_members.cpp) bit
for bit, which the CPU suite checks against plain Python and numpy (tests/test_model_members.py); decompress_gzip_file must return
what gzip_decompress_many([data])[0] returns, for sound files and for broken ones."""
import ctypes as C
import gzip

import numpy as np
import pytest

import memberscheck as M

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
CHUNKS = (64, 4096, 0)


@pytest.fixture(scope="module")
def model():
    return M.MembersModel()


@pytest.fixture(scope="module")
def sound():
    return M.sound_files()


def _arrays(device, host):
    """The arrays as the call wants them: (pointers, fetch) -- fetch() brings them back as numpy arrays."""
    if not device:
        return [h.ctypes.data for h in host], lambda: host
    import torch
    dev = torch.device("cuda", 0)
    ts = [torch.from_numpy(h.view(np.int64) if h.dtype == np.uint64 else h.view(np.int32) if h.dtype == np.uint32 else h).to(dev) for h in host]
    torch.cuda.synchronize()

    def fetch():
        torch.cuda.synchronize()
        return [t.cpu().numpy().view(h.dtype) for t, h in zip(ts, host)]
    return [t.data_ptr() for t in ts], fetch


def find_members(ctx, d, chunk, room, device, flags=0):
    """pzg_gzip_find_members with one guard slot behind the room, 0xCD everywhere -> (rc, count, starts, bsize) incl. the guard slots."""
    from pure_zlib_amd import _ffi
    h_in = np.frombuffer(d + b"\0", dtype=np.uint8).copy()
    host = [h_in, np.full(room + 1, M.GUARD64, dtype=np.uint64), np.full(room + 1, M.GUARD32, dtype=np.uint32)]
    ptrs, fetch = _arrays(device, host)
    n = C.c_uint32(0)
    rc = _ffi.lib().pzg_gzip_find_members(ctx.handle, ptrs[0], len(d), chunk, ptrs[1], ptrs[2], room, C.byref(n), (DEVICE_PTRS if device else 0) | flags)
    _in, starts, bsize = fetch()
    return rc, n.value, starts, bsize


def gzip_layout(ctx, d, starts, base, device, flags=0, m=None):
    """pzg_gzip_layout with a guard slot behind each of the four arrays -> (rc, total, [in_off, in_len, out_off, out_cap])."""
    from pure_zlib_amd import _ffi
    m = len(starts) if m is None else m
    h_in = np.frombuffer(d + b"\0", dtype=np.uint8).copy()
    host = [h_in, np.array(list(starts) + [0], dtype=np.uint64)] + [np.full(len(starts) + 1, M.GUARD64, dtype=np.uint64) for _ in range(4)]
    ptrs, fetch = _arrays(device, host)
    total = C.c_uint64(0)
    rc = _ffi.lib().pzg_gzip_layout(ctx.handle, ptrs[0], len(d), ptrs[1], m, base, ptrs[2], ptrs[3], ptrs[4], ptrs[5], C.byref(total),
                                    (DEVICE_PTRS if device else 0) | flags)
    return rc, total.value, fetch()[2:]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_finder_and_layout_on_the_device(gpu_ctx, model, sound, device):
    for name, z in [(name, z) for name, z, _d, _f in sound] + M.finder_files():
        n, starts, bsize = model.find(z, 256)
        for chunk in CHUNKS:
            rc, got_n, got_starts, got_bsize = find_members(gpu_ctx, z, chunk, n, device)
            what = (name, chunk, device)
            assert (rc, got_n) == (0, n) and got_starts[:n].tolist() == starts and got_bsize[:n].tolist() == bsize, what
            assert got_starts[n] == M.GUARD64 and got_bsize[n] == M.GUARD32, what
        for base in (0, 1 << 33):
            want = model.layout(z, starts, base)
            rc, total, got = gzip_layout(gpu_ctx, z, starts, base, device)
            assert (rc, total) == (0, want[4]), (name, device)
            for w, g in zip(want[:4], got):
                assert np.array_equal(w, g[:n]) and g[n] == M.GUARD64, (name, device, base)
    # more members than room: the full count, the first ones stored, nothing behind them touched
    z = [f for f in sound if f[0] == "thirty-seven"][0][1]
    n, starts, bsize = model.find(z, 256)
    for room in (0, 5):
        rc, got_n, got_starts, got_bsize = find_members(gpu_ctx, z, 64, room, device)
        assert (rc, got_n) == (0, n) and got_starts[:room].tolist() == starts[:room] and got_bsize[:room].tolist() == bsize[:room]
        assert (got_starts[room:] == M.GUARD64).all() and (got_bsize[room:] == M.GUARD32).all()


def test_many_members_on_the_device(gpu_ctx, model):
    """More members than a tile of the prefix sums, more chunks than one, a sum of rooms past 2^32: equal to the model's."""
    one = M.gz(b"") + M.wrap(M.stored(b"x" * 3), b"x" * 3)
    big = M.BARE_HEADER + M.stored(b"") + bytes(4200000) + (0xfffffff0).to_bytes(4, "little")
    z = one * 5000 + big + big
    n, starts, bsize = model.find(z, 4096)
    assert n == 10002
    rc, got_n, got_starts, got_bsize = find_members(gpu_ctx, z, 64, n, True)
    assert (rc, got_n) == (0, n) and got_starts[:n].tolist() == starts and got_bsize[:n].tolist() == bsize
    want = model.layout(z, starts, 7)
    rc, total, got = gzip_layout(gpu_ctx, z, starts, 7, True)
    assert (rc, total) == (0, want[4]) and total > 1 << 32
    for w, g in zip(want[:4], got):
        assert np.array_equal(w, g[:n])


@pytest.mark.parametrize("ring", [11, 15])
def test_sound_files(gpu_ctx, sound, ring):
    import pure_zlib_amd as P
    gpu_ctx.set_ring_bits(ring)
    try:
        for name, z, d, _false in sound:
            for chunk in (None, 64):
                r = P.decompress_gzip_file(z, ctx=gpu_ctx, chunk=chunk)
                assert r.is_right() and r.value == d == gzip.decompress(z), (name, ring, chunk)
            assert r == P.gzip_decompress_many([z], ctx=gpu_ctx)[0], (name, ring)
    finally:
        gpu_ctx.set_ring_bits(11)


class Counted:
    """gzfile's launches counted."""

    def __init__(self, mp):
        from pure_zlib_amd import gzfile
        self.n, real = 0, gzfile._launch

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        mp.setattr(gzfile, "_launch", counted)


def no_one_stream(mp):
    import pure_zlib_amd.zlib as Z

    def refuse(*a, **k):
        raise AssertionError("the file went to the one-stream decode")
    mp.setattr(Z, "gzip_decompress_many", refuse)


def test_the_parallel_path_does_the_work(gpu_ctx, sound, monkeypatch):
    """With the one-stream decode out of reach: the sound files without false candidates in ONE launch, the two with one false
    candidate each in two (one drop)."""
    import pure_zlib_amd as P
    no_one_stream(monkeypatch)
    for name, z, d, false in sound:
        assert false in (0, 1), name
        c = Counted(monkeypatch)
        index, r = P.decompress_gzip_file(z, ctx=gpu_ctx, return_index=True)
        assert r.is_right() and r.value == d and c.n == 1 + false, (name, c.n)
        assert len(index.starts) == M.count_members(z) and index.out_len == len(d), name
    assert sum(f[3] for f in sound) == 2


def broken_files(sound):
    """[(name, file)]: decided with the oracle on the CPU (test_broken_files_report_what_the_one_stream_decode_reports)."""
    z = [f for f in sound if f[0] == "thirty-seven"][0][1]
    starts = [s for s in M.find(z)[0]]
    assert len(starts) == 37
    cut = (starts[3] + starts[4]) // 2
    flip = lambda at: z[:at] + bytes([z[at] ^ 0x55]) + z[at + 1:]
    return [("truncated in member 3", z[:cut]),
            ("flipped CRC in member 2", flip(starts[3] - 8)),
            ("flipped ISIZE in member 5", flip(starts[6] - 4)),
            ("zero padding between members", z[:starts[4]] + bytes(512) + z[starts[4]:]),
            ("garbage behind the last member", z + b"\x00\x01garbage, not a member" * 3),
            ("two-byte magic then garbage behind the last member", z + b"\x1f\x8b\x07\x00" + bytes(20)),
            ("bad first magic", b"\x1f\x8c" + z[2:]),
            ("empty file", b"")]


def test_broken_files_report_what_the_one_stream_decode_reports(gpu_ctx, sound, oracle):
    import pure_zlib_amd as P
    z = [f for f in sound if f[0] == "thirty-seven"][0]
    starts = M.find(z[1])[0]
    expected = {"truncated in member 3": "Left", "flipped CRC in member 2": "Left", "flipped ISIZE in member 5": "Left",
                "zero padding between members": len(gzip.decompress(z[1][:starts[4]])), "garbage behind the last member": len(z[2]),
                "two-byte magic then garbage behind the last member": "Left", "bad first magic": "Left", "empty file": "Left"}
    for name, bad in broken_files(sound):
        res, out = oracle.gzip_decompress(bad, 1 << 20)
        want = P.gzip_decompress_many([bad], ctx=gpu_ctx)[0]
        got = P.decompress_gzip_file(bad, ctx=gpu_ctx)
        if expected[name] == "Left":
            assert res.status != 0 and not want.is_right() and not got.is_right(), name
            assert got.value.show() == want.value.show() == res.message.decode(), (name, got.value.show(), want.value.show())
        else:
            assert res.status == 0 and len(out) == expected[name], name
            assert got.is_right() and want.is_right() and got.value == want.value == out, name
            index, r = P.decompress_gzip_file(bad, ctx=gpu_ctx, return_index=True)
            assert r == got and index.decompress(bad, ctx=gpu_ctx) == got, name


def test_member_index(gpu_ctx, sound, tmp_path):
    import pure_zlib_amd as P
    name, z, d, _f = [f for f in sound if f[0] == "thirty-seven"][0]
    index, r = P.decompress_gzip_file(z, ctx=gpu_ctx, return_index=True)
    assert r.value == d and index.starts.tolist() == M.find(z)[0]
    offs = index.offsets.tolist()
    assert offs[-1] == len(d) and offs == sorted(offs)
    edge = offs[10]
    cases = [(offs[2] + 7, 100), (edge, 50), (edge - 1, 2), (offs[20] - 5, offs[23] - offs[20] + 10), (0, len(d)), (len(d) - 3, 100), (len(d), 5), (5, 0)]
    for off, ln in cases:
        assert index.read(z, off, ln, ctx=gpu_ctx) == d[off:off + ln], (off, ln)
    index.save(tmp_path / "a.pzm")
    loaded = P.MemberIndex.load(tmp_path / "a.pzm")
    assert loaded.starts.tolist() == index.starts.tolist() and loaded.offsets.tolist() == offs and loaded.fingerprint == index.fingerprint
    assert loaded.decompress(z, ctx=gpu_ctx) == P.Right(d) and loaded.read(z, edge, 9, ctx=gpu_ctx) == d[edge:edge + 9]
    other = [f for f in sound if f[0] == "bgzf"][0][1]
    r = loaded.decompress(other, ctx=gpu_ctx)
    assert not r.is_right() and r.value.show() == "Decompression error: index does not match the stream"
    with pytest.raises(P.DecompressionError):
        loaded.read(other, 0, 10, ctx=gpu_ctx)


def test_cli_round_trip(gpu_ctx, sound, tmp_path, capsys, monkeypatch):
    """deflate --members NAME.gz, in this process, on the default context."""
    from pure_zlib_amd import deflate_cli
    name, z, d, _f = [f for f in sound if f[0] == "member-inside"][0]
    (tmp_path / "big.gz").write_bytes(z)
    (tmp_path / "bad.gz").write_bytes(z[:len(z) // 2])
    monkeypatch.chdir(tmp_path)
    assert deflate_cli.main(["--members", "big.gz"]) == 0 and (tmp_path / "big").read_bytes() == d
    capsys.readouterr()
    assert deflate_cli.main(["--members", "bad.gz"]) == 0 and not (tmp_path / "bad").exists()
    assert capsys.readouterr().out.startswith("ERROR: ")
    assert deflate_cli.main(["--members", "big.z"]) == 0 and capsys.readouterr().out == "Unexpected file name.\n"


def test_rejected_arguments(gpu_ctx, sound):
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    z = sound[1][1]
    starts = M.find(z)[0]
    assert len(starts) == 2
    assert find_members(gpu_ctx, z, 64, 4, False)[:2] == (0, 2)
    assert find_members(gpu_ctx, z, 63, 4, False)[0] == _ffi.RC_BAD_ARG
    assert gzip_layout(gpu_ctx, z, starts, 0, False)[0] == 0
    assert gzip_layout(gpu_ctx, z, starts, 0, False, m=0)[0] == _ffi.RC_BAD_ARG
    assert gzip_layout(gpu_ctx, z, starts[::-1], 0, False)[0] == _ffi.RC_BAD_ARG          # descending
    assert gzip_layout(gpu_ctx, z, [0, len(z) + 1], 0, False)[0] == _ffi.RC_BAD_ARG       # beyond the input
    assert gzip_layout(gpu_ctx, z, [0, len(z)], 0, False)[0] == 0                         # (at its end: an empty last extent)
    for flags in (_ffi.GZIP, _ffi.HOST_PINNED, _ffi.ASYNC, _ffi.RAW):
        assert find_members(gpu_ctx, z, 64, 4, False, flags)[0] == _ffi.RC_BAD_ARG, flags
        assert gzip_layout(gpu_ctx, z, starts, 0, False, flags)[0] == _ffi.RC_BAD_ARG, flags
    two = P.Context(devices=[0, 0])
    try:
        assert find_members(two, z, 64, 4, False)[0] == _ffi.RC_BAD_ARG
        assert gzip_layout(two, z, starts, 0, False)[0] == _ffi.RC_BAD_ARG
    finally:
        two.close()
    with pytest.raises(ValueError):
        P.decompress_gzip_file(z, ctx=gpu_ctx, chunk=63)
