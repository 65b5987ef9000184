"""GPU: PZG_RAW (bare RFC 1951 streams) and PZG_CRC32 through pzg_decompress_many on every path that takes flags, against system
zlib and the oracle on the wrapped stream (tests/rawcheck.py); the ZIP reader (pure_zlib_amd/zip.py) against the stdlib's."""
import ctypes as C
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

import corpus
import rawcheck
from devbatch import DeviceBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    return rawcheck.stream_pool()


def _caps(oracle, pool):
    """A capacity per stream: exact for most, generous, one short, zero -- cycling."""
    caps = []
    for k, (_name, d) in enumerate(pool):
        wrapped, _e = rawcheck.wrap(oracle, d)
        need = oracle.decompress(wrapped, rawcheck.BIG)[0].out_len
        caps.append([need, need + 100, max(need - 1, 0), need, 0, need][k % 6])
    return caps


def _layout(lens, align):
    off = np.zeros(len(lens), dtype=np.uint64)
    pos = 0
    for k, n in enumerate(lens):
        off[k] = pos
        pos += (int(n) + align - 1) // align * align if align > 1 else int(n)
    return off, pos


class Dev:
    """One raw launch over device arenas: streams packed `align`-aligned (1: back to back), 0xCD in every gap and past the end."""

    def __init__(self, streams, caps, align=16, gap=0, dicts=None):
        import torch
        self.torch, self.n = torch, len(streams)
        dev = torch.device("cuda", 0)
        self.in_len = np.array([len(s) for s in streams], dtype=np.uint64)
        self.out_cap = np.array(caps, dtype=np.uint64)
        self.in_off, in_bytes = _layout(self.in_len, align)
        self.out_off, self.out_bytes = _layout(self.out_cap + np.uint64(gap), align)
        h_in = np.zeros(in_bytes + 64, dtype=np.uint8)
        for k, s in enumerate(streams):
            h_in[int(self.in_off[k]):int(self.in_off[k]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)  # noqa: E731
        self.d_in = up(h_in)
        self.d_out = torch.full((self.out_bytes + 64,), 0xCD, dtype=torch.uint8, device=dev)
        self.d_in_off, self.d_in_len, self.d_out_off, self.d_out_cap = up(self.in_off), up(self.in_len), up(self.out_off), up(self.out_cap)
        self.d_out_len = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.d_in_used = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.d_status = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.d_adler = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.d_detail = torch.zeros(2 * self.n, dtype=torch.int32, device=dev)
        self.dict_args = None
        if dicts is not None:
            dl = np.array([len(x) for x in dicts], dtype=np.uint64)
            do, nb = _layout(dl, 1)
            self.d_dict = up(np.frombuffer(b"".join(dicts) + b"\0" * 16, dtype=np.uint8).copy())
            self.d_dict_off, self.d_dict_len = up(do), up(dl)
            self.dict_args = (self.d_dict.data_ptr(), self.d_dict_off.data_ptr(), self.d_dict_len.data_ptr())
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(in_base=self.d_in.data_ptr(), in_off=self.d_in_off.data_ptr(), in_len=self.d_in_len.data_ptr(),
                    out_base=self.d_out.data_ptr(), out_off=self.d_out_off.data_ptr(), out_cap=self.d_out_cap.data_ptr(),
                    out_len=self.d_out_len.data_ptr(), status=self.d_status.data_ptr(), detail=self.d_detail.data_ptr(),
                    in_used=self.d_in_used.data_ptr(), adler=self.d_adler.data_ptr())

    def launch(self, ctx, flags):
        from pure_zlib_amd import _ffi
        p = self.ptrs()
        L = _ffi.lib()
        if self.dict_args:
            rc = L.pzg_decompress_many_dict(ctx.handle, p["in_base"], p["in_off"], p["in_len"], *self.dict_args, p["out_base"], p["out_off"],
                                            p["out_cap"], p["out_len"], p["status"], p["detail"], p["in_used"], p["adler"], self.n, flags)
        else:
            rc = L.pzg_decompress_many(ctx.handle, p["in_base"], p["in_off"], p["in_len"], p["out_base"], p["out_off"], p["out_cap"],
                                       p["out_len"], p["status"], p["detail"], p["in_used"], p["adler"], self.n, flags)
        if rc == 0 and flags & _ffi.ASYNC:
            ctx.sync()
        return rc

    def results(self):
        self.torch.cuda.synchronize()
        st, ol, used = self.d_status.cpu().numpy(), self.d_out_len.cpu().numpy(), self.d_in_used.cpu().numpy()
        ad, det = self.d_adler.cpu().numpy().view(np.uint32), self.d_detail.cpu().numpy().view(np.uint32)
        h = self.d_out.cpu().numpy()
        res = []
        for k in range(self.n):
            o, cap = int(self.out_off[k]), int(self.out_cap[k])
            res.append((int(st[k]), int(det[2 * k]), int(det[2 * k + 1]), int(ad[k]), int(ol[k]), int(used[k]), h[o:o + min(int(ol[k]), cap)].tobytes()))
        return res, h

    def guards_intact(self, h, res):
        """Nothing but 0xCD outside [off, off + min(out_len, cap)) of every extent."""
        mask = np.ones(len(h), dtype=bool)
        for k in range(self.n):
            o = int(self.out_off[k])
            mask[o:o + min(res[k][4], int(self.out_cap[k]))] = False
        return bool((h[mask] == 0xCD).all())


def _zlib_detail1_on_gpu(ctx):
    """detail[1] the zlib kernels report for a wrapped stream (PZG_E_HUFF_BUILD's bit offset)."""
    def f(wrapped):
        buf = np.frombuffer(wrapped + b"\0" * 16, dtype=np.uint8).copy()
        out = np.zeros(1 << 16, dtype=np.uint8)
        _ol, st, det, _u, _a = ctx.decompress_many_raw(buf, [0], [len(wrapped)], out, [0], [1 << 16])
        assert int(st[0]) == 7
        return int(det[0][1])
    return f


def _check_all(oracle, pool, caps, res, detail1=None, crc=False):
    for (name, d), cap, got in zip(pool, caps, res):
        if crc:  # adler[] holds the CRC-32 of what was delivered, 0 past the capacity; everything else as without the flag
            exp = 0 if got[4] > cap else zlib.crc32(got[6])
            assert got[3] == exp, (name, "crc32", got[3], exp)
            wrapped, _e = rawcheck.wrap(oracle, d)
            ro, _ = oracle.decompress(wrapped, cap)
            got = got[:3] + ((0 if ro.out_len > cap and ro.status not in (0, 14) else ro.adler),) + got[4:]
        rawcheck.check(oracle, d, cap, got, detail1, name)


@pytest.mark.parametrize("ring", [11, 15])
@pytest.mark.parametrize("mode", ["sync", "async", "lpt"])
def test_raw_device_pointers(gpu_ctx, oracle, pool, ring, mode):
    """Device pointers, synchronous and PZG_ASYNC, with PZG_LPT_ORDER, rings 11 and 15 -- back-to-back UNALIGNED extents with 0xCD
    guards between them: nothing is written outside [0, min(out_len, cap)) of any extent."""
    from pure_zlib_amd import _ffi
    caps = _caps(oracle, pool)
    b = Dev([d for _n, d in pool], caps, align=1, gap=7)
    gpu_ctx.set_ring_bits(ring)
    try:
        flags = _ffi.DEVICE_PTRS | _ffi.RAW | {"sync": 0, "async": _ffi.ASYNC, "lpt": _ffi.ASYNC | _ffi.LPT_ORDER}[mode]
        assert b.launch(gpu_ctx, flags) == 0
        res, h = b.results()
        _check_all(oracle, pool, caps, res, _zlib_detail1_on_gpu(gpu_ctx) if mode == "sync" else None)
        assert b.guards_intact(h, res)
    finally:
        gpu_ctx.set_ring_bits(11)


@pytest.mark.parametrize("ring", [11, 15])
def test_raw_crc32_device(gpu_ctx, oracle, pool, ring):
    """PZG_RAW | PZG_CRC32: adler[] is zlib.crc32 of the delivered bytes -- lengths 0, 1, 1023, 1024, 1025 among them -- and 0 for a
    stream that outgrew its capacity; status, lengths, in_used and bytes as without the flag."""
    from pure_zlib_amd import _ffi
    extra = []
    for n in (0, 1, 1023, 1024, 1025, 4096, 100000):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        extra.append(("len%d" % n, co.compress(corpus.mixed_data(n, n)) + co.flush()))
    both = extra + pool
    caps = [[0, 1, 1023, 1024, 1025, 4096, 99999][k] for k in range(7)] + _caps(oracle, pool)
    b = Dev([d for _n, d in both], caps, align=16)
    gpu_ctx.set_ring_bits(ring)
    try:
        assert b.launch(gpu_ctx, _ffi.DEVICE_PTRS | _ffi.RAW | _ffi.CRC32) == 0
        res, h = b.results()
        assert [r[0] for r in res[:7]] == [0] * 6 + [14] and res[6][3] == 0
        assert [r[3] for r in res[:6]] == [zlib.crc32(corpus.mixed_data(n, n)) for n in (0, 1, 1023, 1024, 1025, 4096)]
        _check_all(oracle, both, caps, res, crc=True)
        assert b.guards_intact(h, res)
    finally:
        gpu_ctx.set_ring_bits(11)


def _host_call(ctx, pool, caps, pinned, crc=False):
    from pure_zlib_amd.zlib import PinnedArena
    in_len = [len(d) for _n, d in pool]
    in_off, nin = _layout(in_len, 16)
    out_off, nout = _layout(caps, 16)
    arenas = [PinnedArena(nin + 16), PinnedArena(nout + 16)] if pinned else []
    try:
        ibuf = arenas[0].a if pinned else np.zeros(nin + 16, dtype=np.uint8)
        obuf = arenas[1].a if pinned else np.zeros(nout + 16, dtype=np.uint8)
        obuf[:] = 0xCD
        for k, (_n, d) in enumerate(pool):
            ibuf[int(in_off[k]):int(in_off[k]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
        ol, st, det, used, ad = ctx.decompress_many_raw(ibuf, in_off, in_len, obuf, out_off, caps, pinned=pinned, raw=True, crc32=crc)
        return [(int(st[k]), int(det[k][0]), int(det[k][1]), int(ad[k]), int(ol[k]), int(used[k]),
                 obuf[int(out_off[k]):int(out_off[k]) + min(int(ol[k]), caps[k])].tobytes()) for k in range(len(pool))]
    finally:
        for a in arenas:
            a.close()


@pytest.mark.parametrize("path", ["staged", "pinned", "two_shards"])
def test_raw_host_paths(gpu_ctx, oracle, pool, path):
    """The staged host path, PZG_HOST_PINNED, and a two-shard context (pzg_init_devices([0, 0])), with and without PZG_CRC32."""
    import pure_zlib_amd as P
    caps = _caps(oracle, pool)
    ctx = P.Context(devices=[0, 0]) if path == "two_shards" else gpu_ctx
    try:
        _check_all(oracle, pool, caps, _host_call(ctx, pool, caps, path == "pinned"))
        _check_all(oracle, pool, caps, _host_call(ctx, pool, caps, path == "pinned", crc=True), crc=True)
        if path == "two_shards":
            _check_all(oracle, pool, caps, _host_call(ctx, pool, caps, True))
    finally:
        if ctx is not gpu_ctx:
            ctx.close()


def test_raw_sharded_call(oracle, pool):
    """pzg_decompress_many_sharded takes the two flags: two batches on the two shards of a pzg_init_devices([0, 0]) context."""
    import pure_zlib_amd as P
    caps = _caps(oracle, pool)
    half = len(pool) // 2
    parts = [(pool[:half], caps[:half]), (pool[half:], caps[half:])]
    ctx = P.Context(devices=[0, 0])
    try:
        for crc in (False, True):
            devs = [Dev([d for _n, d in p], c) for p, c in parts]
            ctx.decompress_many_sharded([dict(shard=s, n=b.n, **b.ptrs()) for s, b in enumerate(devs)], raw=True, crc32=crc, lpt=crc)
            for b, (p, c) in zip(devs, parts):
                res, h = b.results()
                _check_all(oracle, p, c, res, crc=crc)
                assert b.guards_intact(h, res)
    finally:
        ctx.close()


def test_raw_flag_combinations_refused(gpu_ctx):
    """PZG_RAW | PZG_GZIP, PZG_CRC32 alone and PZG_CRC32 | PZG_GZIP are PZG_RC_BAD_ARG, on both entry points."""
    from pure_zlib_amd import _ffi
    b = Dev([b"\x03\x00"], [16])
    for flags in (_ffi.RAW | _ffi.GZIP, _ffi.CRC32, _ffi.CRC32 | _ffi.GZIP):
        assert b.launch(gpu_ctx, _ffi.DEVICE_PTRS | flags) == _ffi.RC_BAD_ARG
        arr = (_ffi.DeviceBatch * 1)()
        for k, v in dict(shard=0, n=1, **b.ptrs()).items():
            setattr(arr[0], k, v)
        assert _ffi.lib().pzg_decompress_many_sharded(gpu_ctx.handle, C.byref(arr), 1, flags) == _ffi.RC_BAD_ARG
    assert b.launch(gpu_ctx, _ffi.DEVICE_PTRS | _ffi.RAW | _ffi.CRC32) == 0 and b.results()[0][0][:1] == (0,)


def test_raw_dictionaries(gpu_ctx):
    """pzg_decompress_many_dict with PZG_RAW: dict_len > 0 is the history, unconditionally; dict_len = 0 is plain raw -- device
    pointers (rings 11 and 15) and the host mirror."""
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    streams, dicts, datas = [], [], []
    for seed in range(24):
        zdict = b"" if seed % 3 == 2 else corpus.zipf_text([40, 700, 5000, 32768, 50000][seed % 5], 100 + seed)
        data = zdict[-300:] * 2 + corpus.zipf_text(3000 + 977 * seed, 100 + seed) + zdict[:200]
        co = zlib.compressobj(1 + seed % 9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(6, zlib.DEFLATED, -15)
        streams.append(co.compress(data) + co.flush())
        dicts.append(zdict)
        datas.append(data)
    for ring in (11, 15):
        gpu_ctx.set_ring_bits(ring)
        b = Dev(streams, [len(x) for x in datas], dicts=dicts)
        assert b.launch(gpu_ctx, _ffi.DEVICE_PTRS | _ffi.RAW) == 0
        res, _h = b.results()
        for k, r in enumerate(res):
            assert (r[0], r[4], r[5], r[3], r[6]) == (0, len(datas[k]), len(streams[k]), zlib.adler32(datas[k]), datas[k]), (ring, k)
    gpu_ctx.set_ring_bits(11)
    got, crcs = P.raw_decompress_many(streams, crc32=True, dicts=[x or None for x in dicts], ctx=gpu_ctx)
    assert [g.value for g in got] == datas and crcs == [zlib.crc32(x) for x in datas]


def test_raw_python_mirror(gpu_ctx, oracle):
    """raw_decompress / raw_decompress_many: the capacity guess and its one relaunch, the error classes, and "Finished with data
    remaining." from in_used."""
    import pure_zlib_amd as P
    data = corpus.zipf_text(300000, 4)
    d = zlib.compress(data, 9)[2:-4]
    assert P.raw_decompress(d, ctx=gpu_ctx) == P.Right(data)  # (the guess is 4 x the input: relaunched with the exact size)
    assert P.raw_decompress([d[:100], d[100:]], ctx=gpu_ctx, size_hint=len(data)) == P.Right(data)
    assert P.raw_decompress([d, b"more"], ctx=gpu_ctx).value.message == "Finished with data remaining."
    assert P.raw_decompress(d + b"more", ctx=gpu_ctx) == P.Right(data)
    left = P.raw_decompress(d[:-5], ctx=gpu_ctx)
    assert not left.is_right() and left.value.status == 1 and left.value.show() == "Decompression error: Ran out of data mid-decompression 2."
    assert P.raw_decompress(b"", ctx=gpu_ctx).value.status == 1
    assert P.raw_decompress(b"\x07", ctx=gpu_ctx).value.show() == oracle.decompress(b"\x78\x9c\x07")[0].message.decode()
    assert P.raw_decompress_many([], ctx=gpu_ctx) == []


def test_raw_32768_fixed_code_streams_stay_out_of_the_bundles(gpu_ctx):
    """A launch of 32,768 raw streams of the fixed code -- the size at which zlib launches go through the bundles: raw launches do
    not (a bundle lane would look for a zlib header), and every result is exact."""
    texts, raws = [], []
    for seed in range(512):
        t = corpus.zipf_text(200 + (seed * 37) % 1800, seed)
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        texts.append(t)
        raws.append(co.compress(t) + co.flush())
    assert all((r[0] >> 1) & 3 == 1 for r in raws)
    pick = np.random.default_rng(0xB5).integers(0, len(raws), size=32768 + 64)
    b = RawBatch(texts, raws, pick)
    gpu_ctx.set_bundles(1)
    for ring in (11, 15):
        b.check_all(*b.run(gpu_ctx, ring))
    gpu_ctx.set_ring_bits(11)


class RawBatch(DeviceBatch):
    """tests/devbatch.py's batch over raw streams: the same arenas and checks, launched with PZG_RAW."""

    def run(self, ctx, ring_bits, crc32=False):
        t = self.torch
        self.d_out.fill_(0xCD)
        self.d_status.fill_(-1)
        t.cuda.synchronize()
        ctx.set_ring_bits(ring_bits)
        ctx.decompress_many_device(self.d_in.data_ptr(), self.d_in_off.data_ptr(), self.d_in_len.data_ptr(),
                                   self.d_out.data_ptr(), self.d_out_off.data_ptr(), self.d_out_cap.data_ptr(),
                                   self.d_out_len.data_ptr(), self.d_status.data_ptr(), self.d_detail.data_ptr(),
                                   self.d_in_used.data_ptr(), self.d_adler.data_ptr(), self.n, sync=True, raw=True, crc32=crc32)
        return (self.d_status.cpu().numpy(), self.d_out_len.cpu().numpy(), self.d_in_used.cpu().numpy(),
                self.d_adler.cpu().numpy().view(np.uint32))


def test_raw_full_size_65536_level6_32k(gpu_ctx):
    """The batch bench.py times -- 65,536 x 32 KiB level-6 payloads -- as raw streams: every stream's status, length, in_used,
    Adler-32 and bytes; then with PZG_CRC32 every CRC-32."""
    texts = [corpus.zipf_text(32768, seed) for seed in range(2048)]
    raws = [zlib.compress(t, 6)[2:-4] for t in texts]
    pick = np.random.default_rng(0xC4).integers(0, len(raws), size=65536)
    b = RawBatch(texts, raws, pick)
    for ring in (11, 15):
        b.check_all(*b.run(gpu_ctx, ring))
    st, ol, used, crc = b.run(gpu_ctx, 11, crc32=True)
    assert (st == 0).all() and (ol == b.out_cap).all() and (used == b.in_len).all()
    assert (crc == np.array([zlib.crc32(t) for t in texts], dtype=np.uint32)[b.pick]).all()
    gpu_ctx.set_ring_bits(11)


# ---- ZIP archives ----------------------------------------------------------------------------------------------------------------

def _zip(members, force_zip64=False):
    """members: [(name, data, method, level)]"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", allowZip64=True) as zf:
        for name, data, method, level in members:
            if force_zip64:
                with zf.open(zipfile.ZipInfo(name), "w", force_zip64=True) as f:  # (stored; zip64 extra in the local header)
                    f.write(data)
                continue
            zf.writestr(zipfile.ZipInfo(name) if name.endswith("/") else name, data, compress_type=method, compresslevel=level)
    return buf.getvalue()


def _members():
    m = [("l1.txt", corpus.zipf_text(50000, 1), zipfile.ZIP_DEFLATED, 1), ("l6.html", corpus.html_slice(90000, 2), zipfile.ZIP_DEFLATED, 6),
         ("l9.bin", corpus.binary_records(70000, 3), zipfile.ZIP_DEFLATED, 9), ("stored.bin", corpus.random_bytes(5000, 4), zipfile.ZIP_STORED, None),
         ("empty.txt", b"", zipfile.ZIP_DEFLATED, 6), ("empty.stored", b"", zipfile.ZIP_STORED, None), ("dir/", b"", zipfile.ZIP_STORED, None),
         ("dir/sub/inner.txt", corpus.mixed_data(12345, 5), zipfile.ZIP_DEFLATED, 6),
         ("big.bin", corpus.zipf_text(3 << 20, 6), zipfile.ZIP_DEFLATED, 6)]
    return m


def _same_as_stdlib(blob, ctx):
    from pure_zlib_amd.zip import read_zip, test_zip
    got = read_zip(blob, ctx)
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        assert list(got) == zf.namelist()
        for name in zf.namelist():
            assert got[name] == zf.read(name), name
    assert test_zip(blob, ctx) == []
    return got


def test_zip_archives_equal_the_stdlib(gpu_ctx, tmp_path):
    """Levels 1 / 6 / 9, stored and empty members, directories, a multi-MiB member; 5,000 small members; an archive forced to
    zip64; from bytes and from a path; the command line."""
    from pure_zlib_amd import zip as Z
    blob = _zip(_members())
    _same_as_stdlib(blob, gpu_ctx)
    p = tmp_path / "a.zip"
    p.write_bytes(blob)
    assert Z.read_zip(str(p), gpu_ctx) == Z.read_zip(blob, gpu_ctx)
    small = [("m/%04d.txt" % k, corpus.mixed_data(1 + (k * 131) % 3000, k), zipfile.ZIP_DEFLATED, 1 + k % 9) for k in range(5000)]
    assert len(_same_as_stdlib(_zip(small), gpu_ctx)) == 5000
    z64 = _zip([("a.bin", corpus.zipf_text(40000, 7), None, None), ("b.bin", b"", None, None)], force_zip64=True)
    buf = io.BytesIO(z64)
    with zipfile.ZipFile(buf, "a") as zf:
        with zf.open(zipfile.ZipInfo("c.txt"), "w", force_zip64=True) as f:
            pass
        zi = zipfile.ZipInfo("d.txt")
        zi.compress_type = zipfile.ZIP_DEFLATED
        with zf.open(zi, "w", force_zip64=True) as f:
            f.write(corpus.zipf_text(60000, 8))
    z64 = buf.getvalue()
    assert b"PK\x06\x06" in z64 or struct.pack("<H", 1) in z64  # (a zip64 record or extra field is there)
    _same_as_stdlib(z64, gpu_ctx)


def test_zip_problems_name_their_member(gpu_ctx):
    """One flipped byte inside a member's data: the error names that member, test_zip lists it alone -- the others still verify; an
    encrypted-flag member and an unknown method are refused by name."""
    from pure_zlib_amd import zip as Z
    import pure_zlib_amd as P
    blob = bytearray(_zip(_members()))
    with zipfile.ZipFile(io.BytesIO(bytes(blob))) as zf:
        zi = zf.getinfo("l6.html")
        enc = zf.getinfo("l1.txt")
        infos = {i.filename: i for i in zf.infolist()}
    nlen, xlen = struct.unpack_from("<HH", blob, zi.header_offset + 26)
    at = zi.header_offset + 30 + nlen + xlen
    bad = bytearray(blob)
    bad[at + zi.compress_size // 2] ^= 0x40
    with pytest.raises(P.DecompressionError) as ei:
        Z.read_zip(bytes(bad), gpu_ctx)
    assert "l6.html" in ei.value.show()
    problems = Z.test_zip(bytes(bad), gpu_ctx)
    assert [n for n, _w in problems] == ["l6.html"]
    # the same byte flipped in the directory's CRC instead: a checksum error by name
    crcbad = bytearray(blob)
    cd = bytes(blob).rfind(b"PK\x01\x02" , 0, len(blob))
    pos = bytes(blob).find(struct.pack("<I", infos["l9.bin"].CRC), bytes(blob).find(b"PK\x01\x02"))
    crcbad[pos] ^= 1
    with pytest.raises(P.DecompressionError) as ei:
        Z.read_zip(bytes(crcbad), gpu_ctx)
    assert ei.value.constructor == "ChecksumError" and "l9.bin" in ei.value.show() and cd > 0
    # flag bit 0 (encrypted) set in the directory entry of l1.txt
    encb = bytearray(blob)
    first_cd = bytes(blob).find(b"PK\x01\x02")
    assert enc.header_offset == 0 and bytes(blob)[first_cd + 46:first_cd + 46 + 6] == b"l1.txt"
    encb[first_cd + 8] |= 1
    with pytest.raises(NotImplementedError) as ni:
        Z.read_zip(bytes(encb), gpu_ctx)
    assert "l1.txt" in str(ni.value)
    assert [n for n, _w in Z.test_zip(bytes(encb), gpu_ctx)] == ["l1.txt"]


def test_cxx_mirror_raw_decompress():
    """rawDecompress / rawDecompressMany of the C++ module mirror, driven by tests/cxx/test_mirror_raw.cpp."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cxx", "test_mirror_raw")
    src = os.path.join(ROOT, "tests", "cxx", "test_mirror_raw.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", src, "-o", exe, "-L" + os.path.join(ROOT, "pure_zlib_amd"),
                           "-lpzg", "-Wl,-rpath," + os.path.join(ROOT, "pure_zlib_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ref")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(" OK") == 16 and "0 failure(s)" in out.stdout
