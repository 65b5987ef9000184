"""GPU: the resumable gzip and raw decoders (pzg_decoder_create_format; resume_gzip_kernel + resume_crc_kernel, resume_raw_kernel)
through the C ABI, held to the rule of include/pzg.h: however the input is cut into feeds and the rooms are sized, the delivered
bytes, the terminal state and detail, the last adler and the sum of in_used are what pzg_decompress_many gives with the same flag
over the whole input.  The case lists are the CPU model's (tests/resume_fmt_cases.py), 64 decoders to an object, fed in one launch
per step; then the pipelined path, the argument checks, reset, the Python mirror, the CLI and the code object's notes."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

import corpus
import resume_fmt_cases as K
from conftest import REF_CASES, ROOT, read_case

pytestmark = pytest.mark.gpu


class Decoders:
    """A pzg_decoder object of n decoders of one format, fed through ctypes."""

    def __init__(self, ctx, n, fmt, entry="format"):
        from pure_zlib_amd import _ffi
        self.L, self.ctx, self.n = _ffi.lib(), ctx, n
        h = C.c_void_p()
        if entry == "format":
            rc = self.L.pzg_decoder_create_format(ctx.handle, n, fmt, C.byref(h))
        else:
            rc = self.L.pzg_decoder_create(ctx.handle, n, C.byref(h))
        _ffi.check(rc, ctx.handle)
        self.h = h

    def close(self):
        if self.h:
            self.L.pzg_decoder_destroy(self.h)
            self.h = None

    def reset(self, ks):
        idx = np.array(ks, dtype=np.uint32)
        assert self.L.pzg_decoder_reset(self.h, idx.ctypes.data, len(ks)) == 0

    def feed(self, ks, datas, finals, rooms):
        """One pzg_decoder_feed call: decoders ks[j] get datas[j]; -> per decoder (state, detail, adler, out_len, in_used, chunks, bytes)."""
        from pure_zlib_amd import _ffi
        m = len(ks)
        idx = np.array(ks, dtype=np.uint32)
        in_len = np.array([len(d) for d in datas], dtype=np.uint64)
        in_off = np.zeros(m, dtype=np.uint64)
        in_off[1:] = np.cumsum(in_len[:-1])
        in_buf = np.frombuffer(b"".join(datas) + b"\0" * 16, dtype=np.uint8)
        out_cap = np.array(rooms, dtype=np.uint64)
        out_off = np.zeros(m, dtype=np.uint64)
        out_off[1:] = np.cumsum((out_cap[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
        total = int(out_off[-1]) + int(out_cap[-1])
        out_buf = np.full(total + 16, 0xCD, dtype=np.uint8)
        out_len = np.zeros(m, dtype=np.uint64)
        state = np.zeros(m, dtype=np.int32)
        detail = np.zeros((m, 2), dtype=np.uint32)
        in_used = np.zeros(m, dtype=np.uint64)
        chunks = np.zeros(m, dtype=np.uint32)
        adler = np.zeros(m, dtype=np.uint32)
        fin = np.array(finals, dtype=np.uint8)
        rc = self.L.pzg_decoder_feed(self.h, idx.ctypes.data, m, in_buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, fin.ctypes.data,
                                     out_buf.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data, state.ctypes.data,
                                     detail.ctypes.data, in_used.ctypes.data, chunks.ctypes.data, adler.ctypes.data)
        _ffi.check(rc, self.ctx.handle)
        res = []
        for j in range(m):
            o = int(out_off[j])
            res.append((int(state[j]), (int(detail[j][0]), int(detail[j][1])), int(adler[j]), int(out_len[j]), int(in_used[j]), int(chunks[j]),
                        out_buf[o:o + int(out_len[j])].tobytes()))
        return res


def batch_results(ctx, cases, fmt):
    """pzg_decompress_many with the format's flag over every case's whole stream, enough capacity: the rule's other side."""
    from test_gpu_parity import run_batch
    from pure_zlib_amd import _ffi
    streams = [c["stream"] for c in cases]
    caps = [1 << 21 if "zerotest3" in c["name"] else 1 << 18 for c in cases]
    if fmt == "gzip":
        (out_len, status, detail, in_used, adler), outs, _, _ = run_batch(ctx, streams, caps, gzip=True)
    else:
        n = len(streams)
        in_len = np.array([len(s) for s in streams], dtype=np.uint64)
        in_off = np.zeros(n, dtype=np.uint64)
        in_off[1:] = np.cumsum((in_len[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
        in_buf = np.zeros(int(in_off[-1]) + len(streams[-1]) + 16, dtype=np.uint8)
        for k, s in enumerate(streams):
            in_buf[int(in_off[k]):int(in_off[k]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
        out_cap = np.array(caps, dtype=np.uint64)
        out_off = np.zeros(n, dtype=np.uint64)
        out_off[1:] = np.cumsum(out_cap[:-1])
        out_buf = np.zeros(int(out_off[-1]) + caps[-1] + 16, dtype=np.uint8)
        out_len, status, detail, in_used, adler = ctx.decompress_many_raw(in_buf, in_off, in_len, out_buf, out_off, out_cap, raw=True)
        outs = [out_buf[int(out_off[k]):int(out_off[k]) + min(int(out_len[k]), caps[k])].tobytes() for k in range(n)]
    out = []
    for k in range(len(cases)):
        assert int(out_len[k]) <= caps[k], cases[k]["name"]
        out.append((int(status[k]), int(detail[k][0]), int(detail[k][1]), int(adler[k]), int(in_used[k]), outs[k]))
    return out


def run_lockstep(ctx, oracle, cases, fmt):
    """The cases of one format, 64 to a decoder object, every step ONE pzg_decoder_feed call over all that still have a call to make."""
    expected = batch_results(ctx, cases, fmt)
    seen = set()
    for g0 in range(0, len(cases), 64):
        group = cases[g0:g0 + 64]
        dec = Decoders(ctx, 64, K.FLAG[fmt])
        drivers = [K.Driver(c) for c in group]
        try:
            while True:
                ks, datas, finals, rooms = [], [], [], []
                for k, d in enumerate(drivers):
                    nxt = d.next_input()
                    if nxt is not None:
                        ks.append(k)
                        datas.append(nxt[0])
                        finals.append(nxt[1])
                        rooms.append(d.c["room"])
                if not ks:
                    break
                for k, r in zip(ks, dec.feed(ks, datas, finals, rooms)):
                    drivers[k].take(*r)
        finally:
            dec.close()
        for k, d in enumerate(drivers):
            K.check_rule(oracle, d.c, d.o, expected[g0 + k])
            K.check_independent(oracle, d.c, d.o)
            seen.add(d.o.status)
    return seen


def gpu_steps(n):
    """Piece sizes for a fixture of n compressed bytes: the small ones only where they make a few hundred feeds."""
    return (1, 7, 4096, 32768) if n < 1200 else (7, 4096, 32768) if n < 5000 else (509, 4096, 32768)


@pytest.mark.parametrize("fmt", ["gzip", "raw"])
def test_case_lists_against_the_batch_path(gpu_ctx, oracle, fmt):
    """The CPU model's case lists -- fixtures re-wrapped, headers and trailers cut at every byte, member boundaries, garbage, wrong
    CRC-32 and ISIZE, truncation, raw streams that end mid-byte, 4 KiB rooms -- 64 decoders per object with mixed piece sizes."""
    cases = [c for c in K.fixture_cases(gpu_steps) + K.corner_cases() if c["fmt"] == fmt]
    seen = run_lockstep(gpu_ctx, oracle, cases, fmt)
    assert ({0, 1, 10, 18, 19} if fmt == "gzip" else {0, 1}) <= seen, seen


def test_pipelined_feed_of_600_decoders(gpu_ctx):
    """600 gzip decoders, 128 KiB rooms: the pipelined path (ranges, dense copy-out) with the CRC pass behind every range's kernel.
    Two feeds per decoder, the second one final; every fourth stream has a wrong CRC-32 in its trailer."""
    n, room = 600, 128 * 1024
    datas = [corpus.zipf_text(60000 + 97 * (k % 50), k % 50) for k in range(50)]
    members = []
    for k in range(n):
        d = datas[k % 50]
        body = zlib.compress(d, 6)[2:-4]
        members.append(K.member(body, d, crc=(zlib.crc32(d) ^ 1) if k % 4 == 3 else None))
    dec = Decoders(gpu_ctx, n, K.GZIP)
    try:
        half = [len(m) // 2 for m in members]
        r1 = dec.feed(list(range(n)), [m[:h] for m, h in zip(members, half)], [0] * n, [room] * n)
        tails = [m[:h][r[4]:] for m, h, r in zip(members, half, r1)]
        r2 = dec.feed(list(range(n)), [t + m[h:] for t, m, h in zip(tails, members, half)], [1] * n, [room] * n)
    finally:
        dec.close()
    for k in range(n):
        d = datas[k % 50]
        assert r1[k][0] == K.NEED_INPUT and r1[k][2] == zlib.crc32(r1[k][6]), k
        assert r1[k][6] + r2[k][6] == d, k
        assert r1[k][4] + r2[k][4] == len(members[k]) and r2[k][2] == zlib.crc32(d), k
        if k % 4 == 3:
            assert r2[k][0] == 10 and r2[k][1] == (zlib.crc32(d) ^ 1, zlib.crc32(d)), (k, r2[k][:3])
        else:
            assert r2[k][0] == 0, (k, r2[k][:3])


def test_bad_formats_are_refused(gpu_ctx):
    from pure_zlib_amd import _ffi
    L = _ffi.lib()
    for fmt in (3, K.GZIP | K.RAW, 1, 64, 1 << 31):
        h = C.c_void_p(1)
        assert L.pzg_decoder_create_format(gpu_ctx.handle, 4, fmt, C.byref(h)) == _ffi.RC_BAD_ARG and not h.value, fmt


def test_format_0_is_pzg_decoder_create(gpu_ctx, oracle):
    """A format-0 object from the new entry goes through the event traces of pzg_decoder_create's (three fixtures)."""
    for name in ("rfctest1", "randtest2", "zerotest3"):
        z, gold = read_case(name)
        pieces = K.by_step(z, 997)
        traces = []
        for entry in ("format", "create"):
            dec = Decoders(gpu_ctx, 1, 0, entry)
            tail, events, data = b"", [], b""
            try:
                for p in pieces:
                    buf = tail + p
                    while True:
                        st, detail, adler, out_len, in_used, chunks, out = dec.feed([0], [buf], [0], [70000])[0]
                        events.append((st, detail, adler, out_len, in_used, chunks))
                        data += out
                        buf = buf[in_used:]
                        if st != K.OUT_FULL:
                            break
                    tail = buf
            finally:
                dec.close()
            assert data == gold and events[-1][0] == 0, (name, entry)
            traces.append(events)
        assert traces[0] == traces[1], name
        eo, ro, _ = oracle.trace(pieces)
        assert traces[0][-1][5] == sum(1 for e in eo if e[0] == "Chunk") - 1


def test_reset_mid_member_clears_the_running_crc(gpu_ctx):
    d1, d2 = corpus.zipf_text(50000, 1), corpus.mixed_data(30000, 2)
    m1, m2 = (K.member(zlib.compress(d, 6)[2:-4], d) for d in (d1, d2))
    dec = Decoders(gpu_ctx, 3, K.GZIP)
    try:
        r = dec.feed([0, 1, 2], [m1[:5000]] * 3, [0] * 3, [1 << 17] * 3)
        assert all(x[0] == K.NEED_INPUT and x[3] > 0 and x[2] == zlib.crc32(x[6]) for x in r)
        dec.reset([1])
        # decoder 1 starts a fresh member; its neighbours go on with theirs
        r2 = dec.feed([0, 1, 2], [m1[:5000][r[0][4]:] + m1[5000:], m2, m1[:5000][r[2][4]:] + m1[5000:]], [1] * 3, [1 << 17] * 3)
    finally:
        dec.close()
    assert (r2[1][0], r2[1][6], r2[1][2], r2[1][4]) == (0, d2, zlib.crc32(d2), len(m2))
    for k in (0, 2):
        assert (r2[k][0], r[k][6] + r2[k][6], r2[k][2]) == (0, d1, zlib.crc32(d1)), k


def test_decoder_pool_and_incremental_formats(gpu_ctx):
    """DecoderPool(format=...) / decompress_incremental(format=...): the event chains of two members fed in pieces, a raw stream, an
    error; the defaults are the zlib decoder's."""
    from pure_zlib_amd.incremental import Chunk, DecoderPool, DecompError, Done, NeedMore, decompress_incremental
    from test_gpu_incremental import drive
    d1, d2 = corpus.zipf_text(90000, 5), corpus.zipf_text(40000, 6)
    g = K.member(zlib.compress(d1, 6)[2:-4], d1, K.rich_header()) + K.member(zlib.compress(d2, 9)[2:-4], d2)
    pool = DecoderPool(2, gpu_ctx, format="gzip")
    events, data, err = drive(pool, 0, K.by_step(g, 7000) + [b"xy"])  # (two bytes behind the last member that are no magic: Done)
    assert err is None and data == d1 + d2 and events[-1] == ("Done",)
    published = [e for e in events if e[0] == "Chunk"]
    assert len(published) >= 3 and all(e == ("Chunk", 32768) for e in published[:-1])
    st = pool.start(1)
    for p in K.by_step(g, 30000):
        st = st.feed(p)
        while isinstance(st, Chunk):
            st = st.next()
    assert isinstance(st, NeedMore)  # no final piece yet: a further member may follow
    st = st.feed(b"", final=True)
    while isinstance(st, Chunk):
        st = st.next()
    assert isinstance(st, Done)
    pool.close()
    bad = g[:len(g) - 8] + bytes([g[-8] ^ 1]) + g[len(g) - 7:]
    st = decompress_incremental(gpu_ctx, format="gzip").feed(bad, final=True)
    while isinstance(st, Chunk):
        st = st.next()
    assert isinstance(st, DecompError) and st.error.status == 10
    raw = zlib.compress(d2, 6)[2:-4]
    pool = DecoderPool(1, gpu_ctx, format="raw", room=8192)
    events, data, err = drive(pool, 0, K.by_step(raw + b"trailing bytes", 5000))
    pool.close()
    assert err is None and data == d2 and events[-1] == ("Done",)
    with pytest.raises(ValueError):
        DecoderPool(1, gpu_ctx, format="lzma")
    pool = DecoderPool(1, gpu_ctx)
    assert pool.format == "zlib"
    events, data, err = drive(pool, 0, [zlib.compress(d2, 6)])
    pool.close()
    assert data == d2 and err is None


def test_cli_gzip_and_raw(tmp_path):
    """deflate --gzip FILE.gz / --raw FILE.suffix: the streaming loop over one resumable decoder of that format."""
    d = corpus.zipf_text(150000, 9)
    two = K.member(zlib.compress(d[:70000], 6)[2:-4], d[:70000]) + K.member(zlib.compress(d[70000:], 1)[2:-4], d[70000:])
    (tmp_path / "a.txt.gz").write_bytes(two)
    (tmp_path / "b.deflate").write_bytes(zlib.compress(d, 6)[2:-4])
    (tmp_path / "c.gz").write_bytes(two[:-3])
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args, target, want, text in ((["--gzip", "a.txt.gz"], "a.txt", d, ""), (["--raw", "b.deflate"], "b", d, ""),
                                     (["--gzip", "c.gz"], "c", None, "ERROR: ")):
        out = subprocess.run([sys.executable, "-m", "pure_zlib_amd.deflate_cli"] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        if want is not None:
            assert out.stdout == "" and (tmp_path / target).read_bytes() == want, (args, out.stdout)
        else:
            assert out.stdout.startswith(text), (args, out.stdout)
    out = subprocess.run([sys.executable, "-m", "pure_zlib_amd.deflate_cli", "--gzip", "b.deflate"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout == "Unexpected file name.\n"


def _kernel_notes():
    """{kernel name: {field: int}} from the gfx950 code objects inside libpzg.so (their AMDGPU metadata notes)."""
    from pure_zlib_amd import _ffi
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.check_call([llvm + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, _ffi.LIB_PATH, os.path.join(d, "unused.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
        notes = ""
        for n, at in enumerate(starts):  # one bundle per translation unit that holds kernels
            part = os.path.join(d, "fat%d.bin" % n)
            open(part, "wb").write(blob[at:starts[n + 1] if n + 1 < len(starts) else len(blob)])
            subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + part, "--output=" + co])
            notes += subprocess.check_output([llvm + "/llvm-readelf", "--notes", co]).decode()
    kernels = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return kernels


def test_new_kernels_use_no_scratch():
    """resume_gzip_kernel and resume_raw_kernel are in the code object under names of their own and keep everything in registers, as
    the zlib resume kernel must; so does the CRC pass."""
    kernels = _kernel_notes()
    for want in ("resume_gzip_kernel", "resume_raw_kernel", "resume_crc_kernel"):
        ks = [(n, k) for n, k in kernels.items() if want in n]
        assert len(ks) == 1, (want, sorted(kernels))
        name, k = ks[0]
        print(name, {f: k[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
        assert "inflate_resume_kernel" not in name
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
