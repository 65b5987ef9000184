"""Large members split over many wavefronts (pure_zlib_amd/split.py) against a wavefront per member.  Not bench.py.

    python tests/tools/split_bench.py curve   --mib 1 2 4 8 16 32 64 [--split 0 | --split 1 --chunks 32 64 128]
    python tests/tools/split_bench.py batched --mib 32          # one pzg_index_scan_many call against eight pzg_index_scan calls
    python tests/tools/split_bench.py zip     --mib 64 [--split 0 | --split 1 --chunks 64]

curve: a gzip file of 8 equal members of level-6 corpus text, --mib MiB compressed each, through decompress_gzip_file (host memory in,
host memory out: the call a user makes).  zip: four such members and 1,000 small ones through read_zip.  --split 0 is today's path; run
with PYTHONPATH at a checkout of the parent commit it is the parent's (the tool uses nothing the parent lacks on that leg).  Two
warm-ups and five samples; a sample is the wall clock of the call and, beside it, the device work timed by the library's own events
(pzg_last_kernel_ms after every library call the mirror makes, added up).  Medians of five, every sample printed.  The inputs are made
first, by a pool of workers that has ended before the package is imported and the device opened.
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests")]
if not any(os.path.isdir(os.path.join(p, "pure_zlib_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

PIECE = 4 << 20  # decoded bytes per piece of text: a member is pieces compressed one after the other into ONE deflate stream


def _piece(seed):
    import corpus
    return corpus.zipf_text(PIECE, 0x5B000 + seed)


def member_body(mib, seed, pool):
    """(raw deflate stream of about `mib` MiB at level 6, CRC-32 of its data, its size)"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    out, crc, size, k = [], 0, 0, 0
    want = mib << 20
    while sum(map(len, out)) < want:
        for text in pool.map(_piece, range(seed * 4096 + k, seed * 4096 + k + 8)):
            out.append(co.compress(text))
            crc, size = zlib.crc32(text, crc), size + len(text)
            if sum(map(len, out)) >= want:
                break
        k += 8
    out.append(co.flush())
    return b"".join(out), crc, size


def gzip_members(mibs):
    """[(mib, one gzip member of about that many MiB compressed, its decoded size)].  The pool of workers lives and ends in here:
    main() calls this BEFORE it opens the device, so no process is ever forked from one that holds the GPU."""
    import multiprocessing as mp
    got = []
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        for mib in mibs:
            body, crc, size = member_body(mib, 1, pool)
            got.append((mib, b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\x03" + body + struct.pack("<II", crc, size & 0xffffffff), size, crc))
    return got


def zip_archive(mib):
    """(archive, its entries, the large members' CRC-32): four members of about `mib` MiB compressed, each in front of 250 small ones.
    Written by hand around the ready-made deflate streams (zipfile would compress them again); zipfile reads it back.  Like
    gzip_members(): before the device is opened."""
    import multiprocessing as mp
    import corpus
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        body, crc, size = member_body(mib, 1, pool)
    bio, central = io.BytesIO(), []
    small = [corpus.zipf_text(6000 + k, 0x7A000 + k) for k in range(1000)]
    entries = []
    for k, text in enumerate(small):
        if k % 250 == 0:
            entries.append(("large%d.txt" % (k // 250), body, crc, size))
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        entries.append(("small%04d.txt" % k, co.compress(text) + co.flush(), zlib.crc32(text), len(text)))
    for name, comp, c, n in entries:
        at = bio.tell()
        nm = name.encode()
        bio.write(struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", 20, 0, 8, 0, 0x21, c, len(comp), n, len(nm), 0) + nm + comp)
        central.append(struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 20, 20, 0, 8, 0, 0x21, c, len(comp), n, len(nm), 0, 0, 0, 0, 0, at) + nm)
    cd = bio.tell()
    bio.write(b"".join(central))
    bio.write(struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, len(entries), len(entries), bio.tell() - cd, cd, 0))
    return bio.getvalue(), len(entries), sum(e[3] for e in entries), crc


def report(what, nbytes, wall, kernel, **more):
    print(json.dumps(dict({"leg": what, "wall_median_ms": round(statistics.median(wall), 3), "wall_ms": [round(s, 3) for s in wall],
                           "wall_spread_ms": round(max(wall) - min(wall), 3), "kernel_median_ms": round(statistics.median(kernel), 3),
                           "kernel_ms": [round(s, 3) for s in kernel], "GiB_per_s_wall": round(nbytes / 2**30 / (statistics.median(wall) / 1e3), 3)},
                          **more)), flush=True)


class KernelClock:
    """Adds up pzg_last_kernel_ms after every call of the library's that the mirrors make."""

    def __init__(self, ctx):
        from pure_zlib_amd import _ffi
        self.ms, self.ctx, L = 0.0, ctx, _ffi.lib()
        for name in ("pzg_gzip_find_members", "pzg_gzip_layout", "pzg_decompress_many", "pzg_decompress_many_segments", "pzg_index_scan_many",
                     "pzg_index_scan"):
            if hasattr(L, name):
                self._wrap(L, name)

    def _wrap(self, L, name):
        real = getattr(L, name)

        def timed(*a):
            rc = real(*a)
            ms = self.ctx.last_kernel_ms()
            self.ms += ms if ms > 0 else 0.0
            return rc
        setattr(L, name, timed)


def sample(fn, clock):
    wall, kernel = [], []
    for k in range(7):
        clock.ms = 0.0
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= 2:
            wall.append((t1 - t0) * 1e3)
            kernel.append(clock.ms)
    return wall, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["curve", "batched", "zip"])
    ap.add_argument("--mib", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--split", type=int, default=1)       # 0: nothing is split; otherwise every member of the file is
    ap.add_argument("--chunks", type=int, nargs="+", default=[32, 64, 128])  # KiB
    a = ap.parse_args()
    # every input first, with its pool of workers; only then the package, the library and the device
    if a.leg == "zip":
        blob, nentries, total, crc = zip_archive(a.mib[0])
    else:
        members = gzip_members(a.mib if a.leg == "curve" else a.mib[:1])
    import numpy as np
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    ctx = P.Context(0)
    clock = KernelClock(ctx)
    lib = os.path.dirname(os.path.abspath(P.__file__))
    if a.leg == "curve":
        from pure_zlib_amd.gzfile import decompress_gzip_file
        for mib, one, each, _crc in members:
            z, size, per = one * 8, each * 8, len(one)  # (equal members: the same bytes eight times decode as eight members do)
            for chunk in (a.chunks if a.split else [0]):
                kw = dict(split=a.split, split_chunk=chunk << 10) if a.split else {}
                got = []
                wall, kernel = sample(lambda: got.append(decompress_gzip_file(z, ctx=ctx, **kw)) or got.__delitem__(slice(0, -1)), clock)
                assert got[-1].is_right() and len(got[-1].value) == size
                report("curve: 8 members of %d MiB compressed, %s" % (mib, "split, chunk %d KiB" % chunk if a.split else "a wavefront per member"),
                       size, wall, kernel, member_bytes=per, decoded_bytes=size, package=lib)
    elif a.leg == "batched":
        mib, one, each, _crc = members[0]
        z, size, per = one * 8, each * 8, len(one)
        buf = np.frombuffer(z, dtype=np.uint8)
        off = np.array([k * per + 10 for k in range(8)], dtype=np.uint64)
        ln = np.full(8, per - 18, dtype=np.uint64)
        room = size // 8 // (1 << 20) + 2
        for chunk in a.chunks:
            def many():
                r = ctx.index_scan_many(buf, off, ln, np.arange(9) * room, chunk << 10, 1 << 20)
                assert (r[4] == 0).all()
            wall, kernel = sample(many, clock)
            report("batched: ONE pzg_index_scan_many over 8 bodies of %d MiB, chunk %d KiB" % (mib, chunk), size, wall, kernel)

            def looped():
                L = _ffi.lib()
                for k in range(8):
                    pts, win = np.zeros((room, 2), dtype=np.uint64), np.zeros((room, 32768), dtype=np.uint8)
                    n, st, ol, used = C.c_uint32(0), C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
                    body = buf[int(off[k]):int(off[k] + ln[k])]
                    _ffi.check(L.pzg_index_scan(ctx.handle, body.ctypes.data, len(body), chunk << 10, 1 << 20, pts.ctypes.data, room, C.byref(n),
                                                win.ctypes.data, C.byref(ol), C.byref(st), None, C.byref(used), 0), ctx.handle)
                    assert st.value == 0
            wall, kernel = sample(looped, clock)
            report("batched: EIGHT pzg_index_scan calls on the same bodies, chunk %d KiB" % chunk, size, wall, kernel)
    else:
        from pure_zlib_amd.zip import read_zip
        for chunk in (a.chunks if a.split else [0]):
            kw = dict(split=a.split, split_chunk=chunk << 10) if a.split else {}
            got = []
            wall, kernel = sample(lambda: got.append(read_zip(blob, ctx=ctx, **kw)) or got.__delitem__(slice(0, -1)), clock)
            assert len(got[-1]) == nentries and zlib.crc32(got[-1]["large3.txt"]) == crc
            report("zip: 4 members of %d MiB compressed and 1,000 small ones, %s" % (a.mib[0], "split, chunk %d KiB" % chunk if a.split else "one launch"),
                   total, wall, kernel, archive_bytes=len(blob), package=lib)
    ctx.close()


if __name__ == "__main__":
    main()
