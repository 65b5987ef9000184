"""One LARGE stream: today's path (one wavefront) against the indexed path (pure_zlib_amd/indexed.py).  Not bench.py.

    python tests/tools/indexed_bench.py make  --mib 1024 --file build/tmp_big.z     # the input, once (CPU only)
    python tests/tools/indexed_bench.py plain --file build/tmp_big.z                # pzg_decompress_many, n = 1
    python tests/tools/indexed_bench.py index --file build/tmp_big.z                # pzg_index_build, ..._many_segments, read()

Every leg is a process of its own (run each under its own `timeout`); PZG_LIB=path/to/libpzg.so times another build of the library --
the parent commit's -- with the same script (`plain` only needs the old ABI).  Device pointers, HIP events (pzg_last_kernel_ms: the
events the library records around its kernels), two warm-ups, then five samples: the median and the samples are printed as one JSON
line per figure.

The input is ONE zlib stream of corpus text compressed at level 6, written the way pigz writes it so that 16 CPUs can make a GiB of it
in seconds: 16 MiB pieces compressed independently and joined with full flushes (byte-aligned, the history reset every 16 MiB), one
Adler-32 over all of it.
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PIECE = 16 << 20


def _piece(args):
    import corpus
    seed, last = args
    text = corpus.zipf_text(PIECE, 1000 + seed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(text) + co.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH), zlib.adler32(text), len(text)


def make(path, mib):
    from multiprocessing import Pool
    from pure_zlib_amd.indexed import adler32_combine
    n = max(1, mib * (1 << 20) // PIECE)
    with Pool(min(16, n)) as pool, open(path, "wb") as f:
        f.write(b"\x78\x9c")
        adler, total = 1, 0
        for body, a, ln in pool.imap(_piece, [(k, k == n - 1) for k in range(n)]):
            f.write(body)
            adler, total = adler32_combine(adler, a, ln), total + ln
        f.write(adler.to_bytes(4, "big"))
    note = {"made": path, "decoded_bytes": total, "compressed_bytes": os.path.getsize(path)}
    with open(path + ".json", "w") as f:
        json.dump(note, f)
    print(json.dumps(note))


def timed(what, nbytes, fn, ms):
    """fn() seven times; ms() after each: the library's own event span of the call."""
    samples = []
    for k in range(7):
        fn()
        if k >= 2:
            samples.append(ms())
    med = statistics.median(samples)
    print(json.dumps({"leg": what, "median_ms": round(med, 3), "samples_ms": [round(s, 3) for s in samples], "spread": round((max(samples) - min(samples)) / med, 4),
                      "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 3)}), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["make", "plain", "index"])
    ap.add_argument("--file", default=os.path.join(ROOT, "build", "tmp_big.z"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--span", type=int, default=1 << 20)
    a = ap.parse_args()
    if a.leg == "make":
        os.makedirs(os.path.dirname(a.file), exist_ok=True)
        return make(a.file, a.mib)
    import numpy as np
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    import ctypes as C
    z = open(a.file, "rb").read()
    ctx = P.Context(0)
    dev = torch.device("cuda", 0)
    as_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t_in = as_dev(np.frombuffer(z, dtype=np.uint8).copy())
    u64 = lambda v: as_dev(np.array([v], dtype=np.int64))  # noqa: E731
    res = dict(out_len=u64(0), status=as_dev(np.array([-1], np.int32)), detail=as_dev(np.zeros(2, np.int32)), in_used=u64(0), adler=as_dev(np.zeros(1, np.int32)))
    out_len = json.load(open(a.file + ".json"))["decoded_bytes"]  # (written by `make`)
    t_out = torch.empty(out_len + 64, dtype=torch.uint8, device=dev)
    print(json.dumps({"file": a.file, "compressed_bytes": len(z), "decoded_bytes": out_len, "lib": _ffi.LIB_PATH}), flush=True)
    in_off, in_len, out_off, out_cap = u64(0), u64(len(z)), u64(0), u64(out_len)

    if a.leg == "plain":
        def plain():
            ctx.decompress_many_device(in_base=t_in.data_ptr(), in_off=in_off.data_ptr(), in_len=in_len.data_ptr(), out_base=t_out.data_ptr(),
                                       out_off=out_off.data_ptr(), out_cap=out_cap.data_ptr(), out_len=res["out_len"].data_ptr(),
                                       status=res["status"].data_ptr(), detail=res["detail"].data_ptr(), in_used=res["in_used"].data_ptr(),
                                       adler=res["adler"].data_ptr(), n=1, sync=True)
            assert int(res["status"].item()) == 0
        timed("plain: pzg_decompress_many, n = 1", out_len, plain, ctx.last_kernel_ms)
        return

    L = _ffi.lib()
    body = t_in[2:]  # (a view: the zlib header parsed by hand, as the mirror does)
    max_points = out_len // a.span + 16
    t_pts = torch.zeros(2 * max_points, dtype=torch.int64, device=dev)
    t_win = torch.zeros(max_points * 32768, dtype=torch.uint8, device=dev)
    npoints, status, adler, olen, used = C.c_uint32(0), C.c_int32(-1), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)

    def build():
        _ffi.check(L.pzg_index_build(ctx.handle, body.data_ptr(), len(z) - 2, t_out.data_ptr(), out_len, a.span, t_pts.data_ptr(), max_points,
                                     C.byref(npoints), t_win.data_ptr(), C.byref(olen), C.byref(status), None, C.byref(used), C.byref(adler), _ffi.DEVICE_PTRS), ctx.handle)
        assert status.value == 0 and olen.value == out_len and npoints.value <= max_points
    timed("build: pzg_index_build, span %d" % a.span, out_len, build, ctx.last_kernel_ms)
    n = npoints.value
    whole = t_out.cpu().numpy().copy()[:out_len]
    pts = t_pts.cpu().numpy().view(np.uint64).reshape(-1, 2)[:n]
    index_bytes = 16 * n + 32768 * n
    print(json.dumps({"points": n, "index_bytes": index_bytes, "share_of_compressed": round(index_bytes / len(z), 4)}), flush=True)
    from pure_zlib_amd.indexed import Index, adler32_combine
    ix = Index("zlib", a.span, pts, t_win.cpu().numpy().reshape(-1, 32768)[:n], out_len, 2, used.value, int.from_bytes(z[-4:], "big"), (0, 0))
    segs = ix.segments()
    m = len(segs)
    arr = lambda k, dt=np.int64: as_dev(np.array([s[k] for s in segs], dtype=dt))  # noqa: E731
    s_off, s_len, s_sb, s_eb = arr(0), arr(1), arr(2, np.uint8), arr(3)
    s_oo, s_cap = arr(4), as_dev(np.array([s[5] - s[4] for s in segs], dtype=np.int64))
    w = np.array([0] + [min(int(p), 32768) for p in pts[:, 1]], dtype=np.int64)
    d_off = as_dev(np.array([0] + [32768 * k + 32768 - int(w[k + 1]) for k in range(n)], dtype=np.int64))
    d_len = as_dev(w)
    r = dict(out_len=torch.zeros(m, dtype=torch.int64, device=dev), status=torch.full((m,), -1, dtype=torch.int32, device=dev),
             detail=torch.zeros(2 * m, dtype=torch.int32, device=dev), in_used=torch.zeros(m, dtype=torch.int64, device=dev),
             sums=torch.zeros(m, dtype=torch.int32, device=dev))
    t_out.zero_()

    def segments():
        _ffi.check(L.pzg_decompress_many_segments(ctx.handle, body.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), s_sb.data_ptr(), s_eb.data_ptr(),
                                                  t_win.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), t_out.data_ptr(), s_oo.data_ptr(), s_cap.data_ptr(),
                                                  r["out_len"].data_ptr(), r["status"].data_ptr(), r["detail"].data_ptr(), r["in_used"].data_ptr(),
                                                  r["sums"].data_ptr(), m, _ffi.DEVICE_PTRS | _ffi.LPT_ORDER), ctx.handle)
        torch.cuda.synchronize()
    timed("segments: pzg_decompress_many_segments, %d segments" % m, out_len, segments, ctx.last_kernel_ms)
    assert (r["status"] == 0).all().item()
    total = 1
    for k, sm in enumerate(r["sums"].cpu().numpy().view(np.uint32)):
        total = adler32_combine(total, int(sm), segs[k][5] - segs[k][4])
    assert total == int.from_bytes(z[-4:], "big") and np.array_equal(t_out.cpu().numpy()[:out_len], whole), "the segments' bytes are not the stream's"
    # a 1 MiB read from the middle, through the mirror (host pointers: staging and copies included -- wall clock)
    ix.fingerprint = __import__("pure_zlib_amd.indexed", fromlist=["_fingerprint"])._fingerprint(z, 2 + used.value)
    walls = []

    def read():
        t0 = time.perf_counter()
        got = ix.read(z, out_len // 2, 1 << 20, ctx=ctx)
        walls.append((time.perf_counter() - t0) * 1e3)
        assert got == whole[out_len // 2:out_len // 2 + (1 << 20)].tobytes()
    timed("read: 1 MiB from the middle (kernel span)", 1 << 20, read, ctx.last_kernel_ms)
    print(json.dumps({"leg": "read: 1 MiB from the middle (wall clock, host pointers)", "median_ms": round(statistics.median(walls[2:]), 3),
                      "samples_ms": [round(x, 3) for x in walls[2:]]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
