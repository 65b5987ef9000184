"""One LARGE stream that arrives once and is decoded once: today's path (one wavefront) against the parallel index scan followed by
the all-segments decode (pzg_index_scan + pzg_decompress_many_segments).  Not bench.py.  The input, the device-pointer event timing
and the sampling (two warm-ups, five samples) are tests/tools/indexed_bench.py's:

    python tests/tools/indexed_bench.py make  --mib 1024 --file build/tmp_big.z     # the input, once (CPU only)
    python tests/tools/indexed_bench.py plain --file build/tmp_big.z                # legs 1 / 2 (PZG_LIB=the parent's library: leg 1)
    python tests/tools/indexed_bench.py index --file build/tmp_big.z                # leg 3 (pzg_index_build; PZG_LIB as above)
    python tests/tools/scan_bench.py --file build/tmp_big.z [--chunk 32768]         # legs 4 and 5

Every leg is a process of its own.  Leg 5's sample k is the scan's kernel span of round k plus the segments' kernel span of round k
(two calls, both timed by the library's own events); the segments' combined Adler-32 must be the trailer's.  Kernel spans leave out
what a caller also waits for -- the scan's scratch (allocated and freed inside the call), the points' way to the host and the
segment arrays' way back -- so the same rounds are reported by the wall clock too: the pzg_index_scan call alone, and the round
from the scan's first line to the segments' last kernel (the checksum check behind it is not in it).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]


def report(what, nbytes, samples):
    med = statistics.median(samples)
    print(json.dumps({"leg": what, "median_ms": round(med, 3), "samples_ms": [round(s, 3) for s in samples],
                      "spread": round((max(samples) - min(samples)) / med, 4), "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=os.path.join(ROOT, "build", "tmp_big.z"))
    ap.add_argument("--span", type=int, default=1 << 20)
    ap.add_argument("--chunk", type=int, default=0)  # 0: the library's default
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    from pure_zlib_amd.indexed import Index, adler32_combine
    z = open(a.file, "rb").read()
    out_len = json.load(open(a.file + ".json"))["decoded_bytes"]
    ctx = P.Context(0)
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    as_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t_in = as_dev(np.frombuffer(z, dtype=np.uint8).copy())
    body = t_in[2:]
    t_out = torch.empty(out_len + 64, dtype=torch.uint8, device=dev)
    max_points = out_len // a.span + 16
    t_pts = torch.zeros(2 * max_points, dtype=torch.int64, device=dev)
    t_win = torch.zeros(max_points * 32768, dtype=torch.uint8, device=dev)
    npoints, status, olen, used = C.c_uint32(0), C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
    detail = (C.c_uint32 * 2)(0, 0)
    print(json.dumps({"file": a.file, "compressed_bytes": len(z), "decoded_bytes": out_len, "chunk": a.chunk or 128 << 10, "span": a.span}), flush=True)

    def scan():
        _ffi.check(L.pzg_index_scan(ctx.handle, body.data_ptr(), len(z) - 2, a.chunk, a.span, t_pts.data_ptr(), max_points, C.byref(npoints),
                                    t_win.data_ptr(), C.byref(olen), C.byref(status), detail, C.byref(used), _ffi.DEVICE_PTRS), ctx.handle)
        assert status.value == 0 and olen.value == out_len and npoints.value <= max_points, (status.value, detail[0], detail[1], olen.value)
        return ctx.last_kernel_ms()

    def segments():
        n = npoints.value
        pts = t_pts.cpu().numpy().view(np.uint64).reshape(-1, 2)[:n]
        ix = Index("zlib", a.span, pts, np.zeros((0, 32768), np.uint8), out_len, 2, used.value, 0, (0, 0))
        segs = ix.segments()
        m = len(segs)
        arr = lambda k, dt=np.int64: as_dev(np.array([s[k] for s in segs], dtype=dt))  # noqa: E731
        w = np.array([0] + [min(int(p), 32768) for p in pts[:, 1]], dtype=np.int64)
        d_off = as_dev(np.array([0] + [32768 * k + 32768 - int(w[k + 1]) for k in range(n)], dtype=np.int64))
        r = dict(out_len=torch.zeros(m, dtype=torch.int64, device=dev), status=torch.full((m,), -1, dtype=torch.int32, device=dev),
                 sums=torch.zeros(m, dtype=torch.int32, device=dev), used=torch.zeros(m, dtype=torch.int64, device=dev))
        keep = [arr(0), arr(1), arr(2, np.uint8), arr(3), d_off, as_dev(w), arr(4), as_dev(np.array([s[5] - s[4] for s in segs], dtype=np.int64))]
        _ffi.check(L.pzg_decompress_many_segments(ctx.handle, body.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                                  keep[3].data_ptr(), t_win.data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), t_out.data_ptr(),
                                                  keep[6].data_ptr(), keep[7].data_ptr(), r["out_len"].data_ptr(), r["status"].data_ptr(), None,
                                                  r["used"].data_ptr(), r["sums"].data_ptr(), m, _ffi.DEVICE_PTRS | _ffi.LPT_ORDER), ctx.handle)
        torch.cuda.synchronize()
        done = time.perf_counter()
        ms = ctx.last_kernel_ms()
        assert (r["status"] == 0).all().item()
        total = 1
        for k, sm in enumerate(r["sums"].cpu().numpy().view(np.uint32)):
            total = adler32_combine(total, int(sm), segs[k][5] - segs[k][4])
        assert total == int.from_bytes(z[-4:], "big"), "the segments' bytes are not the stream's"
        return ms, m, done

    scans, both, m, scan_wall, both_wall = [], [], 0, [], []
    for k in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = scan()
        t1 = time.perf_counter()
        g, m, t2 = segments()
        if k >= 2:
            scans.append(s)
            both.append(s + g)
            scan_wall.append((t1 - t0) * 1e3)
            both_wall.append((t2 - t0) * 1e3)
    report("scan: pzg_index_scan, chunk %d, %d points" % (a.chunk or 128 << 10, npoints.value), out_len, scans)
    report("scan + segments: pzg_index_scan then pzg_decompress_many_segments, %d segments" % m, out_len, both)
    report("scan, wall clock of the call (scratch allocated and freed in it)", out_len, scan_wall)
    report("scan + segments, wall clock (the points to the host, the segment arrays to the device, both calls)", out_len, both_wall)
    ctx.close()


if __name__ == "__main__":
    main()
