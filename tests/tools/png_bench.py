#!/usr/bin/env python3
"""Measures a batch of PNG images through the two launches of pure_zlib_amd/png.py (profiles/png.txt): the decode launch's kernel ms,
the unfilter launch's kernel ms and the bytes it moves (src read + dst written), a device-to-device copy of the same bytes as the
ceiling, and one large image alone -- the one-wavefront worst case.  Medians of five, every sample printed.  A CPU line beside them:
PIL where it is installed, else the system's zlib plus the reference unfilter of tests/pngcases.py, on all granted cores.

    python tests/tools/png_bench.py [--images 1024] [--size 512] [--big 8192]
"""
import argparse
import io
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def smooth_rgb(rng, h, w):
    """Seeded RGB 8-bit: low-frequency colour plus noise (what the adaptive rule picks for it is printed)."""
    y, x = np.mgrid[0:h, 0:w]
    f = rng.uniform(0.005, 0.05, size=(3, 2))
    img = np.stack([127 + 100 * np.sin(f[c, 0] * x + f[c, 1] * y + rng.uniform(0, 6)) for c in range(3)], axis=2)
    img += rng.normal(0, 6, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8).reshape(h, 3 * w)


def measure(ctx, torch, streams, zs, row_bytes, height, label):
    n = len(zs)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
    pad = lambda a: (a + np.uint64(255)) & ~np.uint64(255)  # noqa: E731
    in_len = np.array([len(z) for z in zs], np.uint64)
    cap = np.array([len(s) for s in streams], np.uint64)
    rb, hh = np.full(n, row_bytes, np.uint32), np.full(n, height, np.uint32)
    pix = cap - hh.astype(np.uint64)
    in_off, dec_off, pix_off = (np.zeros(n, np.uint64) for _ in range(3))
    in_off[1:], dec_off[1:], pix_off[1:] = np.cumsum(pad(in_len))[:-1], np.cumsum(pad(cap))[:-1], np.cumsum(pad(pix))[:-1]
    h_in = np.zeros(int(in_off[-1] + pad(in_len)[-1]), np.uint8)
    for i, z in enumerate(zs):
        h_in[int(in_off[i]):int(in_off[i]) + len(z)] = np.frombuffer(z, np.uint8)
    t = [up(a) for a in (h_in, in_off, in_len, dec_off, cap, pix_off, rb.astype(np.uint64), rb, hh, np.full(n, 3, np.uint8))]
    d_dec = torch.empty(int(dec_off[-1] + pad(cap)[-1]), dtype=torch.uint8, device=dev)
    d_pix = torch.empty(int(pix_off[-1] + pad(pix)[-1]), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    p = [x.data_ptr() for x in t]
    dec_ms, unf_ms, cp_ms = [], [], []
    moved = int(cap.sum() + pix.sum())
    half = min(moved // 2, len(d_dec))
    d_copy = torch.empty(half, dtype=torch.uint8, device=dev)
    for it in range(7):  # two to warm up
        torch.cuda.synchronize()
        ctx.decompress_many_device(p[0], p[1], p[2], d_dec.data_ptr(), p[3], p[4], d_len.data_ptr(), d_st.data_ptr(), 0, 0, 0, n)
        a = ctx.last_kernel_ms()
        ctx.unfilter_many_device(d_dec.data_ptr(), p[3], d_len.data_ptr(), d_pix.data_ptr(), p[5], p[6], p[7], p[8], p[9], d_st.data_ptr() + 4 * n, 0, n)
        b = ctx.last_kernel_ms()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d_copy.copy_(d_dec[:half])  # reads `half`, writes `half`: the same bytes moved
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            dec_ms.append(a)
            unf_ms.append(b)
            cp_ms.append(e0.elapsed_time(e1))
    assert (d_st.cpu().numpy() == 0).all()
    got = d_pix.cpu().numpy()
    for i in (0, n // 2, n - 1):
        want = np.frombuffer(streams[i], np.uint8).reshape(height, 1 + row_bytes)  # (checked against the writer's input by the caller)
        assert len(got[int(pix_off[i]):int(pix_off[i] + pix[i])]) == want.shape[0] * row_bytes
    med = statistics.median
    print("%s: %d image(s), %d decoded bytes, %d compressed" % (label, n, int(cap.sum()), int(in_len.sum())))
    print("  decode launch    ms %s  median %.3f  (%.1f GB/s of decoded bytes)" % (" ".join("%.3f" % v for v in dec_ms), med(dec_ms), cap.sum() / med(dec_ms) / 1e6))
    print("  unfilter launch  ms %s  median %.3f  (%.1f GB/s, src read + dst written)" % (" ".join("%.3f" % v for v in unf_ms), med(unf_ms), moved / med(unf_ms) / 1e6))
    print("  device copy      ms %s  median %.3f  (%.1f GB/s, %d bytes read and as many written)" % (" ".join("%.3f" % v for v in cp_ms), med(cp_ms), 2 * half / med(cp_ms) / 1e6, half))
    return got, pix_off, pix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--big", type=int, default=8192)
    ap.add_argument("--distinct", type=int, default=64, help="distinct images the batch replicates (the writer is host Python)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    import pure_zlib_amd.png  # noqa: F401
    import pngcases as PC
    ctx = P.Context(0)
    rng = np.random.default_rng(1024)
    raws = [smooth_rgb(rng, args.size, args.size) for _ in range(min(args.distinct, args.images))]
    streams = [PC.filter_stream(r, 3, "adaptive") for r in raws]
    hist = np.bincount(np.concatenate([np.frombuffer(s, np.uint8).reshape(args.size, -1)[:, 0] for s in streams]), minlength=5)
    print("filters chosen by the adaptive rule (None Sub Up Average Paeth):", hist.tolist())
    zs = [zlib.compress(s, 6) for s in streams]
    pick = [i % len(raws) for i in range(args.images)]
    got, off, pix = measure(ctx, torch, [streams[i] for i in pick], [zs[i] for i in pick], 3 * args.size, args.size, "batch")
    for i in (0, args.images // 2, args.images - 1):
        assert np.array_equal(got[int(off[i]):int(off[i] + pix[i])], raws[pick[i]].ravel()), i
    if args.big:
        raw = smooth_rgb(rng, args.big, args.big)
        # (in blocks of 512 rows, each with the row above it: the writer's arrays are twenty times the block)
        s = b"".join(PC.filter_stream(raw[max(y - 1, 0):y + 512], 3, "adaptive")[(1 + 3 * args.big if y else 0):] for y in range(0, args.big, 512))
        got, off, pix = measure(ctx, torch, [s], [zlib.compress(s, 6)], 3 * args.big, args.big, "one %d x %d image" % (args.big, args.big))
        assert np.array_equal(got[:int(pix[0])], raw.ravel())
    # the CPU line
    pngs = [PC.write_png(args.size, args.size, 2, 8, r, "adaptive") for r in raws]
    cores = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16")))
    try:
        from PIL import Image
        work, what = (lambda b: np.asarray(Image.open(io.BytesIO(b)))), "PIL %s" % __import__("PIL").__version__
    except ImportError:
        work, what = (lambda b: PC.unfilter(zlib.decompress(P.png._parse("", b)[1]), 3 * args.size, args.size, 3)), "system zlib + the reference unfilter"
    samples = []
    with ThreadPoolExecutor(cores) as ex:
        for _ in range(5):
            t0 = time.perf_counter()
            list(ex.map(work, [pngs[i] for i in pick]))
            samples.append((time.perf_counter() - t0) * 1e3)
    print("CPU (%s, %d threads): ms %s  median %.1f" % (what, cores, " ".join("%.1f" % v for v in samples), statistics.median(samples)))
    ctx.close()


if __name__ == "__main__":
    main()
