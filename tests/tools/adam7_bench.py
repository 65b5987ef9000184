#!/usr/bin/env python3
"""Measures the Adam7 path of pure_zlib_amd/png.py (profiles/adam7.txt): a batch of non-interlaced images through read_png_many -- the
figure to hold against the same run on the parent commit, whose plain path issues the same launches (--plain-only runs on a tree
without the adam7 keyword) -- the same pixels interlaced with adam7=True, the kernel ms of the pzg_adam7_many launch alone, and the
bytes a second it moves (passes read + rows written) beside a device-to-device copy of the same bytes: the launch is pure data
movement, so the gap is what is left to win.  Medians of five after two warm-up rounds, every sample printed.

    python tests/tools/adam7_bench.py [--images 1024] [--size 512] [--distinct 16] [--plain-only]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from png_bench import smooth_rgb  # noqa: E402


def timed(fn, rounds=7, warm=2):
    out = []
    for it in range(rounds):
        t0 = time.perf_counter()
        extra = fn()
        if it >= warm:
            out.append(((time.perf_counter() - t0) * 1e3, extra))
    return out


def line(what, samples, tail=""):
    print("  %-22s ms %s  median %.3f%s" % (what, " ".join("%.3f" % v for v in samples), statistics.median(samples), tail))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=16, help="distinct images the batch replicates (the writer is host Python)")
    ap.add_argument("--plain-only", action="store_true", help="the non-interlaced batch only: what a tree without adam7= can run")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import png
    import pngcases as PC
    ctx = P.Context(0)
    rng = np.random.default_rng(1024)
    raws = [smooth_rgb(rng, args.size, args.size) for _ in range(min(args.distinct, args.images))]
    pick = [i % len(raws) for i in range(args.images)]
    plain = [PC.write_png(args.size, args.size, 2, 8, r, "adaptive") for r in raws]
    batch = [plain[i] for i in pick]
    pixels = args.images * args.size * args.size * 3
    print("%d RGB 8-bit images of %d x %d (%d distinct), %d bytes of pixels" % (args.images, args.size, args.size, len(raws), pixels))

    def check(got):
        for i in (0, args.images // 2, args.images - 1):
            assert got[i].data.tobytes() == raws[pick[i]].tobytes(), i

    def run_plain():
        check(png.read_png_many(batch, ctx=ctx))
    line("plain, read_png_many", [ms for ms, _x in timed(run_plain)], "  (host parse and upload, two launches, one copy out)")
    if not args.plain_only:
        import adam7cases as A
        laced = [A.write_png(args.size, args.size, 2, 8, r, "adaptive") for r in raws]
        lbatch = [laced[i] for i in pick]

        def run_laced():
            check(png.read_png_many(lbatch, ctx=ctx, adam7=True))
            return ctx.last_kernel_ms()  # the last launch of the call: pzg_adam7_many
        s = timed(run_laced)
        line("interlaced, adam7=True", [ms for ms, _x in s], "  (three launches)")
        k = [x for _ms, x in s]
        moved = 2 * pixels  # the passes read, the rows written
        line("pzg_adam7_many launch", k, "  (%.1f GB/s, passes read + rows written)" % (moved / statistics.median(k) / 1e6))
        a, b = torch.empty(pixels, dtype=torch.uint8, device="cuda"), torch.empty(pixels, dtype=torch.uint8, device="cuda")
        cp = []
        for it in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                cp.append(e0.elapsed_time(e1))
        line("device copy", cp, "  (%.1f GB/s, %d bytes read and as many written)" % (moved / statistics.median(cp) / 1e6, pixels))
    ctx.close()


if __name__ == "__main__":
    main()
