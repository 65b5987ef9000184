#!/usr/bin/env python3
"""Measures the floating-point predictor's path (profiles/tiff_fp.txt): the pzg_unshuffle_many launch alone (pzg_last_kernel_ms) on a
batch of 256 x 256 tiles for float32 gray, float32 RGB, float16 gray, float64 gray and float32 gray without the sum (the shuffle filter
alone), each beside a device-to-device copy of the same bytes and beside pzg_unpredict_many with Predictor 2 on the same geometry, in
the same process; one whole-image float32 strip, which only the row slices spread over the device; read_tiff_many(float_predictor=True)
end to end on one large tiled float32 file, with PIL / libtiff beside it where PIL is installed (measured first, in a process that
is gone before the device is opened).  Medians of five after two warm-up rounds, every sample printed.

    python tests/tools/tiff_fp_bench.py [--tiles 16384] [--strip 8192] [--large 8192]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from adam7_bench import line, timed  # noqa: E402
from expand_bench import device_copy_ms  # noqa: E402
from tiff_bench import pil_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16384)
    ap.add_argument("--strip", type=int, default=8192, help="side of the whole-image strip (float32 gray)")
    ap.add_argument("--large", type=int, default=8192, help="side of the large tiled file (float32 gray, 256 x 256 tiles)")
    args = ap.parse_args()
    import fpcases as F
    import tiffcases as T
    rng = np.random.default_rng(4096)
    side = args.large
    big = (np.add.outer(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32)) * np.float32(0.125)
           + rng.standard_normal((side, side), dtype=np.float32)).reshape(side, side, 1)  # a slope with noise on it: an elevation model's bytes
    large = T.write_tiff([F.float_page(big, False, tile=(256, 256), level=1)])
    pil = pil_ms([("large file", [large])], 1)

    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import tiff
    from pure_zlib_amd.zlib import UNPREDICT_DESC, UNSHUFFLE_DESC
    ctx = P.Context(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda")  # noqa: E731
    n, s = args.tiles, 256
    print("%d tiles of %d x %d: the launch alone" % (n, s, s))

    def stage(name, jobs, rows, pixels, b, spp, summed=True):
        srb = pixels * spp * b
        moved = jobs * rows * srb
        src = torch.randint(0, 256, (moved + 16,), dtype=torch.uint8, device="cuda")
        dst = torch.empty(moved + 16, dtype=torch.uint8, device="cuda")
        d_len = up(np.full(jobs, rows * srb, np.uint64))
        d_status, d_detail = torch.zeros(jobs, dtype=torch.int32, device="cuda"), torch.zeros(2 * jobs, dtype=torch.int32, device="cuda")

        def geometry(dtype):
            desc = np.zeros(jobs, dtype)
            desc["src_off"] = desc["dst_off"] = np.arange(jobs, dtype=np.uint64) * (rows * srb)
            desc["dst_stride"], desc["src_row_bytes"], desc["rows"], desc["win_rows"], desc["win_bytes"] = srb, srb, rows, rows, srb
            return desc
        fp, p2 = geometry(UNSHUFFLE_DESC), geometry(UNPREDICT_DESC)
        fp["elem_bytes"], fp["sum_stride"], fp["reverse"] = b, spp if summed else 0, 1
        p2["predictor"], p2["sample_bytes"], p2["samples"] = 2, b, spp
        d_fp, d_p2 = up(fp), up(p2)
        torch.cuda.synchronize()

        def launch(call, d_desc):
            call(src.data_ptr(), d_len.data_ptr(), dst.data_ptr(), d_desc.data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), jobs)
            return ctx.last_kernel_ms()
        k2 = [x for _ms, x in timed(lambda: launch(ctx.unpredict_many_device, d_p2))]
        assert not d_status.any()
        k = [x for _ms, x in timed(lambda: launch(ctx.unshuffle_many_device, d_fp))]
        assert not d_status.any()
        # the first and the last rows of the launch back against the reference
        few = min(rows, 3)
        for at in (0, moved - few * srb):
            one = F.reconstruct(src[at:at + few * srb].cpu().numpy().reshape(few, srb), b, spp if summed else 0, True)
            assert np.array_equal(dst[at:at + few * srb].cpu().numpy().reshape(few, srb), one)
        line(name, k, "  (%.1f GB/s, %d bytes read and as many written)" % (2 * moved / statistics.median(k) / 1e6, moved))
        del src, dst
        cp = device_copy_ms(torch, moved)
        line("  device copy", cp, "  (%.1f GB/s; the launch takes %.2f times as long)" % (2 * moved / statistics.median(cp) / 1e6,
                                                                                          statistics.median(k) / statistics.median(cp)))
        line("  predictor 2 stage", k2, "  (%.1f GB/s; the launch takes %.2f times as long)" % (2 * moved / statistics.median(k2) / 1e6,
                                                                                               statistics.median(k) / statistics.median(k2)))
    stage("float32 gray", n, s, s, 4, 1)
    stage("float32 RGB", n, s, s, 4, 3)
    stage("float16 gray", n, s, s, 2, 1)
    stage("float64 gray", n, s, s, 8, 1)
    stage("float32 gray, no sum", n, s, s, 4, 1, summed=False)
    print("one strip of %d x %d float32 gray: the row slices, rows of several chunks read twice" % (args.strip, args.strip))
    stage("float32 gray", 1, args.strip, args.strip, 4, 1)

    print("read_tiff_many(float_predictor=True) end to end (host parse and upload, two launches, one copy out)")

    def run_large():
        got = tiff.read_tiff_many([large], ctx=ctx, float_predictor=True)
        assert got[0][0].data.tobytes() == big.tobytes()
    k = [ms for ms, _x in timed(run_large)]
    line("one file %d x %d" % (side, side), k, "  (float32 gray, %d tiles of 256 x 256, %d bytes of file, %.1f MB/s of pixels)" %
         ((side // 256) ** 2, len(large), big.nbytes / statistics.median(k) / 1e3))
    if pil is None:
        print("  PIL / libtiff: not installed")
    else:
        for name, samples in pil:
            line("  PIL, one process, %s" % name, samples, "  (read_tiff_many takes %.2f times as long)" % (statistics.median(k) / statistics.median(samples)))
    ctx.close()


if __name__ == "__main__":
    main()
