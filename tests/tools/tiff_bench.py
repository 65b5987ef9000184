#!/usr/bin/env python3
"""Measures the TIFF path (profiles/tiff.txt): the pzg_unpredict_many launch alone (pzg_last_kernel_ms) on a batch of 256 x 256 tiles
for four formats, beside a device-to-device copy of the same bytes -- the launch is pure data movement, so the copy is the yardstick
(profiles/expand.txt) --; one whole-image strip, which only the row slices spread over the device; read_tiff_many end to end on one
large tiled file and on a batch of small ones, with PIL / libtiff on all granted cores beside it where PIL is installed (measured
first, in processes that are gone before the device is opened).  Medians of five after two warm-up rounds, every sample printed.

    python tests/tools/tiff_bench.py [--tiles 16384] [--strip 8192] [--large 8192] [--files 1024]
"""
import argparse
import io
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
from png_bench import smooth_rgb  # noqa: E402


def _pil_decode(blob):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob))).shape


def pil_ms(batches, procs):
    """[(name, samples)]: every batch decoded by PIL in `procs` processes, or None where PIL or its libtiff is missing."""
    try:
        from PIL import features
        if not features.check("libtiff"):
            return None
    except ImportError:
        return None
    import multiprocessing as mp
    out = []
    with mp.get_context("fork").Pool(procs) as pool:
        for name, blobs in batches:
            out.append((name, [ms for ms, _x in timed(lambda: pool.map(_pil_decode, blobs, chunksize=max(1, len(blobs) // (4 * procs))))]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16384)
    ap.add_argument("--strip", type=int, default=8192, help="side of the whole-image strip (RGB8)")
    ap.add_argument("--large", type=int, default=8192, help="side of the large tiled file (RGB8, 256 x 256 tiles)")
    ap.add_argument("--files", type=int, default=1024, help="small files of the batch (256 x 256 RGB8, one strip)")
    ap.add_argument("--distinct", type=int, default=16)
    args = ap.parse_args()
    import tiffcases as T
    rng = np.random.default_rng(4096)
    big = smooth_rgb(rng, args.large, args.large).reshape(args.large, args.large, 3)
    large = T.write_tiff([T.Page(big, tile=(256, 256), predictor=2, level=1)])
    smalls = [smooth_rgb(rng, 256, 256).reshape(256, 256, 3) for _ in range(min(args.distinct, args.files))]
    small_blobs = [T.write_tiff([T.Page(a, predictor=2)]) for a in smalls]
    pick = [i % len(smalls) for i in range(args.files)]
    batch = [small_blobs[i] for i in pick]
    procs = min(16, len(os.sched_getaffinity(0)))
    pil = pil_ms([("large file", [large]), ("batch", batch)], procs)

    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import tiff
    from pure_zlib_amd.zlib import UNPREDICT_DESC
    ctx = P.Context(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda")  # noqa: E731
    n, s = args.tiles, 256
    print("%d tiles of %d x %d: the launch alone" % (n, s, s))

    def stage(name, jobs, rows, srb, predictor, sb, spp):
        src = torch.randint(0, 256, (jobs * rows * srb + 16,), dtype=torch.uint8, device="cuda")
        dst = torch.empty(jobs * rows * srb + 16, dtype=torch.uint8, device="cuda")
        desc = np.zeros(jobs, UNPREDICT_DESC)
        desc["src_off"] = desc["dst_off"] = np.arange(jobs, dtype=np.uint64) * (rows * srb)
        desc["dst_stride"], desc["src_row_bytes"], desc["rows"], desc["win_rows"], desc["win_bytes"] = srb, srb, rows, rows, srb
        desc["predictor"], desc["sample_bytes"], desc["samples"] = predictor, sb, spp
        d_desc, d_len = up(desc), up(np.full(jobs, rows * srb, np.uint64))
        d_status, d_detail = torch.zeros(jobs, dtype=torch.int32, device="cuda"), torch.zeros(2 * jobs, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def launch():
            ctx.unpredict_many_device(src.data_ptr(), d_len.data_ptr(), dst.data_ptr(), d_desc.data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), jobs)
            return ctx.last_kernel_ms()
        k = [x for _ms, x in timed(launch)]
        assert not d_status.any()
        # one job back against the reference
        one = T.reconstruct(src[:rows * srb].cpu().numpy().reshape(rows, srb), predictor, sb, spp, False)
        assert np.array_equal(dst[:rows * srb].cpu().numpy().reshape(rows, srb), one)
        moved = jobs * rows * srb
        line(name, k, "  (%.1f GB/s, %d bytes read and as many written)" % (2 * moved / statistics.median(k) / 1e6, moved))
        del src, dst
        cp = device_copy_ms(torch, moved)
        line("  device copy", cp, "  (%.1f GB/s; the launch takes %.2f times as long)" % (2 * moved / statistics.median(cp) / 1e6,
                                                                                          statistics.median(k) / statistics.median(cp)))
    stage("RGB8, predictor 2", n, s, s * 3, 2, 1, 3)
    stage("Gray16, predictor 2", n, s, s * 2, 2, 2, 1)
    stage("RGBA8, predictor 2", n, s, s * 4, 2, 1, 4)
    stage("Gray32, predictor 1", n, s, s * 4, 1, 4, 1)
    print("one strip of %d x %d RGB8: the row slices" % (args.strip, args.strip))
    stage("RGB8, predictor 2", 1, args.strip, args.strip * 3, 2, 1, 3)

    print("read_tiff_many end to end (host parse and upload, two launches, one copy out)")

    def run_large():
        got = tiff.read_tiff_many([large], ctx=ctx)
        assert got[0][0].data.tobytes() == big.tobytes()
    k = [ms for ms, _x in timed(run_large)]
    line("one file %d x %d" % (args.large, args.large), k, "  (RGB8, %d tiles of 256 x 256, %d bytes of file, %.1f MB/s of pixels)" %
         ((args.large // 256) ** 2, len(large), big.nbytes / statistics.median(k) / 1e3))

    def run_batch():
        got = tiff.read_tiff_many(batch, ctx=ctx)
        for i in (0, len(batch) // 2, len(batch) - 1):
            assert got[i][0].data.tobytes() == smalls[pick[i]].tobytes(), i
    k2 = [ms for ms, _x in timed(run_batch)]
    line("%d files of 256 x 256" % len(batch), k2, "  (RGB8, one strip each, %d distinct, %.1f MB/s of pixels)" %
         (len(smalls), len(batch) * 256 * 256 * 3 / statistics.median(k2) / 1e3))
    if pil is None:
        print("  PIL / libtiff: not installed")
    else:
        for (name, samples), ours in zip(pil, (k, k2)):
            line("  PIL, %d processes, %s" % (procs, name), samples, "  (read_tiff_many takes %.2f times as long)" % (statistics.median(ours) / statistics.median(samples)))
    ctx.close()


if __name__ == "__main__":
    main()
