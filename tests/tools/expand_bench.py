#!/usr/bin/env python3
"""Measures the pixel expansion (profiles/expand.txt): the pzg_expand_many launch alone (pzg_last_kernel_ms) on a batch of images for
four source types, beside a device-to-device copy of as many bytes as the launch reads plus writes -- the launch is pure data
movement, so the gap is what is left to win; read_png_many on the non-interlaced RGB batch of tests/tools/adam7_bench.py without
expand -- the figure to hold against the same run on the parent commit (--plain-only runs on a tree without the keyword) -- and with
expand="rgba8" into device_out.  Medians of five after two warm-up rounds, every sample printed.

    python tests/tools/expand_bench.py [--images 1024] [--size 512] [--distinct 16] [--plain-only]
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
from png_bench import smooth_rgb  # noqa: E402


def device_copy_ms(torch, nbytes):
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = []
    for it in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=16, help="distinct images the batch replicates (the writer is host Python)")
    ap.add_argument("--plain-only", action="store_true", help="read_png_many without expand only: what a tree without the keyword can run")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import png
    import pngcases as PC
    ctx = P.Context(0)
    rng = np.random.default_rng(1024)
    n, s = args.images, args.size
    raws = [smooth_rgb(rng, s, s) for _ in range(min(args.distinct, n))]
    pick = [i % len(raws) for i in range(n)]
    plain = [PC.write_png(s, s, 2, 8, r, "adaptive") for r in raws]
    batch = [plain[i] for i in pick]
    print("%d images of %d x %d (%d distinct)" % (n, s, s, len(raws)))

    def run_plain():
        got = png.read_png_many(batch, ctx=ctx)
        for i in (0, n // 2, n - 1):
            assert got[i].data.tobytes() == raws[pick[i]].tobytes(), i
    line("plain, read_png_many", [ms for ms, _x in timed(run_plain)], "  (RGB 8, no expand: host parse and upload, two launches, one copy out)")
    if args.plain_only:
        ctx.close()
        return
    import expandcases as X
    from pure_zlib_amd.zlib import EXPAND_DESC
    out = torch.empty((n, s, s, 4), dtype=torch.uint8, device="cuda")
    offs, strides = [i * s * s * 4 for i in range(n)], [s * 4] * n

    def run_expand():
        got = png.read_png_many(batch, ctx=ctx, device_out=(out.data_ptr(), offs, strides), expand="rgba8")
        assert all(isinstance(g, png.PngImage) for g in got)
    line("expand='rgba8', device_out", [ms for ms, _x in timed(run_expand)], "  (three launches, nothing copied out)")
    ref = X.expand_reference(s, s, 2, 8, raws[pick[n - 1]].reshape(s, -1))
    assert np.array_equal(out[n - 1].cpu().numpy(), ref)
    # the launch alone
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda")  # noqa: E731
    pal = up(rng.integers(0, 1 << 32, size=256, dtype=np.uint64).astype(np.uint32))
    d_status, d_detail = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    for name, ct, depth, fmt in (("RGB 8 -> RGBA8", 2, 8, X.RGBA8), ("palette 8 -> RGBA8", 3, 8, X.RGBA8), ("gray 1 -> RGB8", 0, 1, X.RGB8),
                                 ("RGBA 16 -> RGBA8", 6, 16, X.RGBA8)):
        srb, orb = X.src_row_bytes(s, ct, depth), s * X.out_bytes(fmt)
        src = torch.randint(0, 256, (n * s * srb + 16,), dtype=torch.uint8, device="cuda")
        dst = torch.empty(n * s * orb + 16, dtype=torch.uint8, device="cuda")
        desc = np.zeros(n, EXPAND_DESC)
        desc["src_off"], desc["dst_off"] = np.arange(n, dtype=np.uint64) * (s * srb), np.arange(n, dtype=np.uint64) * (s * orb)
        desc["src_stride"], desc["dst_stride"], desc["width"], desc["height"] = srb, orb, s, s
        desc["color_type"], desc["bit_depth"], desc["out_format"], desc["pal_len"] = ct, depth, fmt, 256 if ct == 3 else 0
        d_desc = up(desc)
        torch.cuda.synchronize()

        def launch():
            ctx.expand_many_device(src.data_ptr(), dst.data_ptr(), pal.data_ptr(), d_desc.data_ptr(), d_status.data_ptr(), d_detail.data_ptr(), n)
            return ctx.last_kernel_ms()
        k = [x for _ms, x in timed(launch)]
        assert not d_status.any()
        moved = n * s * (srb + orb)
        line(name, k, "  (%.1f GB/s, %d bytes read + %d written)" % (moved / statistics.median(k) / 1e6, n * s * srb, n * s * orb))
        cp = device_copy_ms(torch, moved // 2)
        line("  device copy", cp, "  (%.1f GB/s, %d bytes read and as many written; the launch takes %.2f times as long)" %
             (moved / statistics.median(cp) / 1e6, moved // 2, statistics.median(k) / statistics.median(cp)))
    ctx.close()


if __name__ == "__main__":
    main()
