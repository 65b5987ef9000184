"""Lab tool (GPU box): the headline batch -- 65,536 x 32 KiB level-6 payloads, device pointers, ring 11 -- timed in ONE process as
zlib streams, as the same payloads raw (PZG_RAW) and raw with the CRC-32 pass (PZG_RAW | PZG_CRC32).  Launches alternate between the
three; six warm-ups each, then the median of five kernel times each (HIP events on the launch stream), as the headline does.
The yardstick is the zlib figure of the same run.  Usage:
    python tests/tools/raw_bench.py [--pool 2048] [--streams 65536] [--out profiles/raw_vs_zlib.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import bench
    import pure_zlib_amd as P
    from devbatch import DeviceBatch
    texts, zs = bench.build_pool(argparse.Namespace(workload="l6_32k", pool=args.pool, blob_bytes=32768, level=6, gzip=False))
    pick = np.random.default_rng(0xC4).integers(0, len(zs), size=args.streams)
    legs = {"zlib": (DeviceBatch(texts, zs, pick), {}),
            "raw": (DeviceBatch(texts, [z[2:-4] for z in zs], pick), dict(raw=True))}
    legs["raw+crc32"] = (legs["raw"][0], dict(raw=True, crc32=True))
    ctx = P.Context(0)
    ctx.set_ring_bits(11)
    ms = {k: [] for k in legs}

    def launch(name):
        b, kw = legs[name]
        ctx.decompress_many_device(b.d_in.data_ptr(), b.d_in_off.data_ptr(), b.d_in_len.data_ptr(), b.d_out.data_ptr(), b.d_out_off.data_ptr(),
                                   b.d_out_cap.data_ptr(), b.d_out_len.data_ptr(), b.d_status.data_ptr(), b.d_detail.data_ptr(),
                                   b.d_in_used.data_ptr(), b.d_adler.data_ptr(), b.n, sync=True, **kw)
        assert int((b.d_status != 0).sum()) == 0, name
        return ctx.last_kernel_ms()

    for _ in range(args.warmup):
        for name in legs:
            launch(name)
    for _ in range(args.samples):
        for name in legs:
            ms[name].append(launch(name))
    nbytes = float(legs["zlib"][0].out_cap.sum())
    rate = {k: nbytes / 2**30 / (float(np.median(v)) * 1e-3) for k, v in ms.items()}
    lines = ["raw_bench: %d x 32 KiB level-6 payloads (pool %d), ring 11, device pointers, one process, launches alternating;" % (args.streams, args.pool),
             "%d warm-ups each, median of %d kernel times each (GiB/s of decoded bytes)" % (args.warmup, args.samples)]
    for k in legs:
        lines.append("  %-10s %8.2f GiB/s   median %.3f ms   samples %s" % (k, rate[k], float(np.median(ms[k])), " ".join("%.3f" % x for x in ms[k])))
    lines.append("  raw / zlib        %.4f" % (rate["raw"] / rate["zlib"]))
    lines.append("  raw+crc32 / zlib  %.4f   (the CRC-32 pass: %.3f ms)" % (rate["raw+crc32"] / rate["zlib"], float(np.median(ms["raw+crc32"])) - float(np.median(ms["raw"]))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
