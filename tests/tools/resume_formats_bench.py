#!/usr/bin/env python3
"""The incremental bench's shape (bench.py's incremental leg: 4,096 resumable decoders fed 32 KiB pieces of 256 KiB level-6 text
streams, 192 KiB rooms, the median of five passes) for zlib decoders and for gzip decoders over the same DEFLATE bodies, measured one
after the other in one process; and what the gzip path costs per feed call beyond the zlib one (its CRC pass, the 8-byte longer
headers aside).  Prints one JSON line.

    python tests/tools/resume_formats_bench.py [--decoders 4096] [--passes 5]
"""
import argparse
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decoders", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import corpus
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi, benchmark as HB
    plain = [corpus.zipf_text(256 * 1024, 7000 + k) for k in range(32)]
    zs = [zlib.compress(t, 6) for t in plain]
    gz = [b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + z[2:-4] + struct.pack("<II", zlib.crc32(t), len(t)) for z, t in zip(zs, plain)]
    ctx = P.Context(0)
    out = {}
    for name, streams, fmt in (("zlib", zs, 0), ("gzip", gz, _ffi.GZIP), ("zlib_again", zs, 0)):
        r = HB.incremental_throughput(ctx, streams, plain, n_decoders=args.decoders, passes=args.passes, format=fmt)
        out[name] = {k: r[k] for k in ("decoders", "feed_calls", "GiBps", "GiBps_samples", "ms_per_feed_call", "us_per_decoder_feed", "ok")}
        out[name]["waiting_for_kernels_ms"] = (r.get("per_call_ms") or {}).get("waiting_for_kernels")
    base = (out["zlib"]["ms_per_feed_call"] + out["zlib_again"]["ms_per_feed_call"]) / 2
    out["gzip_minus_zlib_ms_per_feed_call"] = round(out["gzip"]["ms_per_feed_call"] - base, 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
