"""Measures pzg_unlzw_many and read_tiff_many(lzw=True) on one device: medians of five after a warm-up, one JSON line per figure.

    python tests/tools/tiff_lzw_bench.py [--tiles 16384] [--distinct 32] [--side 8192]

The launch alone on `tiles` tiles of 256 x 256 RGB8 pixels -- corpus-like (a smooth random walk per channel), all-zero and random --
compressed by libtiff through PIL, against the pzg_decompress_many launch on the same pixels as Deflate tiles and a device copy of
the decoded bytes.  `distinct` different tiles are compressed and their streams repeated (every stream has its own copy in the input
buffer and its own output): compressing 16,384 tiles on the host would take longer than everything measured.  Then read_tiff_many on
one tiled side x side RGB8 file of the corpus-like tiles against PIL / libtiff reading the same file."""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 256
TILE_BYTES = T * T * 3


def libtiff_lzw(tile):
    from PIL import Image
    from pure_zlib_amd.tiff import parse_tiff
    buf = io.BytesIO()
    Image.fromarray(tile.reshape(T, T * 3)).save(buf, format="TIFF", compression="tiff_lzw", tiffinfo={278: T})
    blob = buf.getvalue()
    pg = parse_tiff(blob)[0]
    assert len(pg.offsets) == 1 and pg.compression == 5
    return blob[pg.offsets[0]:pg.offsets[0] + pg.byte_counts[0]]


def tiles_of(kind, distinct, rng):
    if kind == "zero":
        return [np.zeros((T, T, 3), np.uint8)]
    if kind == "random":
        return [rng.integers(0, 256, size=(T, T, 3), dtype=np.uint8) for _ in range(distinct)]
    return [(np.cumsum(rng.integers(-2, 3, size=(T, T, 3)), axis=1) + rng.integers(0, 256, size=(T, 1, 3))).astype(np.uint8) for _ in range(distinct)]


def median_ms(fn, reps=5):
    fn()
    return statistics.median(fn() for _ in range(reps))


def launch_ms(ctx, streams, n, lzw):
    import torch
    from pure_zlib_amd._batch import pack
    lens = np.array([len(streams[i % len(streams)]) for i in range(n)], np.uint64)
    in_off, tot_in = pack(lens)
    h_in = np.zeros(tot_in, np.uint8)
    for i, o in enumerate(in_off.tolist()):
        s = streams[i % len(streams)]
        h_in[o:o + len(s)] = np.frombuffer(s, np.uint8)
    cap = np.full(n, TILE_BYTES, np.uint64)
    out_off, tot_out = pack(cap, slack=4)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
    t = [up(a) for a in (h_in, in_off, lens, out_off, cap)]
    out = torch.empty(tot_out, dtype=torch.uint8, device=dev)
    res = torch.zeros(20 * n, dtype=torch.uint8, device=dev)
    p = [x.data_ptr() for x in t]
    torch.cuda.synchronize()

    def once():
        if lzw:
            ctx.unlzw_many_device(p[0], p[1], p[2], out.data_ptr(), p[3], p[4], res.data_ptr(), res.data_ptr() + 8 * n, res.data_ptr() + 12 * n, n)
        else:
            ctx.decompress_many_device(p[0], p[1], p[2], out.data_ptr(), p[3], p[4], res.data_ptr(), res.data_ptr() + 8 * n, res.data_ptr() + 12 * n, 0, 0, n)
        return ctx.last_kernel_ms()
    ms = median_ms(once)
    host = res.cpu().numpy()
    assert (host[8 * n:12 * n].view(np.int32) == 0).all() and (host[:8 * n].view(np.uint64) == TILE_BYTES).all()
    return ms, int(lens.sum()), out, out_off


def copy_ms(nbytes):
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    return median_ms(once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16384)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--side", type=int, default=8192)
    a = ap.parse_args()
    import torch
    torch.cuda.init()  # (before the library's context: both then share the device's primary context)
    import pure_zlib_amd as P
    from pure_zlib_amd import tiff
    import tiffcases as TC
    ctx = P.Context(0)
    rng = np.random.default_rng(7)
    n = a.tiles
    decoded = n * TILE_BYTES
    print(json.dumps({"figure": "device copy", "tiles": n, "ms": round(copy_ms(decoded), 3), "decoded_GB": round(decoded / 1e9, 3)}), flush=True)
    corpus = None
    for kind in ("corpus", "zero", "random"):
        tiles = tiles_of(kind, a.distinct, rng)
        lz = [libtiff_lzw(t) for t in tiles]
        ms, nin, out, out_off = launch_ms(ctx, lz, n, True)
        got = out[int(out_off[n - 1]):int(out_off[n - 1]) + TILE_BYTES].cpu().numpy()
        assert got.tobytes() == tiles[(n - 1) % len(tiles)].tobytes()
        print(json.dumps({"figure": "pzg_unlzw_many launch", "pixels": kind, "tiles": n, "ms": round(ms, 3), "decoded_GB_s": round(decoded / ms / 1e6, 1),
                          "compressed_MB": round(nin / 1e6, 1)}), flush=True)
        del out
        if kind == "corpus":
            corpus = (tiles, lz)
            zs = [zlib.compress(t.tobytes(), 6) for t in tiles]
            ms, nin, out, _ = launch_ms(ctx, zs, n, False)
            print(json.dumps({"figure": "pzg_decompress_many launch", "pixels": kind, "tiles": n, "ms": round(ms, 3), "decoded_GB_s": round(decoded / ms / 1e6, 1),
                              "compressed_MB": round(nin / 1e6, 1)}), flush=True)
            del out
    # one tiled file
    tiles, lz = corpus
    across = a.side // T
    image = np.zeros((a.side, a.side, 3), np.uint8)
    for k in range(across * across):
        y, x = divmod(k, across)
        image[y * T:(y + 1) * T, x * T:(x + 1) * T] = tiles[k % len(tiles)]
    blob = TC.write_tiff([TC.Page(image, tile=(T, T), compression=5, level=0, edit=lambda k, z: lz[k % len(lz)])])

    def ours():
        t0 = time.perf_counter()
        img = tiff.read_tiff(blob, ctx=ctx, lzw=True)
        dt = (time.perf_counter() - t0) * 1e3
        assert img.data.shape == image.shape
        return dt

    def pil():
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
        t0 = time.perf_counter()
        got = np.asarray(Image.open(io.BytesIO(blob)))
        dt = (time.perf_counter() - t0) * 1e3
        assert got.shape == image.shape
        return dt
    assert tiff.read_tiff(blob, ctx=ctx, lzw=True).data.tobytes() == image.tobytes()
    print(json.dumps({"figure": "read_tiff(lzw=True), one tiled file", "side": a.side, "ms": round(median_ms(ours), 1), "file_MB": round(len(blob) / 1e6, 1)}), flush=True)
    print(json.dumps({"figure": "PIL / libtiff, the same file", "side": a.side, "ms": round(median_ms(pil), 1)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
