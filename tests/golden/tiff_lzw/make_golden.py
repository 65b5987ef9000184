"""Writes the golden LZW files of this directory with PIL's libtiff (Compression 5), each with the pixels it was written from beside
it (.npy).  Run once, by hand, where PIL has libtiff; the files are committed.  PIL does not write tiles: the tiled file is put together
by the test suite's writer (tests/tiffcases.py) from streams that libtiff compressed, one strip of a tile's differenced rows each."""
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(2026)


def smooth(shape, top):
    return (np.cumsum(rng.integers(-3, 4, size=shape), axis=1) % top)


def save(name, a, tiffinfo=None):
    Image.fromarray(a).save(os.path.join(HERE, name + ".tif"), format="TIFF", compression="tiff_lzw", tiffinfo=tiffinfo or {})
    np.save(os.path.join(HERE, name + ".npy"), a)


save("rgb8_strips", smooth((60, 50, 3), 256).astype(np.uint8), {278: 16})
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
import tiffcases as T  # noqa: E402
from pure_zlib_amd.tiff import parse_tiff  # noqa: E402


def libtiff_lzw(k, z):
    rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(32, 96)
    buf = io.BytesIO()
    Image.fromarray(rows).save(buf, format="TIFF", compression="tiff_lzw", tiffinfo={278: 32})
    blob = buf.getvalue()
    pg = parse_tiff(blob)[0]
    assert len(pg.offsets) == 1 and pg.compression == 5 and pg.predictor == 1
    return blob[pg.offsets[0]:pg.offsets[0] + pg.byte_counts[0]]


tiled = smooth((70, 90, 3), 256).astype(np.uint8)
with open(os.path.join(HERE, "rgb8_pred2_tiles.tif"), "wb") as f:
    f.write(T.write_tiff([T.Page(tiled, tile=(32, 32), predictor=2, compression=5, edit=libtiff_lzw)]))
np.save(os.path.join(HERE, "rgb8_pred2_tiles.npy"), tiled)
save("gray16_pred2", smooth((50, 70), 65536).astype(np.uint16), {317: 2, 278: 8})
save("gray8_random", rng.integers(0, 256, size=(200, 201), dtype=np.uint8))
save("gray8_zero", np.zeros((120, 130), np.uint8))
