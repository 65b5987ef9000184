"""Shared by tests/test_model_raw.py (CPU) and tests/test_gpu_raw.py (GPU): what a bare RFC 1951 stream `d` must decode to.

The oracle has no raw mode, so the expectation has two sources:

(a) system zlib -- zlib.decompressobj(-15[, zdict]) -- for every stream it accepts: the bytes, in_used = len(d) - len(unused_data),
    zlib.adler32 and zlib.crc32 of them.
(b) the oracle on the WRAPPED stream, for status, errors and what a failed stream delivers.  A first oracle call on
    78 9c + d + 00 00 00 00 tells whether the blocks end inside d: it then gets as far as the trailer (a checksum mismatch, as a rule) having
    consumed e + 6 bytes, and reports the Adler-32 `a` of what the oracle itself delivered.  The wrapped stream is 78 9c + d[:e] + a + d[e:]
    (the trailer where a zlib stream has it, trailing bytes behind it): raw status = wrapped status, in_used_raw = in_used_wrapped - 6.
    When the blocks do not end inside d (an error in them, or d runs out -- in the first call the final block then ends in the zero
    bytes, or reads them as tokens) nothing is appended: the wrapped stream is 78 9c + d, which fails where and as d fails, never for
    want of a trailer only.
"""
import zlib

HDR = b"\x78\x9c"
BIG = 1 << 22


def zlib_raw(d, zdict=None):
    """(data, in_used) if system zlib accepts d as a complete raw stream, else None."""
    o = zlib.decompressobj(-15, zdict) if zdict else zlib.decompressobj(-15)
    try:
        data = o.decompress(d)
    except zlib.error:
        return None
    if not o.eof:
        return None
    return data, len(d) - len(o.unused_data)


def wrap(O, d):
    """(wrapped stream, e): e is the byte at which the blocks end inside d, or None (see the module text)."""
    r0, _ = O.decompress(HDR + d + b"\0\0\0\0", BIG)
    # (status 0: the bytes behind the final block happen to be the right trailer -- a zlib stream stripped of less than its own)
    if r0.status in (O.OK, O.E_CHECKSUM) and r0.in_used - 6 <= len(d):
        e = r0.in_used - 6
        return HDR + d[:e] + r0.adler.to_bytes(4, "big") + d[e:], e
    return HDR + d, None


def message(d, status, detail):
    """pzg_error_message over the RAW bytes (host code of libpzg.so: no device needed)."""
    import pure_zlib_amd.zlib as Z
    return Z.error_from_status(d, status, detail).show()


def check(O, d, cap, got, zlib_detail1=None, what=None):
    """got = (status, detail0, detail1, adler, out_len, in_used, bytes below the capacity) of the raw decode of d into `cap` bytes.
    zlib_detail1(wrapped): detail[1] a zlib decode of the wrapped stream reports (PZG_E_HUFF_BUILD only), or None to skip that."""
    st, d0, d1, adler, out_len, in_used, out = got
    out = bytes(out[: min(out_len, cap)])
    z = zlib_raw(d)
    if z is not None:  # (a)
        data, used = z
        if cap >= len(data):
            assert (st, out_len, in_used, adler) == (0, len(data), used, zlib.adler32(data)) and out == data, (what, "zlib", st, out_len, in_used)
        else:
            assert (st, out_len) == (14, len(data)), (what, "zlib", st, out_len)
    wrapped, e = wrap(O, d)  # (b)
    ro, oo = O.decompress(wrapped, cap)
    assert st == ro.status, (what, "status", st, ro.status, ro.message)
    assert st not in (2, 3, 4, 10, 20), (what, st)  # no header, no checksum, no DICTID
    assert out_len == ro.out_len, (what, "out_len", out_len, ro.out_len)
    if st == 14:
        return
    assert out == oo, (what, "bytes")
    if st == 0:
        # (z may be None: the reference accepts codes system zlib refuses -- incomplete ones, runs past HLIT + HDIST)
        assert e is not None and in_used == ro.in_used - 6 == e and adler == ro.adler, (what, in_used, ro.in_used, e, adler, ro.adler)
        return
    assert adler == (0 if ro.out_len > cap else ro.adler), (what, "failed adler", adler, ro.adler)
    if st in (6, 11, 12, 13):
        assert (d0, d1) == (ro.detail0, ro.detail1), (what, "detail")
    if st == 7:
        assert d0 == ro.detail0 & 0xff, (what, "tree id")
        if zlib_detail1 is not None:
            assert d1 == zlib_detail1(wrapped) - 16, (what, "bit offset")
    assert message(d, st, (d0, d1)) == ro.message.decode(), (what, "message", message(d, st, (d0, d1)), ro.message)


def stream_pool():
    """[(name, raw stream)]: the reference fixtures and the pinned vectors with their wrapper stripped, writer-made streams (stored /
    fixed / dynamic mixes, hundreds of tiny blocks, 13-15-bit codes), zlib-made ones of every strategy, and corrupted ones."""
    import corpus
    import deflate_writer as W
    from conftest import REF_CASES, read_case
    from test_oracle_golden import load_vectors
    pool = []
    for name in REF_CASES:
        pool.append((name, read_case(name)[0][2:-4]))
    for v in load_vectors():
        z = bytes.fromhex(v["z"])
        if len(z) < 2 or v["status"] in (2, 3, 4):  # (no stream behind the header, or none the header admits)
            continue
        pool.append((v["name"] + "/strip", z[2:-4]))
        if v["status"] != 0:
            pool.append((v["name"] + "/body", z[2:]))  # (an error vector has no trailer to strip)
    for seed in range(16):
        pool.append(("exotic%d" % seed, W.exotic_stream(seed)[1][2:-4]))
    for seed in range(3):
        pool.append(("pool%d" % seed, W.pool_stream(seed)[1][2:-4]))
    for seed in range(40):
        d = corpus.mixed_data([0, 1, 2, 5, 100, 1000, 5000, 40000, 70000][seed % 9] if seed % 4 == 0 else (seed * 337) % 12000, seed)
        z = corpus.compress_variant(d, seed)
        pool.append(("variant%d" % seed, z[2:-4]))
        pool.append(("corrupt%d" % seed, corpus.corrupt(z, seed)[2:-4]))
    return pool
