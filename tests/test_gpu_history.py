"""GPU: the streams of tests/history_cases.py -- the history in front of the output at its edges -- through the C ABI, every case
of a form in ONE batch per launch: pzg_decompress_many_dict with host and with device pointers, the context at ring 11 (every
stream with a history then answers through the 32 KiB-ring retry) and at ring 15 (strips and groups with a history), as zlib
streams with FDICT, as raw streams (PZG_RAW) and with PZG_RAW | PZG_CRC32; pzg_decompress_many_segments with host and device
pointers, all eight start bits and windows of 1 to 32768 bytes in one call.  The dictionaries lie back to back at every address
modulo 16, the outputs back to back between 0xCD guards.  Expected: the case list's own bytes, status and detail words (the
writer's, not a decoder's); the failing zlib streams are held against the oracle as well."""
import zlib

import numpy as np
import pytest

import history_cases as H
from test_gpu_indexed import SegBatch
from test_gpu_raw import Dev

pytestmark = pytest.mark.gpu

E_TRUNCATED, E_BAD_DISTANCE, E_OUT_TOO_SMALL, E_DICT = 1, 11, 14, 20
DEVICE_PTRS, RAW, CRC32 = 1, 32, 64
ROOM = 300


def _planned(c, crc=False):
    d = c["data"]
    if c["expect"] == ("ok",):
        return (0, 0, 0, len(d), zlib.crc32(d) if crc else zlib.adler32(d)), d
    _kind, dist, op = c["expect"]
    return (E_BAD_DISTANCE, dist, op, op, zlib.crc32(d) if crc else zlib.adler32(d)), d


def _items(form, oracle=None):
    """[(name, stream, dictionary, capacity, (status, d0, d1, out_len, checksum), bytes, in_used or None)] of one launch"""
    raw, crc = form != "zlib", form == "raw_crc"
    items = []
    for c in H.cases():
        if crc and c["expect"] != ("ok",):
            continue
        want, d = _planned(c, crc)
        z = c["raw"] if raw else H.zlib_wrap(c)
        items.append((c["name"], z, c["zdict"], len(d) + ROOM, want, d, len(z) if want[0] == 0 else None))
        if not raw and want[0] != 0:  # the oracle with the dictionary installed: status, detail, length, bytes
            ro, oo = oracle.decompress_dict(z, c["zdict"], len(d) + ROOM)
            assert (ro.status, ro.detail0, ro.detail1, ro.out_len, ro.adler) == want and oo == d, c["name"]
    ck = zlib.crc32 if crc else zlib.adler32
    for name in H.CONTRACT:  # capacities and a cut, with a history
        c = H.by_name(name)
        d, zd = c["data"], c["zdict"]
        z = c["raw"] if raw else H.zlib_wrap(c)
        items.append((name + "/half", z, zd, len(d) // 2, (E_OUT_TOO_SMALL, 0, 0, len(d), 0), b"", None))
        items.append((name + "/exact", z, zd, len(d), (0, 0, 0, len(d), ck(d)), d, len(z)))
        cut, prefix = H.truncated(c)
        zc = cut if raw else H.FDICT_HDR + zlib.adler32(zd).to_bytes(4, "big") + cut
        items.append((name + "/cut", zc, zd, len(d), (E_TRUNCATED, 0, 0, len(prefix), ck(prefix)), prefix, None))
    if raw:
        return items
    seen = set()
    for c in H.cases():  # a DICTID one bit off, for every history length
        zd = c["zdict"]
        if (len(zd), zd[:1]) not in seen:
            seen.add((len(zd), zd[:1]))
            ours = zlib.adler32(zd)
            items.append((c["name"] + "/dictid", H.zlib_wrap(c, dictid=ours ^ 0x10000), zd, len(c["data"]) + ROOM, (E_DICT, ours ^ 0x10000, ours, 0, 1), b"", None))
    for c in H.cases():  # neighbours without a dictionary: FDICT with dict_len = 0, and no FDICT beside a dictionary
        nd = c["nodict"]
        d = nd[-1]
        want = (0, 0, 0, len(d), zlib.adler32(d)) if nd[0] == "ok" else (E_BAD_DISTANCE, nd[1], nd[2], len(d), zlib.adler32(d))
        zf = H.FDICT_HDR + zlib.adler32(c["zdict"]).to_bytes(4, "big") + c["raw"] + zlib.adler32(d).to_bytes(4, "big")
        for tag, z, zd in (("/fdict_nodict", zf, b""), ("/plain_dict", H.plain_wrap(c), c["zdict"])):
            items.append((c["name"] + tag, z, zd, len(d) + ROOM, want, d, len(z) if want[0] == 0 else None))
            ro, oo = oracle.decompress_dict(z, zd, len(d) + ROOM) if zd else oracle.decompress(z, len(d) + ROOM)
            assert (ro.status, ro.detail0 if ro.status else 0, ro.detail1 if ro.status else 0, ro.out_len, ro.adler) == want and oo == d, c["name"] + tag
    return items


@pytest.fixture(scope="module")
def batches(oracle):
    return {form: _items(form, oracle) for form in ("zlib", "raw", "raw_crc")}


def _hold(items, res, tag):
    """res[k] = (status, d0, d1, checksum, out_len, in_used, bytes below min(out_len, cap)) against the plan"""
    for (name, _z, _zd, cap, want, d, used), got in zip(items, res):
        st, d0, d1, ck, out_len, in_used, out = got
        what = (tag, name, got[:6], want)
        assert (st, out_len) == (want[0], want[3]), what
        if st in (E_BAD_DISTANCE, E_DICT):
            assert (d0, d1) == want[1:3], what
        assert ck == want[4], what
        if st != E_OUT_TOO_SMALL:
            assert out == d, what
        if used is not None:
            assert in_used == used, what


@pytest.mark.parametrize("ring", [11, 15])
@pytest.mark.parametrize("form", ["zlib", "raw", "raw_crc"])
def test_dictionaries_device_pointers(gpu_ctx, batches, form, ring):
    items = batches[form]
    b = Dev([it[1] for it in items], [it[3] for it in items], align=1, gap=7, dicts=[it[2] for it in items])
    offs = {int(o) % 16 for o, it in zip(b.d_dict_off.cpu().numpy(), items) if len(it[2]) >= 64}
    assert offs >= {1, 7, 15}, "vacuous: the dictionaries do not start at odd addresses"
    try:
        gpu_ctx.set_ring_bits(ring)
        assert b.launch(gpu_ctx, DEVICE_PTRS | {"zlib": 0, "raw": RAW, "raw_crc": RAW | CRC32}[form]) == 0
        res, h = b.results()
        _hold(items, res, (form, ring, "device"))
        assert b.guards_intact(h, res), "written outside [0, min(out_len, cap)) of an extent"
    finally:
        gpu_ctx.set_ring_bits(11)


def _host_dict_call(ctx, items, flags):
    from pure_zlib_amd import _ffi
    n = len(items)
    u64 = lambda v: np.array(v, dtype=np.uint64)  # noqa: E731
    in_len, d_len, cap = u64([len(it[1]) for it in items]), u64([len(it[2]) for it in items]), u64([it[3] for it in items])
    off = lambda lens, gap: u64(np.concatenate(([0], np.cumsum(lens[:-1] + np.uint64(gap)))))  # noqa: E731
    in_off, d_off, out_off = off(in_len, 0), off(d_len, 0), off(cap, 7)
    ibuf = np.frombuffer(b"".join(it[1] for it in items) + bytes(16), dtype=np.uint8).copy()
    dbuf = np.frombuffer(b"".join(it[2] for it in items) + bytes(16), dtype=np.uint8).copy()
    obuf = np.full(int(out_off[-1] + cap[-1]) + 64, 0xCD, dtype=np.uint8)
    out_len, in_used = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    status, detail, adler = np.full(n, -1, np.int32), np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    rc = _ffi.lib().pzg_decompress_many_dict(ctx.handle, p(ibuf), p(in_off), p(in_len), p(dbuf), p(d_off), p(d_len), p(obuf), p(out_off), p(cap),
                                             p(out_len), p(status), p(detail), p(in_used), p(adler), n, flags)
    assert rc == 0
    res, mask = [], np.ones(len(obuf), dtype=bool)
    for k in range(n):
        o, m = int(out_off[k]), min(int(out_len[k]), int(cap[k]))
        mask[o:o + m] = False
        res.append((int(status[k]), int(detail[2 * k]), int(detail[2 * k + 1]), int(adler[k]), int(out_len[k]), int(in_used[k]), obuf[o:o + m].tobytes()))
    return res, bool((obuf[mask] == 0xCD).all())


@pytest.mark.parametrize("ring", [11, 15])
@pytest.mark.parametrize("form", ["zlib", "raw", "raw_crc"])
def test_dictionaries_host_pointers(gpu_ctx, batches, form, ring):
    items = batches[form]
    try:
        gpu_ctx.set_ring_bits(ring)
        res, clean = _host_dict_call(gpu_ctx, items, {"zlib": 0, "raw": RAW, "raw_crc": RAW | CRC32}[form])
        _hold(items, res, (form, ring, "host"))
        assert clean, "written outside [0, min(out_len, cap)) of an extent"
    finally:
        gpu_ctx.set_ring_bits(11)


@pytest.fixture(scope="module")
def segment_items():
    """every case as a segment, start bit k % 8; the contract cases once more with half the capacity, the exact one, and cut short"""
    items = []
    for k, c in enumerate(H.cases()):
        s = H.seg_wrap(c, k % 8)
        want, d = _planned(c)
        items.append((c["name"], s["inp"], s["start_bit"], s["end_bit"] if k % 3 else 0, s["window"], len(d) + ROOM, want, d, s["in_used"] if want[0] == 0 else None))
    for name in H.CONTRACT:
        c = H.by_name(name)
        s, d = H.seg_wrap(c, 3), c["data"]
        items.append((name + "/half", s["inp"], 3, s["end_bit"], s["window"], len(d) // 2, (E_OUT_TOO_SMALL, 0, 0, len(d), 0), b"", None))
        items.append((name + "/exact", s["inp"], 3, s["end_bit"], s["window"], len(d), (0, 0, 0, len(d), zlib.adler32(d)), d, s["in_used"]))
        scut, sprefix = H.truncated_segment(c, s)  # (end_bit 0: host pointers refuse an end_bit past the input)
        items.append((name + "/cut", scut, 3, 0, s["window"], len(d), (E_TRUNCATED, 0, 0, len(sprefix), zlib.adler32(sprefix)), sprefix, None))
    assert {it[2] for it in items} == set(range(8)) and {len(it[4]) for it in items} >= {1, 2, 64, 258, 32767, 32768}
    return items


def _hold_segments(items, out, st, out_len, in_used, sums, det, tag):
    at = 0
    for k, (name, _inp, _sb, _eb, _win, cap, want, d, used) in enumerate(items):
        mine = out[at:at + cap]
        at += cap
        got = (int(st[k]), int(det[k][0]) if st[k] else 0, int(det[k][1]) if st[k] else 0, int(out_len[k]), int(sums[k]))
        assert got == want, (tag, name, got, want)
        n = 0 if want[0] == E_OUT_TOO_SMALL else len(d)
        assert mine[:n].tobytes() == d[:n] and (mine[min(want[3], cap):] == 0xCD).all(), (tag, name, "bytes")
        if used is not None:
            assert int(in_used[k]) == used, (tag, name, int(in_used[k]), used)


def test_segments_device_pointers(gpu_ctx, segment_items):
    b = SegBatch([it[1:6] for it in segment_items])
    out, st, out_len, in_used, sums, det = b.run(gpu_ctx, 0)
    _hold_segments(segment_items, out, st, out_len, in_used, sums, det, "device")


def test_segments_host_pointers(gpu_ctx, segment_items):
    from pure_zlib_amd import _ffi
    items = segment_items
    n = len(items)
    i64 = lambda v: np.array(v, dtype=np.int64)  # noqa: E731
    off = lambda lens: np.concatenate(([0], np.cumsum(lens[:-1])))  # noqa: E731
    in_len, d_len, cap = i64([len(it[1]) for it in items]), i64([len(it[4]) for it in items]), i64([it[5] for it in items])
    in_off, d_off, out_off = off(in_len), off(d_len), 64 + off(cap)
    ibuf = np.frombuffer(b"".join(it[1] for it in items) + bytes(16), dtype=np.uint8).copy()
    dbuf = np.frombuffer(b"".join(it[4] for it in items) + bytes(16), dtype=np.uint8).copy()
    start, end = np.array([it[2] for it in items], dtype=np.uint8), i64([it[3] for it in items])
    total = int(cap.sum())
    obuf = np.full(total + 128, 0xCD, dtype=np.uint8)
    out_len, in_used = np.zeros(n, np.int64), np.zeros(n, np.int64)
    status, detail, sums = np.full(n, -1, np.int32), np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    _ffi.check(_ffi.lib().pzg_decompress_many_segments(gpu_ctx.handle, p(ibuf), p(in_off), p(in_len), p(start), p(end), p(dbuf), p(d_off), p(d_len), p(obuf),
                                                       p(out_off), p(cap), p(out_len), p(status), p(detail), p(in_used), p(sums), n, 0), gpu_ctx.handle)
    assert (obuf[:64] == 0xCD).all() and (obuf[64 + total:] == 0xCD).all(), "written outside the buffer"
    _hold_segments(items, obuf[64:64 + total], status, out_len, in_used, sums, detail.reshape(-1, 2), "host")
