"""CPU: the host model of inflate_core.h on streams that sit on the edges the VALU pass touches in strip_step_b and seq_group
(tests/valu_pass_cases.py says how each is met): literal runs of 3 .. 17 bytes across the ring's end, far matches of 3 .. 33 bytes
at every distance around the near / far boundary and below the flushed part's end, lanes whose strips end on their 4th, 8th, 9th
record, two literals at a 16-byte literal group's end and at a strip's end, a span that a lane out of steps ends.  Rings 11 and
15, zlib and gzip, and the resumable instance with small output rooms: status, out_len, in_used, checksum and every byte
against the oracle."""
import zlib

import pytest

import valu_pass_cases as V
from test_model_vs_oracle import ModelDecoder, model, model_lib  # noqa: F401  (fixtures)

RINGS = [11, 15]


@pytest.fixture(scope="module")
def streams():
    return {rb: V.cases(rb) for rb in RINGS}


@pytest.mark.parametrize("rb", RINGS)
def test_the_cases_are_what_they_claim(streams, rb):
    """the writer's streams are valid and hold what the docstrings say (zlib itself decodes them to the writer's bytes)"""
    ring = 1 << rb
    for name, d, raw in streams[rb]:
        assert zlib.decompress(raw, -15) == d, name
    name, d, raw = streams[rb][0]
    assert name == "lit_runs_wrap" and len(d) > ring * len(V.RUNS)
    if rb == 11:
        assert sum(len(d) for _, d, _ in streams[rb]) < 1 << 20


@pytest.fixture(scope="module")
def stats_model():
    """the host model built with -DPZG_STATS (tests/tools/model_stats.py): its event counters say which paths a stream took"""
    import ctypes as C
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import model_stats as MS
    M = MS.build()
    M.pzm_stats.restype = C.POINTER(C.c_ulonglong)
    M.pzm_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(MS.R)]

    def run(z, cap, rb):
        v = M.pzm_stats()
        before = [v[i] for i in range(32)]
        out, r = C.create_string_buffer(cap), MS.R()
        assert M.pzm_decompress(z, len(z), out, cap, rb, C.byref(r)) == 0 and r.status == 0
        return [v[i] - before[i] for i in range(32)]
    return run


@pytest.mark.parametrize("rb", RINGS)
def test_the_cases_reach_the_paths_they_name(stats_model, streams, rb):
    """Not vacuous: by the model's counters (PZG_STAT in inflate_core.h) every stream is decoded by spans and groups (13, 20);
    the run that wraps the ring's end and the short-distance matches take byte steps (27); the far sweeps have groups with far
    matches (25) on the hybrid rings; the out-of-steps stream ends a span with a lane out of steps (29); matches past SEQ_CAP go
    the long way (24)."""
    for name, d, raw in streams[rb]:
        st = stats_model(V.zlib_wrap(d, raw), len(d), rb)
        assert st[13] > 0 and st[20] > 0 and st[17] > 0, (name, st)
        if name == "lit_runs_wrap":
            assert st[27] > 0, (name, st)
        if name.startswith("far_") and rb < 15:
            assert st[25] > 0, (name, st)
        if name in ("far_sweep_2", "far_deep") or (name == "far_sweep_0" and rb == 15):
            assert st[24] > 0, (name, st)  # (length 33 is in these)
        if name == "out_of_steps":
            assert st[29] > 0, (name, st)


@pytest.mark.parametrize("rb", RINGS)
def test_model_zlib(model, oracle, streams, rb):  # noqa: F811
    for name, d, raw in streams[rb]:
        z = V.zlib_wrap(d, raw)
        ro, oo = oracle.decompress(z, len(d))
        assert ro.status == 0 and oo == d, name
        rm, om = model(z, len(d), rb)
        assert (rm.status, rm.out_len, rm.in_used, rm.adler) == (0, len(d), len(z), zlib.adler32(d)), (name, rm.status, rm.out_len)
        assert om == d, name
        # ... and a capacity that the stream outgrows: what was decoded by then, as the oracle has it
        cap = len(d) - 700
        ro, oo = oracle.decompress(z, cap)
        rm, om = model(z, cap, rb)
        assert (rm.status, rm.out_len) == (ro.status, ro.out_len) and om == oo, (name, "cap")


@pytest.mark.parametrize("rb", RINGS)
def test_model_gzip(model, oracle, streams, rb):  # noqa: F811
    for name, d, raw in streams[rb]:
        z = V.gzip_wrap(d, raw)
        ro, oo = oracle.gzip_decompress(z, len(d))
        assert ro.status == 0 and oo == d, name
        rm, om = model(z, len(d), rb, gzip=True)
        assert (rm.status, rm.out_len, rm.in_used) == (0, len(d), len(z)) and om == d, (name, rm.status, rm.out_len)
        assert rm.adler == ro.adler == zlib.crc32(d), name  # (gzip: the CRC-32 rides in the checksum field)


@pytest.mark.parametrize("rb", RINGS)
@pytest.mark.parametrize("room", [1024, 4096, 1024 + 4096 + 1])
def test_model_resumable_small_rooms(model_lib, oracle, streams, rb, room):  # noqa: F811
    """decompressIncremental on the model: rooms of 1 KiB, 4 KiB and 1 KiB + 4 KiB + 1 byte cut every span short (a span is
    cut behind the last lane whose output still fits); the whole event trace and every byte."""
    for name, d, raw in streams[rb]:
        step = 20000
        z = V.zlib_wrap(d, raw)
        pieces = [z[i:i + step] for i in range(0, len(z), step)]
        eo, ro, oo = oracle.trace(pieces)
        assert ro.status == 0 and oo == d, name
        dec = ModelDecoder(model_lib, room, rb)
        for p in pieces:
            if not dec.feed(p):
                break
        assert dec.events == eo, (name, room)
        assert bytes(dec.total) == d, (name, room)
