"""CPU: what the kernel source (its host model) hands back for a stream that FAILED, against the oracle and against plain zlib
checksums -- include/pzg.h, adler[]: for a status other than PZG_OK and PZG_E_OUT_TOO_SMALL,
  out_len  the bytes the reference had emitted before the error (nothing of a stored block it could not read whole),
  bytes    [0, min(out_len, cap)) of the extent are those bytes, and nothing past the capacity is written,
  adler    the Adler-32 of those bytes (gzip: their CRC-32), or 0 when out_len > cap.
Rings 11-15, strips on and off, the build whose strips guess wrong; corrupted and truncated streams of every block type, capacities
below, at and above the failure point, gzip members, and the bundles' lanes that report a checksum mismatch."""
import ctypes as C
import os
import random
import zlib

import pytest

import corpus
import deflate_writer as W
from test_model_vs_oracle import GUARD, R, _build_model, model, model_bad_guesses  # noqa: F401  (fixtures)

RINGS = [11, 12, 13, 14, 15]


def check(oracle, run, z, cap, rb, gzip=False, what=None):
    """One stream through the oracle and the model (whose runner checks the GUARD bytes past `cap`).  Returns its status."""
    ro, oo = (oracle.gzip_decompress if gzip else oracle.decompress)(z, cap)
    rm, om = run(z, cap, rb, gzip=gzip)
    if gzip and ro.out_len > cap and ro.status in (10, 19):
        ro.status = 14  # the CRC-32 and ISIZE of a member are checked on the stored output: not past the capacity (include/pzg.h)
    assert rm.status == ro.status, (what, ro.status, rm.status, ro.message)
    if ro.status == 14:
        assert rm.out_len == ro.out_len, what
        return ro.status
    assert rm.out_len == ro.out_len, (what, ro.status, ro.out_len, rm.out_len)
    assert om == oo, (what, ro.status, ro.out_len, cap, next((i for i, (a, b) in enumerate(zip(om, oo)) if a != b), None))
    if ro.out_len > cap:
        want = 0
    else:
        want = zlib.crc32(oo) if gzip else zlib.adler32(oo)  # plain zlib over the delivered bytes ...
        assert ro.adler == want, (what, "oracle")          # ... which is the oracle's running checksum
    assert rm.adler == want, (what, ro.status, hex(rm.adler), hex(want))
    if ro.status == 0:
        assert rm.in_used == ro.in_used, what
    return ro.status


def cuts(n, k):
    """k cut points spread over [0, n), the last few bytes included."""
    pts = {max(0, n - j) for j in range(1, 6)} | {n * i // k for i in range(k)}
    return sorted(p for p in pts if p < n)


def stored_stream(d, seed):
    """Level 0 with seeded flush points: several stored blocks, some of them empty (sync flushes)."""
    rng = random.Random(seed)
    co = zlib.compressobj(0)
    z, pos = b"", 0
    while pos < len(d):
        step = rng.randint(1, 9000)
        z += co.compress(d[pos:pos + step]) + (co.flush(zlib.Z_SYNC_FLUSH) if rng.random() < 0.5 else b"")
        pos += step
    return z + co.flush()


def truncation_cases():
    """(name, data, stream): stored, fixed, dynamic and strip-sized streams, one block and several."""
    d1 = corpus.zipf_text(20000, 1)
    fx = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    yield "stored", d1, stored_stream(d1, 1)
    yield "fixed", d1, fx.compress(d1) + fx.flush()
    yield "dynamic", d1, zlib.compress(d1, 6)
    d2 = corpus.mixed_data(12000, 2)
    yield "multi", d2, corpus.compress_variant(d2, 2)
    d3, z3 = corpus.strip_case(0)
    yield "strips", d3, z3


@pytest.mark.parametrize("strips", [True, False])
@pytest.mark.parametrize("rb", RINGS)
def test_corrupt_corpus_failed_streams(model, oracle, rb, strips, monkeypatch):
    """corpus.corrupt() of seeded zlib streams (every level and strategy, flush points), three capacities."""
    if not strips:
        monkeypatch.setenv("PZM_NO_STRIPS", "1")
    failed = 0
    for seed in range(300):
        d = corpus.mixed_data((seed * 131) % 3000 + 1, seed)
        z = corpus.corrupt(corpus.compress_variant(d, seed), seed)
        cap = [len(d), len(d) + 100, 1 << 17][seed % 3]
        failed += check(oracle, model, z, cap, rb, what=seed) not in (0, 14)
    assert failed > 200, failed


@pytest.mark.parametrize("rb", [11, 15])
def test_corrupted_exotic_streams(model, oracle, rb):
    """deflate_writer.exotic_stream (long codes, incomplete codes, tiny blocks at odd offsets, 258 / 32768 matches) corrupted."""
    failed = 0
    for seed in range(24):
        d, z, _ = W.exotic_stream(seed)
        for k in range(5):
            zc = corpus.corrupt(z, 31 * seed + k)
            cap = [len(d), len(d) + 64, len(d) // 3][k % 3]
            failed += check(oracle, model, zc, cap, rb, what=(seed, k)) not in (0, 14)
    assert failed > 60, failed


@pytest.mark.parametrize("rb", RINGS)
def test_truncated_streams(model, oracle, rb):
    """Every block type cut at many points: what was decoded before the input ran out, nothing of a stored block cut short."""
    for name, d, z in truncation_cases():
        for cut in cuts(len(z), 48):
            assert check(oracle, model, z[:cut], len(d) + 64, rb, what=(name, cut)) == 1


@pytest.mark.parametrize("rb", [11, 15])
def test_truncated_streams_without_strips_and_with_bad_guesses(model, model_bad_guesses, oracle, rb, monkeypatch):
    """The same cuts decoded by the windows alone (no scratch) and by strips whose speculative starts nearly all fail."""
    for name, d, z in truncation_cases():
        for cut in cuts(len(z), 24):
            assert check(oracle, model_bad_guesses, z[:cut], len(d), rb, what=("bad guesses", name, cut)) == 1
    monkeypatch.setenv("PZM_NO_STRIPS", "1")
    for name, d, z in truncation_cases():
        for cut in cuts(len(z), 24):
            assert check(oracle, model, z[:cut], len(d), rb, what=("no strips", name, cut)) == 1


@pytest.mark.parametrize("rb", RINGS)
def test_capacity_around_the_failure_point(model, oracle, rb):
    """A failed stream's capacity below, at and above what it had decoded: the bytes that fit, the Adler-32 or 0."""
    for name, d, z in truncation_cases():
        for cut in cuts(len(z), 6)[1:]:
            zc = z[:cut]
            r, _ = oracle.decompress(zc, len(d))
            assert r.status == 1
            got = r.out_len
            for cap in sorted({0, 1, got // 2, max(0, got - 17), max(0, got - 1), got, got + 1, got + 4096}):
                check(oracle, model, zc, cap, rb, what=(name, cut, got, cap))
    for seed in range(40):  # corrupted ones that fail in the middle: a bad distance, a bad code, a checksum
        d, z = corpus.strip_case(seed % 12) if seed % 4 == 0 else (lambda x: (x, zlib.compress(x, 1 + seed % 9)))(corpus.zipf_text(9000, seed))
        zc = corpus.corrupt(z, 7000 + seed)
        r, _ = oracle.decompress(zc, len(d) + 64)
        if r.status in (0, 14):
            continue
        for cap in sorted({0, r.out_len // 3, max(0, r.out_len - 1), r.out_len, r.out_len + 100}):
            check(oracle, model, zc, cap, rb, what=(seed, r.status, r.out_len, cap))


@pytest.mark.parametrize("rb", [11, 13, 15])
def test_gzip_members_that_fail(model, oracle, rb):
    """PZG_GZIP: adler[] of a failed member is the CRC-32 of the bytes it delivered (0 past the capacity)."""
    failed = 0
    for seed in range(60):
        d = corpus.mixed_data((seed * 97) % 5000 + 1, seed)
        g = corpus.gzip_member(d, seed)
        for k in range(3):
            zc = corpus.corrupt(g, 40 * seed + k)
            cap = [len(d), len(d) + 8, len(d) // 2][k]
            failed += check(oracle, model, zc, cap, rb, gzip=True, what=(seed, k)) not in (0, 14)
        for cut in cuts(len(g), 4):
            failed += check(oracle, model, g[:cut], len(d), rb, gzip=True, what=(seed, "cut", cut)) not in (0, 14)
    assert failed > 250, failed


def test_bundle_lanes_that_fail_the_checksum(oracle):
    """The bundles (one lane per stream of the fixed code): a lane that reports a checksum mismatch (status 10) has decoded the
    whole stream -- out_len, every byte and the Adler-32 of them are the oracle's, and nothing past the capacity is written."""
    from conftest import ROOT
    _build_model([])
    M = C.CDLL(os.path.join(ROOT, "tests", "model", "libpzgmodel.so"))
    M.pzm_bundle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    rng = random.Random(11)
    tens = 0
    for batch in range(4):
        streams, caps = [], []
        for k in range(64):
            d = corpus.zipf_text(rng.randrange(1, 4096), 64 * batch + k)
            co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
            z = bytearray(co.compress(d) + co.flush())
            if k % 4 != 3:
                z[-1 - rng.randrange(4)] ^= 1 << rng.randrange(8)  # the Adler-32 trailer: status 10
            else:
                z = corpus.corrupt(bytes(z), 500 * batch + k)     # anything else
            streams.append(bytes(z))
            caps.append([len(d), len(d) + 64, max(0, len(d) - 100)][k % 3])
        n = len(streams)
        bufs = [C.create_string_buffer(b"\x5a" * c + GUARD, c + len(GUARD)) for c in caps]
        res = (R * n)()
        assert M.pzm_bundle((C.c_char_p * n)(*streams), (C.c_uint64 * n)(*[len(z) for z in streams]),
                            (C.c_void_p * n)(*[C.addressof(b) for b in bufs]), (C.c_uint64 * n)(*caps), n, res) == 0
        for k in range(n):
            assert bufs[k].raw[caps[k]:] == GUARD, (batch, k)
            r = res[k]
            if r.status == 103:  # handed back to the ordinary kernel
                continue
            ro, oo = oracle.decompress(streams[k], caps[k])
            assert r.status == ro.status, (batch, k, ro.status, r.status)
            if r.status in (0, 14):
                continue
            om = bufs[k].raw[: min(r.out_len, caps[k])]
            assert (r.out_len, om) == (ro.out_len, oo), (batch, k, ro.status)
            assert r.adler == (0 if ro.out_len > caps[k] else zlib.adler32(oo)), (batch, k, ro.status, hex(r.adler))
            tens += r.status == 10
    assert tens > 60, tens
