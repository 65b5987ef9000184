"""CPU: the bundles (inflate_core.h bundle_decode / bundle_emit -- small streams of the fixed code, 64 to a wave, one lane per
stream) compiled as a host program and checked against the oracle: what a bundle calls clean must be the oracle's result bit for
bit, everything else must come back as "the ordinary kernel's" (status 103) -- and plain streams of the fixed code must be clean.
The model is test infrastructure; libpzg.so never contains it.  Reference semantics: Deflate.hs:79-82, 106-120, 241-251."""
import ctypes as C
import random
import zlib

import pytest

import corpus
from oracle import oracle as O
from test_model_vs_oracle import R, _build_model, same  # noqa: F401  (builds tests/model/libpzgmodel.so)

TODO = 103


@pytest.fixture(scope="session")
def bundle():
    import os
    from conftest import ROOT
    _build_model([])
    M = C.CDLL(os.path.join(ROOT, "tests", "model", "libpzgmodel.so"))

    def run(streams, caps):
        n = len(streams)
        assert n <= 64
        ins = (C.c_char_p * n)(*streams)
        lens = (C.c_uint64 * n)(*[len(z) for z in streams])
        bufs = [C.create_string_buffer(max(c, 1) + 64) for c in caps]
        outs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        capa = (C.c_uint64 * n)(*caps)
        res = (R * n)()
        M.pzm_bundle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        assert M.pzm_bundle(ins, lens, outs, capa, n, res) == 0
        return [(res[k], bufs[k].raw[: min(res[k].out_len, caps[k])]) for k in range(n)]
    return run


def fixed(data, level=1, blocks=1):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    if blocks == 1:
        return co.compress(data) + co.flush()
    step = max(1, len(data) // blocks)
    z = b""
    for i in range(0, len(data), step):
        z += co.compress(data[i:i + step]) + co.flush(zlib.Z_BLOCK)  # ends the block; the next one is of the fixed code again
    return z + co.flush()


def check(bundle, streams, caps, expect_clean=None):
    got = bundle(streams, caps)
    nclean = 0
    for k, (z, cap, (r, out)) in enumerate(zip(streams, caps, got)):
        if r.status == TODO:
            assert expect_clean is None or not expect_clean[k], (k, len(z), cap)
            continue
        nclean += 1
        ro, oo = O.decompress(z, cap)
        assert same(ro, oo, r, out), (k, ro.status, r.status, ro.out_len, r.out_len, ro.in_used, r.in_used, hex(ro.adler), hex(r.adler))
        assert expect_clean is None or expect_clean[k], (k, "a stream that is not a bundle's came back clean", r.status)
    return nclean


def test_bundle_of_text_streams_of_every_size(bundle):
    datas = [corpus.zipf_text(n, 100 + n) for n in [0, 1, 2, 3, 7, 64, 255, 256, 257, 1000, 2048, 3000, 4095, 4096] + [random.Random(5).randrange(1, 4097) for _ in range(50)]]
    streams = [fixed(d) for d in datas]
    n = check(bundle, streams, [len(d) for d in datas], [True] * len(datas))
    assert n == len(datas)


def test_literal_heavy_runs_and_many_blocks(bundle):
    rng = random.Random(7)
    datas, streams = [], []
    for k in range(64):
        kind = k % 4
        if kind == 0:
            d = bytes(b % 144 for b in corpus.random_bytes(rng.randrange(1, 4096), k))  # nothing but (8-bit) literals: runs of more than 255 of them
        elif kind == 1:
            d = bytes([65 + k % 7]) * rng.randrange(1, 4096)            # distance 1, length 258
        elif kind == 2:
            d = (corpus.zipf_text(300, k) * 20)[: rng.randrange(1, 4096)]  # long matches at a distance of 300
        else:
            d = corpus.zipf_text(rng.randrange(100, 4096), k)
        datas.append(d)
        streams.append(fixed(d, level=rng.choice([1, 6, 9]), blocks=rng.choice([1, 1, 2, 5, 17])))
    assert check(bundle, streams, [len(d) for d in datas], [True] * 64) == 64


def test_what_is_not_a_bundles_business_is_left_alone(bundle):
    """Dynamic and stored blocks, every kind of damage, capacities too small: the bundle must not call them clean -- except a wrong
    checksum, which it reports as the ordinary path does (detail words and all)."""
    rng = random.Random(11)
    streams, caps, exp = [], [], []

    def add(z, cap, clean):
        streams.append(z)
        caps.append(cap)
        exp.append(clean)
    d = corpus.zipf_text(3000, 1)
    good = fixed(d)
    add(good, len(d), True)
    add(zlib.compress(d, 6), len(d), False)                        # a dynamic block
    add(zlib.compress(corpus.random_bytes(500, 1), 0), 500, False)  # a stored block
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    add(co.compress(d[:1000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(d[1000:]) + co.flush(), len(d), False)  # fixed, stored (empty), fixed
    add(good[:-1], len(d), False)                                  # the trailer is short
    add(good[:-5], len(d), False)
    add(good[: len(good) // 2], len(d), False)                     # truncated inside the tokens
    add(good, len(d) - 1, False)                                   # capacity too small
    add(good, 0, False)
    add(good[:-4] + bytes([good[-4] ^ 1]) + good[-3:], len(d), True)  # a wrong checksum: reported with both words
    add(bytes([0x78, 0x9d]) + good[2:], len(d), False)             # FCHECK
    add(bytes([0x79, 0x9c - 0x1f + 0x1f]) + good[2:], len(d), False)
    z = bytearray(good)
    z[1] |= 0x20                                                   # FDICT (and FCHECK now wrong)
    add(bytes(z), len(d), False)
    add(good + b"trailing", len(d), True)                          # bytes behind the trailer are not the stream's (Zlib.hs:46-49 is the mirror's business)
    add(b"", 10, False)
    add(good[:2], 10, False)
    add(good[:7], 10, False)
    big = fixed(corpus.zipf_text(20000, 3))
    add(big, 20000, True)                                          # distances of up to 20,000: far matches all the way
    for k in range(40):                                            # flipped bits anywhere: bad distances, bad symbols, wrong lengths ...
        z = bytearray(good)
        p = rng.randrange(2, len(z) - 4)
        z[p] ^= 1 << rng.randrange(8)
        add(bytes(z), len(d), None)
    got = bundle(streams, caps)
    for k, (z, cap, e, (r, out)) in enumerate(zip(streams, caps, exp, got)):
        if r.status == TODO:
            assert e is not True, k
            continue
        assert e is not False, (k, r.status)
        ro, oo = O.decompress(z, cap)
        assert same(ro, oo, r, out), (k, ro.status, r.status)
        if e is None:
            assert ro.status in (0, 10), (k, ro.status)  # a flipped bit the bundle decoded through: valid, or only the checksum differs


def test_fewer_than_64_streams_and_large_ones(bundle):
    datas = [corpus.zipf_text(1500 + 100 * k, k) for k in range(5)]
    streams = [fixed(d) for d in datas]
    assert check(bundle, streams, [len(d) for d in datas], [True] * 5) == 5
    # larger streams: far matches (older than the lane's 512-byte window), long matches, matches that overlap themselves, a level-9 parse
    datas = [corpus.zipf_text(30000 + 1111 * k, k) for k in range(6)] + [bytes([7]) * 70000, (corpus.zipf_text(700, 9) * 90)[:60000],
             bytes(b % 144 for b in corpus.random_bytes(40000, 5)), corpus.mixed_data(50000, 2), corpus.mixed_data(50000, 3)]
    streams = [fixed(d, level=9 if k % 2 else 1, blocks=1 + k % 3) for k, d in enumerate(datas)]
    assert check(bundle, streams, [len(d) for d in datas], [True] * len(datas)) == len(datas)


# ---- tests/bundle_cases.py: streams written token by token at the lanes' edges -------------------------------------------------------
GUARD = 64  # bytes of 0xCD behind every capacity


def _model_lib():
    import os
    from conftest import ROOT
    _build_model([])
    M = C.CDLL(os.path.join(ROOT, "tests", "model", "libpzgmodel.so"))
    M.pzm_bundle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    M.pzm_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(R)]
    return M


def run_lanes(M, lanes):
    """One bundle: lanes[k] is the Case of lane k, or None for a lane without a stream.  Returns, per lane, (result, the output buffer
    as the bundle left it: capacity + GUARD bytes that were 0xCD)."""
    n = len(lanes)
    assert n <= 64
    streams = [c.stream if c else b"" for c in lanes]
    caps = [c.cap if c else 0 for c in lanes]
    ins = (C.c_char_p * n)(*streams)
    lens = (C.c_uint64 * n)(*[len(z) for z in streams])
    bufs = [C.create_string_buffer(b"\xcd" * (cap + GUARD), cap + GUARD) for cap in caps]
    outs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    capa = (C.c_uint64 * n)(*caps)
    res = (R * n)()
    assert M.pzm_bundle(ins, lens, outs, capa, n, res) == 0
    return [(res[k], bufs[k]) for k in range(n)]


def check_lane(M, c, r, buf, expect):
    """What lane results must be: a clean lane is the oracle's result bit for bit; a stream a lane hands back is decoded by the ordinary
    model from byte 0 INTO THE BUFFER THE LANE WROTE TO, as on the device, and is the oracle's result then -- status, out_len, the bytes
    below min(out_len, cap), the checksum rule of include/pzg.h for failed streams; nothing behind the capacity is touched, and nothing
    is said about the bytes between out_len and the capacity.  Returns whether the lane was clean."""
    ro, oo = expect
    guard = b"\xcd" * GUARD
    assert buf.raw[c.cap:] == guard, (c.name, "a lane wrote past the capacity")
    if r.status != TODO:
        assert same(ro, oo, r, buf.raw[: min(r.out_len, c.cap)], c.cap), (c.name, ro.status, r.status, ro.out_len, r.out_len, ro.in_used, r.in_used, hex(ro.adler), hex(r.adler))
        return True
    for rb in (11, 15):
        again = C.create_string_buffer(buf.raw, c.cap + GUARD)
        rm = R()
        assert M.pzm_decompress(c.stream, len(c.stream), again, c.cap, rb, C.byref(rm)) == 0
        assert again.raw[c.cap:] == guard, (c.name, rb, "written past the capacity")
        assert same(ro, oo, rm, again.raw[: min(rm.out_len, c.cap)], c.cap), (c.name, rb, ro.status, rm.status, ro.out_len, rm.out_len)
    return False


def shuffled_bundles(cases, seed=0xB5):
    """The cases in seeded order, 48 to 64 to a bundle, the other lanes without a stream: families mix, every lane is used."""
    rng = random.Random(seed)
    order = list(cases)
    rng.shuffle(order)
    k = 0
    while k < len(order):
        n = rng.randrange(48, 65)
        lanes = order[k:k + n] + [None] * (64 - len(order[k:k + n]))
        rng.shuffle(lanes)
        yield lanes
        k += n


def model_clean_set(cases):
    """Names of the cases a lane of the host model decodes itself (everything else it hands back): what a device lane must do too --
    a lane's outcome depends on its own stream alone.  tests/test_gpu_bundle_edges.py holds the lab library to it."""
    M = _model_lib()
    clean = set()
    for lanes in shuffled_bundles(cases):
        for c, (r, _buf) in zip(lanes, run_lanes(M, lanes)):
            if c is not None and r.status != TODO:
                clean.add(c.name)
    return clean


def expected_clean(c):
    """plain: a lane decodes it, without exception; a wrong trailer: a lane reports it (as the reference does, Deflate.hs:52-63); everything else: 103."""
    return c.plain or c.wrong_trailer


@pytest.fixture(scope="module")
def edge_cases():
    import bundle_cases
    cases = bundle_cases.all_cases()
    return cases, {c.name: O.decompress(c.stream, c.cap) for c in cases}


def test_edge_cases_are_what_they_say(edge_cases):
    """The oracle on every case: a plain one decodes to its data, whole; the count is the grid's 3,900 and the other families."""
    import collections
    import bundle_cases
    cases, expect = edge_cases
    count = collections.Counter(c.family for c in cases)
    print("bundle cases: %d" % len(cases), dict(count))
    assert count["grid"] >= 3900 and len(cases) >= 3900 + 736 and all(count[f] for f in ("handover", "overlap", "bitrate", "blocks", "tails", "capacity", "sizes"))
    for c in cases:
        ro, oo = expect[c.name]
        if c.plain:
            assert ro.status == 0 and oo == c.data and ro.out_len == len(c.data) and ro.adler == zlib.adler32(c.data), c.name
            assert ro.in_used <= len(c.stream)
        elif c.wrong_trailer:
            assert ro.status == 10, (c.name, ro.status)
        elif c.family == "sizes":  # valid, and a MiB or more: not a lane's
            assert ro.status == 0 and oo == c.data and max(len(c.stream), c.cap) >= bundle_cases.MAX_BYTES, c.name
        else:
            assert ro.status != 0, (c.name, ro.status)


@pytest.mark.parametrize("lane", [0, 63])
def test_edge_cases_alone_in_a_bundle(edge_cases, lane):
    """Every case as the only stream of its bundle, in the first lane and in the last (the model gives lane k's input the alignment k % 4)."""
    cases, expect = edge_cases
    M = _model_lib()
    for c in cases:
        r, buf = run_lanes(M, [None] * lane + [c])[lane]
        clean = check_lane(M, c, r, buf, expect[c.name])
        assert clean == expected_clean(c), (c.name, lane, r.status, "plain" if c.plain else "not plain")


def test_edge_cases_mixed_in_bundles(edge_cases):
    """Every case among 47 to 63 others of every family, some lanes without a stream; twice, in different company and lanes."""
    cases, expect = edge_cases
    M = _model_lib()
    for seed in (0xB5, 0xB6):
        seen = 0
        for lanes in shuffled_bundles(cases, seed):
            for c, (r, buf) in zip(lanes, run_lanes(M, lanes)):
                if c is None:
                    assert r.status == TODO
                    continue
                seen += 1
                clean = check_lane(M, c, r, buf, expect[c.name])
                assert clean == expected_clean(c), (c.name, seed, r.status, "plain" if c.plain else "not plain")
        assert seen == len(cases)
    assert model_clean_set(cases) == {c.name for c in cases if expected_clean(c)}


def test_high_and_low_bit_rates_share_a_bundle(edge_cases):
    """Steps of 49 bits, runs of 9-bit literals and distance-1 matches of 258 bytes (the fewest bits a step) next to each other: the
    rings of all lanes are refilled when one lane is down to BQ_LOW pairs."""
    import bundle_cases
    cases, expect = edge_cases
    M = _model_lib()
    rate = bundle_cases.family("bitrate")
    lanes = (rate * 4)[:64]
    random.Random(3).shuffle(lanes)
    for c, (r, buf) in zip(lanes, run_lanes(M, lanes)):
        assert check_lane(M, c, r, buf, expect[c.name]), c.name
