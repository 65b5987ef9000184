"""CPU: every kernel core that compiles for the host, under AddressSanitizer and UBSan as stand-alone programs (tests/cxx/san_*.cpp
with the model files of tests/model/): the gzip, FDICT, raw, segment / index-build and resumable instances of inflate_core.h,
the member finder and layout of member_core.h and the scanline unfilter of unfilter_core.h.  The kernels' READ contracts -- "nothing
is read but the aligned dwords that hold input bytes", a dictionary of dict_len bytes, a resume slot of ResumeSlot<RB>::BYTES --
show nowhere on the device; here every buffer is a heap block of exactly its size, so a read or a write one byte outside it is a report.

The cases are the shared lists of the unsanitized model tests, whole unless a stride is stated, and each program compares what it
gets with the expectation in its case file (tests/sancases.py: system zlib, the oracle, the plain-Python references), so a clean run
that decoded garbage fails too.  Each test asserts that the program ran as many cases as were written."""
import struct
import zlib

import numpy as np
import pytest

import sancases as S


def _u64(xs):
    return np.asarray(xs, dtype=np.uint64).tobytes()


# ---- unfilter_core.h ---------------------------------------------------------------------------------------------------------------------

def test_unfilter_core(tmp_path_factory):
    """All of pngcases.shape_cases(), filter_cases(), error_cases() and empty_case() at the two layouts of
    test_model_unfilter.check(): src exactly the aligned dwords that hold it at misalignment 0-3, dst exactly those that hold the
    image's extent."""
    import pngcases as PC
    d = tmp_path_factory.mktemp("san_unfilter")
    exe = S.build(str(d / "san_unfilter"), ["tests/cxx/san_unfilter.cpp", "tests/model/model_unfilter.cpp"])
    cases = []
    for group in (PC.shape_cases(), PC.filter_cases(), PC.error_cases() + [PC.empty_case()]):
        for i, c in enumerate(group):
            for mis, dst_off, extra in ((i % 4, (1, 7, 12, 3, 0)[i % 5], 5), ((i + 1) % 4, 16, 0)):
                stride = c.row_bytes + extra
                want = np.full(dst_off + c.height * stride + 9, PC.FILL, np.uint8)
                for r, row in enumerate(c.rows):
                    want[dst_off + r * stride:dst_off + r * stride + c.row_bytes] = np.frombuffer(row, np.uint8)
                cases.append(["%s mis %d off %d" % (c.name, mis, dst_off), c.stream, mis, dst_off, stride, c.row_bytes, c.height, c.bpp,
                              c.status, c.d0, c.d1, want.tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == 2 * (len(PC.shape_cases()) + len(PC.filter_cases()) + len(PC.error_cases()) + 1)
    S.run(exe, str(d / "cases.bin"), n)


# ---- member_core.h -----------------------------------------------------------------------------------------------------------------------

def test_member_core(tmp_path_factory):
    """memberscheck.sound_files() + finder_files() at chunks 64, 4096 and 0 (64 KiB), every misalignment: starts / bsize of exactly
    max_members entries -- the count, none, and one fewer than the count --, then the layouts of test_model_members.py in arrays of
    exactly m entries.  Expected: the plain-Python finder and the numpy layout."""
    import memberscheck as M
    d = tmp_path_factory.mktemp("san_members")
    exe = S.build(str(d / "san_members"), ["tests/cxx/san_members.cpp", "tests/model/model_members.cpp"])
    files = [(name, z) for name, z, _d, _f in M.sound_files()] + M.finder_files()
    cases = []
    for k, (name, z) in enumerate(files):
        starts, bsize = M.find(z)
        for chunk in (64, 4096, 0):
            for j, room in enumerate((len(starts), 0, len(starts) - 1)):
                mis = (k + j + (chunk >> 6)) % 4
                cases.append(["%s chunk %d room %d" % (name, chunk, room), 0, z, mis, chunk, room, len(starts), _u64(starts[:room]),
                              np.asarray(bsize[:room], dtype=np.uint32).tobytes()])
        for some in (starts, starts[:1], starts[::2]):
            for base, mis in ((0, 0), (12345678901, 3)):
                io, il, oo, oc, total = M.layout(z, some, base)
                cases.append(["%s layout of %d" % (name, len(some)), 1, z, mis, _u64(some), base, io.tobytes(), il.tobytes(), oo.tobytes(), oc.tobytes(), total])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == len(files) * (9 + 6)
    S.run(exe, str(d / "cases.bin"), n)


# ---- inflate_core.h: the raw instances and the FDICT path --------------------------------------------------------------------------------

RINGS = (11, 12, 15)
ROOM = 300  # as tests/test_model_history.py: a stream that goes on where it must stop has room to show it


def planned(c):
    """tests/test_model_history.py: what a case of history_cases plans, as (cmp, status, d0, d1, out_len, in_used, checksum, bytes)"""
    d = c["data"]
    if c["expect"] == ("ok",):
        return S.OUT_LEN | S.SUM | S.BYTES, 0, 0, 0, len(d), 0, zlib.adler32(d), d
    _kind, dist, op = c["expect"]
    return S.D0 | S.D1 | S.OUT_LEN | S.SUM | S.BYTES, 11, dist, op, op, 0, zlib.adler32(d), d


@pytest.fixture(scope="module")
def raw_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("san_raw")
    return S.build(str(d / "san_raw"), ["tests/cxx/san_inflate.cpp", "tests/model/model_raw.cpp"], ["SAN_RAW"]), d


@pytest.fixture(scope="module")
def harness_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("san_harness")
    return S.build(str(d / "san_harness"), ["tests/cxx/san_inflate.cpp", "tests/model/model_harness.cpp"], ["SAN_HARNESS"]), d


@pytest.fixture(scope="module")
def pool_cases(oracle):
    """rawcheck.stream_pool(), every stream with a generous capacity and every third at capacities 0, 1, len - 1 and len
    (tests/test_model_raw.py), without a ring yet: [(name, stream, cap, expectation)]"""
    import rawcheck
    out = []
    for k, (name, d) in enumerate(rawcheck.stream_pool()):
        big = S.raw_expect(oracle, d, 1 << 21)
        out.append((name, d, 1 << 21, big))
        if k % 3 == 0:
            full = big[4]
            for cap in sorted({0, 1, max(full - 1, 0), full}):
                out.append(("%s cap %d" % (name, cap), d, cap, S.raw_expect(oracle, d, cap)))
    return out


@pytest.mark.parametrize("no_strips", [False, True])
def test_raw_instances_stream_pool(raw_exe, pool_cases, no_strips):
    """Decoder<RB, false, false, true> for rings 11, 12 and 15 (the small rings' ST_RETRY_FULL_RING second pass included) over
    rawcheck.stream_pool(): exact input dwords in both placements, an output of exactly cap bytes, cap 0 and cap < out_len included."""
    exe, d = raw_exe
    cases = [S.inflate_case("%s ring %d" % (name, rb), S.RAW, z, b"", cap, rb, *e) for name, z, cap, e in pool_cases for rb in RINGS]
    n = S.write_cases(str(d / "pool.bin"), cases)
    assert n == len(pool_cases) * len(RINGS)
    S.run(exe, str(d / "pool.bin"), n, no_strips)


@pytest.mark.parametrize("no_strips", [False, True])
def test_raw_instances_history(raw_exe, no_strips):
    """history_cases.cases() through the raw instances with a dictionary of exactly dict_len bytes (1, 32767, 32768 bytes and the
    rest; distances that reach byte 0 of it and one past it), and the CONTRACT cases at capacities len / 2 and 0 and cut at 2/3."""
    import history_cases as H
    exe, d = raw_exe
    cases = []
    for c in H.cases():
        for rb in RINGS:
            cases.append(S.inflate_case("%s ring %d" % (c["name"], rb), S.RAW, c["raw"], c["zdict"], len(c["data"]) + ROOM, rb, *planned(c)))
    for name in H.CONTRACT:
        c = H.by_name(name)
        data = c["data"]
        cut, prefix = H.truncated(c)
        for rb in RINGS:
            for cap in (len(data) // 2, 0):
                cases.append(S.inflate_case("%s ring %d cap %d" % (name, rb, cap), S.RAW, c["raw"], c["zdict"], cap, rb, S.OUT_LEN | S.SUM, 14, 0, 0, len(data)))
            cases.append(S.inflate_case("%s ring %d cut" % (name, rb), S.RAW, cut, c["zdict"], len(data), rb, S.OUT_LEN | S.SUM | S.BYTES, 1, 0, 0,
                                        len(prefix), 0, zlib.adler32(prefix), prefix))
    n = S.write_cases(str(d / "history.bin"), cases)
    assert n == len(RINGS) * (len(H.cases()) + 3 * len(H.CONTRACT))
    S.run(exe, str(d / "history.bin"), n, no_strips)


def test_fdict_path(harness_exe, oracle):
    """pzm_decompress_dict over history_cases.cases() in their zlib form, a wrong DICTID for every history length, and the CONTRACT
    cases at capacities len / 2 and 0 and cut at 2/3: the dictionary is exactly dict_len bytes.  Expected: the plan, and the oracle
    with the dictionary installed for what fails."""
    import history_cases as H
    exe, d = harness_exe
    cases, seen = [], set()
    for c in H.cases():
        z, zd = H.zlib_wrap(c), c["zdict"]
        e = planned(c)
        cap = len(c["data"]) + ROOM
        if e[1] == 0:
            e = (e[0] | S.IN_USED,) + e[1:5] + (len(z),) + e[6:]
        else:
            ro, oo = oracle.decompress_dict(z, zd, cap)
            assert S.oracle_expect(ro, oo, cap) == e, c["name"]
        cases.append(S.inflate_case(c["name"], S.FDICT, z, zd, cap, 15, *e))
        if (len(zd), zd[:1]) not in seen:
            seen.add((len(zd), zd[:1]))
            ours = zlib.adler32(zd)
            zbad = H.zlib_wrap(c, dictid=ours ^ (1 << 16))
            ro, oo = oracle.decompress_dict(zbad, zd, cap)
            assert (ro.status, ro.detail0, ro.detail1, ro.out_len) == (20, ours ^ (1 << 16), ours, 0)
            cases.append(S.inflate_case(c["name"] + " wrong dictid", S.FDICT, zbad, zd, cap, 15, S.D0 | S.D1 | S.OUT_LEN | S.BYTES, 20, ro.detail0, ro.detail1))
    for name in H.CONTRACT:
        c = H.by_name(name)
        data, zd, z = c["data"], c["zdict"], H.zlib_wrap(c)
        for cap in (len(data) // 2, 0):
            cases.append(S.inflate_case("%s cap %d" % (name, cap), S.FDICT, z, zd, cap, 15, S.OUT_LEN | S.SUM, 14, 0, 0, len(data)))
        cut, prefix = H.truncated(c)
        zc = H.FDICT_HDR + zlib.adler32(zd).to_bytes(4, "big") + cut
        ro, oo = oracle.decompress_dict(zc, zd, len(data))
        assert (ro.status, ro.out_len, ro.adler, oo) == (1, len(prefix), zlib.adler32(prefix), prefix)
        cases.append(S.inflate_case(name + " cut", S.FDICT, zc, zd, len(data), 15, S.OUT_LEN | S.SUM | S.BYTES, 1, 0, 0, len(prefix), 0, ro.adler, prefix))
    n = S.write_cases(str(d / "fdict.bin"), cases)
    assert n == len(H.cases()) + len(seen) + 3 * len(H.CONTRACT) and len(seen) >= len(H.LENGTHS)
    S.run(exe, str(d / "fdict.bin"), n)


# ---- inflate_core.h: the gzip instance ---------------------------------------------------------------------------------------------------

def _gzip_header_len(z):
    """RFC 1952 2.3: the bytes in front of the compressed blocks of a member with a sound header"""
    flg, at = z[3], 10
    if flg & 4:
        at += 2 + struct.unpack_from("<H", z, at)[0]
    for bit in (8, 16):
        if flg & bit:
            at = z.index(b"\0", at) + 1
    return at + (2 if flg & 2 else 0)


def _gzip_expect(oracle, z, cap, clean=None):
    """tests/test_model_vs_oracle.py (test_model_gzip_members): the oracle's gzip reader; an output that outgrows its capacity is not
    stored, so its CRC-32 and ISIZE are not verified.  clean: the data of a stream system zlib wrote."""
    ro, oo = oracle.gzip_decompress(z, cap)
    if clean is not None:
        assert (ro.status, oo, ro.adler, ro.in_used) == (0, clean, zlib.crc32(clean), len(z))
        return S.OUT_LEN | S.IN_USED | S.SUM | S.BYTES, 0, 0, 0, len(clean), len(z), ro.adler, oo
    if ro.status in (10, 19) and ro.out_len > cap:
        return S.OUT_LEN, 14, 0, 0, ro.out_len, 0, 0, b""
    if ro.status == 0:
        return S.OUT_LEN | S.SUM | S.BYTES, 0, 0, 0, ro.out_len, 0, ro.adler, oo
    # a failed stream delivers what the oracle had decoded by then: out_len, the bytes below the capacity, their CRC-32 (0 past it)
    return (S.OUT_LEN | S.SUM | S.BYTES | (S.D0 | S.D1 if ro.status in (10, 19) else 0), ro.status, ro.detail0, ro.detail1, ro.out_len, 0,
            0 if ro.out_len > cap else ro.adler, oo)


def test_gzip_instance(harness_exe, oracle):
    """pzm_decompress_gzip: corpus.gzip_member with every mix of FEXTRA, FNAME, FCOMMENT and FHCRC, sound and corrupted, files of
    several members, and every header that has all four fields cut at each of its bytes (and at each byte of the trailer)."""
    import gzip
    import corpus
    import resume_fmt_cases as K
    exe, d = harness_exe
    cases, flags, ncut = [], set(), 0

    def add(name, z, cap, e, rings=RINGS):
        for rb in rings:
            cases.append(S.inflate_case("%s ring %d" % (name, rb), S.GZIP, z, b"", cap, rb, *e))

    all_fields = []
    for seed in range(60):
        data = corpus.mixed_data((seed * 613) % 30000, seed)
        z = corpus.gzip_member(data, seed)
        flags.add(z[3])
        if z[3] == 0x1e:
            all_fields.append(z)
        add("member %d" % seed, z, len(data) + 8, _gzip_expect(oracle, z, len(data) + 8, data))
        for c in range(8):
            zc = corpus.corrupt(z, seed * 64 + c)
            add("member %d corrupt %d" % (seed, c), zc, len(data) + 8, _gzip_expect(oracle, zc, len(data) + 8))
    assert len(flags) >= 12 and len(all_fields) >= 2  # (of the 16 mixes of the four optional fields)
    for seed in range(30):
        parts = [corpus.mixed_data((seed * 977 + 131 * k) % 40000, seed + k) for k in range(1 + seed % 4)]
        g = b"".join(corpus.gzip_member(p, seed + k) if k % 2 else gzip.compress(p, 1 + seed % 9) for k, p in enumerate(parts))
        data = b"".join(parts)
        assert gzip.decompress(g) == data
        add("members %d" % seed, g, len(data) + 8, _gzip_expect(oracle, g, len(data) + 8, data), (15, 11))
        for c in range(6):
            gc = corpus.corrupt(g, seed * 32 + c)
            add("members %d corrupt %d" % (seed, c), gc, len(data) + 8, _gzip_expect(oracle, gc, len(data) + 8), (15,))
    text = corpus.zipf_text(900, 11)
    rich = K.member(zlib.compress(text, 6)[2:-4], text, K.rich_header())
    for k, z in enumerate([rich] + all_fields[:2]):
        n = _gzip_header_len(z)
        for cut in list(range(n + 1)) + list(range(len(z) - 8, len(z))):
            e = _gzip_expect(oracle, z[:cut], 1 << 16)
            assert e[1] == 1 and (cut > n or e[4] == 0)  # (inside the header: nothing is delivered)
            add("header %d cut at %d" % (k, cut), z[:cut], 1 << 16, e, (11, 15))
            ncut += 1
    n = S.write_cases(str(d / "gzip.bin"), cases)
    assert n == 60 * 9 * 3 + 30 * (2 + 6) + 2 * ncut and 100 < ncut < 1000
    S.run(exe, str(d / "gzip.bin"), n)
    S.run(exe, str(d / "gzip.bin"), n, no_strips=True)


# ---- inflate_core.h: the segment decoder and the index build ---------------------------------------------------------------------------

def test_segment_decoder_and_index_build(tmp_path_factory):
    """Decoder<15, false, false, true, true> over indexcheck.model_inputs(): index builds at spans 1, 4096 and 40000 into exactly
    max_points points -- more than the stream has, 3 and none (idx_points up to and past idx_cap) --, every segment the points cut
    a stream into (seg_start / seg_end inside a byte, a window of exactly the bytes in front of it: shorter than 32 KiB for the first
    ones, an output of exactly its bytes), the segments of history_cases at all eight start bits, capacities one short and 0.
    Bytes, lengths and checksums are system zlib's.  The points are those of the unsanitized model, which
    tests/test_model_segments.py holds to system zlib one by one (check_point); the sparsest lists are checked so here as well."""
    import history_cases as H
    import indexcheck as X
    d = tmp_path_factory.mktemp("san_seg")
    exe = S.build(str(d / "san_seg"), ["tests/cxx/san_inflate.cpp", "tests/model/model_seg.cpp"], ["SAN_SEG"])
    m = X.SegModel()
    inputs = X.model_inputs()
    cases, nbuild, nseg = [], 0, 0

    def seg(name, inp, sb, eb, win, cap, e, span=0, max_points=0, npoints=0, pts=()):
        cases.append(S.inflate_case(name, S.SEG, inp, win, cap, 15, *e, more=[sb, eb, span, max_points, npoints, _u64([x for p in pts for x in p])]))

    for k, (name, z, data) in enumerate(inputs):
        ends = m.build(z, len(data), 1, 8192)[3]
        whole = (S.OUT_LEN | S.IN_USED | S.SUM | S.BYTES, 0, 0, 0, len(data), len(z), zlib.adler32(data), data)
        for span in (1, 4096, 40000):
            pts = X.expected_points(ends, span)
            assert len(pts) < 8192
            if span == 40000:
                for bit, pos in pts:
                    X.check_point(z, bit, pos, data[max(0, pos - X.WINDOW):pos], data, (name, span))
            for room in (len(pts) + 1, 3, 0) if span != 1 else (len(pts),):
                seg("%s build span %d room %d" % (name, span, room), z, 0, 0, b"", len(data), whole, span, room, len(pts), pts[:room])
                nbuild += 1
            if span == 1 and k % 4:  # stride: the segments of every block end for every fourth input, of the wider spans for all
                continue
            for off, ln, sb, eb, a, b in X.segments(pts, len(z), len(data)):
                e = (S.OUT_LEN | S.IN_USED | S.SUM | S.BYTES, 0, 0, 0, b - a, ln, zlib.adler32(data[a:b]), data[a:b])
                seg("%s span %d segment at %d" % (name, span, a), z[off:off + ln], sb, eb, data[max(0, a - X.WINDOW):a], b - a, e)
                nseg += 1
                if b - a and nseg % 16 == 0:
                    for cap in (b - a - 1, 0):
                        seg("%s span %d segment at %d cap %d" % (name, span, a, cap), z[off:off + ln], sb, eb, data[max(0, a - X.WINDOW):a], cap,
                            (S.OUT_LEN | S.SUM, 14, 0, 0, b - a, 0, 0, b""))
                        nseg += 1
    nhist = 0
    for k, c in enumerate(H.cases()):
        s = H.seg_wrap(c, k % 8)
        e = planned(c)
        if e[1] == 0:
            e = (e[0] | S.IN_USED,) + e[1:5] + (s["in_used"],) + e[6:]
        for end_bit in (s["end_bit"], 0):
            seg("%s start bit %d end bit %d" % (c["name"], k % 8, end_bit), s["inp"], s["start_bit"], end_bit, s["window"], len(c["data"]) + ROOM, e)
            nhist += 1
    n = S.write_cases(str(d / "seg.bin"), cases)
    assert n == nbuild + nseg + nhist and nbuild == 7 * len(inputs) and nseg > 1000 and nhist == 2 * len(H.cases())
    S.run(exe, str(d / "seg.bin"), n)



# ---- inflate_core.h: the resumable decoders ----------------------------------------------------------------------------------------------

PAIRS = [(feed, room) for feed in (1, 7, 0) for room in (0, 1, 4096)]  # bytes per feed (0: the whole input) x bytes of room per call


def resume_cases(oracle):
    """The streams of resume_fmt_cases.fixture_cases() and corner_cases(), each once per format it has there -- and, where a case
    carries the same body as a zlib stream, that one for the zlib decoders, rings 15, 12 and 11 in turn --, as [(name, format, ring,
    stream, expectation)].  (The lists cut one stream in many ways; here the program does the cutting.)  Expected: system zlib for
    what it accepts (bytes, the input consumed, Adler-32 or CRC-32), else the oracle: its gzip reader, and for raw streams the
    wrapped stream of tests/rawcheck.py -- status, length and the bytes delivered."""
    import resume_fmt_cases as K
    out, seen = [], set()
    for c in K.fixture_cases(lambda n: (4096,)) + K.corner_cases():
        forms = [(K.FLAG[c["fmt"]], 12, c["stream"])]
        if c["zpieces"] is not None:
            forms.append((0, (15, 12, 11)[sum(1 for f, _s in seen if f == 0) % 3], b"".join(c["zpieces"])))
        for fmt, ring, s in forms:
            if (fmt, s) in seen:
                continue
            seen.add((fmt, s))
            if fmt == 0:
                ro, oo = oracle.decompress(s, 1 << 21)
                e = S.oracle_expect(ro, oo, 1 << 21, details=False)
                assert ro.status != 0 or oo == zlib.decompress(s)
            else:
                o = zlib.decompressobj(31 if fmt == K.GZIP else -15)
                try:
                    data = o.decompress(s)
                    while fmt == K.GZIP and o.eof and o.unused_data[:2] == b"\x1f\x8b":  # the members that follow
                        rest = o.unused_data
                        o = zlib.decompressobj(31)
                        data += o.decompress(rest)
                    ok = o.eof
                except zlib.error:
                    ok = False
                if ok:
                    e = (S.OUT_LEN | S.IN_USED | S.SUM | S.BYTES, 0, 0, 0, len(data), len(s) - len(o.unused_data),
                         zlib.crc32(data) if fmt == K.GZIP else zlib.adler32(data), data)
                elif fmt == K.GZIP:
                    ro, oo = oracle.gzip_decompress(s, 1 << 21)
                    assert ro.status != 0, c["name"]
                    e = (S.OUT_LEN | S.BYTES, ro.status, 0, 0, ro.out_len, 0, 0, oo)
                else:
                    e = S.raw_expect(oracle, s, 1 << 21)
                    assert e[1] != 0, c["name"]
                    e = (S.OUT_LEN | S.BYTES,) + e[1:]
            out.append((c["name"], fmt, ring, s, e))
    return out


def _resume_file(path, cases, formats, per):
    """Every stream at `per` of the nine pairs of feed size and room: all nine, or three -- a stride of four through PAIRS that
    starts one further for each stream, so every pair meets every third stream; final_in with the last piece for every other one."""
    rows = []
    for k, (name, fmt, ring, s, e) in enumerate(c for c in cases if c[1] in formats):
        for j in range(per):
            feed, room = PAIRS[(k + 4 * j) % 9]
            rows.append(S.inflate_case("%s format %d feed %d room %d" % (name, fmt, feed, room), S.RESUME, s, b"", 0, ring, *e,
                                       more=[fmt, feed, (k + j) & 1, room]))
    return S.write_cases(path, rows), rows


@pytest.fixture(scope="module")
def resumable(oracle):
    return resume_cases(oracle)


def test_resumable_zlib_decoders(harness_exe, resumable):
    """pzm_resume_feed_rb for rings 15, 12 and 11: the slot is exactly pzm_resume_state_bytes_rb(ring) bytes, every feed exactly the
    aligned dwords that cover it, every room exactly its bytes -- none at all and one byte among them.  All nine pairs for every
    stream (the nine fixtures and the bodies of three corner cases)."""
    exe, d = harness_exe
    n, rows = _resume_file(str(d / "resume.bin"), resumable, (0,), 9)
    assert n == 9 * sum(1 for c in resumable if c[1] == 0) and n >= 100 and {r[5] for r in rows} == {11, 12, 15}
    S.run(exe, str(d / "resume.bin"), n)
    S.run(exe, str(d / "resume.bin"), n, no_strips=True)


def test_resumable_gzip_and_raw_decoders(tmp_path_factory, resumable):
    """model_resume_fmt.cpp, Decoder<12, true, true> and Decoder<12, false, true, true>: the slot is exactly pzm_fmt_state_bytes()
    bytes, the LDS image and the 32 KiB history inside it.  STRIDE: three of the nine pairs for each stream (see _resume_file)."""
    d = tmp_path_factory.mktemp("san_fmt")
    exe = S.build(str(d / "san_fmt"), ["tests/cxx/san_inflate.cpp", "tests/model/model_resume_fmt.cpp"], ["SAN_FMT"])
    n, rows = _resume_file(str(d / "resume.bin"), resumable, (4, 32), 3)
    assert n == 3 * sum(1 for c in resumable if c[1] != 0) and n >= 200
    assert {(r[15], r[17]) for r in rows} == set(PAIRS) and {r[14] for r in rows} == {4, 32}
    S.run(exe, str(d / "resume.bin"), n)
    S.run(exe, str(d / "resume.bin"), n, no_strips=True)
