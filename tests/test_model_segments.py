"""CPU: the SEGMENT instance of the kernel source -- Decoder<15, false, false, true, true>: a raw decoder that starts at a bit inside
a byte, stops at a block boundary that need not be the final block's, and records access points -- compiled as a host program
(tests/model/model_seg.cpp) and checked against system zlib alone (tests/indexcheck.py)."""
import zlib

import pytest

import indexcheck as X

SPANS = [1, 4096, 40000]


@pytest.fixture(scope="session")
def seg_model():
    return X.SegModel()


@pytest.fixture(scope="session")
def inputs():
    return X.model_inputs()


@pytest.fixture(scope="session")
def built(seg_model, inputs):
    """(name, span) -> the points of the model's index build; every build must itself be what PZG_RAW delivers."""
    got = {}
    for name, d, data in inputs:
        for span in SPANS:
            r, out, n, pts = seg_model.build(d, len(data), span, 8192)
            assert (r.status, r.out_len, r.in_used, r.adler) == (0, len(data), len(d), zlib.adler32(data)) and out == data, (name, span, r.status)
            assert n == len(pts), (name, span, n)
            got[name, span] = pts
    return got


def test_inputs_reach_every_bit_offset(inputs, built):
    """A condition on the inputs: points at all eight values of in_bit & 7, streams of every block type, many points."""
    assert len(inputs) > 60
    assert {bit & 7 for (name, span), pts in built.items() for bit, _ in pts} == set(range(8))
    assert sum(len(p) for p in built.values()) > 1000


def test_recorder(inputs, built):
    total, phases = 0, set()
    for name, d, data in inputs:
        ends = built[name, 1]  # span 1: every non-final block end (that produced anything since the last)
        for span in SPANS:
            pts = built[name, span]
            assert pts == X.expected_points(ends, span), (name, span)  # none missing, none extra
            for k, (bit, pos) in enumerate(pts):
                assert 0 < bit < 8 * len(d) and 0 < pos <= len(data), (name, span, k)
                if k:
                    assert bit > pts[k - 1][0] and pos - pts[k - 1][1] >= span, (name, span, k)
                else:
                    assert pos >= span
            for bit, pos in pts:  # the independent check, every point
                X.check_point(d, bit, pos, data[max(0, pos - X.WINDOW):pos], data, (name, span))
                total += 1
                phases.add(bit & 7)
    assert total > 1000 and phases == set(range(8))


def test_over_capacity_reports_the_full_count(seg_model, inputs, built):
    for name, d, data in inputs[-7:]:
        full = built[name, 4096]
        r, out, n, pts = seg_model.build(d, len(data), 4096, 3)
        assert r.status == 0 and n == len(full) and pts == full[:3], name


def test_segments(seg_model, inputs, built):
    """Each segment decoded alone -- its own start bit, its end bit, the window as its dictionary, its input cut to the bytes that
    hold its bits, an exact capacity between guards -- is its slice of the reference."""
    count, phases = 0, set()
    for name, d, data in inputs:
        for span in SPANS:
            segs = X.segments(built[name, span], len(d), len(data))
            assert segs[0][4] == 0 and segs[-1][5] == len(data) and all(s[5] == t[4] for s, t in zip(segs, segs[1:])), (name, span)
            for off, ln, sb, eb, a, b in segs:
                r, out = seg_model.segment(d[off:off + ln], sb, eb, data[max(0, a - X.WINDOW):a], b - a)
                assert (r.status, r.out_len, r.adler) == (0, b - a, zlib.adler32(data[a:b])) and out == data[a:b], (name, span, a, b, r.status, r.detail0)
                assert r.in_used == ln, (name, span, a, r.in_used, ln)
                count += 1
                phases.add(sb)
    assert count > 1000 and phases == set(range(8))


@pytest.mark.parametrize("first", [(258, 32768), (258, 1), (3, 1)])
def test_seam(seg_model, first):
    data, d = X.seam_stream(first)
    assert zlib.decompressobj(-15).decompress(d) == data
    r, out, n, pts = seg_model.build(d, len(data), 32768)
    assert r.status == 0 and out == data and n == 1 and pts[0][1] == 32768
    X.check_point(d, pts[0][0], 32768, data[:32768], data)
    (s0, s1) = X.segments(pts, len(d), len(data))
    for off, ln, sb, eb, a, b in (s0, s1):
        r, out = seg_model.segment(d[off:off + ln], sb, eb, data[max(0, a - X.WINDOW):a], b - a)
        assert (r.status, r.out_len, r.adler) == (0, b - a, zlib.adler32(data[a:b])) and out == data[a:b], (first, a)
    assert data[32768:32768 + first[0]] == bytes(data[32768 - first[1] + k % first[1]] for k in range(first[0]))


def test_errors(seg_model, inputs, built):
    for name, d, data in inputs[-7:-1]:  # (the six big inputs)
        cases, (a, b, la, lb) = X.error_cases(d, data, built[name, 4096])
        for what, inp, sb, eb, win, cap, ok in cases:
            r, out = seg_model.segment(inp, sb, eb, win, cap)  # (asserts the guards on both sides of the capacity)
            assert r.status != 0 and ok(r.status, r.detail0, r.out_len), (name, what, r.status, r.detail0, r.detail1, r.out_len)
            base = la if what == "beyond the final block" else a
            if r.status != X.E_OUT_TOO_SMALL:  # what was decoded by then is delivered, and is the stream's
                assert out == data[base:base + len(out)] and len(out) == min(r.out_len, cap), (name, what)
                if r.out_len <= cap:
                    assert r.adler == zlib.adler32(out), (name, what)
            if r.status == X.E_SEGMENT:
                assert r.detail1 > 0, (name, what)


def test_wrong_window_decodes_to_other_bytes(seg_model, inputs, built):
    """A segment cannot know its window is wrong: PZG_OK, other bytes.  (The mirror's checksum combine catches it: tests/test_indexed_host.py
    and tests/test_gpu_indexed.py.)"""
    name, d, data = inputs[-7]
    assert name == "text6"
    off, ln, sb, eb, a, b = X.segments(built[name, 40000], len(d), len(data))[2]
    r, out = seg_model.segment(d[off:off + ln], sb, eb, b"\0" * X.WINDOW, b - a)
    assert (r.status, r.out_len) == (0, b - a) and out != data[a:b] and r.adler == zlib.adler32(out) != zlib.adler32(data[a:b])
