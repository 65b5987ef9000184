"""CPU: the three passes of pzg_index_scan (pure_zlib_amd/csrc/scan_core.h: block finder, marker pass, chain walk) as a host program
(tests/model/model_scan.cpp), checked against a plain-Python restatement of the finder's predicate and against system zlib
(tests/scancheck.py, tests/indexcheck.py)."""
import os
import subprocess
import zlib

import pytest

import indexcheck as X
import scancheck as S

CHUNKS = [256, 1024, 4096]
SPANS = [1, 4096]


@pytest.fixture(scope="session")
def scan_model():
    return S.ScanModel()


@pytest.fixture(scope="session")
def inputs():
    """indexcheck.model_inputs() behind four more streams of many small blocks: a chain has a link per block start found, and the
    conditions below want more than a thousand of them."""
    more = []
    for seed in (12, 13, 14, 15):
        data, d = X.tiny_blocks(seed, 800)
        assert zlib.decompressobj(-15).decompress(d) == data
        more.append(("tiny800_%d" % seed, d, data))
    return more + X.model_inputs()


@pytest.fixture(scope="session")
def ends(inputs):
    """name -> the stream's non-final block ends (the points of the segment model's span-1 build)."""
    seg = X.SegModel()
    got = {}
    for name, d, data in inputs:
        r, out, n, pts = seg.build(d, len(data), 1, 8192)
        assert r.status == 0 and out == data and n == len(pts), name
        got[name] = _with_empty_blocks(d, pts)
    return got


def _with_empty_blocks(d, pts):
    """The span-1 build records a block end only where output was produced since the last point: the end of an EMPTY block behind a
    point (a flush leaves an empty stored block, a partial flush an empty fixed one) is a block end of the stream all the same."""
    out = []
    for bit, pos in [(0, 0)] + list(pts):
        out.append((bit, pos))
        while True:
            head = S._bits(d, bit, 3)
            at = (bit + 3 + 7) & ~7
            if head == 0 and S._bits(d, at, 16) == 0 and S._bits(d, at + 16, 16) == 0xffff:
                bit = at + 32
            elif head == 2 and S._bits(d, bit + 3, 7) == 0:
                bit += 10
            else:
                break
            out.append((bit, pos))
    return out[1:]


@pytest.fixture(scope="session")
def scanned(scan_model, inputs):
    """(name, chunk, span) -> the model's scan; each must be a success with system zlib's sizes."""
    got = {}
    for name, d, data in inputs:
        for chunk in CHUNKS:
            for span in SPANS:
                res = scan_model.scan(d, chunk, span, 1024, mis=(chunk >> 8) & 3)
                assert (res["status"], res["out_len"], res["in_used"]) == (0, len(data), len(d)), (name, chunk, span, res["status"], res["d0"])
                assert res["npoints"] == len(res["points"]), (name, chunk, span)
                got[name, chunk, span] = res
    return got


def test_predicate_shortcut_is_the_predicate(inputs):
    """all_candidates() asks is_candidate() only where numpy's three rules hold: over whole small streams, asking everywhere gives the same."""
    for name, d, data in inputs[:6] + [inputs[-3]]:
        d = d[:1500]
        assert [p for p in range(8 * len(d)) if S.is_candidate(d, p)] == S.all_candidates(d), name


def test_finder(scanned, inputs):
    none = set()
    for name, d, data in inputs:
        for chunk in CHUNKS:
            want = S.expected_candidates(d, chunk)
            assert scanned[name, chunk, 1]["cand"] == want, (name, chunk)
            if want[1:] and all(c is None for c in want[1:]):
                none.add(name)
    assert {"fixed", "stored"} <= none  # streams of fixed or stored blocks alone have no candidates: one segment


def test_true_block_starts_are_candidates(inputs, ends):
    total = 0
    for name, d, data in inputs:
        for bit, _pos in ends[name]:
            if S._bits(d, bit, 3) == 4:  # a non-final dynamic block starts there
                assert S.is_candidate(d, bit), (name, bit)
                total += 1
    assert total > 300


def test_marker_pass_and_chain(scanned, inputs, ends):
    """Every segment on the true chain: the bytes it produced and the bit it reached are the reference's, and its successor's window,
    resolved, is system zlib's output -- decoding from there with it gives the rest of the stream."""
    links, phases, short = 0, set(), set()
    for name, d, data in inputs:
        true_ends = dict(ends[name])
        for chunk in CHUNKS:
            res = scanned[name, chunk, 1]
            ch = S.chain(res)
            for (k, bit, pos), (k2, bit2, pos2) in zip(ch, ch[1:]):
                assert res["endbit"][k] == bit2 and res["count"][k] == pos2 - pos, (name, chunk, k)
                assert true_ends[bit2] == pos2, (name, chunk, k)  # a block end of the stream, at the reference's output position
                if res["count"][k] < X.WINDOW:
                    short.add(name)
                phases.add(bit2 & 7)
                links += 1
            last = ch[-1]
            assert (res["endbit"][last[0]] + 7) >> 3 == len(d) and last[2] + res["count"][last[0]] == len(data), (name, chunk)
            S.check_windows(res, data, (name, chunk))
    assert links > 1000 and phases == set(range(8)) and short


def test_end_to_end(scanned, inputs, ends):
    seen = set()  # (a point whose window is the reference's -- check_windows -- is checked once, however many scans found it)
    for name, d, data in inputs:
        for chunk in CHUNKS:
            for span in SPANS:
                res = scanned[name, chunk, span]
                pts = res["points"]
                S.check_windows(res, data, (name, chunk, span))
                for k, (bit, pos) in enumerate(pts):
                    if (name, bit, pos) not in seen:
                        X.check_point(d, bit, pos, res["windows"][k][X.WINDOW - min(pos, X.WINDOW):].tobytes(), data, (name, chunk, span))
                        seen.add((name, bit, pos))
                    assert pos - (pts[k - 1][1] if k else 0) >= span, (name, chunk, span, k)
                assert set(pts) <= set(ends[name]), (name, chunk, span)


def test_over_capacity_reports_the_full_count(scan_model, scanned, inputs):
    for name, d, data in inputs[-7:]:
        full = scanned[name, 1024, 4096]
        res = scan_model.scan(d, 1024, 4096, 2)
        assert res["status"] == 0 and res["npoints"] == full["npoints"] and res["points"] == full["points"][:2], name


def test_false_candidate(scan_model):
    body, data, bit = S.false_candidate_stream(1024)
    assert S.is_candidate(body, bit) and S.first_candidate(body, bit, 2 * bit) == bit
    assert scan_model.find(body, bit, 2 * bit) == bit  # the finder does return it
    for span in SPANS:
        res = scan_model.scan(body, 1024, span)
        assert res["cand"][1] == bit
        assert (res["status"], res["out_len"], res["in_used"]) == (0, len(data), len(body))
        assert 1 not in [k for k, _b, _p in S.chain(res)]  # the chain skips it
        assert res["next"][1] & S.NEXT_FAIL
        assert len(res["points"]) >= 1 and all(b != bit for b, _p in res["points"])
        S.check_windows(res, data)
        for b, p in res["points"]:
            X.check_point(body, b, p, data[max(0, p - X.WINDOW):p], data)


def test_dead_ends(scan_model, inputs):
    """A chain that does not reach the final block is PZG_E_SCAN with the status its last segment met (the guards are checked in scan())."""
    for name, d, data in inputs[-7:-1]:
        cut = d[:len(d) * 2 // 3]
        want = X.SegModel().build(cut, len(data), 1 << 20)[0].status
        for chunk in CHUNKS:
            res = scan_model.scan(cut, chunk, 4096, 64)
            assert res["status"] == S.E_SCAN and res["d0"] == S.E_TRUNCATED == want, (name, chunk, res["status"], res["d0"])
            assert res["d1"] in [c & 0xffffffff for c in res["cand"] if c is not None]
    name, d, data = inputs[-7]
    assert name == "text6"
    clean = scan_model.scan(d, 1024, 4096, 64)
    ch = S.chain(clean)
    assert len(ch) >= 3
    k, bit, _pos = ch[2]
    bad, at = bytearray(d), bit + 1  # BTYPE of a block on the chain becomes 3
    bad[at >> 3] |= 1 << (at & 7)
    bad[(at + 1) >> 3] |= 1 << ((at + 1) & 7)
    res = scan_model.scan(bytes(bad), 1024, 4096, 64)
    # the segment in front of it runs into the block: PZG_E_FMT_BTYPE, and d1 is that segment's start
    assert (res["status"], res["d0"], res["d1"]) == (S.E_SCAN, 6, ch[1][1] & 0xffffffff) and ch[1][1] > 0, (res["status"], res["d0"], res["d1"])
    assert zlib.decompressobj(-15).decompress(d) == data  # (and the stream itself was sound)
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(bytes(bad))


def test_sanitized_program(inputs, tmp_path):
    """model_scan.cpp as a program of its own under AddressSanitizer and UBSan, over the big inputs and a truncated one."""
    from conftest import ROOT
    exe = str(tmp_path / "model_scan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DPZS_MAIN",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "model", "model_scan.cpp")])
    files = []
    for name, d, data in inputs[-7:]:
        for tag, blob in ((name, d), (name + "_cut", d[:len(d) // 2])):
            p = str(tmp_path / (tag + ".raw"))
            with open(p, "wb") as f:
                f.write(blob)
            files.append(p)
    out = subprocess.run([exe] + files, capture_output=True, text=True)  # (the runtimes are linked in: the environment stays as it is)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.count("rc 0 status 0") == 3 * 7 and out.stdout.count("rc 0 status 22") == 3 * 7, out.stdout
