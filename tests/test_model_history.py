"""CPU: the host model of inflate_core.h on the streams of tests/history_cases.py -- the history that install_dictionary() lays in
front of the output, at its edges: a first token that is a match at the oldest byte of the history and one byte in front of it,
for dictionaries of 1 to 40000 bytes, behind 0 to 600 literals (the head-token checks, a segment's SRC_OUT, a group's BAD);
matches across the join; a full window on the 32 KiB ring and the MIX threshold; a history the ring evicts; capacities, cuts,
wrong DICTIDs and neighbours without a dictionary.  Through pzm_decompress_dict (zlib with FDICT), pzm_raw_decompress on every
ring (the small rings answer through the 32 KiB-ring retry) and pzm_seg_decompress (all eight start bits, end_bit exact and 0).
Expected: the writer's own bytes and the planned status and detail words; for the failing streams the oracle's as well.  The path
counters of a -DPZG_STATS build say that the cases reach the paths they are named for."""
import ctypes as C
import os
import subprocess
import zlib

import pytest

import history_cases as H
import indexcheck as X
from conftest import ROOT
from test_model_raw import raw_model  # noqa: F401  (fixture)
from test_model_vs_oracle import GUARD, R, model, model_lib  # noqa: F401  (fixtures)

E_TRUNCATED, E_BAD_DISTANCE, E_OUT_TOO_SMALL, E_DICT = 1, 11, 14, 20
ROOM = 300  # capacity beyond the planned bytes: a stream that goes on where it must stop has room to show it


@pytest.fixture(scope="module")
def cases():
    return H.cases()


@pytest.fixture(scope="module")
def dict_model(model_lib):  # noqa: F811
    def run(z, zdict, cap):
        out = C.create_string_buffer(b"\xa5" * cap + GUARD, cap + len(GUARD))
        r = R()
        assert model_lib.pzm_decompress_dict(z, len(z), zdict, len(zdict), out, cap, C.byref(r)) == 0
        assert out.raw[cap:] == GUARD, ("written past the capacity", cap, r.status, r.out_len)
        return r, out.raw[: min(r.out_len, cap)]
    return run


def planned(c):
    """(status, detail0, detail1, out_len, adler) of a case and its bytes"""
    d = c["data"]
    if c["expect"] == ("ok",):
        return (0, 0, 0, len(d), zlib.adler32(d)), d
    _kind, dist, op = c["expect"]
    return (E_BAD_DISTANCE, dist, op, op, zlib.adler32(d)), d


def got_of(r):
    return (r.status, r.detail0 if r.status else 0, r.detail1 if r.status else 0, r.out_len, r.adler)


def test_the_list_is_what_it_claims():
    assert H.self_check() >= 300


def test_zlib_form_with_fdict(dict_model, oracle, cases):
    for c in cases:
        z = H.zlib_wrap(c)
        want, d = planned(c)
        cap = len(d) + ROOM
        r, out = dict_model(z, c["zdict"], cap)
        assert got_of(r) == want and out == d, (c["name"], got_of(r), want)
        if r.status == 0:
            assert r.in_used == len(z), c["name"]
        else:  # the oracle with the dictionary installed: the same status, detail words, length and bytes
            ro, oo = oracle.decompress_dict(z, c["zdict"], cap)
            assert (ro.status, ro.detail0, ro.detail1, ro.out_len, ro.adler) == want and oo == d, (c["name"], ro.status, ro.detail0, ro.detail1, ro.out_len)


@pytest.mark.parametrize("rb", [15, 14, 13, 12, 11])
def test_raw_form_every_ring(raw_model, cases, rb):  # noqa: F811
    for c in cases:
        want, d = planned(c)
        st, d0, d1, adler, out_len, in_used, out = raw_model(c["raw"], len(d) + ROOM, rb, c["zdict"])
        assert (st, d0 if st else 0, d1 if st else 0, out_len, adler) == want and out == d, (c["name"], rb, st, d0, d1, out_len)
        if st == 0:
            assert in_used == len(c["raw"]), (c["name"], rb)


def test_segment_form_every_start_bit(cases):
    m = X.SegModel()
    bits = set()
    for k, c in enumerate(cases):
        s = H.seg_wrap(c, k % 8)
        want, d = planned(c)
        bits.add((s["start_bit"], len(s["window"])))
        for end_bit in (s["end_bit"], 0):
            r, out = m.segment(s["inp"], s["start_bit"], end_bit, s["window"], len(d) + ROOM)
            assert got_of(r) == want and out == d, (c["name"], k % 8, end_bit, got_of(r), want)
            if r.status == 0:
                assert r.in_used == s["in_used"], (c["name"], k % 8, end_bit, r.in_used)
    assert {b for b, _n in bits} == set(range(8)) and {n for _b, n in bits} >= {1, 2, 64, 258, 32767, 32768}


def test_wrong_dictid_and_the_sums_of_dict_adler(dict_model, oracle, cases):
    """PZG_E_DICT with d0 = the stream's DICTID and d1 = the Adler-32 of the dictionary supplied, for every history length (the
    partial last step of dict_adler, 40000 bytes of 0xff): a DICTID one bit off, and a dictionary one byte off."""
    seen = set()
    for c in cases:
        zd = c["zdict"]
        if (len(zd), zd[:1]) in seen:
            continue
        seen.add((len(zd), zd[:1]))
        ours = zlib.adler32(zd)
        for bit in (0, 16, 31):
            z = H.zlib_wrap(c, dictid=ours ^ (1 << bit))
            r, out = dict_model(z, zd, len(c["data"]) + ROOM)
            assert (r.status, r.detail0, r.detail1, r.out_len, out) == (E_DICT, ours ^ (1 << bit), ours, 0, b""), (c["name"], bit, r.status, hex(r.detail0), hex(r.detail1))
            ro, _ = oracle.decompress_dict(z, zd)
            assert (ro.status, ro.detail0, ro.detail1) == (E_DICT, ours ^ (1 << bit), ours)
        other = zd[:-1] + bytes([zd[-1] ^ 0x80])
        r, _out = dict_model(H.zlib_wrap(c), other, len(c["data"]) + ROOM)
        assert (r.status, r.detail0, r.detail1) == (E_DICT, ours, zlib.adler32(other)), c["name"]
    assert {n for n, _b in seen} >= set(H.LENGTHS) and (40000, b"\xff") in seen


def test_capacity_and_truncation_with_a_history(dict_model, raw_model, oracle, cases):  # noqa: F811
    """adler[] is the Adler-32 of the delivered bytes alone, from 1: the dictionary is never part of it; 0 past the capacity."""
    m = X.SegModel()
    for name in H.CONTRACT:
        c = H.by_name(name)
        d, zd, z = c["data"], c["zdict"], H.zlib_wrap(c)
        s = H.seg_wrap(c, 5)
        for cap in (len(d) // 2, 0):
            r, out = dict_model(z, zd, cap)
            assert (r.status, r.out_len, r.adler) == (E_OUT_TOO_SMALL, len(d), 0), (name, cap, r.status, r.out_len)
            for rb in (15, 11):
                st, _d0, _d1, adler, out_len, _u, _o = raw_model(c["raw"], cap, rb, zd)
                assert (st, out_len, adler) == (E_OUT_TOO_SMALL, len(d), 0), (name, cap, rb)
            r, _o = m.segment(s["inp"], 5, s["end_bit"], s["window"], cap)
            assert (r.status, r.out_len, r.adler) == (E_OUT_TOO_SMALL, len(d), 0), (name, cap, "segment")
        r, out = dict_model(z, zd, len(d))
        assert (r.status, r.out_len, r.adler, r.in_used) == (0, len(d), zlib.adler32(d), len(z)) and out == d, (name, "exact")
        r, out = m.segment(s["inp"], 5, s["end_bit"], s["window"], len(d))
        assert (r.status, r.out_len, r.adler) == (0, len(d), zlib.adler32(d)) and out == d, (name, "exact", "segment")
        cut, prefix = H.truncated(c)
        want = (E_TRUNCATED, len(prefix), zlib.adler32(prefix))
        zc = H.FDICT_HDR + zlib.adler32(zd).to_bytes(4, "big") + cut
        r, out = dict_model(zc, zd, len(d))
        assert (r.status, r.out_len, r.adler) == want and out == prefix, (name, "cut", r.status, r.out_len, len(prefix))
        ro, oo = oracle.decompress_dict(zc, zd, len(d))
        assert (ro.status, ro.out_len, ro.adler) == want and oo == prefix, (name, "cut", "oracle")
        for rb in (15, 11):
            st, _d0, _d1, adler, out_len, _u, out = raw_model(cut, len(d), rb, zd)
            assert (st, out_len, adler) == want and out == prefix, (name, "cut", rb)
        scut, sprefix = H.truncated_segment(c, s)
        for end_bit in (0, s["end_bit"]):
            r, out = m.segment(scut, 5, end_bit, s["window"], len(d))
            assert (r.status, r.out_len, r.adler) == (E_TRUNCATED, len(sprefix), zlib.adler32(sprefix)) and out == sprefix, (name, "cut", "segment", r.status, r.out_len, len(sprefix))


def test_neighbours_without_a_dictionary(dict_model, oracle, cases):
    """An FDICT stream with dict_len = 0 takes the reference's path (DICTID skipped, empty history); a stream without FDICT that
    is handed a dictionary ignores it: both give what the body gives with an empty history -- for most of these cases
    PZG_E_BAD_DISTANCE with d1 = op -- and what the oracle gives."""
    nbad = 0
    for c in cases:
        nd = c["nodict"]
        d = nd[-1]
        want = (0, 0, 0, len(d), zlib.adler32(d)) if nd[0] == "ok" else (E_BAD_DISTANCE, nd[1], nd[2], len(d), zlib.adler32(d))
        nbad += nd[0] != "ok"
        cap = len(d) + ROOM
        zf = H.FDICT_HDR + zlib.adler32(c["zdict"]).to_bytes(4, "big") + c["raw"] + zlib.adler32(d).to_bytes(4, "big")
        for z, zd in ((zf, b""), (H.plain_wrap(c), c["zdict"])):
            r, out = dict_model(z, zd, cap)
            assert got_of(r) == want and out == d, (c["name"], len(zd), got_of(r), want)
            ro, oo = oracle.decompress_dict(z, zd, cap) if zd else oracle.decompress(z, cap)
            assert (ro.status, ro.detail0 if ro.status else 0, ro.detail1 if ro.status else 0, ro.out_len, ro.adler) == want and oo == d, (c["name"], len(zd))
    assert nbad > 150


@pytest.fixture(scope="module")
def raw_stats():
    """the raw instance of the host model (strips, groups AND a history) built with -DPZG_STATS: the counters of one decode"""
    d = os.path.join(ROOT, "tests", "model")
    so, glue = os.path.join(d, "libpzgmodelraw_stats.so"), os.path.join(ROOT, "build", "model_raw_stats_glue.cpp")
    os.makedirs(os.path.dirname(glue), exist_ok=True)
    with open(glue, "w") as f:
        f.write('#include "%s"\nPzgStats pzg_stats;\nextern "C" unsigned long long *pzm_stats(void) { return pzg_stats.v; }\n' % os.path.join(d, "model_raw.cpp"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-DPZG_STATS", "-o", so, glue])
    M = C.CDLL(so)
    M.pzm_stats.restype = C.POINTER(C.c_ulonglong)
    M.pzm_raw_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(R)]

    def run(c):
        v = M.pzm_stats()
        before = [v[i] for i in range(40)]
        cap = len(c["data"]) + ROOM
        out, r = C.create_string_buffer(cap), R()
        assert M.pzm_raw_decompress(c["raw"], len(c["raw"]), c["zdict"], len(c["zdict"]), out, cap, 15, C.byref(r)) == 0
        assert r.status == (0 if c["expect"] == ("ok",) else E_BAD_DISTANCE) and out.raw[:r.out_len] == c["data"], c["name"]
        return [v[i] - before[i] for i in range(40)]
    return run


HEAD, SOLO, SEG_TOKENS, GROUPS, CUT, SEG_SRC_OUT, GRP_BAD, GRP_MIX = 11, 35, 9, 20, 18, 32, 33, 34  # PZG_STAT slots of inflate_core.h


def test_the_cases_reach_the_paths_they_name(raw_stats, cases):
    """Not vacuous, by the model's counters: every case that names a path is held to it, one by one.  No valid stream ends a
    segment by SRC_OUT or a group by BAD (a comparison that is one off does, at the oldest byte of the history).  A failing head
    token is found by a head-token check; a failing token behind 1 to 17 literals ends the segment that holds those literals by
    SRC_OUT.  Behind 600 bytes of body the span of strips is whole (no lane cut it short) and its groups hold the 600 literals:
    the failing match ends a group by BAD, inside it and again at the head of the next, and seq_solo reports it; the valid one is
    copied by its group -- or, with a history of SOLO_LENGTHS, is MIX and goes through seq_solo, where its distance EQUALS op +
    hist_extra.  The three streams around the MIX threshold differ in one distance's extra bits: the one below the threshold ends
    one or two groups more by MIX than the other two, which end as many as each other."""
    mix = {}
    reached = {"head": 0, "segment": 0, "group": 0, "solo": 0, "join": 0}
    for c in cases:
        st = raw_stats(c)
        ok = c["expect"] == ("ok",)
        if ok:
            assert st[SEG_SRC_OUT] == 0 and st[GRP_BAD] == 0, (c["name"], st)
        if c["path"] == "mix":
            assert st[GROUPS] > 0, (c["name"], st)
            mix[c["name"]] = st[GRP_MIX]
        elif c["path"] in ("group", "solo"):
            assert st[GROUPS] > 0 and st[CUT] == 0 and st[SEG_TOKENS] < 600, (c["name"], st)
            if not ok:
                assert st[GRP_BAD] == 2 and st[SOLO] == 1 and st[SEG_SRC_OUT] == 0 and st[HEAD] == 0, (c["name"], st)
            elif c["path"] == "solo":
                assert st[GRP_MIX] == 2 and st[SOLO] == 1, (c["name"], st)
            else:
                assert st[GRP_MIX] == 0 and st[SOLO] == 0, (c["name"], st)
            reached[c["path"]] += 1
        elif c["path"] == "segment" and not ok:  # (every segment that holds some of the k literals meets it inside, the next one at its head)
            assert st[SEG_SRC_OUT] >= 2 and st[SEG_TOKENS] == c["expect"][2] and st[HEAD] >= 1 and st[GROUPS] == 0, (c["name"], st)
            reached["segment"] += 1
        elif c["path"] == "head" and not ok:
            assert st[SEG_SRC_OUT] == 1 and st[SEG_TOKENS] == 0 and st[HEAD] == 1 and st[GROUPS] == 0, (c["name"], st)
            reached["head"] += 1
        elif c["name"].startswith("join_") and c["tokens"][0][0] > c["tokens"][0][1]:  # (a source that runs into its own output)
            assert st[HEAD] >= 1, (c["name"], st)
            reached["join"] += 1
    assert min(reached.values()) >= 4, reached
    assert len(mix) == 2 * 3 * len(H.MIX_MS)
    for name, n in mix.items():  # (a match that is MIX inside a group is MIX again at the head of the next: one or two more)
        if name.endswith("_at"):
            stem = name[:-3]
            assert n >= 1 and mix[stem + "_above"] == n and mix[stem + "_below"] > n, (stem, mix[stem + "_below"], n, mix[stem + "_above"])
