"""CPU: the resumable gzip and raw instances of the kernel source -- Decoder<12, true, true> and Decoder<12, false, true, true>, what
resume_gzip_kernel and resume_raw_kernel run (pzg_decoder_create_format) -- compiled as a one-lane host program
(tests/model/model_resume_fmt.cpp) and held to the rule of include/pzg.h: however the input is cut into feeds and the rooms are
sized, the bytes, the terminal state and detail, the last adler and the sum of in_used are the batch path's over the whole input
(the existing host models of the batch gzip and raw instances), system zlib's and the oracle's; the count of published chunks
follows oracle.trace of the same body as a zlib stream.  The CRC pass behind the decode kernel (resume_crc_kernel) is modelled here:
oracle.crc32 of each call's delivery, appended to the running value, compared when the decoder ends."""
import ctypes as C
import os
import subprocess

import pytest

import resume_fmt_cases as K
from conftest import ROOT

GUARD = bytes(range(0x40, 0x80))


class R(C.Structure):
    _fields_ = [("status", C.c_int32), ("detail0", C.c_uint32), ("detail1", C.c_uint32), ("adler", C.c_uint32),
                ("out_len", C.c_uint64), ("in_used", C.c_uint64)]


@pytest.fixture(scope="session")
def fmt_model():
    d = os.path.join(ROOT, "tests", "model")
    so = os.path.join(d, "libpzgmodelresfmt.so")
    srcs = [os.path.join(d, "model_resume_fmt.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "inflate_core.h"),
            os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    M = C.CDLL(so)
    M.pzm_fmt_state_bytes.restype = C.c_uint32
    M.pzm_fmt_resume_feed.argtypes = [C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(R),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    M.pzm_crc32_append.restype = C.c_uint32
    M.pzm_crc32_append.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    return M


@pytest.fixture(scope="session")
def batch_models():
    """The batch path on the CPU: the host models of inflate_kernel<12, false, true> (gzip, with its verify pass) and
    inflate_raw_kernel<12, false>."""
    from test_model_vs_oracle import _build_model
    gz = _build_model([])
    rawso = os.path.join(ROOT, "tests", "model", "libpzgmodelraw.so")
    srcs = [os.path.join(ROOT, "tests", "model", "model_raw.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "inflate_core.h"),
            os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
    if not os.path.exists(rawso) or os.path.getmtime(rawso) < max(map(os.path.getmtime, srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", rawso, srcs[0]])
    MR = C.CDLL(rawso)
    MR.pzm_raw_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(R)]
    cap = 1 << 21

    def batch(c):
        s = c["stream"]
        if c["fmt"] == "gzip":
            r, out = gz(s, cap, 12, gzip=True)
        else:
            buf = C.create_string_buffer(cap)
            r = R()
            assert MR.pzm_raw_decompress(s, len(s), b"", 0, buf, cap, 12, C.byref(r)) == 0
            out = buf.raw[:r.out_len]
        assert r.out_len <= cap
        return r.status, r.detail0, r.detail1, r.adler, r.in_used, bytes(out)
    return batch


def drive(M, O, c):
    """One decoder through all its pieces; the CRC pass of a gzip decoder is modelled as the module text says."""
    d = K.Driver(c)
    state = C.create_string_buffer(M.pzm_fmt_state_bytes())
    gzip = c["fmt"] == "gzip"
    run_crc = 0
    while True:
        nxt = d.next_input()
        if nxt is None:
            break
        data, fin = nxt
        room = c["room"]
        out = C.create_string_buffer(b"\xa5" * room + GUARD, room + len(GUARD))
        r, ch, expect = R(), C.c_uint32(0), C.c_uint32(0)
        assert M.pzm_fmt_resume_feed(K.FLAG[c["fmt"]], state, data, len(data), fin, out, room, C.byref(r), C.byref(ch), C.byref(expect)) == 0
        assert out.raw[room:] == GUARD, (c["name"], "written past the room")
        delivered = out.raw[:r.out_len]
        status, detail, adler = r.status, (r.detail0, r.detail1), r.adler
        if gzip:
            run_crc = M.pzm_crc32_append(run_crc, O.crc32(delivered), len(delivered))
            adler = run_crc
            if status in (0, 19) and run_crc != expect.value:
                status, detail = 10, (expect.value, run_crc)
        d.take(status, detail, adler, r.out_len, r.in_used, ch.value, delivered)
    return d.o


def run_cases(M, O, batch, cases):
    seen = set()
    for c in cases:
        o = drive(M, O, c)
        K.check_rule(O, c, o, batch(c))
        K.check_independent(O, c, o)
        seen.add(o.status)
    return seen


def test_reference_fixtures_rewrapped(fmt_model, oracle, batch_models):
    """The nine fixtures as gzip and as raw, in pieces of 1, 7, 4,096 and 32,768 bytes of their bodies."""
    seen = run_cases(fmt_model, oracle, batch_models, K.fixture_cases(lambda n: (1, 7, 4096, 32768)))
    assert seen == {0}


def test_headers_trailers_members_and_errors(fmt_model, oracle, batch_models):
    cases = K.corner_cases()
    seen = run_cases(fmt_model, oracle, batch_models, cases)
    # truncation, block errors, checksum, gzip header, gzip length: all of them are reached
    assert {0, 1, 10, 18, 19} <= seen, seen
    assert any(c["room"] == 4096 for c in cases)


def test_suspension_points(fmt_model, oracle):
    """What a caller sees between the feeds: a header that is not all there suspends in front of its first byte (in_used 0 for the
    first member), a trailer likewise; behind a trailer fewer than two bytes and no final_in ask for input."""
    M = fmt_model
    import zlib
    data = b"suspension " * 300
    body = zlib.compress(data, 6)[2:-4]
    rh = K.rich_header()
    s = K.member(body, data, rh)

    def feed(state, piece, fin=0, room=1 << 16):
        out = C.create_string_buffer(room)
        r, ch, ex = R(), C.c_uint32(0), C.c_uint32(0)
        assert M.pzm_fmt_resume_feed(K.GZIP, state, piece, len(piece), fin, out, room, C.byref(r), C.byref(ch), C.byref(ex)) == 0
        return r, out.raw[:r.out_len]

    # (a call that does not end the stream delivers whole 16-byte groups: the last few bytes come with a later call)
    for n in range(0, len(rh)):
        state = C.create_string_buffer(M.pzm_fmt_state_bytes())
        r, _ = feed(state, s[:n])
        assert (r.status, r.in_used, r.out_len) == (K.NEED_INPUT, 0, 0), n
        r, out = feed(state, s)  # the header again, from its start
        # (the trailer is all there, but not the two bytes that say whether a member follows: it waits with the trailer unread)
        assert r.status == K.NEED_INPUT and len(s) - 9 <= r.in_used <= len(s) - 8 and len(out) == len(data) & ~15, n
        used = r.in_used
        r, more = feed(state, s[used:], 1)
        assert (r.status, used + r.in_used, out + more) == (0, len(s), data), n
    for n in range(0, 8):  # the trailer: nothing of it is consumed before all of it is there
        state = C.create_string_buffer(M.pzm_fmt_state_bytes())
        r, out = feed(state, s[:len(s) - 8 + n])
        assert r.status == K.NEED_INPUT and len(s) - 9 <= r.in_used <= len(s) - 8 and len(out) == len(data) & ~15, n
        used = r.in_used
        rest = s[used:] + b"\x1f"
        r, more = feed(state, rest)
        assert r.status == K.NEED_INPUT and more == b""  # one byte behind the trailer: a member may follow
        used += r.in_used
        r, more = feed(state, rest[r.in_used:] + b"x")
        assert r.status == 0 and used + r.in_used == len(s) and out + more == data  # 1f 78 is no member: left alone
    # a second member's header suspends in front of ITS first byte
    two = s + s
    state = C.create_string_buffer(M.pzm_fmt_state_bytes())
    r, out = feed(state, two[:len(s) + 5])
    assert (r.status, r.in_used) == (K.NEED_INPUT, len(s)) and out == data[:len(data) & ~15]
    r, more = feed(state, two[len(s):], 1)
    assert (r.status, r.in_used) == (0, len(s)) and out + more == data + data
