"""Shared by tests/test_model_members.py (CPU) and tests/test_gpu_members.py (GPU): the members of a gzip file
(pzg_gzip_find_members, pzg_gzip_layout; pure_zlib_amd/csrc/member_core.h) restated.

  * is_candidate(d, p) / block_size(d, p) / find(d): the finder's predicate and the BGZF subfield in plain Python, written from
    their specification (include/pzg.h), nothing of the code under test (bytes.find only narrows down where the predicate is asked);
  * layout(d, starts, base): the layout in numpy;
  * builders of the files the two suites share: sound_files() and finder_files();
  * MembersModel: tests/model/model_members.cpp, member_core.h as a host program between guards.
"""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

import corpus

GUARD64, GUARD32 = 0xCDCDCDCDCDCDCDCD, 0xCDCDCDCD
CHUNKS = (64, 256, 4096)


# ---- the specification ---------------------------------------------------------------------------------------------------------------

def is_candidate(d, p):
    if p + 10 > len(d):
        return False
    if d[p] != 0x1f or d[p + 1] != 0x8b or d[p + 2] != 0x08:
        return False
    if d[p + 3] & 0xe0:
        return False
    if d[p + 8] not in (0, 2, 4):
        return False
    return d[p + 9] <= 13 or d[p + 9] == 255


def block_size(d, p):
    """0, or the value + 1 of the first subfield 'B' 'C' of two bytes that lies wholly inside XLEN and inside the input."""
    if not d[p + 3] & 4 or p + 12 > len(d):
        return 0
    xlen = d[p + 10] | (d[p + 11] << 8)
    q, end = p + 12, min(p + 12 + xlen, len(d))
    while q + 4 <= end:
        slen = d[q + 2] | (d[q + 3] << 8)
        if d[q] == 66 and d[q + 1] == 67 and slen == 2:
            return (d[q + 4] | (d[q + 5] << 8)) + 1 if q + 6 <= end else 0
        q += 4 + slen
    return 0


def find(d):
    """(starts, bsize): position 0, then every candidate behind it, ascending."""
    starts, bsize = [0], [block_size(d, 0) if is_candidate(d, 0) else 0]
    p = d.find(b"\x1f\x8b\x08", 1)
    while p >= 0:
        if is_candidate(d, p):
            starts.append(p)
            bsize.append(block_size(d, p))
        p = d.find(b"\x1f\x8b\x08", p + 1)
    return starts, bsize


def layout(d, starts, base=0):
    """(in_off, in_len, out_off, out_cap, total) of the members that start at `starts`."""
    in_off = np.array(starts, dtype=np.uint64)
    ends = np.array(list(starts[1:]) + [len(d)], dtype=np.uint64)
    in_len = ends - in_off
    isize = np.array([int.from_bytes(d[e - 4:e], "little") if e - s >= 18 else 0 for s, e in zip(in_off.tolist(), ends.tolist())], dtype=np.uint64)
    out_cap = np.minimum(isize, np.uint64(1032) * in_len)
    out_off = np.uint64(base) + np.concatenate(([0], np.cumsum(out_cap)[:-1])).astype(np.uint64)
    return in_off, in_len, out_off, out_cap, int(out_cap.sum())


def prune(starts, bsize):
    """The list without the candidates strictly inside a member that states its size."""
    keep, until = [], 0
    for s, b in zip(starts, bsize):
        if s >= until:
            keep.append(s)
            until = s + b if b else 0
    return keep


# ---- the files -------------------------------------------------------------------------------------------------------------------------

def member(data, extra=None, level=6, xfl=0, os_=3):
    """One member around a raw deflate body, FEXTRA when `extra` is given."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return wrap(co.compress(data) + co.flush(), data, extra, xfl, os_)


def wrap(body, data, extra=None, xfl=0, os_=3):
    hdr = b"\x1f\x8b\x08" + bytes([4 if extra is not None else 0]) + bytes(4) + bytes([xfl, os_])
    if extra is not None:
        hdr += struct.pack("<H", len(extra)) + extra
    return hdr + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def bgzf_member(data, before=b""):
    """A BGZF block: the 'BC' subfield holds the member's total size minus one (`before`: another subfield in front of it)."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    total = 12 + len(before) + 6 + len(body) + 8
    return wrap(body, data, before + b"BC" + struct.pack("<HH", 2, total - 1), os_=255)


def stored(payload, final=True):
    """A raw deflate stream of stored blocks."""
    out, cuts = b"", [payload[i:i + 65535] for i in range(0, len(payload), 65535)] or [b""]
    for k, c in enumerate(cuts):
        out += bytes([1 if final and k == len(cuts) - 1 else 0]) + struct.pack("<HH", len(c), len(c) ^ 0xffff) + c
    return out


def gz(data, level=9):
    """gzip.compress without the clock in the header."""
    return gzip.compress(data, level, mtime=0)


BARE_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"

_FILES = {}


def sound_files():
    """[(name, file, data, false candidates)]: sound gzip files, and how many of their candidates are no member starts."""
    if "sound" in _FILES:
        return _FILES["sound"]
    text = lambda n, seed: corpus.zipf_text(n, seed)
    files = []
    d1 = text(3000, 1)
    files.append(("one", gz(d1), d1))
    files.append(("two", gz(d1) + corpus.gzip_member(text(5000, 2), 2), d1 + text(5000, 2)))
    sizes = [0, 1, 5000, 17, 4096, 300] + [(131 * k) % 5001 for k in range(31)]
    parts = [corpus.mixed_data(n, 40 + k) if k % 3 else text(n, 40 + k) for k, n in enumerate(sizes)]
    files.append(("thirty-seven", b"".join(gz(p, 1 + k % 9) if k % 2 else corpus.gzip_member(p, 100 + k) for k, p in enumerate(parts)),
                  b"".join(parts)))
    blocks = [text(65280, 7), text(65280, 8), text(12345, 9)]
    files.append(("bgzf", b"".join(bgzf_member(b) for b in blocks), b"".join(blocks)))
    files.append(("bc-behind-another", bgzf_member(d1, before=b"AB\x03\x00xyz") + bgzf_member(text(700, 3), before=b"ZZ\x00\x00"), d1 + text(700, 3)))
    files.append(("empty-members", gz(b"") * 9, b""))
    # false candidates: the payload of a stored block holds the bytes of a bare header / a complete valid member
    pay = text(500, 11) + BARE_HEADER + text(800, 12)
    files.append(("bare-header-inside", member(text(900, 13)) + wrap(stored(pay), pay) + member(text(1100, 14)), text(900, 13) + pay + text(1100, 14)))
    inner = gz(text(2000, 15))
    pay = text(512, 16) + inner + text(100, 17)
    files.append(("member-inside", member(text(900, 18)) + wrap(stored(pay), pay) + member(text(1100, 19)) + gz(text(10, 20)),
                  text(900, 18) + pay + text(1100, 19) + text(10, 20)))
    out = []
    for name, z, d in files:
        assert gzip.decompress(z) == d, name
        out.append((name, z, d, len(find(z)[0]) - count_members(z)))
    _FILES["sound"] = out
    return out


def count_members(z):
    """The members of a sound file, counted by system zlib."""
    n = 0
    while z:
        do = zlib.decompressobj(31)
        do.decompress(z)
        assert do.eof
        z = do.unused_data
        n += 1
    return n


def finder_files():
    """[(name, bytes)]: inputs for the finder alone -- headers at the edges of chunks and of the input, an FEXTRA that runs past it."""
    if "finder" in _FILES:
        return _FILES["finder"]
    fill = corpus.zipf_text(12 * 4096 + 777, 21)  # (text: no byte 1f in it)
    edges = bytearray(fill)
    for k in range(1, 11):  # a header that starts at each of the last 10 bytes of a chunk, for every chunk size of the tests
        edges[4096 * k - k:4096 * k - k + 10] = BARE_HEADER
    edges[len(edges) - 10:] = BARE_HEADER  # at in_len - 10: the last candidate there can be
    nine = bytearray(fill[:5000])
    nine[len(nine) - 9:] = BARE_HEADER[:9]  # at in_len - 9: no candidate
    one = bytearray(fill[:4097])
    one[-1] = 0x1f
    past = bytearray(fill[:3000])
    past[-17:] = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 100) + b"BC\x02\x00\x10"  # XLEN 100, 5 bytes of it there
    past2 = bytearray(fill[:3000])
    past2[-18:] = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 5) + b"BC\x02\x00\x10\x20"  # 'BC' runs past XLEN
    files = [("edges", bytes(edges)), ("nine", bytes(nine)), ("one", bytes(one)), ("xlen-past-input", bytes(past)), ("bc-past-xlen", bytes(past2)),
             ("empty", b""), ("short", b"\x1f\x8b\x08"), ("no-magic", fill[:1000])]
    _FILES["finder"] = files
    return files


# ---- the host model ------------------------------------------------------------------------------------------------------------------

class MembersModel:
    """The host build of member_core.h (tests/model/model_members.cpp)."""

    def __init__(self):
        from conftest import ROOT
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelmembers.so")
        srcs = [os.path.join(d, "model_members.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "member_core.h"),
                os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        self.M = C.CDLL(so)
        vp = C.c_void_p
        self.M.pzm_find.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(C.c_uint64)]
        self.M.pzm_layout.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_uint64)]

    def find(self, d, chunk, max_members=None, mis=0):
        """(count, starts, bsize) with one guard slot behind the room, which must come back untouched."""
        room = len(find(d)[0]) if max_members is None else max_members
        starts, bsize = np.full(room + 1, GUARD64, dtype=np.uint64), np.full(room + 1, GUARD32, dtype=np.uint32)
        n = C.c_uint64(0)
        rc = self.M.pzm_find(d, len(d), mis, chunk, starts.ctypes.data, bsize.ctypes.data, room, C.byref(n))
        assert rc == 0, ("written outside a buffer: guard %d" % (rc - 1), chunk)
        stored = min(n.value, room)
        assert (starts[stored:] == GUARD64).all() and (bsize[stored:] == GUARD32).all(), "an entry stored past the count or the room"
        return n.value, starts[:stored].tolist(), bsize[:stored].tolist()

    def layout(self, d, starts, base=0, mis=0):
        st = np.array(starts, dtype=np.uint64)
        arrays = [np.zeros(len(st), dtype=np.uint64) for _ in range(4)]
        total = C.c_uint64(0)
        rc = self.M.pzm_layout(d, len(d), mis, st.ctypes.data, len(st), base, *[a.ctypes.data for a in arrays], C.byref(total))
        assert rc == 0, "written outside a buffer: guard %d" % (rc - 1)
        return (*arrays, total.value)
