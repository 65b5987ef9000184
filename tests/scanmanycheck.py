"""Shared by tests/test_model_scan_many.py (CPU) and tests/test_gpu_scan_many.py (GPU): pzg_index_scan_many restated as "every stream
of the batch gives what the one-stream scan gives for it alone".

  * extra_cases(): the streams the batch holds besides the ordinary inputs (empty, short, exactly three chunks, a false candidate,
    a truncated stream between two sound ones, a stream with two slots for more points);
  * Batch: the streams packed back to back at byte offsets that give every misalignment 0..3, the slots of each;
  * ScanManyModel: tests/model/model_scan_many.cpp, the three many-stream passes of pure_zlib_amd/csrc/scan_core.h between guards;
  * reference(): scancheck.ScanModel().scan of each stream alone -- the one-stream model, which tests/test_model_scan.py checks
    against a plain-Python finder and system zlib;
  * check_stream(): one stream's result, points, windows and slots against its reference.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

import scancheck as S

W = S.WINDOW
FILL = 0xCD
FILL64 = 0xCDCDCDCDCDCDCDCD


def exactly(nbytes, seed):
    """(raw stream, data) of exactly nbytes: a sync-flushed deflate of a text, then a final stored block that fills up the rest."""
    import corpus
    text = corpus.zipf_text(nbytes, seed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = co.compress(text) + co.flush(zlib.Z_SYNC_FLUSH)
    pay = corpus.zipf_text(nbytes - len(head) - 5, seed + 1)
    body = head + b"\x01" + len(pay).to_bytes(2, "little") + (len(pay) ^ 0xffff).to_bytes(2, "little") + pay
    assert len(body) == nbytes and zlib.decompressobj(-15).decompress(body) == text + pay
    return body, text + pay


def extra_cases(sound, chunks):
    """[(name, raw stream, room or None)] to put behind the ordinary inputs.  sound: [(name, stream, data)] with text6 and text1 among
    them.  room None: as many slots as the stream has points, and one more; a number: that many."""
    import indexcheck as X
    by = {name: d for name, d, _data in sound}
    short = X.raw_of(b"a stream shorter than one chunk. " * 3)
    assert len(short) < min(chunks)
    cases = [("empty", b"", None), ("short", short, None)]
    for c in chunks:
        cases.append(("three_chunks_%d" % c, exactly(3 * c, 31)[0], None))
    cases.append(("false_candidate", S.false_candidate_stream(1024)[0], None))
    cases.append(("before_cut", by["text1"], None))
    cases.append(("cut", by["text6"][:len(by["text6"]) * 2 // 3], None))  # PZG_E_SCAN between two sound streams
    cases.append(("after_cut", by["text6"], None))
    cases.append(("two_slots", by["text1"], 2))  # it has more points than that
    cases.append(("last", short, None))
    return cases


class Batch:
    """The streams [(name, raw stream, room or None)] packed into one buffer: stream i starts i & 3 bytes past a dword boundary (a
    few filler bytes between the streams), so every misalignment occurs."""

    def __init__(self, cases):
        self.names = [c[0] for c in cases]
        self.streams = [c[1] for c in cases]
        self.rooms = [c[2] for c in cases]
        buf, off = bytearray(), []
        for i, d in enumerate(self.streams):
            while len(buf) % 4 != i % 4:
                buf.append(0xEE)
            off.append(len(buf))
            buf += d
        self.n = len(cases)
        self.packed = bytes(buf) + b"\xEE" * 5
        self.in_off = np.array(off, dtype=np.uint64)
        self.in_len = np.array([len(d) for d in self.streams], dtype=np.uint64)

    def mis(self, i):
        return int(self.in_off[i]) & 3

    def point_off(self, refs):
        """uint32 [n + 1]: the slots of every stream from its reference's count (room None: the count plus one)."""
        rooms = [r if r is not None else ref["npoints"] + 1 for r, ref in zip(self.rooms, refs)]
        return np.concatenate(([0], np.cumsum(rooms))).astype(np.uint32)

    def first_chunk(self, chunk):
        return np.concatenate(([0], np.cumsum([max(1, -(-len(d) // chunk)) for d in self.streams]))).astype(np.uint32)

    def write(self, path, point_off):
        """The file model_scan_many.cpp's own main() reads."""
        with open(path, "wb") as f:
            f.write(np.array([self.n, len(self.packed)], dtype="<u8").tobytes() + self.in_off.astype("<u8").tobytes() +
                    self.in_len.astype("<u8").tobytes() + point_off.astype("<u8").tobytes() + self.packed)


_REF = {}


def reference(model, batch, chunk, span):
    """[ScanModel().scan of stream i alone] with the room the batch gives it (None: 1024, more than any stream here has)."""
    refs = []
    for i, d in enumerate(batch.streams):
        key = (zlib.crc32(d), len(d), chunk, span, batch.rooms[i], batch.mis(i))
        if key not in _REF:
            _REF[key] = model.scan(d, chunk, span, batch.rooms[i] if batch.rooms[i] is not None else 1024, mis=batch.mis(i))
        refs.append(_REF[key])
    return refs


class Result(C.Structure):
    _fields_ = S.Result._fields_


class ScanManyModel:
    """The host build of the many-stream passes (tests/model/model_scan_many.cpp)."""

    def __init__(self):
        from conftest import ROOT
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "libpzgmodelscanmany.so")
        self.src = os.path.join(d, "model_scan_many.cpp")
        srcs = [self.src, os.path.join(ROOT, "pure_zlib_amd", "csrc", "scan_core.h"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, self.src])
        self.M = C.CDLL(so)
        vp = C.c_void_p
        self.M.pzsm_scan_many.argtypes = [C.c_char_p, C.c_uint64, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
        self.M.pzsm_locate.argtypes = [vp, C.c_uint32, C.c_uint32]
        self.M.pzsm_locate.restype = C.c_uint32

    def locate(self, first_chunk, g):
        fc = np.ascontiguousarray(first_chunk, dtype=np.uint32)
        return int(self.M.pzsm_locate(fc.ctypes.data, len(fc) - 1, g))

    def scan_many(self, batch, chunk, span, point_off):
        """-> dict(results [n], points uint64 [slots, 2], windows uint8 [slots, W], cand, next, count, endbit over all chunks)."""
        slots, total = int(point_off[-1]), int(batch.first_chunk(chunk)[-1])
        pts = np.full((slots, 2), FILL64, dtype=np.uint64)
        win = np.full((slots, W), FILL, dtype=np.uint8)
        res = (Result * batch.n)()
        cand, nxt = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint32)
        count, endbit = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64)
        rc = self.M.pzsm_scan_many(batch.packed, len(batch.packed), batch.in_off.ctypes.data, batch.in_len.ctypes.data, batch.n, chunk, span,
                                   pts.ctypes.data, point_off.ctypes.data, win.ctypes.data, res, cand.ctypes.data, nxt.ctypes.data,
                                   count.ctypes.data, endbit.ctypes.data)
        assert rc == 0, ("written outside a buffer (or into an input): %d" % (rc - 1), chunk, span)
        results = [dict(status=r.status, d0=r.d0, d1=r.d1, npoints=r.npoints, out_len=r.out_len, in_used=r.in_used) for r in res]
        return dict(results=results, points=pts, windows=win, cand=cand, next=nxt, count=count, endbit=endbit)


RESULT_FIELDS = ("status", "d0", "d1", "npoints", "out_len", "in_used")


def check_stream(what, ref, result, pts, win, stored=True):
    """One stream: its result block is the reference's; the points stored are the reference's first ones and their windows lie at
    the END of their slots with the front left alone; every slot behind them keeps its fill.  pts / win: the stream's OWN slots.
    stored False: nothing was to be stored at all (a failed stream of the host-pointer form)."""
    assert {f: result[f] for f in RESULT_FIELDS} == {f: ref[f] for f in RESULT_FIELDS}, what
    k = min(ref["npoints"], len(pts)) if stored else 0
    assert k == len(ref["points"]) or not stored, what
    assert [tuple(int(x) for x in p) for p in pts[:k]] == ref["points"][:k], what
    assert (pts[k:] == FILL64).all() and (win[k:] == FILL).all(), (what, "a slot behind the points stored")
    for j in range(k):
        w = min(ref["points"][j][1], W)
        assert win[j, W - w:].tobytes() == ref["windows"][j][W - w:].tobytes(), (what, j)
        assert (win[j, :W - w] == FILL).all(), (what, j, "front of the slot")
