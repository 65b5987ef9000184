"""CPU: the RAW instance of the kernel source -- Decoder<RB, false, false, true>, bare RFC 1951 streams (PZG_RAW) -- compiled as a
host program (tests/model/model_raw.cpp) and checked against system zlib and the oracle on the wrapped stream (tests/rawcheck.py),
for every ring; and the budgets of the ring-11 raw kernel in the gfx950 code object of libpzg.so."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile
import zlib

import pytest

import corpus
import rawcheck
from conftest import ROOT, read_case

RINGS = [15, 14, 13, 12, 11]
GUARD = bytes(range(0x40, 0x80))  # 64 bytes that must stay as they are past a stream's capacity


class R(C.Structure):
    _fields_ = [("status", C.c_int32), ("detail0", C.c_uint32), ("detail1", C.c_uint32), ("adler", C.c_uint32),
                ("out_len", C.c_uint64), ("in_used", C.c_uint64)]


@pytest.fixture(scope="session")
def raw_model():
    d = os.path.join(ROOT, "tests", "model")
    so = os.path.join(d, "libpzgmodelraw.so")
    srcs = [os.path.join(d, "model_raw.cpp"), os.path.join(ROOT, "pure_zlib_amd", "csrc", "inflate_core.h"),
            os.path.join(ROOT, "pure_zlib_amd", "csrc", "wave.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    M = C.CDLL(so)
    M.pzm_raw_decompress.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(R)]

    def run(d, cap, rb, zdict=b""):
        out = C.create_string_buffer(b"\xa5" * cap + GUARD, cap + len(GUARD))
        r = R()
        assert M.pzm_raw_decompress(d, len(d), zdict, len(zdict), out, cap, rb, C.byref(r)) == 0
        assert out.raw[cap:] == GUARD, ("written past the capacity", cap, r.status, r.out_len)
        return r.status, r.detail0, r.detail1, r.adler, r.out_len, r.in_used, out.raw[: min(r.out_len, cap)]
    return run


@pytest.fixture(scope="session")
def zlib_detail1():
    """detail[1] of the zlib instance (the existing host model) on a wrapped stream: a PZG_E_HUFF_BUILD block's bit offset."""
    from test_model_vs_oracle import _build_model
    m = _build_model([])
    return lambda wrapped: m(wrapped, 1 << 16, 15)[0].detail1


@pytest.fixture(scope="session")
def pool():
    return rawcheck.stream_pool()


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_stream_pool(raw_model, oracle, zlib_detail1, pool, rb):
    """Reference fixtures and pinned vectors with the wrapper stripped (the block-level error vectors too), writer-made and
    zlib-made streams, corrupted ones: generous capacity."""
    statuses = set()
    for name, d in pool:
        got = raw_model(d, 1 << 21, rb)
        rawcheck.check(oracle, d, 1 << 21, got, zlib_detail1, (name, rb))
        statuses.add(got[0])
    assert {0, 1, 5, 6, 7, 11} <= statuses, statuses  # the pool does reach the block-level errors


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_reference_fixtures_exact(raw_model, rb):
    for name in ("randtest1", "rfctest2", "zerotest3"):
        z, gold = read_case(name)
        st, _d0, _d1, adler, out_len, in_used, out = raw_model(z[2:-4], len(gold), rb)
        assert (st, out_len, in_used, adler) == (0, len(gold), len(z) - 6, zlib.adler32(gold)) and out == gold, name


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_capacities(raw_model, oracle, pool, rb):
    """Capacities 0, 1, len - 1, len: PZG_E_OUT_TOO_SMALL with the size needed, nothing written past the capacity (the guard
    bytes), failed streams deliver what fits."""
    n = 0
    for name, d in pool[::3]:
        z = rawcheck.zlib_raw(d)
        full = len(z[0]) if z else raw_model(d, 1 << 21, 15)[4]
        for cap in sorted({0, 1, max(full - 1, 0), full}):
            rawcheck.check(oracle, d, cap, raw_model(d, cap, rb), None, (name, rb, cap))
            n += 1
    assert n > 40


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_truncated_at_every_byte(raw_model, oracle, rb):
    """Three streams cut at every byte (0 bytes too): PZG_E_TRUNCATED -- or the error the cut leaves in view -- and what had been
    decoded by then."""
    d0 = zlib.compress(corpus.zipf_text(1500, 3), 6)[2:-4]                       # one dynamic block
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    d1 = co.compress(corpus.mixed_data(700, 5)) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(b"tail" * 40) + co.flush()  # fixed, stored marker, fixed
    d2 = zlib.compress(corpus.random_bytes(600, 1), 0)[2:-4]                     # stored
    for k, d in enumerate((d0, d1, d2)):
        assert rawcheck.zlib_raw(d) is not None
        for cut in range(len(d)):
            got = raw_model(d[:cut], 4096, rb)
            assert got[0] != 0, (k, cut)
            if cut == 0:
                assert got[0] == 1 and got[4] == 0
            rawcheck.check(oracle, d[:cut], 4096, got, None, (k, cut, rb))


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_trailing_garbage(raw_model, oracle, rb):
    """in_used stops at the byte that holds the last bit of the final block; what follows is left alone."""
    rng = random.Random(9)
    for seed in range(12):
        data = corpus.mixed_data(1 + seed * 531, seed)
        d = corpus.compress_variant(data, seed)[2:-4]
        for tail in (b"\0", b"\xff" * 3, bytes(rng.getrandbits(8) for _ in range(40)), d):
            got = raw_model(d + tail, len(data), rb)
            assert (got[0], got[4], got[5], got[6]) == (0, len(data), len(d), data), (seed, len(tail))
            rawcheck.check(oracle, d + tail, len(data), got, None, (seed, len(tail), rb))


@pytest.mark.parametrize("rb", RINGS)
def test_raw_model_dictionaries(raw_model, oracle, rb):
    """A dictionary is the history in front of the output, unconditionally (zlib's raw inflateSetDictionary); the small rings
    hand such a stream to the 32 KiB-ring instance."""
    for seed in range(10):
        zdict = corpus.zipf_text([40, 700, 5000, 32768, 50000][seed % 5], 100 + seed)
        data = zdict[-300:] * 2 + corpus.zipf_text(3000 + 977 * seed, 100 + seed) + zdict[:200]
        co = zlib.compressobj(1 + seed % 9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict)
        d = co.compress(data) + co.flush()
        assert rawcheck.zlib_raw(d, zdict) == (data, len(d))
        for cap in (len(data), len(data) + 50, len(data) - 1, 0):
            st, _d0, _d1, adler, out_len, in_used, out = raw_model(d, cap, rb, zdict)
            if cap >= len(data):
                assert (st, out_len, in_used, adler) == (0, len(data), len(d), zlib.adler32(data)) and out == data, (seed, cap)
            else:
                assert (st, out_len) == (14, len(data)), (seed, cap)
        # (b) the oracle with the dictionary installed, on the stream wrapped with FDICT and DICTID: a cut and a flipped bit
        for bad in (d[: len(d) * 2 // 3], d[:50] + bytes([d[50] ^ 0x10]) + d[51:]):
            wrapped = b"\x78\xbb" + zlib.adler32(zdict).to_bytes(4, "big") + bad
            ro, oo = oracle.decompress_dict(wrapped + (b"" if rawcheck.zlib_raw(bad, zdict) is None else b"\0\0\0\0"), zdict, 1 << 17)
            st, _d0, _d1, adler, out_len, _used, out = raw_model(bad, 1 << 17, rb, zdict)
            if ro.status == 10:  # (the flipped bit left a valid stream: only the zero trailer is wrong)
                assert (st, out_len) == (0, ro.out_len) and out == oo
            else:
                assert (st, out_len, adler) == (ro.status, ro.out_len, ro.adler) and out == oo, (seed, st, ro.status)
        # without the dictionary the same stream refers to bytes that are not there (or decodes to something else): never the data
        st, _d0, _d1, _a, out_len, _u, out = raw_model(d, len(data), rb)
        assert st != 0 or out != data


def _kernel_notes():
    """name -> the integer fields of every kernel's metadata note in the gfx950 code objects of libpzg.so."""
    import pure_zlib_amd._ffi as _ffi
    llvm = "/opt/rocm/lib/llvm/bin"
    notes = {}
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.check_call([llvm + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, _ffi.LIB_PATH, os.path.join(d, "unused.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
        for n, at in enumerate(starts):  # one bundle per translation unit that holds kernels
            part = os.path.join(d, "fat%d.bin" % n)
            with open(part, "wb") as f:
                f.write(blob[at:starts[n + 1] if n + 1 < len(starts) else len(blob)])
            subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + part, "--output=" + co])
            text = subprocess.check_output([llvm + "/llvm-readelf", "--notes", co]).decode()
            for block in text.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                notes[name] = {a: int(b) for a, b in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return notes


def test_raw_ring11_kernel_keeps_the_zlib_instance_occupancy():
    """The ring-11 raw kernel is in the gfx950 code object under a name of its own and fits what the zlib instance fits: 72 vector
    registers (seven waves per SIMD), 6 KiB of LDS (26 stream-waves per CU), no vector spills, nothing in scratch.  Every ring has
    its raw instance, and the 32 KiB ring its fixup pass."""
    notes = _kernel_notes()
    raw = {n: k for n, k in notes.items() if "inflate_raw_kernel" in n}
    assert sorted(re.search(r"inflate_raw_kernelILi(\d+)ELb(\d)", n).groups() for n in raw) == \
        [("11", "0"), ("12", "0"), ("13", "0"), ("14", "0"), ("15", "0"), ("15", "1")], sorted(raw)
    (k,) = [k for n, k in raw.items() if "inflate_raw_kernelILi11E" in n]
    print("inflate_raw_kernel<11, false>:", {f: k[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                             "private_segment_fixed_size", "group_segment_fixed_size")})
    assert k["vgpr_count"] <= 72 and k["group_segment_fixed_size"] <= 6144 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert len([n for n in notes if re.search(r"inflate_kernelILi11E", n)]) == 2  # the zlib and gzip instances: no third one
