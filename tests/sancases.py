"""Shared by tests/test_sanitized_cores.py: the case files of the sanitizer programs (tests/cxx/san_*.cpp; the container is described
in tests/cxx/san_cases.h), how the programs are built and run, and the expectations of the inflate cases -- which come from system
zlib, the oracle and the case lists' own planned results, the sources the unsanitized model tests use, never from the code under
test."""
import os
import struct
import subprocess
import zlib

from conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-Wno-unknown-pragmas"]  # (the runtimes are linked in: the environment of the run stays as it is)

# san_inflate.cpp: what is compared
D0, D1, OUT_LEN, IN_USED, SUM, BYTES = 1, 2, 4, 8, 16, 32
ALL = D0 | D1 | OUT_LEN | IN_USED | SUM | BYTES
RAW, GZIP, FDICT, SEG, RESUME = 0, 1, 2, 3, 4  # its entries


def pack(fields):
    out = [struct.pack("<I", len(fields))]
    for f in fields:
        if isinstance(f, str):
            f = f.encode()
        elif not isinstance(f, (bytes, bytearray)):
            f = struct.pack("<Q", int(f) & 0xffffffffffffffff)
        out.append(struct.pack("<Q", len(f)))
        out.append(bytes(f))
    return b"".join(out)


def write_cases(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            f.write(pack(c))
    return len(cases)


def build(out, sources, defines=()):
    subprocess.check_call(SAN + ["-D" + d for d in defines] + ["-o", out] + [os.path.join(ROOT, s) for s in sources])
    return out


def run(exe, casefile, n, no_strips=False):
    """Runs the program over the file: a clean exit, no mismatch, and as many cases as were written."""
    env = {k: v for k, v in os.environ.items() if k not in ("PZM_NO_STRIPS", "PZM_FRESH_SCRATCH", "PZM_TIGHT_INPUT")}
    if no_strips:
        env["PZM_NO_STRIPS"] = "1"
    env.update(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (a model "wave" keeps its scratch for good)
    r = subprocess.run([exe, casefile], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.strip().splitlines()[-1] == "%d cases, 0 mismatches" % n, r.stdout[-3000:]


def inflate_case(name, entry, inp, zdict, cap, ring, cmp, status, d0=0, d1=0, out_len=0, in_used=0, checksum=0, data=b"", more=()):
    return [name, entry, inp, zdict, cap, ring, cmp, status, d0, d1, out_len, in_used, checksum, data] + list(more)


def raw_expect(O, d, cap):
    """What tests/rawcheck.py's check() holds a raw decode of d into cap bytes to, as (cmp, status, d0, d1, out_len, in_used,
    checksum, bytes): system zlib where it accepts d, and the oracle on the wrapped stream."""
    import rawcheck
    wrapped, e = rawcheck.wrap(O, d)
    ro, oo = O.decompress(wrapped, cap)
    st = ro.status
    assert st not in (2, 3, 4, 10, 20), st
    z = rawcheck.zlib_raw(d)
    if z is not None:  # (a): the two references agree
        data, used = z
        if cap >= len(data):
            assert (st, ro.out_len, e, ro.adler, oo) == (0, len(data), used, zlib.adler32(data), data)
        else:
            assert (st, ro.out_len) == (14, len(data))
    if st == 14:
        return OUT_LEN, st, 0, 0, ro.out_len, 0, 0, b""
    if st == 0:
        assert e is not None and e == ro.in_used - 6
        return OUT_LEN | IN_USED | SUM | BYTES, 0, 0, 0, ro.out_len, e, ro.adler, oo
    cmp = OUT_LEN | SUM | BYTES | (D0 | D1 if st in (6, 11, 12, 13) else D0 if st == 7 else 0)
    return cmp, st, ro.detail0 & 0xff if st == 7 else ro.detail0, ro.detail1, ro.out_len, 0, 0 if ro.out_len > cap else ro.adler, oo


def oracle_expect(ro, oo, cap, details=True):
    """A decode the oracle itself can do (zlib with a dictionary, gzip): everything it reports, as include/pzg.h promises it -- of a
    failed stream the bytes it had decoded, and their checksum unless they outgrew the capacity."""
    st = ro.status
    if st == 14:
        return OUT_LEN, st, 0, 0, ro.out_len, 0, 0, b""
    if st == 0:
        return OUT_LEN | IN_USED | SUM | BYTES, 0, 0, 0, ro.out_len, ro.in_used, ro.adler, oo
    return OUT_LEN | SUM | BYTES | (D0 | D1 if details else 0), st, ro.detail0, ro.detail1, ro.out_len, 0, 0 if ro.out_len > cap else ro.adler, oo
