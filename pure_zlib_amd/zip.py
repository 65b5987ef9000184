"""ZIP archives (.zip / .jar / .whl / .docx / .apk) read and tested on the GPU: EXTENSION, the reference has no archive reader.

A deflated member holds a bare RFC 1951 stream and the central directory gives its exact decoded size and CRC-32, so an archive is
ONE launch: every method-8 member through pzg_decompress_many with PZG_RAW | PZG_CRC32 | PZG_HOST_PINNED, capacities exact, no
capacity guess and no relaunch; sizes, the input each stream consumed and the CRC-32s (computed on the device) are then compared
with the directory.  The stdlib `zipfile` only parses the central directory (zip64 included); nothing here inflates on the CPU.
A LARGE deflated member (`split`: that many compressed bytes or more) is decoded by many wavefronts instead (pure_zlib_amd/split.py)
and taken from there only when its size and CRC-32 come out as the directory says; every other one is in the launch as before.

    read_zip(path_or_bytes)  -> {name: bytes}
    test_zip(path_or_bytes)  -> [(name, problem)]        (empty: the archive is sound)
    python -m pure_zlib_amd.zip [--split BYTES] -t A.zip | -d DIR A.zip
"""
import io
import os
import struct
import sys
import zipfile
import zlib as _sys_zlib  # crc32 of STORED members only (their bytes are in host memory and never decoded)
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _ffi
from . import split as _split
from ._batch import pack
from .zlib import Context, DecompressionError, PinnedArena, default_context, error_from_status

_LOCAL_SIG = b"PK\x03\x04"


def _checksum_error(msg: str) -> DecompressionError:
    return DecompressionError("ChecksumError", msg, _ffi.E_CHECKSUM)


def _archive_bytes(src: Union[str, os.PathLike, bytes, bytearray, memoryview]) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def _member_data(blob: bytes, zi: zipfile.ZipInfo) -> Tuple[int, Optional[str]]:
    """Offset of the member's data: behind its local header, whose own name and extra lengths count (they may differ from the
    directory's).  (offset, problem)."""
    h = zi.header_offset
    if h + 30 > len(blob) or blob[h:h + 4] != _LOCAL_SIG:
        return 0, "no local file header at offset %d" % h
    nlen, xlen = struct.unpack_from("<HH", blob, h + 26)
    at = h + 30 + nlen + xlen
    if at + zi.compress_size > len(blob):
        return 0, "data runs past the end of the archive"
    return at, None


def _scan(src, ctx: Optional[Context], strict: bool, split: Optional[int] = None, split_chunk: Optional[int] = None):
    """The work of read_zip / test_zip: ({name: bytes}, [(name, problem)]).  strict: raise at the first problem."""
    blob = _archive_bytes(src)
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        infos = zf.infolist()
    out: Dict[str, bytes] = {}
    problems: List[Tuple[str, str]] = []

    def problem(name, err):
        if strict:
            raise err
        problems.append((name, str(err)))

    deflated = []  # (info, data offset)
    for zi in infos:
        if zi.flag_bits & 1:
            problem(zi.filename, NotImplementedError("%s: encrypted member (flag bit 0)" % zi.filename))
            continue
        if zi.compress_type not in (zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED):
            problem(zi.filename, NotImplementedError("%s: compression method %d is not supported (0 and 8 are)" % (zi.filename, zi.compress_type)))
            continue
        at, bad = _member_data(blob, zi)
        if bad:
            problem(zi.filename, zipfile.BadZipFile("%s: %s" % (zi.filename, bad)))
            continue
        if zi.compress_type == zipfile.ZIP_STORED:
            data = blob[at:at + zi.compress_size]
            if len(data) != zi.file_size:
                problem(zi.filename, _checksum_error("%s: size mismatch: %d != %d" % (zi.filename, zi.file_size, len(data))))
            elif _sys_zlib.crc32(data) != zi.CRC:
                problem(zi.filename, _checksum_error("%s: checksum mismatch: %08x != %08x" % (zi.filename, zi.CRC, _sys_zlib.crc32(data))))
            else:
                out[zi.filename] = data
        else:
            deflated.append((zi, at))
    if deflated:
        n = len(deflated)
        in_len = np.array([zi.compress_size for zi, _ in deflated], dtype=np.uint64)
        out_cap = np.array([zi.file_size for zi, _ in deflated], dtype=np.uint64)
        (in_off, tot_in), (out_off, tot_out) = pack(in_len), pack(out_cap)
        ain, aout = PinnedArena(tot_in), PinnedArena(tot_out)
        try:
            for k, (zi, at) in enumerate(deflated):
                o = int(in_off[k])
                ain.a[o:o + zi.compress_size] = np.frombuffer(blob, dtype=np.uint8, count=zi.compress_size, offset=at)
            ctx = ctx or default_context()
            split = _split.DEFAULT_SPLIT if split is None else int(split)
            large = [k for k in range(n) if split and int(in_len[k]) >= split]
            if not large:
                out_len, status, detail, in_used, crc = ctx.decompress_many_raw(
                    ain.a, in_off, in_len, aout.a, out_off, out_cap, pinned=True, raw=True, crc32=True)
            else:
                # The other members first: a launch on the arenas copies ONE range out, from its first member's bytes to its last one's,
                # the large members' places between them included; those are filled afterwards.  A large member is many wavefronts'
                # work (split.py); one that does not come back verified is decoded like the others, in a launch that copies member by
                # member.
                out_len, status, in_used = out_cap.copy(), np.zeros(n, dtype=np.int32), in_len.copy()  # (what a verified member has)
                detail, crc = np.zeros((n, 2), dtype=np.uint32), np.array([zi.CRC for zi, _ in deflated], dtype=np.uint32)

                def launch(which, pinned):
                    w = np.array(which, dtype=np.int64)
                    out_len[w], status[w], detail[w], in_used[w], crc[w] = ctx.decompress_many_raw(
                        ain.a, in_off[w], in_len[w], aout.a, out_off[w], out_cap[w], pinned=pinned, raw=True, crc32=True)
                is_large = set(large)
                launch([k for k in range(n) if k not in is_large], True)
                bodies = [_split.Body(int(in_off[k]), int(in_len[k]), int(out_cap[k]), deflated[k][0].CRC, int(out_off[k])) for k in large]
                done = _split.split_decode(ain.a, bodies, aout.a, ctx, split_chunk)
                launch([k for k, ok in zip(large, done) if not ok], False)
            for k, (zi, at) in enumerate(deflated):
                name, st = zi.filename, int(status[k])
                if st == _ffi.E_OUT_TOO_SMALL or (st == _ffi.OK and int(out_len[k]) != zi.file_size):
                    problem(name, _checksum_error("%s: size mismatch: %d != %d" % (name, zi.file_size, int(out_len[k]))))
                elif st != _ffi.OK:
                    e = error_from_status(blob[at:at + zi.compress_size], st, detail[k])
                    problem(name, DecompressionError(e.constructor, "%s: %s" % (name, e.message), e.status, e.detail))
                elif int(in_used[k]) != zi.compress_size:
                    problem(name, _checksum_error("%s: compressed size mismatch: %d != %d" % (name, zi.compress_size, int(in_used[k]))))
                elif int(crc[k]) != zi.CRC:
                    problem(name, _checksum_error("%s: checksum mismatch: %08x != %08x" % (name, zi.CRC, int(crc[k]))))
                else:
                    o = int(out_off[k])
                    out[name] = aout.a[o:o + zi.file_size].tobytes()
        finally:
            ain.close()
            aout.close()
    order = {zi.filename: k for k, zi in enumerate(infos)}
    return {name: out[name] for name in sorted(out, key=order.get)}, problems


def read_zip(path_or_bytes, ctx: Optional[Context] = None, split: Optional[int] = None, split_chunk: Optional[int] = None) -> Dict[str, bytes]:
    """Every member of the archive (directories are empty members), in directory order.  Raises at the first member that cannot be
    read: NotImplementedError naming an encrypted member or one of another method than 0 / 8, DecompressionError naming the member
    whose stream is bad or whose size or CRC-32 is not the directory's ("Checksum error: <member>: ...").
    split: deflated members of that many compressed bytes or more are decoded by many wavefronts each (None: split.DEFAULT_SPLIT, 0:
    none; split_chunk: the compressed bytes per wavefront of their scan).  Only the time depends on it."""
    return _scan(path_or_bytes, ctx, True, split, split_chunk)[0]


def test_zip(path_or_bytes, ctx: Optional[Context] = None, split: Optional[int] = None, split_chunk: Optional[int] = None) -> List[Tuple[str, str]]:
    """What `unzip -t` does: [(member, problem)] for every member that read_zip would refuse; the others are verified all the same.
    split, split_chunk: as for read_zip."""
    return _scan(path_or_bytes, ctx, False, split, split_chunk)[1]


test_zip.__test__ = False  # (not a pytest test, whatever imports it)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    argv, split = list(argv), None
    if "--split" in argv:  # (wherever it stands)
        at = argv.index("--split")
        if at + 1 < len(argv) and argv[at + 1].isdigit():
            split = int(argv[at + 1])
            del argv[at:at + 2]
    if len(argv) == 2 and argv[0] == "-t":
        bad = test_zip(argv[1], split=split)
        for name, why in bad:
            print("%s: %s" % (name, why))
        print("%s: %s" % (argv[1], "%d bad member(s)" % len(bad) if bad else "OK"))
        return 1 if bad else 0
    if len(argv) == 3 and argv[0] == "-d":
        root = os.path.realpath(argv[1])
        for name, data in read_zip(argv[2], split=split).items():
            dest = os.path.realpath(os.path.join(root, name))
            if dest != root and not dest.startswith(root + os.sep):
                raise ValueError("%s: member path leaves the target directory" % name)
            if name.endswith("/"):
                os.makedirs(dest, exist_ok=True)
                continue
            os.makedirs(os.path.dirname(dest), exist_ok=True)
            with open(dest, "wb") as f:
                f.write(data)
        return 0
    print("usage: python -m pure_zlib_amd.zip [--split BYTES] -t ARCHIVE.zip | -d DIR ARCHIVE.zip", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
