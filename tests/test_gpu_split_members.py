"""GPU: the large members of a gzip file and of a ZIP archive decoded by many wavefronts each (pure_zlib_amd/split.py:
pzg_index_scan_many, then every segment in one pzg_decompress_many_segments launch).  Only the time may depend on `split`: the bytes
returned and the errors raised are those of split=0 and of the one-stream decode, for sound and for broken files."""
import io
import struct
import zipfile
import zlib

import pytest

import corpus
import indexcheck as X
import memberscheck as M
import scancheck as S

pytestmark = pytest.mark.gpu

SPLIT, CHUNK = 4096, 1024


@pytest.fixture(scope="module")
def big():
    """name -> (raw stream, data) of indexcheck.big_inputs()"""
    return {name: (d, data) for name, d, data in X.big_inputs()}


def named_member(body, data, name=b"a name", extra=b"XY\x03\x00abc"):
    """A member with FEXTRA and FNAME in front of its body."""
    hdr = b"\x1f\x8b\x08\x0c" + bytes(4) + b"\x00\x03" + struct.pack("<H", len(extra)) + extra + name + b"\0"
    return hdr + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def small(seed):
    data = corpus.zipf_text(3000 + 17 * seed, seed)
    return M.member(data), data


@pytest.fixture(scope="module")
def sound(big):
    """(file, data, [(start, end) of the large members in the output])"""
    parts = [small(1), small(2), (M.wrap(*big["text6"]), big["text6"][1]), small(3), (named_member(*big["text1"]), big["text1"][1]), small(4),
             (M.wrap(*big["tiny400"]), big["tiny400"][1])]
    assert sorted(len(z) >= SPLIT for z, _d in parts) == [False] * 4 + [True] * 3
    data = b"".join(d for _z, d in parts)
    at = len(parts[0][1]) + len(parts[1][1])
    return b"".join(z for z, _d in parts), data, [(at, at + len(parts[2][1]))]


class Calls(list):
    """[[True / False per body]] of every call of split.split_decode, and in .segments how many segments each body it decoded had."""


@pytest.fixture
def helper_calls(monkeypatch):
    """What split.split_decode was asked and what it answered.  A segment is about 4 KiB of output here, not 1 MiB, so that members of
    a few hundred KiB are MANY segments with windows between them."""
    from pure_zlib_amd import split
    calls, real, real_segments = Calls(), split.split_decode, split.segments_of
    calls.segments = []

    def counted(buf, bodies, out, ctx, chunk=None, span=None):
        done = real(buf, bodies, out, ctx, chunk, span)
        calls.append(list(done))
        return done

    def segments_of(points, body_len, out_len):
        segs = real_segments(points, body_len, out_len)
        calls.segments.append(len(segs))
        return segs
    monkeypatch.setattr(split, "SPAN", 4096)
    monkeypatch.setattr(split, "segments_of", segments_of)
    monkeypatch.setattr(split, "split_decode", counted)
    return calls


def same(a, b):
    return a.is_right() == b.is_right() and (a.value == b.value if a.is_right() else a.value.show() == b.value.show())


def test_gzip_sound_file(gpu_ctx, sound, helper_calls):
    import pure_zlib_amd as P
    from pure_zlib_amd.gzfile import decompress_gzip_file
    f, data, _large = sound
    one = P.gzip_decompress_many([f], ctx=gpu_ctx)[0]
    assert one.is_right() and one.value == data
    got = decompress_gzip_file(f, ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK)
    assert got.is_right() and got.value == data
    assert helper_calls == [[True, True, True]]  # every large member went through the helper, none was put back
    assert len(helper_calls.segments) == 3 and min(helper_calls.segments) >= 3 and max(helper_calls.segments) >= 20  # (as several segments each)


def test_gzip_split_off(gpu_ctx, sound, helper_calls):
    from pure_zlib_amd.gzfile import decompress_gzip_file
    f, data, _large = sound
    got = decompress_gzip_file(f, ctx=gpu_ctx, split=0)
    assert got.is_right() and got.value == data and helper_calls == []
    with pytest.raises(ValueError):
        decompress_gzip_file(f, ctx=gpu_ctx, split=SPLIT, split_chunk=255)


def broken_files(big):
    d, data = big["text6"]
    whole = M.wrap(d, data)
    a, b, c = small(5), small(6), small(7)
    flip = lambda z, at: z[:at] + bytes([z[at] ^ 0x10]) + z[at + 1:]  # noqa: E731
    files = [("crc", a[0] + flip(whole, len(whole) - 7) + b[0]), ("isize", a[0] + flip(whole, len(whole) - 3) + b[0]),
             ("truncated", a[0] + whole[:len(whole) * 2 // 3] + b[0]), ("truncated at the end", a[0] + whole[:len(whole) * 2 // 3])]
    ch = S.chain(S.ScanModel().scan(d, 1024, 4096, 64))
    assert len(ch) >= 3
    bad, at = bytearray(d), ch[1][1] + 1  # BTYPE of a block in the middle becomes 3
    bad[at >> 3] |= 1 << (at & 7)
    bad[(at + 1) >> 3] |= 1 << ((at + 1) & 7)
    files.append(("btype 3", a[0] + M.wrap(bytes(bad), data) + b[0]))
    # a whole large member as the payload of stored blocks of another member: a candidate that is no member start, and a large one
    payload = c[1] + whole + a[1]
    files.append(("false candidate", a[0] + M.wrap(M.stored(payload), payload) + M.wrap(*big["text1"]) + b[0]))
    return files


def test_gzip_broken_files(gpu_ctx, big, helper_calls):
    import pure_zlib_amd as P
    from pure_zlib_amd.gzfile import decompress_gzip_file
    lefts = 0
    for what, f in broken_files(big):
        one = P.gzip_decompress_many([f], ctx=gpu_ctx)[0]
        off = decompress_gzip_file(f, ctx=gpu_ctx, split=0)
        del helper_calls[:]
        on = decompress_gzip_file(f, ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK)
        assert same(on, off) and same(on, one), (what, on.value if not on.is_right() else len(on.value), one.value if not one.is_right() else len(one.value))
        assert (what == "false candidate") == on.is_right(), what
        # where the large member's extent ends in its own trailer the helper was asked about it (and answered "not split" for a broken one)
        assert helper_calls or what not in ("crc", "btype 3", "false candidate"), what
        lefts += not on.is_right()
    assert lefts == 5


def test_gzip_member_index(gpu_ctx, sound):
    from pure_zlib_amd.gzfile import decompress_gzip_file
    f, data, large = sound
    ix0, r0 = decompress_gzip_file(f, ctx=gpu_ctx, split=0, return_index=True)
    ix, r = decompress_gzip_file(f, ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK, return_index=True)
    assert r.is_right() and r0.is_right() and r.value == r0.value == data
    assert (ix.starts == ix0.starts).all() and (ix.offsets == ix0.offsets).all() and ix.fingerprint == ix0.fingerprint
    lo, hi = large[0]
    for off, ln in ((lo + 1000, 70000), (lo + (hi - lo) // 2, 10), (hi - 5, 300)):
        assert ix.read(f, off, ln, ctx=gpu_ctx) == data[off:off + ln], (off, ln)


@pytest.fixture(scope="module")
def archive(big):
    """(archive bytes, {name: bytes})"""
    members = {"small.txt": corpus.zipf_text(5000, 9), "stored.bin": corpus.random_bytes(3000, 2), "dir/large6.txt": big["text6"][1],
               "tiny.txt": b"x", "large_random.bin": big["random6"][1], "large1.txt": big["text1"][1]}
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w") as zf:
        for name, data in members.items():
            zf.writestr(zipfile.ZipInfo(name), data, zipfile.ZIP_STORED if name == "stored.bin" else zipfile.ZIP_DEFLATED)
    with zipfile.ZipFile(io.BytesIO(bio.getvalue())) as zf:
        assert sorted(zi.compress_size >= SPLIT for zi in zf.infolist()) == [False] * 3 + [True] * 3
        assert {n: zf.read(n) for n in zf.namelist()} == members
    return bio.getvalue(), members


def test_zip(gpu_ctx, archive, helper_calls):
    from pure_zlib_amd.zip import read_zip, test_zip as check_zip
    blob, members = archive
    assert read_zip(blob, ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK) == members and helper_calls == [[True, True, True]]
    assert sorted(helper_calls.segments)[0] == 1 and sorted(helper_calls.segments)[1] >= 3  # (stored blocks alone: one segment; the texts: several)
    assert check_zip(blob, ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK) == []
    del helper_calls[:]
    assert read_zip(blob, ctx=gpu_ctx, split=0) == members and helper_calls == []


def test_zip_broken(gpu_ctx, archive, helper_calls):
    from pure_zlib_amd.zip import test_zip as check_zip
    blob, members = archive
    bad = bytearray(blob)
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        sizes = {zi.filename: zi.compress_size for zi in zf.infolist()}
    at = blob.find(b"PK\x01\x02")
    while at >= 0:  # the central directory's entries: CRC-32 at 16, compressed size at 20, the name from 46
        nlen, xlen, clen = struct.unpack_from("<HHH", blob, at + 28)
        name = blob[at + 46:at + 46 + nlen].decode()
        if name == "dir/large6.txt":
            bad[at + 16] ^= 1
        if name == "large_random.bin":  # its data cut at two thirds
            struct.pack_into("<I", bad, at + 20, sizes[name] * 2 // 3)
        at = blob.find(b"PK\x01\x02", at + 46 + nlen + xlen + clen)
    off = check_zip(bytes(bad), ctx=gpu_ctx, split=0)
    assert helper_calls == []
    on = check_zip(bytes(bad), ctx=gpu_ctx, split=SPLIT, split_chunk=CHUNK)
    assert on == off and sorted(name for name, _why in on) == ["dir/large6.txt", "large_random.bin"], (on, off)
    assert helper_calls == [[False, False, True]]  # (the sound large member beside them is still split)


def test_cli_round_trips(gpu_ctx, sound, archive, tmp_path, monkeypatch, capsys, helper_calls):
    from pure_zlib_amd import deflate_cli
    from pure_zlib_amd import zip as Z
    f, data, _large = sound
    (tmp_path / "many.gz").write_bytes(f)
    (tmp_path / "a.zip").write_bytes(archive[0])
    monkeypatch.chdir(tmp_path)
    assert deflate_cli.main(["--members", "--split", str(SPLIT), "many.gz"]) == 0 and (tmp_path / "many").read_bytes() == data
    assert helper_calls == [[True, True, True]]
    assert Z.main(["-t", "--split", str(SPLIT), "a.zip"]) == 0 and "a.zip: OK" in capsys.readouterr().out
    assert helper_calls == [[True, True, True], [True, True, True]]
    assert Z.main(["--split", str(SPLIT), "-d", "out", "a.zip"]) == 0
    assert (tmp_path / "out" / "dir" / "large6.txt").read_bytes() == archive[1]["dir/large6.txt"]
