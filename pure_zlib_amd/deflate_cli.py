"""The reference's `deflate` executable (/Deflate.hs:15-48) over the GPU path:  deflate foo.z -> foo.

SURVEY.md section 8f row 2 ("next" row).  Same messages as the reference; the file is read in the chunk
size `L.readFile` uses (bytestring's defaultChunkSize = 32 KiB minus two words) and driven through
the ZlibDecoder protocol exactly like `runDecompression` (Deflate.hs:30-48).

Batch mode (on top of the reference; behind its own flag so that everything the reference's
binary prints -- "USAGE: deflate [filename]" for anything but exactly one argument -- stays as it is):
deflate --many a.z b.z c.z ...  decodes every file in ONE `decompressMany` call -- one wavefront per file, one launch -- and writes a, b, c.  Each file is handed over as the lazy
ByteString `L.readFile` would make of it, so `decompress`'s own outcomes apply per file: "ERROR: <show e>" for a Left
(including Zlib.hs:48-49's "Finished with data remaining."), "Unexpected file name." for a name that does not end in
".z"; the other files are still decoded.

Indexed mode (on top of the reference too; pure_zlib_amd/indexed.py), for ONE large file -- foo.z (zlib) or foo.gz (gzip, one member):
deflate --index foo.pzi foo.z                          one sequential pass: writes foo and the index of access points foo.pzi
deflate --index foo.pzi --parallel foo.z               the same without the sequential pass: the access points are found in parallel
                                                       (Index.build_parallel), the file is decoded by segments and verified
deflate --use-index foo.pzi [--range OFF:LEN] foo.z    decodes foo with a wavefront per segment of the index and writes it; with
                                                       --range only the segments that cover LEN bytes from OFF, written to stdout

Streaming mode for the other containers (on top of the reference): the same loop, the same messages, one resumable decoder
deflate --gzip foo.gz                                  a gzip file (a series of members) -> foo
deflate --raw foo.deflate                              a bare RFC 1951 stream -> foo (the name's last suffix is stripped)

Members mode (pure_zlib_amd/gzfile.py), for a gzip file of MANY members -- BGZF, WARC, `cat a.gz b.gz`:
deflate --members foo.gz                               finds the members on the device, decodes them with a wavefront per member in
                                                       one launch and writes foo; "ERROR: <show e>" for a file that does not decode
deflate --members --split BYTES foo.gz                 the same; members of BYTES compressed bytes or more are split over many
                                                       wavefronts each (pure_zlib_amd/split.py; 0: none)
"""
import sys

from .incremental import Chunk, DecompError, Done, NeedMore, decompress_incremental

LAZY_CHUNK = 32 * 1024 - 16


def run_decompression(out, chunks, decoder, signal_end: bool = False) -> None:
    """signal_end (--gzip, --raw): the last chunk is fed as the last one, so that a gzip decoder knows no further member follows."""
    while True:
        if isinstance(decoder, Done):
            if chunks:
                print("WARNING: Finished decompression with data left.")
            return
        if isinstance(decoder, DecompError):
            print("ERROR: " + decoder.error.show())
            return
        if isinstance(decoder, NeedMore):
            if chunks:
                decoder = decoder.feed(chunks.pop(0), True) if signal_end and len(chunks) == 1 else decoder.feed(chunks.pop(0))
                continue
            print("ERROR: Ran out of data mid-decompression.")
            return
        if isinstance(decoder, Chunk):
            out.write(decoder.chunk)
            decoder = decoder.next()


def _lazy_chunks(data: bytes):
    return [data[i:i + LAZY_CHUNK] for i in range(0, len(data), LAZY_CHUNK)]


def run_many(files) -> None:
    """Batch mode: every `.z` file of `files` through one decompress_many call."""
    from .zlib import decompress_many
    good = []
    for f in files:
        if f.endswith(".z"):
            good.append(f)
        else:
            print(f"{f}: Unexpected file name.")
    streams = []
    for f in good:
        with open(f, "rb") as h:
            streams.append(_lazy_chunks(h.read()))
    for f, r in zip(good, decompress_many(streams)):
        if r.is_right():
            with open(f[:-2], "wb") as out:
                out.write(r.value)
        else:
            print(f"{f}: ERROR: " + r.value.show())


def _kind_and_target(name):
    for ext, kind in ((".z", "zlib"), (".gz", "gzip")):
        if name.endswith(ext):
            return kind, name[:-len(ext)]
    return None, None


def run_indexed(args) -> None:
    """Indexed mode: --index FILE.pzi [--parallel] NAME | --use-index FILE.pzi [--range OFF:LEN] NAME."""
    from .indexed import Index
    from .zlib import DecompressionError
    build = args[0] == "--index"
    rng = None
    rest = args[2:]
    parallel = build and rest[:1] == ["--parallel"]
    if parallel:
        rest = rest[1:]
    if not build and len(rest) >= 2 and rest[0] == "--range":
        try:
            rng = tuple(int(x) for x in rest[1].split(":"))
        except ValueError:
            rng = ()
        rest = rest[2:]
    if len(args) < 2 or len(rest) != 1 or (rng is not None and (len(rng) != 2 or min(rng) < 0)):
        print("USAGE: deflate --index FILE.pzi [--parallel] filename | deflate --use-index FILE.pzi [--range OFF:LEN] filename")
        return
    kind, target = _kind_and_target(rest[0])
    if kind is None:
        print("Unexpected file name.")
        return
    with open(rest[0], "rb") as f:
        data = f.read()
    if build:
        index, r = (Index.build_parallel if parallel else Index.build)(data, kind)
        if index is not None:
            index.save(args[1])
    elif rng is not None:
        try:
            sys.stdout.buffer.write(Index.load(args[1]).read(data, rng[0], rng[1]))
        except DecompressionError as e:
            print("ERROR: " + e.show())
        return
    else:
        r = Index.load(args[1]).decompress(data)
    if r.is_right():
        with open(target, "wb") as out:
            out.write(r.value)
    else:
        print("ERROR: " + r.value.show())


def run_members(args) -> None:
    """Members mode: --members [--split BYTES] NAME.gz."""
    from .gzfile import decompress_gzip_file
    args, split = list(args), None
    if "--split" in args:  # (in front of the name or behind it)
        at = args.index("--split")
        if at + 1 < len(args) and args[at + 1].isdigit():
            split = int(args[at + 1])
            del args[at:at + 2]
    if len(args) != 1:
        print("USAGE: deflate --members [--split BYTES] filename")
        return
    if not args[0].endswith(".gz"):
        print("Unexpected file name.")
        return
    with open(args[0], "rb") as f:
        r = decompress_gzip_file(f.read(), split=split)
    if r.is_right():
        with open(args[0][:-3], "wb") as out:
            out.write(r.value)
    else:
        print("ERROR: " + r.value.show())


def run_format(args, fmt) -> None:
    """--gzip NAME.gz | --raw NAME.suffix: the streaming loop over one resumable decoder of that format."""
    import os
    if len(args) != 1:
        print("USAGE: deflate --%s filename" % fmt)
        return
    target = args[0][:-3] if fmt == "gzip" and args[0].endswith(".gz") else os.path.splitext(args[0])[0] if fmt == "raw" else None
    if not target or target == args[0]:
        print("Unexpected file name.")
        return
    with open(args[0], "rb") as f:
        data = f.read()
    chunks = _lazy_chunks(data) or [b""]
    with open(target, "wb") as out:
        run_decompression(out, chunks, decompress_incremental(format=fmt), signal_end=True)


def main(argv=None) -> int:
    args = sys.argv[1:] if argv is None else argv
    if args and args[0] in ("--gzip", "--raw"):
        run_format(args[1:], args[0][2:])
        return 0
    if args and args[0] == "--many":
        run_many(args[1:])
        return 0
    if args and args[0] == "--members":
        run_members(args[1:])
        return 0
    if args and args[0] in ("--index", "--use-index"):
        run_indexed(args)
        return 0
    if len(args) != 1:  # Deflate.hs:17-29
        print("USAGE: deflate [filename]")
        return 0
    ifile = args[0]
    if not ifile.endswith(".z"):
        print("Unexpected file name.")
        return 0
    with open(ifile, "rb") as f:
        data = f.read()
    chunks = _lazy_chunks(data)
    with open(ifile[:-2], "wb") as out:
        run_decompression(out, chunks, decompress_incremental())
    return 0


if __name__ == "__main__":
    sys.exit(main())
