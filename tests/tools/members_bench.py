"""A gzip file of MANY members that is already in device memory: today's path (the whole file as ONE PZG_GZIP stream, one
wavefront) against the members found and laid out on the device and decoded in one launch, a wavefront per member.  Not bench.py.

    python tests/tools/members_bench.py make   --mib 256 --file build/tmp_members.gz   # the input, once (CPU only)
    python tests/tools/members_bench.py plain  --file build/tmp_members.gz             # leg 1 (PZG_LIB=the parent's library: the parent's leg 1)
    python tests/tools/members_bench.py find   --file build/tmp_members.gz             # leg 2: pzg_gzip_find_members alone
    python tests/tools/members_bench.py layout --file build/tmp_members.gz             # leg 3: pzg_gzip_layout alone
    python tests/tools/members_bench.py all    --file build/tmp_members.gz             # leg 4: find, layout and the one launch

The file is a BGZF layout: the corpus text at level 6 in members of 65,280 bytes, each with the 'BC' subfield.  Every leg is a
process of its own, with device pointers, two warm-ups and five samples; a sample is the library's own kernel span
(pzg_last_kernel_ms; leg 4: the three calls' spans added up) and, beside it, the wall clock from the first call's first line to the
last kernel's end.  Leg 4 uses the candidates as they come (no pruning by the stated sizes, no repair): it asserts that they are
exactly the members, which is also the count of false hits on this file, and that every member decodes to its room.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BLOCK = 65280


def _member(seed):
    import corpus
    data = corpus.zipf_text(BLOCK, 0x6D000 + seed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    total = 18 + len(body) + 8
    hdr = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return hdr + body + struct.pack("<II", zlib.crc32(data), len(data)), zlib.crc32(data)


def make(a):
    import multiprocessing as mp
    n = a.mib * (1 << 20) // BLOCK
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        parts = pool.map(_member, range(n), chunksize=16)
    os.makedirs(os.path.dirname(a.file), exist_ok=True)
    with open(a.file, "wb") as f:
        for p, _crc in parts:
            f.write(p)
    json.dump({"members": n, "decoded_bytes": n * BLOCK, "compressed_bytes": sum(len(p) for p, _ in parts)}, open(a.file + ".json", "w"))
    print(open(a.file + ".json").read())


def report(what, nbytes, samples, **more):
    med = statistics.median(samples)
    print(json.dumps(dict({"leg": what, "median_ms": round(med, 4), "samples_ms": [round(s, 4) for s in samples],
                           "spread_ms": round(max(samples) - min(samples), 4), "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 3)}, **more)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["make", "plain", "find", "layout", "all"])
    ap.add_argument("--file", default=os.path.join(ROOT, "build", "tmp_members.gz"))
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=0)  # 0: the library's default
    a = ap.parse_args()
    if a.leg == "make":
        return make(a)
    import numpy as np
    import torch
    torch.cuda.init()
    import pure_zlib_amd as P
    from pure_zlib_amd import _ffi
    z = open(a.file, "rb").read()
    meta = json.load(open(a.file + ".json"))
    n_true, out_len = meta["members"], meta["decoded_bytes"]
    ctx = P.Context(0)
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    t_in = torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).to(dev)
    t_out = torch.empty(out_len + 64, dtype=torch.uint8, device=dev)
    room = n_true + 1024
    i64 = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int64, device=dev)  # noqa: E731
    t_starts, t_bsize = i64(room), torch.zeros(room, dtype=torch.int32, device=dev)
    t_arr = [i64(room) for _ in range(4)]
    t_olen, t_used, t_status = i64(room), i64(room), torch.full((room,), -1, dtype=torch.int32, device=dev)
    count, total = C.c_uint32(0), C.c_uint64(0)
    torch.cuda.synchronize()

    def find():
        _ffi.check(L.pzg_gzip_find_members(ctx.handle, t_in.data_ptr(), len(z), a.chunk, t_starts.data_ptr(), t_bsize.data_ptr(), room,
                                           C.byref(count), _ffi.DEVICE_PTRS), ctx.handle)
        return ctx.last_kernel_ms()

    def layout(m):
        _ffi.check(L.pzg_gzip_layout(ctx.handle, t_in.data_ptr(), len(z), t_starts.data_ptr(), m, 0, *[t.data_ptr() for t in t_arr], C.byref(total),
                                     _ffi.DEVICE_PTRS), ctx.handle)
        return ctx.last_kernel_ms()

    def decode(m):
        ctx.decompress_many_device(t_in.data_ptr(), t_arr[0].data_ptr(), t_arr[1].data_ptr(), t_out.data_ptr(), t_arr[2].data_ptr(), t_arr[3].data_ptr(),
                                   t_olen.data_ptr(), t_status.data_ptr(), 0, t_used.data_ptr(), 0, m, sync=True, gzip=True)
        return ctx.last_kernel_ms()

    kernel, wall = [], []
    for k in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.leg == "plain":
            one = torch.tensor([0, len(z), 0, out_len], dtype=torch.int64, device=dev)
            ctx.decompress_many_device(t_in.data_ptr(), one[0:].data_ptr(), one[1:].data_ptr(), t_out.data_ptr(), one[2:].data_ptr(), one[3:].data_ptr(),
                                       t_olen.data_ptr(), t_status.data_ptr(), 0, t_used.data_ptr(), 0, 1, sync=True, gzip=True)
            ms = ctx.last_kernel_ms()
            assert int(t_status[0]) == 0 and int(t_olen[0]) == out_len
        elif a.leg == "find":
            ms = find()
        elif a.leg == "layout":
            if k == 0:
                find()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            ms = layout(count.value)
        else:
            ms = find()
            assert count.value <= room
            ms += layout(count.value)
            ms += decode(count.value)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= 2:
            kernel.append(ms)
            wall.append((t1 - t0) * 1e3)
    more = {}
    if a.leg != "plain":
        more = {"candidates": count.value, "members": n_true, "false_hits": count.value - n_true, "chunk": a.chunk or 64 << 10}
        assert count.value == n_true, "a false hit on the bench file: prune and repair as pure_zlib_amd/gzfile.py does"
    if a.leg in ("layout", "all"):
        assert total.value == out_len
    if a.leg == "all":
        m = count.value
        assert bool((t_status[:m] == 0).all()) and bool((t_olen[:m] == t_arr[3][:m]).all()) and bool((t_used[:m] == t_arr[1][:m]).all())
    if a.leg in ("plain", "all"):
        got = zlib.crc32(t_out[:out_len].cpu().numpy().tobytes())
        more["crc32"] = "%08x" % got
    nbytes = len(z) if a.leg == "find" else out_len
    names = {"plain": "1: the whole file as ONE PZG_GZIP stream", "find": "2: pzg_gzip_find_members (GiB/s of COMPRESSED bytes swept, both passes together)",
             "layout": "3: pzg_gzip_layout", "all": "4: find + layout + one launch over all members"}
    report(names[a.leg] + ", kernel spans", nbytes, kernel, lib=os.path.basename(os.path.dirname(_ffi.LIB_PATH)), **more)
    report(names[a.leg] + ", wall clock", nbytes, wall)
    ctx.close()


if __name__ == "__main__":
    main()
