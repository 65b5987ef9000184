#!/usr/bin/env python3
"""bench.py -- decompressed GiB/s of the batched zlib decompressor on MI355X.

Metric (BASELINE.json): "decompressed GiB/s (whole node) on 64K level-6 zlib blobs; bit-exact vs ref".
Workload at N=1: BASELINE config 4, 65,536 x 32 KiB dynamic-Huffman (level-6) blobs, one stream per
wavefront, inputs and outputs resident in HBM when the timed region starts.  A "step" is one pass
of pzg_decompress_many over the whole batch.  N>1: one process per GPU, every rank decodes its own
65,536-stream shard of an N x 65,536 batch (weak scaling, no data-path collective).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline.  --full adds everything else this file
measures or checks: every stream of the timed batch verified on one more step, the 32 KiB LDS-ring variant, the other
BASELINE configs, the host-buffer and incremental paths, the CPU baselines and the Adler-32 microbench.
--dump-outputs DIR writes what the last timed step computed as DIR/*.npy (see dump_outputs).

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch  # first: libpzg.so then binds to the HIP runtime torch already loaded

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corpus  # noqa: E402
import pure_zlib_amd as P  # noqa: E402
from pure_zlib_amd.shard import plan_shards  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
HBM_MEASURED_GBS = 6290.0  # same guide: float4 copy


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_sha256():
    """What the measured traffic belongs to: the kernels' source (profiles/traffic.json records it with every entry)."""
    import hashlib
    h = hashlib.sha256()
    for fn in ("inflate_core.h", "bundle_core.h", "pzg_inflate_kernel.h", "pzg_bundle_kernel.h", "pzg_kernels.hip", "pzg_kernels_b.hip", "wave.h"):
        with open(os.path.join(ROOT, "pure_zlib_amd", "csrc", fn), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def traffic_from_profiles(args, ring_bits, n):
    """HBM bytes per launch measured with rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE, separate runs, counters only) of
    this same command, recorded in profiles/traffic.json after each profiling session (tests/tools/r6_profiles.sh, tests/tools/traffic_update.py) together
    with the SHA-256 of the kernels' source and the pool size of the run.  Returns (bytes or None, where the number comes
    from -- or WHY there is none: an entry measured on other kernel source, or with another pool, is not this kernel's traffic)."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            t = json.load(f)
    except Exception as e:
        return None, {"reason": f"profiles/traffic.json: {e}"}
    sha = kernel_sha256()
    why = "no entry for this workload / ring / stream count"
    for e in t["entries"]:
        if e["workload"] == args.workload and e["ring_bits"] == ring_bits and e["streams"] == n and bool(e.get("gzip")) == bool(args.gzip):
            if e.get("kernel_sha256") != sha:
                why = f"the entry was measured on other kernel source (sha256 {str(e.get('kernel_sha256'))[:12]}..., this build {sha[:12]}...): re-run tests/tools/r6_profiles.sh traffic + tests/tools/traffic_update.py"
                continue
            if e.get("pool") not in (None, args.pool):
                why = f"the entry was measured with --pool {e.get('pool')}, this run uses {args.pool}"
                continue
            src = {"file": e.get("file", t.get("source")), "counters": "FETCH_SIZE + WRITE_SIZE (TCC_EA0_RDREQ / WRREQ based), one rocprofv3 --pmc pass each",
                   "fetch_bytes": e["fetch_bytes"], "write_bytes": e["write_bytes"],
                   "fetch_correction": e.get("fetch_correction", "raw (dword and byte requests at the lanes' own addresses dominate the reads; the x2 of the guide applies "
                                                                 "to 16 B/lane streaming reads only)"),
                   "kernel_sha256": sha, "pool": e.get("pool"), **({"note": e["note"]} if e.get("note") else {})}
            return e["hbm_bytes_per_launch"], src
    return None, {"reason": why}


def hetero_blob(seed):
    """A batch of mixed KINDS: text, html, literal-heavy skewed bytes and binary-looking data, 8 / 16 / 32 / 64 KiB,
    levels 1 / 6 / 9 -- neighbours in the batch differ in all three, so a stream-wave's profile of one stream is rarely the next one's."""
    kind, size, level = seed % 4, [8, 16, 32, 64][(seed // 4) % 4] * 1024, [6, 1, 9][(seed // 16) % 3]
    if kind == 0:
        t = corpus.zipf_text(size, seed)
    elif kind == 1:
        t = corpus.html_slice(size, seed)
    elif kind == 2:
        t = corpus.skewed_bytes(size, seed)
    else:
        t = corpus.binary_records(size, seed)  # binary-looking: 16-byte records
    return t, zlib.compress(t, level)


def pool_blob(args, seed):
    """The (text, zlib stream) pair of pool seed `seed`: a function of the arguments and the seed alone."""
    if args.workload == "fixed_4k":
        t = corpus.zipf_text(4096, seed)
        co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        z = co.compress(t) + co.flush()
    elif args.workload == "skewed_bytes":  # literal-heavy, many codes longer than the primary table
        t = corpus.skewed_bytes(args.blob_bytes, seed)
        z = zlib.compress(t, args.level)
    elif args.workload == "fixed_bin":  # fixed-Huffman blocks whose literals are all >= 144: 9-bit codes
        t = bytes(b | 0x80 for b in corpus.zipf_text(4096, seed))
        co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        z = co.compress(t) + co.flush()
    elif args.workload == "runs":  # overlapping matches: byte runs and short repeating patterns (dist < len)
        t = corpus.mixed_data(args.blob_bytes, 2 + (seed & 1) + 4 * seed)
        z = zlib.compress(t, args.level)
    elif args.workload == "html":  # slices of the reference's own RFC html fixtures
        t = corpus.html_slice(args.blob_bytes, seed)
        z = zlib.compress(t, args.level)
    elif args.workload == "mixed":
        size = 1024 * (1 + (seed * 2654435761 >> 7) % 64)
        t = corpus.zipf_text(size, seed)
        z = zlib.compress(t, 6)
    elif args.workload == "hetero":
        t, z = hetero_blob(seed)
    else:
        t = corpus.zipf_text(args.blob_bytes, seed)
        z = zlib.compress(t, args.level)
    if args.gzip:  # same DEFLATE body, gzip header and CRC-32 + ISIZE trailer instead of the zlib ones
        import struct
        z = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + z[2:-4] + struct.pack("<II", zlib.crc32(t), len(t) & 0xffffffff)
    return t, z


def build_pool(args):
    """P distinct (text, zlib stream) pairs, seeds 0..P-1, identical on every rank.  Built on up to 16 threads (zlib and
    numpy release the GIL; 8,192 level-6 compressions take ~11 s of one core), in seed order whatever the thread count."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
        pairs = list(ex.map(lambda seed: pool_blob(args, seed), range(args.pool)))
    return [p[0] for p in pairs], [p[1] for p in pairs]


def dump_outputs(path, n, out_off, out_cap, d_out, d_status, d_out_len, d_in_used, d_adler):
    """--dump-outputs: what the caller of the timed step receives, from its last step, as float64 / float32 .npy files that
    two builds can be compared by (the inputs are a function of the arguments).  Per stream, for every stream of the batch
    or a seeded sample of 65,536 (`streams`): `status`, `out_len`, `in_used` and `checksum` (the Adler-32, or the CRC-32 with
    --gzip).  The decoded bytes of a seeded sample of streams (`byte_streams`, in that order), each stream's whole extent,
    cut at 8 MiB in all: `bytes` (float32).  32 MiB + 2.5 MiB at most.  (detail[] is left out: unspecified on success.)"""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(0xD0D0)
    rows = np.arange(n) if n <= 65536 else np.sort(rng.choice(n, 65536, replace=False))
    rows_d = torch.from_numpy(rows).to(d_out.device)
    per_stream = lambda d, np_type: d[rows_d].cpu().numpy().view(np_type).astype(np.float64)  # noqa: E731
    arrays = {"streams": rows.astype(np.float64), "status": per_stream(d_status, np.int32), "out_len": per_stream(d_out_len, np.int64),
              "in_used": per_stream(d_in_used, np.int64), "checksum": per_stream(d_adler, np.uint32)}
    budget, picked, pieces = 8 << 20, [], []
    for k in rng.permutation(n):
        if budget == 0:
            break
        take = min(int(out_cap[k]), budget)
        pieces.append(d_out[int(out_off[k]):int(out_off[k]) + take])
        picked.append(k)
        budget -= take
    arrays["byte_streams"] = np.array(picked, dtype=np.float64)
    arrays["bytes"] = torch.cat(pieces).cpu().numpy().astype(np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sum(a.nbytes for a in arrays.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)  # (the rate settles over a process' first five or six launches: profiles/r06_strips.txt 11)
    ap.add_argument("--workload", default="l6_32k", choices=["l6_32k", "fixed_4k", "mixed", "skewed_bytes", "html", "runs", "fixed_bin", "hetero"])
    ap.add_argument("--streams", type=int, default=65536, help="streams per GPU")
    ap.add_argument("--blob-bytes", type=int, default=32768)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--pool", type=int, default=8192, help="distinct blobs (SURVEY.md 8d: P = 8192); the batch replicates them at distinct addresses")
    ap.add_argument("--cpu-sample", type=int, default=8192, help="streams of the ONE-THREAD CPU baseline legs (rank 0, N=1); 0 = no CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-cores CPU baseline legs (0 = every core)")
    ap.add_argument("--adler-gib", type=float, default=16.0, help="Adler-32 microbench size (BASELINE config 2); 0 = skip")
    ap.add_argument("--ring-bits", type=int, default=0, help="LDS ring size class 11..15 (0 = library default); 15 = the whole 32 KiB window in LDS")
    ap.add_argument("--bundles", type=int, default=-1, help="diagnostic: PZG_OPT_BUNDLES (0 off, 1 launches of 32,768 streams or more, 2 always; -1 = library default)")
    ap.add_argument("--no-ab", action="store_true", help="skip the secondary measurement of the pure 32 KiB LDS-ring variant")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--gzip", action="store_true", help="diagnostic: the same payloads as RFC 1952 members (extension; CRC-32 pass on the device)")
    ap.add_argument("--no-host-path", action="store_true", help="skip the host-buffer (PCIe-inclusive) measurement")
    ap.add_argument("--no-variants", action="store_true", help="skip the config 3 / config 5 share / 64 KiB legs of the default run")
    ap.add_argument("--incremental-decoders", type=int, default=4096, help="decoders of the incremental-path leg (pzg_decoder_feed, 32 KiB pieces); 0 = skip")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: verify every stream, and run the variants, host-path, incremental, CPU-baseline and Adler-32 legs "
                         "(the options above that skip or size those legs apply only here)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/*.npy (rank 0's shard when --gpus > 1)")
    args = ap.parse_args()
    verify = args.full and not args.no_verify

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # test knobs (tests/test_gpu_fullsize.py runs the N>1 path with two ranks on ONE device): RCCL refuses two ranks
    # on the same GPU, so that run rendezvous over gloo; the driver's multi-GPU runs use neither knob
    local_rank = int(os.environ.get("PZG_BENCH_DEVICE", local_rank))
    backend = os.environ.get("PZG_BENCH_BACKEND", "nccl")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    rdev = dev if backend == "nccl" else torch.device("cpu")  # where the cross-rank scalars live

    t_setup = time.time()
    if world > 1:
        # the pool is built ONCE, on rank 0 (8,192 level-6 compressions: ~11 s of one host core -- times N on the node's shared
        # cores if every rank did it), and handed to the others: lengths, then the bytes
        if rank == 0:
            texts, zs = build_pool(args)
            lens = torch.tensor([len(t) for t in texts] + [len(z) for z in zs], dtype=torch.int64)
            blob = torch.from_numpy(np.frombuffer(b"".join(texts) + b"".join(zs), dtype=np.uint8).copy())
        else:
            lens = torch.zeros(2 * args.pool, dtype=torch.int64)
        lens = lens.to(rdev)
        dist.broadcast(lens, src=0)
        lens_h = lens.cpu().numpy()
        if rank != 0:
            blob = torch.zeros(int(lens_h.sum()), dtype=torch.uint8)
        blob = blob.to(rdev)
        dist.broadcast(blob, src=0)
        if rank != 0:
            raw = blob.cpu().numpy().tobytes()
            cuts = np.concatenate([[0], np.cumsum(lens_h)])
            pieces = [raw[int(cuts[k]):int(cuts[k + 1])] for k in range(2 * args.pool)]
            texts, zs = pieces[:args.pool], pieces[args.pool:]
        del blob
    else:
        texts, zs = build_pool(args)
    npool = len(zs)
    total_streams = args.streams * world
    rng = np.random.default_rng(0xB00C)
    perm = rng.integers(0, npool, size=total_streams)  # which pool blob stream g replicates
    dec_len = np.array([len(t) for t in texts], dtype=np.int64)
    shards = plan_shards(dec_len[perm], world)
    mine = shards[rank]
    n = len(mine)
    pick = perm[mine]

    # arenas: every stream at its own 256-byte aligned address (footprint >> 256 MiB Infinity Cache)
    zlen = np.array([len(z) for z in zs], dtype=np.int64)
    in_len = zlen[pick]
    out_cap = dec_len[pick]
    in_off = np.zeros(n, dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    in_off[1:] = np.cumsum((in_len[:-1] + 255) // 256 * 256)
    out_off[1:] = np.cumsum((out_cap[:-1] + 255) // 256 * 256)
    in_bytes = int(in_off[-1] + (in_len[-1] + 255) // 256 * 256)
    out_bytes = int(out_off[-1] + (out_cap[-1] + 255) // 256 * 256)
    h_in = np.zeros(in_bytes, dtype=np.uint8)
    zarr = [np.frombuffer(z, dtype=np.uint8) for z in zs]
    for k in range(n):
        h_in[in_off[k]:in_off[k] + in_len[k]] = zarr[pick[k]]
    d_in = torch.from_numpy(h_in).to(dev)
    d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    d_in_off, d_in_len, d_out_off, d_out_cap = as_dev(in_off), as_dev(in_len), as_dev(out_off), as_dev(out_cap)
    d_out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    d_in_used = torch.zeros(n, dtype=torch.int64, device=dev)
    d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_adler = torch.zeros(n, dtype=torch.int32, device=dev)
    d_detail = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if rank == 0:
        log(f"[bench] setup {time.time() - t_setup:.1f}s: {n} streams/GPU, in {in_bytes / 2**20:.0f} MiB, "
            f"out {out_bytes / 2**20:.0f} MiB, pool {npool}")

    ctx = P.Context(local_rank)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    from pure_zlib_amd import _ffi
    ring_bits = args.ring_bits or int(os.environ.get("PZG_RING_BITS", _ffi.DEFAULT_RING_BITS))
    ctx.set_ring_bits(ring_bits)
    if args.bundles >= 0:
        ctx.set_bundles(args.bundles)

    def step():
        ctx.decompress_many_device(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_out.data_ptr(),
                                   d_out_off.data_ptr(), d_out_cap.data_ptr(), d_out_len.data_ptr(),
                                   d_status.data_ptr(), d_detail.data_ptr(), d_in_used.data_ptr(), d_adler.data_ptr(),
                                   n, sync=False, gzip=args.gzip)

    def barrier():
        if world > 1:
            dist.barrier()

    cold_ms = None
    for w in range(args.warmup):
        step()
        if w == 0:  # the process' FIRST launch: scratch as the allocator left it -- no stream-wave has a profile, no run-up has adapted
            cold_ms = ctx.last_kernel_ms()
    torch.cuda.synchronize()
    kernel_ms = []
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        kernel_ms.append(ctx.last_kernel_ms())  # HIP events on the launch stream (waits for the step)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0  # this rank's K steps, between a barrier + synchronize in front and a synchronize behind
    barrier()
    if args.dump_outputs and rank == 0:
        nb_dump = dump_outputs(args.dump_outputs, n, out_off, out_cap, d_out, d_status, d_out_len, d_in_used, d_adler)
        log(f"[bench] {nb_dump / 2**20:.1f} MiB of outputs written to {args.dump_outputs}")
    per_rank = None
    if world > 1:
        # the job's time is the slowest rank's (MAX); every rank's own wall time, kernel time and share are reported beside it
        mine_v = torch.tensor([elapsed, float(np.mean(kernel_ms)), float(out_cap.sum()), float(in_len.sum()), float(n)], dtype=torch.float64, device=rdev)
        allv = [torch.zeros_like(mine_v) for _ in range(world)]
        dist.all_gather(allv, mine_v)
        allv = np.stack([v.cpu().numpy() for v in allv])
        elapsed = float(allv[:, 0].max())
        per_rank = {"wall_ms_per_step": [round(float(x) / args.steps * 1e3, 3) for x in allv[:, 0]],
                    "kernel_ms": [round(float(x), 3) for x in allv[:, 1]],
                    "kernel_ms_min": round(float(allv[:, 1].min()), 3), "kernel_ms_max": round(float(allv[:, 1].max()), 3),
                    "decoded_MiB": [round(float(x) / 2**20, 1) for x in allv[:, 2]],
                    "streams": [int(x) for x in allv[:, 4]],
                    "shard_imbalance": round(float(allv[:, 2].max() / allv[:, 2].mean()), 4),
                    "note": "time = MAX over ranks of the rank's own wall time for its K steps (barrier + synchronize in front, synchronize behind, "
                            "the closing barrier outside); shard_imbalance = largest shard's decoded bytes / mean"}

    # ---- verification: EVERY stream of the timed batch, bit-exact ---------------------------------
    # The outputs are POISONED first and one more step -- the same call on the same arenas, outside the timed region -- is
    # what gets verified: a step that did nothing cannot pass on what an earlier one left behind.  Its kernel time (HIP
    # events) is reported beside the timed steps': the same work takes the same time.
    verify_ms = None
    if verify:
        d_out.fill_(0xCD)
        d_status.fill_(-1)
        d_out_len.zero_()
        d_in_used.zero_()
        d_adler.zero_()
        torch.cuda.synchronize()
        step()
        verify_ms = ctx.last_kernel_ms()
        torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    out_len = d_out_len.cpu().numpy()
    adler = d_adler.cpu().numpy().view(np.uint32)
    bit_exact = None
    if verify:
        exp_adler = np.array([(zlib.crc32(t) if args.gzip else zlib.adler32(t)) for t in texts], dtype=np.uint32)[pick]
        ok = bool((status == 0).all() and (out_len == out_cap).all() and (adler == exp_adler).all()
                  and (d_in_used.cpu().numpy() == in_len).all())
        if ok and len(set(dec_len.tolist())) == 1:
            # full byte compare on the device: out arena vs the expected texts gathered the same way
            width = int(dec_len[0])
            stride = (width + 255) // 256 * 256
            pool_t = torch.from_numpy(np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(npool, width)).to(dev)
            got = d_out.view(n, stride)[:, :width]
            idx = torch.from_numpy(pick).to(dev)
            for lo in range(0, n, 8192):
                ok = ok and bool(torch.equal(got[lo:lo + 8192], pool_t[idx[lo:lo + 8192]]))
        elif ok:
            h_out = d_out.cpu().numpy()
            for k in range(0, n):
                if h_out[out_off[k]:out_off[k] + out_cap[k]].tobytes() != texts[pick[k]]:
                    ok = False
                    break
        bit_exact = ok
        if world > 1:
            tt = torch.tensor([1 if ok else 0], dtype=torch.int32, device=rdev)
            dist.all_reduce(tt, op=dist.ReduceOp.MIN)
            bit_exact = bool(tt.item())
        if not bit_exact:
            bad = np.nonzero(status != 0)[0]
            log(f"[bench] rank {rank}: VERIFICATION FAILED; {len(bad)} bad statuses, first {bad[:5]} {status[bad[:5]]}")

    # ---- A/B evidence: the same batch through the pure 32 KiB LDS-ring variant (north_star's literal design) ----
    ab = None
    if rank == 0 and world == 1 and args.full and not args.no_ab and ring_bits != 15:
        ctx.set_ring_bits(15)
        step()
        torch.cuda.synchronize()
        ms15 = []
        for _ in range(2):
            step()
            ms15.append(ctx.last_kernel_ms())
        ok15 = bool((d_status.cpu().numpy() == 0).all() and (d_adler.cpu().numpy().view(np.uint32) == exp_adler).all()) if verify else None
        ab = {"ring_bits": 15, "kernel_ms": round(float(np.mean(ms15)), 3),
              "GiBps": round(int(out_cap.sum()) / (float(np.mean(ms15)) * 1e-3) / 2**30, 2), "bit_exact": ok15,
              "note": "whole DEFLATE window as an LDS ring: 4 stream-waves per CU (LDS-bound occupancy)"}
        ctx.set_ring_bits(ring_bits)

    dec_total = int(out_cap.sum()) * world  # decoded bytes per step, whole job (the shards hold the same amount: plan_shards balances them)
    if per_rank is not None:
        dec_total = int(allv[:, 2].sum())
    comp_total = int(in_len.sum())
    value = dec_total * args.steps / elapsed / 2**30

    result = None
    if rank == 0:
        k_ms = float(np.mean(kernel_ms))
        algo_bytes = comp_total + int(out_cap.sum())  # per launch on this GPU: compressed read once + decoded written once
        achieved = algo_bytes / (k_ms * 1e-3) / 1e9
        result = {
            "metric": "decompressed GiB/s (whole node) on 64K level-6 zlib blobs; bit-exact vs ref",
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "bit_exact": bit_exact,
            "config": {
                "workload": {
                    "l6_32k": f"BASELINE config 4: {args.streams} x {args.blob_bytes // 1024} KiB level-{args.level} "
                              "dynamic-Huffman zlib blobs per GPU, one stream per wavefront",
                    "fixed_4k": f"BASELINE config 3: {args.streams} x 4 KiB fixed-Huffman (Z_FIXED level-1) blobs per GPU",
                    "mixed": f"BASELINE config 5 shape: {args.streams} mixed 1-64 KiB level-6 blobs per GPU",
                    "hetero": f"diagnostic: {args.streams} blobs of mixed KINDS (text / html / literal-heavy / binary-looking, 8-64 KiB, levels 1 / 6 / 9) per GPU",
                    "skewed_bytes": f"diagnostic: {args.streams} x {args.blob_bytes // 1024} KiB literal-heavy skewed-byte blobs, level {args.level}",
                    "fixed_bin": f"diagnostic: {args.streams} x 4 KiB fixed-Huffman blobs of text with the high bit set (every literal a 9-bit code)",
                    "runs": f"diagnostic: {args.streams} x {args.blob_bytes // 1024} KiB byte runs / short repeating patterns (overlapping matches), level {args.level}",
                    "html": f"diagnostic: {args.streams} x {args.blob_bytes // 1024} KiB slices of the reference's RFC html fixtures, level {args.level}",
                }[args.workload],
                "streams_per_gpu": n,
                "distinct_blobs": npool,
                "compressed_MiB_per_gpu": round(comp_total / 2**20, 1),
                "decompressed_MiB_per_gpu": round(int(out_cap.sum()) / 2**20, 1),
                "parallelism": f"shard{world}" if world > 1 else "single",
                "ring_bits": ring_bits,
                **({"container": "gzip members (extension): CRC-32 + ISIZE verified by a second kernel"} if args.gzip else {}),
                "window": "32 KiB LDS ring" if ring_bits == 15 else f"{2**ring_bits // 1024} KiB LDS near ring + far back-references from the stream's flushed output (HBM/L2)",
                "decode": ("bundles: 64 streams of the fixed code to a wave, one lane per stream -- every lane a sequential inflater with its own 512-byte "
                           "window in LDS (dword-interleaved), up to three literals and a match's first bytes a step, far matches from the stream's own flushed "
                           "output; what is not plain goes to the one-stream-per-wave kernel") if args.workload in ("fixed_4k", "fixed_bin") and not args.gzip and args.bundles != 0 and n >= 32768 else
                          ("strips: 64 lanes decode 64 consecutive pieces of a stream's input token by token, up to two literals a step (speculative starts, "
                           "verified) and write them as sequences (literal run + match: a record and the literal bytes) to a per-wave scratch in HBM (64.8 KiB per "
                           "resident stream-wave, allocated by the library); then one lane copies one whole sequence inside the LDS ring, up to 64 sequences a "
                           "group; a stream's first span is cut into strips of equal WORK by the wave's profile of the stream before it (checked by "
                           "the run-ups); 128-bit windows for stream tails and short streams"),
                "verified": ("every stream: status, length, in_used, Adler-32 and full byte compare, on one more step run after the "
                             "timed region over POISONED output / status arrays") if bit_exact is not None else
                            "skipped" if args.full else "not in a plain run (--full verifies every stream)",
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "bundle_kernel" if args.workload in ("fixed_4k", "fixed_bin") and not args.gzip and args.bundles != 0 and n >= 32768
                          else f"inflate_kernel<{ring_bits},false,{str(bool(args.gzip)).lower()}>",
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5),
                "frac_of_measured_copy_6290": round(achieved / HBM_MEASURED_GBS, 5),
                "read_only_GBps": round(comp_total / (k_ms * 1e-3) / 1e9, 2),
                "algorithmic_bytes_per_launch": algo_bytes,
                "kernel_ms_avg": round(k_ms, 4),
                "cold_first_launch_kernel_ms": None if cold_ms is None else round(cold_ms, 4),
                "cold_first_launch_GiBps": None if cold_ms is None else round(int(out_cap.sum()) / (cold_ms * 1e-3) / 2**30, 2),
                "verified_step_kernel_ms": None if verify_ms is None else round(verify_ms, 4),
                "traffic": traffic_from_profiles(args, ring_bits, n)[0],
                "traffic_source": traffic_from_profiles(args, ring_bits, n)[1],
            },
        }
        if ab is not None:
            result["lds_ring_32k_variant"] = ab
        if per_rank is not None:
            result["per_rank"] = per_rank

    # ---- BASELINE configs 3 and 5 and the 64 KiB batch of SURVEY.md 8d in the same run: one launch each over
    # arenas resident in HBM, three timed launches (HIP events), every stream verified (status, length, in_used, Adler-32, every
    # byte) on a run over poisoned outputs; each with its own algorithmic bytes and roofline fraction.
    if rank == 0 and world == 1 and args.full and not args.no_variants and args.workload == "l6_32k":
        from devbatch import DeviceBatch

        def variant(name, what, texts_v, zs_v, count, seed, profile=None):
            pick_v = np.random.default_rng(seed).integers(0, len(zs_v), size=count)
            vb = DeviceBatch(texts_v, zs_v, pick_v, dev=local_rank)
            # (another kind of batch begins: the context looks for streams for the bundles again instead of waiting out the launches it
            # goes without looking after the headline's sixteen -- pzg.h PZG_OPT_BUNDLES; what an application that knows its data does)
            ctx.set_bundles(args.bundles if args.bundles >= 0 else 1)
            if profile is not None:
                ctx.set_profile(profile)
            ok_v = True
            try:
                vb.check_all(*vb.run(ctx, ring_bits))  # (poisons the arenas first; raises on any difference)
            except AssertionError as e:
                ok_v = False
                log(f"[bench] variant {name}: VERIFICATION FAILED {e}")
            ms_v = []
            for _ in range(3):
                ctx.decompress_many_device(vb.d_in.data_ptr(), vb.d_in_off.data_ptr(), vb.d_in_len.data_ptr(), vb.d_out.data_ptr(),
                                           vb.d_out_off.data_ptr(), vb.d_out_cap.data_ptr(), vb.d_out_len.data_ptr(), vb.d_status.data_ptr(),
                                           vb.d_detail.data_ptr(), vb.d_in_used.data_ptr(), vb.d_adler.data_ptr(), vb.n, sync=True)
                ms_v.append(ctx.last_kernel_ms())
            dec_b, comp_b = int(vb.out_cap.sum()), int(vb.in_len.sum())
            k = float(np.mean(ms_v))
            result[name] = {"workload": what, "streams": int(vb.n), "distinct_blobs": len(zs_v), "kernel_ms": round(k, 3),
                            "GiBps": round(dec_b / (k * 1e-3) / 2**30, 2), "compressed_GiBps": round(comp_b / (k * 1e-3) / 2**30, 2),
                            "algorithmic_bytes_per_launch": dec_b + comp_b, "achieved_GBps": round((dec_b + comp_b) / (k * 1e-3) / 1e9, 2),
                            "frac": round((dec_b + comp_b) / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "bit_exact": ok_v,
                            "verified": "every stream: status, length, in_used, Adler-32, every byte (poisoned arenas)"}
            if profile is not None:
                result[name]["profile"] = "on" if profile else "off (PZG_OPT_PROFILE 0: pieces of equal length)"
                ctx.set_profile(True)
            del vb
            torch.cuda.empty_cache()
            return ok_v

        npv = min(args.pool, 1024)
        tv = [corpus.zipf_text(4096, s_) for s_ in range(npv)]
        zv = []
        for t_ in tv:
            co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
            zv.append(co.compress(t_) + co.flush())
        v_ok = variant("fixed_4k_variant", "BASELINE config 3: 65,536 x 4 KiB fixed-Huffman (Z_FIXED level-1) blobs", tv, zv, 65536, 0xC3)
        tv = [corpus.zipf_text(1024 * (1 + (s_ * 2654435761 >> 7) % 64), s_) for s_ in range(npv)]
        zv = [zlib.compress(t_, 6) for t_ in tv]
        v_ok &= variant("mixed_share_variant", "BASELINE config 5's per-GPU share: 131,072 mixed 1-64 KiB level-6 blobs (1 M over 8 GPUs)",
                        tv, zv, 131072, 0xC5)
        tv = [corpus.zipf_text(65536, 5000 + s_) for s_ in range(npv)]
        zv = [zlib.compress(t_, 6) for t_ in tv]
        v_ok &= variant("blob_64k_variant", "SURVEY.md 8d: 32,768 x 64 KiB level-6 blobs (same code path, ring wrap)", tv, zv, 32768, 0xC6)
        # ... and a batch of mixed KINDS, with the stream-waves' profiles on and off: what the headline's "strips of equal work" are worth
        # when the streams of a batch do NOT resemble one another
        hv = [hetero_blob(s_) for s_ in range(min(args.pool, 768))]
        tv, zv = [h[0] for h in hv], [h[1] for h in hv]
        what_h = "32,768 blobs of mixed kinds: text / html / literal-heavy / binary-looking, 8-64 KiB, levels 1 / 6 / 9"
        v_ok &= variant("hetero_variant", what_h, tv, zv, 32768, 0xC7, profile=True)
        v_ok &= variant("hetero_variant_profile_off", what_h, tv, zv, 32768, 0xC7, profile=False)
        if not v_ok:
            bit_exact = False
            result["bit_exact"] = False

    # ---- the same batch handed over as HOST buffers (what a `decompress` caller pays): staging + H2D + kernel + D2H.
    # Reported beside `value`, never as `value` (which is measured with the arenas resident in HBM).
    if rank == 0 and world == 1 and args.full and not args.no_host_path:
        h_out = np.empty(int(d_out.numel()), dtype=np.uint8)
        ctx.decompress_many_raw(h_in, in_off, in_len, h_out, out_off, out_cap)  # warm the staging buffers

        def every_stream_equal(arena):
            """Every stream's bytes in a host output arena against the plaintext it was compressed from."""
            if len(set(dec_len.tolist())) == 1:
                width = int(dec_len[0])
                stride = (width + 255) // 256 * 256
                pool_np = np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(npool, width)
                got_np = arena[:n * stride].reshape(n, stride)[:, :width]
                return all(np.array_equal(got_np[lo:lo + 4096], pool_np[pick[lo:lo + 4096]]) for lo in range(0, n, 4096))
            return all(arena[int(out_off[k]):int(out_off[k]) + int(out_cap[k])].tobytes() == texts[pick[k]] for k in range(n))

        h_out[:] = 0xCD  # poisoned, then a call whose results are verified: EVERY stream's status, length and bytes
        o_len, o_st, _det, _used, _ad = ctx.decompress_many_raw(h_in, in_off, in_len, h_out, out_off, out_cap)
        ok_h = bool((o_st == 0).all() and (o_len == out_cap).all()) and (not verify or every_stream_equal(h_out))
        dts = []
        for _ in range(5):  # (median of five calls, every sample listed: VERDICT r4 item 5)
            t0h = time.perf_counter()
            o_len, o_st, _det, _used, _ad = ctx.decompress_many_raw(h_in, in_off, in_len, h_out, out_off, out_cap)
            dts.append(time.perf_counter() - t0h)
            ok_h = ok_h and bool((o_st == 0).all() and (o_len == out_cap).all())
        dth = float(np.median(dts))
        result["host_buffers_variant"] = {
            "GiBps": round(int(out_cap.sum()) / dth / 2**30, 2), "ms": round(dth * 1e3, 1), "ok": ok_h,
            "ms_samples": [round(x * 1e3, 1) for x in dts],
            "verified": "every stream: status, length and every byte, on a call over a poisoned arena",
            "note": "pageable host arenas in and out through pzg_decompress_many without PZG_DEVICE_PTRS: "
                    "pinned staging + PCIe both ways + kernel, one call (median of five)",
        }
        del h_out
        # ... and as PAGE-LOCKED arenas (pzg_host_alloc + PZG_HOST_PINNED: what the module mirrors hand over): the copy engines
        # read and write the caller's memory, nothing is packed or copied out
        try:
            from pure_zlib_amd.zlib import PinnedArena
            p_in, p_out = PinnedArena(h_in.size), PinnedArena(int(d_out.numel()))
            p_in.a[:] = h_in
            ctx.decompress_many_raw(p_in.a, in_off, in_len, p_out.a, out_off, out_cap, pinned=True)  # allocates the device mirrors
            p_out.a[:] = 0xCD  # poisoned, then a call whose results are verified ...
            o_len, o_st, _det, _used, o_ad = ctx.decompress_many_raw(p_in.a, in_off, in_len, p_out.a, out_off, out_cap, pinned=True)
            ok_p = bool((o_st == 0).all() and (o_len == out_cap).all() and (o_ad == exp_adler).all()) if verify else None
            if ok_p:
                ok_p = every_stream_equal(p_out.a)
            dtps = []
            for _ in range(5):  # ... then five timed ones over the arena as it stands (freshly CPU-written lines slow the copy engine's writes down)
                t0h = time.perf_counter()
                o_len, o_st, _det, _used, o_ad = ctx.decompress_many_raw(p_in.a, in_off, in_len, p_out.a, out_off, out_cap, pinned=True)
                dtps.append(time.perf_counter() - t0h)
                if ok_p is not None:
                    ok_p = ok_p and bool((o_st == 0).all() and (o_ad == exp_adler).all())
            dtp = float(np.median(dtps))
            result["host_buffers_variant"]["pinned"] = {
                "GiBps": round(int(out_cap.sum()) / dtp / 2**30, 2), "ms": round(dtp * 1e3, 1), "ok": ok_p,
                "ms_samples": [round(x * 1e3, 1) for x in dtps],
                "note": "the same batch in page-locked arenas (pzg_host_alloc) with PZG_HOST_PINNED: PCIe both ways + kernel, no staging copy "
                        "(median of five; every stream's bytes verified on a call over a poisoned arena)",
            }
            p_in.close()
            p_out.close()
        except MemoryError as e:
            result["host_buffers_variant"]["pinned"] = {"skipped": str(e)}

    # ---- the incremental path (Benchmark.hs:53-70): 4,096 resumable decoders fed 32 KiB pieces,
    # host buffers both ways, one launch per feed call.  Reported beside `value`, never as it.
    if rank == 0 and world == 1 and args.full and args.incremental_decoders > 0 and not args.no_host_path:
        from pure_zlib_amd import benchmark as HB
        inc_plain = [corpus.zipf_text(256 * 1024, 7000 + k) for k in range(32)]
        inc_z = [zlib.compress(t, 6) for t in inc_plain]
        result["incremental_variant"] = HB.incremental_throughput(ctx, inc_z, inc_plain, n_decoders=args.incremental_decoders)
        result["incremental_variant"]["note"] = ("pzg_decoder_feed: resumable decoders on the device (4 KiB LDS ring + a 32 KiB history per decoder in "
                                                 "HBM, 16 decoders per CU; a feed is pipelined in 8 ranges), 256 KiB level-6 text streams; time = the feed "
                                                 "calls only (pack + H2D + launch + D2H + copy-out)")

    # ---- CPU baseline, rank 0 at N=1 only: the oracle ("port": the bit-at-a-time restatement of pure-zlib) and system
    # zlib, on this box's host cores.  All cores: the WHOLE timed batch.  One thread: a bounded sample of it (the whole
    # batch would take most of a minute per decoder).  A reported baseline, not a target.
    if rank == 0 and world == 1 and args.full and args.cpu_sample > 0:
        from oracle import oracle as O
        L = O.lib()
        cores = os.cpu_count() or 1
        nthreads = max(1, min(cores, args.cpu_threads or cores))

        import ctypes as C
        for fn in (L.pzo_decompress_many_mt, L.pzo_zlib_many_mt):  # oracle/pz_baseline_mt.c: POSIX threads over the batch layout
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p]
            fn.restype = C.c_uint32
        u_off, u_len, u_cap = (np.ascontiguousarray(a, dtype=np.uint64) for a in (in_off, in_len, out_cap))
        cpu_adler = np.zeros(n, dtype=np.uint32)  # the Adler-32 each CPU decoder computed over ITS output, per stream

        def timed(fn, count, threads):
            nb = C.c_uint64(0)
            cpu_adler[:] = 0
            t0 = time.perf_counter()
            bad = fn(h_in.ctypes.data, u_off.ctypes.data, u_len.ctypes.data, u_cap.ctypes.data, count, threads, C.byref(nb),
                     cpu_adler.ctypes.data)
            dt = time.perf_counter() - t0
            if bad:
                raise SystemExit(f"the CPU baseline rejected {bad} bench stream(s)")
            return int(nb.value), dt

        def cpu_quota():
            """What the box grants this process: cgroup CPU quota (cores' worth of time) and the affinity mask's size."""
            q = None
            try:
                with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2: "<quota> <period>" or "max <period>"
                    a, b = f.read().split()
                    q = None if a == "max" else round(int(a) / int(b), 2)
            except Exception:
                try:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                        a, b = int(f.read()), int(g.read())
                        q = None if a < 0 else round(a / b, 2)
                except Exception:
                    pass
            try:
                aff = len(os.sched_getaffinity(0))
            except Exception:
                aff = None
            return q, aff

        m1 = min(args.cpu_sample, n)
        nb_o1, dt_o1 = timed(L.pzo_decompress_many_mt, m1, 1)
        nb_z1, dt_z1 = timed(L.pzo_zlib_many_mt, m1, 1)
        # all cores: the box may hand this process less than its logical CPU count (quota), so a few thread counts are
        # tried on the whole batch and the best one is what is reported, with its thread count
        best = None
        gpu_vs_port = verify and not args.gzip
        for th in sorted({nthreads, max(1, nthreads // 2), max(1, nthreads // 4), min(nthreads, 32), min(nthreads, 16)}, reverse=True):
            nb_o, dt_o = timed(L.pzo_decompress_many_mt, n, th)
            # GPU output against the restatement on EVERY stream of the timed batch -- the oracle's per-stream
            # Adler-32 (computed over the bytes the oracle itself produced) against the adler[] the kernel returned
            gpu_vs_port = gpu_vs_port and nb_o == int(out_cap.sum()) and bool((cpu_adler == adler).all())
            if best is None or nb_o / dt_o > best[0] / best[1]:
                best = (nb_o, dt_o, th)
        nb_oa, dt_oa, nthreads = best
        nb_za, dt_za = timed(L.pzo_zlib_many_mt, n, nthreads)
        quota, affinity = cpu_quota()
        model = ""
        try:
            with open("/proc/cpuinfo") as f:
                model = next(ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name"))
        except Exception:
            pass
        result["cpu_baseline"] = {
            "value": round(nb_oa / dt_oa / 2**30, 3),
            "unit": "GiB/s",
            "cores": nthreads,
            "kind": "port",
            "sample": f"all {n} streams of the timed batch ({nb_oa / 2**20:.0f} MiB decoded) through oracle/pz_oracle.c on {nthreads} "
                      f"threads, {dt_oa:.1f}s",
            "one_thread_GiBps": round(nb_o1 / dt_o1 / 2**30, 4),
            "one_thread_sample": f"first {m1} streams ({nb_o1 / 2**20:.0f} MiB), {dt_o1:.1f}s",
            "system_zlib_all_cores_GiBps": round(nb_za / dt_za / 2**30, 2),
            "system_zlib_one_thread_GiBps": round(nb_z1 / dt_z1 / 2**30, 3),
            "gpu_equals_port_on_every_stream": gpu_vs_port,
            "gpu_vs_port_check": f"per-stream Adler-32 + length of all {n} streams of the timed batch: the oracle's own checksum over its "
                                 "own output vs the kernel's adler[] (beside the full byte compare with the plaintext above)",
            "host": model,
            "host_cores_available": cores,
            "cgroup_cpu_quota_cores": quota,
            "sched_affinity_cpus": affinity,
            "cores_note": "cores = the thread count with the best all-core rate among {all, 1/2, 1/4, 32, 16}; the box's cgroup quota / "
                          "affinity (above; null = unlimited) is what keeps it below host_cores_available",
            "note": "the Haskell reference itself cannot run here (no GHC); README.md:6-8 of the reference puts it ~100x below C zlib. "
                    "system zlib = libz's uncompress() on the same batch and threads (oracle/pz_baseline_mt.c).",
        }

    # ---- BASELINE config 2: Adler-32 over one large buffer (HBM-bound microbench) -------------------
    if rank == 0 and world == 1 and args.full and args.adler_gib > 0:
        nb = int(args.adler_gib * 2**30)
        free, _tot = torch.cuda.mem_get_info()
        nb = min(nb, int(free * 0.8))
        nb &= ~7
        buf = torch.empty(nb, dtype=torch.uint8, device=dev)
        chunk = 1 << 28
        # byte i = byte (i & 7) of splitmix64(0x5EED0002 + (i >> 3)), little-endian; filled on the device
        words = buf.view(torch.int64)
        for lo in range(0, nb // 8, chunk // 8):
            hi = min(nb // 8, lo + chunk // 8)
            words[lo:hi] = corpus.splitmix64_torch(lo, hi - lo, dev)
        gen_ok = all(np.array_equal(buf[lo:lo + 4096].cpu().numpy(), corpus.splitmix64_numpy(lo // 8, 512).view(np.uint8))
                     for lo in (0, (nb // 2) & ~7, nb - 4096))  # the CPU generator, same definition, at three places
        d_res = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(2):
            ctx.adler32_device(buf.data_ptr(), nb, d_res.data_ptr(), sync=True)
        ms = []
        for _ in range(10):
            ctx.adler32_device(buf.data_ptr(), nb, d_res.data_ptr(), sync=True)
            ms.append(ctx.last_kernel_ms())
        got = int(d_res.cpu().numpy().view(np.uint32)[0])
        exp = 1
        for lo in range(0, nb, chunk):
            exp = zlib.adler32(buf[lo:lo + chunk].cpu().numpy().tobytes(), exp)
        med = float(np.median(ms))
        result["adler32_microbench"] = {
            "workload": f"BASELINE config 2: Adler-32 over one {nb / 2**30:.1f} GiB device buffer",
            "GBps": round(nb / (med * 1e-3) / 1e9, 1),
            "frac_of_8000": round(nb / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "frac_of_measured_copy_6290": round(nb / (med * 1e-3) / 1e9 / HBM_MEASURED_GBS, 4),
            "kernel_ms_median": round(med, 3),
            "matches_zlib_adler32": bool(got == exp),
            "buffer": "splitmix64(0x5EED0002 + (i >> 3)) bytes, little-endian (SURVEY.md 8d); device fill == CPU generator: " + str(gen_ok),
        }
        # ... and its batched form: 64 KiB buffers, one wave each, pzg_adler32_many
        nbuf = nb // 65536
        if nbuf >= 1024:
            d_off = torch.arange(nbuf, dtype=torch.int64, device=dev) * 65536
            d_len = torch.full((nbuf,), 65536, dtype=torch.int64, device=dev)
            d_many = torch.zeros(nbuf, dtype=torch.int32, device=dev)
            msb = []
            for it in range(6):
                ctx.adler32_many_device(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_many.data_ptr(), nbuf, sync=True)
                if it:
                    msb.append(ctx.last_kernel_ms())
            gotb = d_many.cpu().numpy().view(np.uint32)
            ks = np.random.default_rng(9).integers(0, nbuf, size=64)
            okb = all(int(gotb[k]) == zlib.adler32(buf[int(k) * 65536:(int(k) + 1) * 65536].cpu().numpy().tobytes()) for k in ks)
            medb = float(np.median(msb))
            result["adler32_microbench"]["batched"] = {
                "workload": f"{nbuf} x 64 KiB buffers, one wave each",
                "GBps": round(nbuf * 65536 / (medb * 1e-3) / 1e9, 1),
                "frac_of_8000": round(nbuf * 65536 / (medb * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "kernel_ms_median": round(medb, 3),
                "matches_zlib_adler32": bool(okb),
            }
        del buf

    if rank == 0:
        print(json.dumps(result), flush=True)
    ctx.close()
    if world > 1:
        dist.destroy_process_group()
    if bit_exact is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
