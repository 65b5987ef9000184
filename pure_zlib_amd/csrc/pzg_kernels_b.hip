// pzg_kernels_b.hip -- the kernels that are compiled WITHOUT the compiler's SDWA peephole (Makefile: KERNELFLAGS_B):
//
//   inflate_resume_kernel           the resumable decoder (decompressIncremental); resume_gzip_kernel, resume_raw_kernel: its gzip and raw forms
//   inflate_kernel<RB, *, true>     the gzip instances
//   inflate_raw_kernel<RB, *>       the raw instances
//   inflate_seg_kernel              the segment instance (indexed streams), and index_windows_kernel beside it
//   scan_find / scan_decode / scan_resolve_kernel   the parallel index scan (scan_core.h)
//   scan_many_find / _decode / _resolve_kernel      the same over many streams in one launch (scan_core.h ScanMany)
//   member_* / sums_*_kernel        the members of a gzip file, found and laid out (member_core.h)
//
// SDWA forms save a vector instruction here and there (an extract folded into an add) but take their operands from registers
// only: with the peephole on, a dozen small constants live in vector registers from the kernel's first line to its last.  The
// zlib instances pay that and are ~1 % faster for it (measured, round 5: 301.6 vs 298.6 GiB/s on the headline batch).  These two
// have more state: without it the resumable kernel needs no scratch memory (12 spilled vector registers with it) and runs
// 27 % faster (31.1 vs 24.4 GiB/s, bench.py's incremental leg), and the ring-11 gzip instance fits 72 registers (80 and one spill).
#include "pzg_inflate_kernel.h"
#include "member_core.h"
#include "scan_core.h"

namespace pzg {

hipError_t launch_inflate_gzip(const InflateArgs &a, int ring_bits, bool fixup, uint32_t waves, hipStream_t stream)
{
    dim3 grid(waves), block(64);
    if (fixup)
        hipLaunchKernelGGL((inflate_kernel<15, true, true>), grid, block, 0, stream, a);
    else if (ring_bits == 15)
        hipLaunchKernelGGL((inflate_kernel<15, false, true>), grid, block, 0, stream, a);
    else if (ring_bits == 14)
        hipLaunchKernelGGL((inflate_kernel<14, false, true>), grid, block, 0, stream, a);
    else if (ring_bits == 13)
        hipLaunchKernelGGL((inflate_kernel<13, false, true>), grid, block, 0, stream, a);
    else if (ring_bits == 12)
        hipLaunchKernelGGL((inflate_kernel<12, false, true>), grid, block, 0, stream, a);
    else if (ring_bits == 11)
        hipLaunchKernelGGL((inflate_kernel<11, false, true>), grid, block, 0, stream, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// The raw instances (PZG_RAW).  Here and not beside the zlib instances by their code objects' notes (profiles/raw_kernel_notes.txt).
hipError_t launch_inflate_raw(const InflateArgs &a, int ring_bits, bool fixup, uint32_t waves, hipStream_t stream)
{
    dim3 grid(waves), block(64);
    if (fixup)
        hipLaunchKernelGGL((inflate_raw_kernel<15, true>), grid, block, 0, stream, a);
    else if (ring_bits == 15)
        hipLaunchKernelGGL((inflate_raw_kernel<15, false>), grid, block, 0, stream, a);
    else if (ring_bits == 14)
        hipLaunchKernelGGL((inflate_raw_kernel<14, false>), grid, block, 0, stream, a);
    else if (ring_bits == 13)
        hipLaunchKernelGGL((inflate_raw_kernel<13, false>), grid, block, 0, stream, a);
    else if (ring_bits == 12)
        hipLaunchKernelGGL((inflate_raw_kernel<12, false>), grid, block, 0, stream, a);
    else if (ring_bits == 11)
        hipLaunchKernelGGL((inflate_raw_kernel<11, false>), grid, block, 0, stream, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Indexed streams (pzg_index_build / pzg_decompress_many_segments).  The segment instance: the raw kernel's persistent stream-waves
// around Decoder<15, false, false, true, true> -- a segment starts at a bit inside its first byte, ends with the block that ends at its
// end bit, and has the 32 KiB in front of it as its dictionary; the index build is ONE such "segment", the whole stream, that records
// the access points as it goes.  The 32 KiB ring only (a dictionary is history on that ring alone), without the token scratch, as
// the fixup pass.
__global__ __launch_bounds__(64, waves_per_simd(15)) void inflate_seg_kernel(InflateArgs)
{
    typedef Decoder<15, false, false, true, true> SegDecoder;
    __shared__ WaveLds<15> lds;
    if (threadIdx.x == 0) lds.fixed_ready = 0u;  // LDS is not zeroed at launch
    __syncthreads();
    for (;;) {
        uint32_t i = 0, npoints = 0;
        StreamResult r;
        {
            LaunchArgs a = launch_args();
            if (threadIdx.x == 0) i = atomicAdd(a->counter, 1u);
            i = uni(i);
            if (i >= a->n) break;
            if (a->order) i = a->order[i];
            SegDecoder dec(lds);
            uint32_t *none = nullptr;  // (made opaque: see inflate_raw_kernel)
            asm volatile("" : "+s"(none));
            dec.strip = none;
            const uint8_t *dict = nullptr;
            uint32_t dict_len = 0;
            if (a->dict_len) {
                const uint64_t dl = a->dict_len[i];
                dict = a->dict_base + a->dict_off[i];
                dict_len = uni(dl > 0xffffffffull ? 0xffffffffu : (uint32_t)dl);
            }
            dec.seg_start = a->seg_start_bit ? uni((uint32_t)a->seg_start_bit[i]) : 0u;
            dec.seg_end = a->seg_end_bit ? uni64(a->seg_end_bit[i]) : 0ull;
            dec.idx_points = (IndexPoint *)(void *)a->idx_points;
            dec.idx_cap = a->idx_cap;
            dec.idx_span = a->idx_points ? a->idx_span : 0ull;
            dec.run(a->in_base + a->in_off[i], a->in_len[i], a->out_base + a->out_off[i], a->out_cap[i], &r, dict, dict_len);
            npoints = dec.idx_n;
        }
        LaunchArgs a = launch_args();
        if (threadIdx.x == 0) {
            a->status[i] = r.status;
            a->out_len[i] = r.out_len;
            if (a->detail) {
                a->detail[2 * (size_t)i] = r.detail0;
                a->detail[2 * (size_t)i + 1] = r.detail1;
            }
            if (a->in_used) a->in_used[i] = r.in_used;
            if (a->adler) a->adler[i] = r.adler;  // (PZG_CRC32: crc32_report_kernel then writes the CRC-32 over it)
            if (a->idx_count) *a->idx_count = npoints;
        }
        __syncthreads();
    }
}

hipError_t launch_inflate_seg(const InflateArgs &a, uint32_t waves, hipStream_t stream)
{
    hipLaunchKernelGGL(inflate_seg_kernel, dim3(waves), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// One workgroup per stored point (grid-stride): w = min(out_pos, 32768) bytes out[out_pos - w .. out_pos) to the end of the point's slot.
// Bytes up to the first 16-byte boundary of the destination, then a vector per lane (the source is wherever it is), then a byte tail.
__global__ __launch_bounds__(256) void index_windows_kernel(const uint8_t *out, const uint64_t *out_cap, const uint64_t *points, const uint32_t *count,
                                                            uint32_t cap, const int32_t *status, uint8_t *windows)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (*status != ST_OK) return;
    const uint32_t n = *count < cap ? *count : cap;
    const uint64_t room = *out_cap;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t pos = points[2 * (size_t)k + 1];
        if (pos > room) continue;  // (never with status 0: nothing outside the output is ever read)
        const uint32_t w = pos < 32768u ? (uint32_t)pos : 32768u;
        const uint8_t *src = out + (pos - w);
        uint8_t *dst = windows + (size_t)k * 32768u + (32768u - w);
        uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
        head = head < w ? head : w;
        const uint32_t nv = (w - head) >> 4;
        for (uint32_t t = threadIdx.x; t < head; t += blockDim.x) dst[t] = src[t];
        for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
            u32x4 x;
            __builtin_memcpy(&x, src + head + 16u * v, 16);
            *(u32x4 *)(void *)(dst + head + 16u * v) = x;
        }
        for (uint32_t t = head + 16u * nv + threadIdx.x; t < w; t += blockDim.x) dst[t] = src[t];
    }
}

hipError_t launch_index_windows(const uint8_t *out, const uint64_t *out_cap, const uint64_t *points, const uint32_t *count, uint32_t cap,
                                const int32_t *status, uint8_t *windows, hipStream_t stream)
{
    if (cap == 0u || !windows) return hipSuccess;
    hipLaunchKernelGGL(index_windows_kernel, dim3(cap < 4096u ? cap : 4096u), dim3(256), 0, stream, out, out_cap, points, count, cap, status, windows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The parallel index scan (pzg_index_scan; scan_core.h): a wave per chunk finds a candidate block start, a wave per candidate decodes
// over markers until it lands on a later candidate, one workgroup walks the chain and writes the points and their windows.
__device__ __forceinline__ void scan_input(const ScanArgs &a, const uint32_t *&src, uint64_t &ndw, uint32_t &mis_bits, uint64_t &end_bit)
{
    const uint32_t mis = (uint32_t)((uintptr_t)a.in & 3u);
    src = (const uint32_t *)(const void *)(a.in - mis);
    ndw = (mis + a.in_len + 3u) >> 2;
    mis_bits = 8u * mis;
    end_bit = 8u * (mis + a.in_len);
}

__global__ __launch_bounds__(64) void scan_find_kernel(ScanArgs a)
{
    __shared__ ScanLds lds;
    const uint32_t k = blockIdx.x;
    if (k >= a.nchunks) return;
    uint64_t q = 0;
    if (k) {
        const uint32_t *src;
        uint64_t ndw, end_bit;
        uint32_t mis_bits;
        scan_input(a, src, ndw, mis_bits, end_bit);
        const uint64_t from = 8u * k * a.chunk, all = 8u * a.in_len;
        const uint64_t to = from + 8u * a.chunk < all ? from + 8u * a.chunk : all;
        q = Scan::find(lds, src, ndw, end_bit, from + mis_bits, to + mis_bits);
        if (q != Scan::NONE) q -= mis_bits;
    }
    if (threadIdx.x == 0) a.cand[k] = q;
}

__global__ __launch_bounds__(64) void scan_decode_kernel(ScanArgs a)
{
    __shared__ ScanLds lds;
    const uint32_t k = blockIdx.x;
    if (k >= a.nchunks) return;
    const uint32_t *src;
    uint64_t ndw, end_bit;
    uint32_t mis_bits;
    scan_input(a, src, ndw, mis_bits, end_bit);
    Scan::decode(lds, src, ndw, mis_bits, end_bit, a.cand, a.nchunks, k, a.rings + (size_t)k * Scan::RING, a.next, a.count, a.endbit);
}

__global__ __launch_bounds__(1024) void scan_resolve_kernel(ScanArgs a)
{
    Scan::resolve(threadIdx.x, blockDim.x, a.cand, a.next, a.count, a.endbit, a.rings, a.nchunks, a.span, a.wbuf, a.points, a.max_points,
                  a.windows, a.result);
}

size_t scan_scratch_bytes(uint32_t nchunks)
{
    // per chunk: the ring (64 KiB) and 32 bytes -- cand, count, endbit (8 each), next (4), 4 to spare; the chain walk's two windows
    // (64 KiB) and 256 bytes of slack: the figure include/pzg.h documents
    return (size_t)nchunks * (2u * Scan::RING + 32u) + 2u * Scan::RING + 256u;
}

hipError_t launch_scan(ScanArgs a, uint8_t *scratch, hipStream_t stream)
{
    const size_t n = a.nchunks;
    a.rings = (uint16_t *)(void *)scratch;
    uint8_t *p = scratch + n * 2u * Scan::RING;
    a.wbuf = p;
    p += 2u * Scan::RING;
    a.cand = (uint64_t *)(void *)p;
    a.count = a.cand + n;
    a.endbit = a.count + n;
    a.next = (uint32_t *)(void *)(a.endbit + n);
    hipLaunchKernelGGL(scan_find_kernel, dim3(a.nchunks), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(scan_decode_kernel, dim3(a.nchunks), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(scan_resolve_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

// ... of many streams in one launch (pzg_index_scan_many; scan_core.h ScanMany): the same three passes over the chunks of all streams
// as one list -- a wave finds its stream by a binary search over first_chunk -- and a workgroup per stream for the walk.
__global__ __launch_bounds__(64) void scan_many_find_kernel(ScanManyArgs a)
{
    __shared__ ScanLds lds;
    if (blockIdx.x >= a.nchunks) return;
    ScanMany::find(lds, a.in_base, a.streams, a.first_chunk, a.n, a.chunk, blockIdx.x, a.cand);
}

__global__ __launch_bounds__(64) void scan_many_decode_kernel(ScanManyArgs a)
{
    __shared__ ScanLds lds;
    if (blockIdx.x >= a.nchunks) return;
    ScanMany::decode(lds, a.in_base, a.streams, a.first_chunk, a.n, blockIdx.x, a.cand, a.rings, a.next, a.count, a.endbit);
}

__global__ __launch_bounds__(1024) void scan_many_resolve_kernel(ScanManyArgs a)
{
    if (blockIdx.x >= a.n) return;
    ScanMany::resolve(threadIdx.x, blockDim.x, a.streams, a.first_chunk, blockIdx.x, a.cand, a.next, a.count, a.endbit, a.rings, a.span, a.wbuf,
                      a.points, a.windows, a.results);
}

// the tables the host uploads in one piece: n stream entries, then first_chunk (n + 1 entries), padded to the results' alignment
size_t scan_many_table_bytes(uint32_t n) { return sizeof(ScanStream) * (size_t)n + ((4u * ((size_t)n + 1u) + 7u) & ~(size_t)7u); }

size_t scan_many_scratch_bytes(uint32_t n, uint32_t nchunks)
{
    // per chunk: the ring (64 KiB) and 32 bytes -- cand, count, endbit (8 each), next (4), 4 to spare; per stream: the chain walk's two
    // windows (64 KiB) and 256 bytes -- its entry (32), its result (32), its first_chunk (4, and 4 of the table's last entry), the
    // rest to spare: the figure include/pzg.h documents
    return (size_t)nchunks * (2u * Scan::RING + 32u) + (size_t)n * (2u * Scan::RING + 256u);
}

void scan_many_layout(ScanManyArgs &a, uint8_t *scratch)
{
    static_assert(sizeof(ScanStream) == 32 && sizeof(ScanResult) == 32, "the per-stream entries");
    const size_t nc = a.nchunks, n = a.n;
    a.rings = (uint16_t *)(void *)scratch;
    uint8_t *p = scratch + nc * 2u * Scan::RING;
    a.wbuf = p;
    p += n * 2u * Scan::RING;
    a.cand = (uint64_t *)(void *)p;
    a.count = a.cand + nc;
    a.endbit = a.count + nc;
    a.next = (uint32_t *)(void *)(a.endbit + nc);
    p += 32u * nc;
    a.streams = (ScanStream *)(void *)p;
    a.first_chunk = (uint32_t *)(void *)(a.streams + n);
    a.results = (ScanResult *)(void *)(p + scan_many_table_bytes(a.n));
}

hipError_t launch_scan_many(const ScanManyArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(scan_many_find_kernel, dim3(a.nchunks), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(scan_many_decode_kernel, dim3(a.nchunks), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(scan_many_resolve_kernel, dim3(a.n), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The members of a gzip file (pzg_gzip_find_members, pzg_gzip_layout; member_core.h).  Bandwidth-bound sweeps and prefix sums: a
// workgroup is one wave, the grids stride over their chunks, tiles and members.
constexpr uint32_t MEMBER_GRID = 1u << 16;

__global__ __launch_bounds__(64) void member_count_kernel(MemberArgs a)
{
    for (uint64_t k = blockIdx.x; k < a.nchunks; k += gridDim.x) {
        const uint64_t n = Members::chunk_sweep<false>(a.in, a.in_len, a.chunk, k, 0u, nullptr, nullptr, 0u);
        if (threadIdx.x == 0) a.counts[k] = n;
    }
}

__global__ __launch_bounds__(64) void member_write_kernel(MemberArgs a)
{
    for (uint64_t k = blockIdx.x; k < a.nchunks; k += gridDim.x)
        Members::chunk_sweep<true>(a.in, a.in_len, a.chunk, k, uni64(a.counts[k]), a.starts, a.bsize, a.max_members);
}

__global__ __launch_bounds__(64) void sums_tile_kernel(const uint64_t *x, uint64_t n, uint64_t *part)
{
    for (uint64_t t = blockIdx.x; t < Members::tiles(n); t += gridDim.x) Members::tile_sum(x, n, t, part);
}

__global__ __launch_bounds__(64) void sums_offsets_kernel(uint64_t *part, uint64_t ntiles, uint64_t base, uint64_t *total)
{
    Members::tile_offsets(part, ntiles, base, total);
}

__global__ __launch_bounds__(64) void sums_scan_kernel(const uint64_t *x, uint64_t n, const uint64_t *part, uint64_t *out)
{
    for (uint64_t t = blockIdx.x; t < Members::tiles(n); t += gridDim.x) Members::tile_scan(x, n, t, part, out);
}

__global__ __launch_bounds__(256) void member_layout_kernel(LayoutArgs a)
{
    Members::Input I;
    I.init(a.in, a.in_len);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * blockDim.x)
        Members::member(I, a.starts, a.m, j, a.in_off, a.in_lenv, a.out_cap);
}

// out[i] = base + x[0] + ... + x[i - 1] (out may be x), *total = the sum of all n; part: tiles(n) entries of scratch
static hipError_t launch_sums(const uint64_t *x, uint64_t n, uint64_t base, uint64_t *out, uint64_t *part, uint64_t *total, hipStream_t stream)
{
    const uint64_t nt = Members::tiles(n);
    const dim3 grid((uint32_t)(nt < MEMBER_GRID ? nt : MEMBER_GRID));
    hipLaunchKernelGGL(sums_tile_kernel, grid, dim3(64), 0, stream, x, n, part);
    hipLaunchKernelGGL(sums_offsets_kernel, dim3(1), dim3(64), 0, stream, part, nt, base, total);
    hipLaunchKernelGGL(sums_scan_kernel, grid, dim3(64), 0, stream, x, n, (const uint64_t *)part, out);
    return hipGetLastError();
}

size_t members_find_scratch_bytes(uint64_t nchunks)
{
    // per chunk its count, then its offset (8 bytes); per 4,096 chunks their sum (8 bytes); the total: the figure include/pzg.h documents
    return (size_t)(8u * nchunks + 8u * Members::tiles(nchunks) + 8u);
}

hipError_t launch_members_find(MemberArgs a, uint8_t *scratch, hipStream_t stream)
{
    a.counts = (uint64_t *)(void *)scratch;
    uint64_t *part = a.counts + a.nchunks;
    a.total = part + Members::tiles(a.nchunks);
    const dim3 grid((uint32_t)(a.nchunks < MEMBER_GRID ? a.nchunks : MEMBER_GRID));
    hipLaunchKernelGGL(member_count_kernel, grid, dim3(64), 0, stream, a);
    hipError_t e = launch_sums(a.counts, a.nchunks, 0u, a.counts, part, a.total, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(member_write_kernel, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}
const uint64_t *members_find_total(uint64_t nchunks, const uint8_t *scratch)
{
    return (const uint64_t *)(const void *)scratch + nchunks + Members::tiles(nchunks);
}

size_t members_layout_scratch_bytes(uint64_t m) { return (size_t)(8u * Members::tiles(m) + 8u); }

hipError_t launch_members_layout(const LayoutArgs &a, uint8_t *scratch, hipStream_t stream)
{
    uint64_t *part = (uint64_t *)(void *)scratch, *total = part + Members::tiles(a.m);
    const uint64_t blocks = (a.m + 255u) / 256u;
    hipLaunchKernelGGL(member_layout_kernel, dim3((uint32_t)(blocks < MEMBER_GRID ? blocks : MEMBER_GRID)), dim3(256), 0, stream, a);
    return launch_sums(a.out_cap, a.m, a.out_base_off, a.out_off, part, total, stream);
}
const uint64_t *members_layout_total(uint64_t m, const uint8_t *scratch) { return (const uint64_t *)(const void *)scratch + Members::tiles(m); }

// ------------------------------------------------------------------------------------------------
// The resumable decoder (decompressIncremental, Monad.hs:163-197): one launch continues a batch of suspended decoders,
// one wave each, as far as their new input and output room go.  Round 4: the small-ring instance (PZG_RES_RING = 12: 8 KiB
// of LDS, four waves per SIMD, 16 decoders per CU where the 32 KiB LDS ring allowed 4).  What is older than the ring comes
// from the decoder's own 32 KiB history in HBM (every flush writes there as well as to the call's room), and a call saves /
// restores 8 KiB of LDS image instead of 37.
#ifndef PZG_RES_RING
#define PZG_RES_RING 12
#endif
#ifndef PZG_RES_WAVES_PER_SIMD
#define PZG_RES_WAVES_PER_SIMD 4
#endif
constexpr int RES_RING = PZG_RES_RING;
// What a stream-wave of the three resume kernels does; DEC is the zlib, the gzip or the raw instance of the resumable decoder.  One
// copy of the text, expanded in each kernel and not a __device__ function template that the three call: as a function -- the
// argument block handed over by reference, by value or as a pointer into the kernel-argument segment, all three were built -- the
// zlib kernel spilled a vector register (8 bytes of scratch per lane), which it does not when the body stands in the kernel itself
// and reads the kernel's own parameter.
#define PZG_RESUME_WAVE(DEC)  \
    __shared__ WaveLds<RES_RING> lds;                                                                                                    \
    for (;;) {                                                                                                                             \
        uint32_t i = 0;                                                                                                                    \
        if (threadIdx.x == 0) i = atomicAdd(a.counter, 1u);                                                                                \
        i = uni(i);                                                                                                                        \
        if (i >= a.n) break;                                                                                                               \
        uint8_t *slot = a.state_base + (size_t)i * a.state_stride;                                                                         \
        ResumeState *rs = (ResumeState *)slot;                                                                                             \
        uint32_t *image = (uint32_t *)(slot + ResumeSlot<RES_RING>::IMAGE_OFF);                                                            \
        DEC dec(lds);                                                                                                                      \
        if (a.strip && blockIdx.x < a.strip_waves) dec.strip = a.strip + (size_t)blockIdx.x * DEC::STRIP_WORDS;                            \
        StreamResult r;                                                                                                                    \
        uint32_t chunks = 0;                                                                                                               \
        dec.run_resume(rs, image, slot + ResumeSlot<RES_RING>::HIST_OFF, a.in_base + a.in_off[i], a.in_len[i], a.out_base + a.out_off[i],  \
                       a.out_cap[i], a.final_in ? (uint32_t)a.final_in[i] : 0u, &r, &chunks);                                              \
        if (threadIdx.x == 0) {                                                                                                            \
            a.status[i] = r.status;                                                                                                        \
            a.out_len[i] = r.out_len;                                                                                                      \
            a.in_used[i] = r.in_used;                                                                                                      \
            a.chunks[i] = chunks;                                                                                                          \
            if (a.adler) a.adler[i] = r.adler;                                                                                             \
            if (a.detail) {                                                                                                                \
                a.detail[2 * (size_t)i] = r.detail0;                                                                                       \
                a.detail[2 * (size_t)i + 1] = r.detail1;                                                                                   \
            }                                                                                                                              \
        }                                                                                                                                  \
        if (a.dense) {                                                                                                                     \
            /* what this decoder delivered, once more, behind what the others of its range delivered: the host then fetches ONE */         \
            /* linear span per range instead of rooms that are mostly empty (the bytes are this wave's own stores of a moment */           \
            /* ago: L2 hits; 64 lanes x 16 bytes per step, four steps in flight) */                                                        \
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));                                                                    \
            const uint32_t nv = (uint32_t)((r.out_len + 15u) >> 4);                                                                        \
            uint32_t at = 0;                                                                                                               \
            if (threadIdx.x == 0) at = atomicAdd(a.dense_cursor, nv);                                                                      \
            at = uni(at);                                                                                                                  \
            const uint64_t off = a.dense_region + 16ull * at;                                                                              \
            if (threadIdx.x == 0) a.dense_off[i] = off;                                                                                    \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  /* the flushes' stores have landed */                                        \
            const u32x4 *src = (const u32x4 *)(const void *)(a.out_base + a.out_off[i]);                                                   \
            u32x4 *dst = (u32x4 *)(void *)(a.dense + off);                                                                                 \
            for (uint32_t v0 = 0; v0 < nv; v0 += 256u) {                                                                                   \
                u32x4 t[4];                                                                                                                \
_Pragma("unroll")                                                                                                                          \
                for (uint32_t q = 0; q < 4u; ++q) {                                                                                        \
                    const uint32_t v = v0 + 64u * q + threadIdx.x;                                                                         \
                    t[q] = __builtin_nontemporal_load(src + (v < nv ? v : nv - 1u));                                                       \
                }                                                                                                                          \
_Pragma("unroll")                                                                                                                          \
                for (uint32_t q = 0; q < 4u; ++q) {                                                                                        \
                    const uint32_t v = v0 + 64u * q + threadIdx.x;                                                                         \
                    if (v < nv) dst[v] = t[q];                                                                                             \
                }                                                                                                                          \
            }                                                                                                                              \
        }                                                                                                                                  \
        __syncthreads();                                                                                                                   \
    }                                                                                                                                      \
    do {} while (0)
__global__ __launch_bounds__(64, RES_RING == 15 ? 1 : PZG_RES_WAVES_PER_SIMD) void inflate_resume_kernel(ResumeArgs a)
{
    typedef Decoder<RES_RING, false, true> Dec;
    PZG_RESUME_WAVE(Dec);
}
// The gzip and the raw decoders (pzg_decoder_create_format).  Names of their own, and no template instances of the kernel above: the
// zlib kernel stays the one kernel of its name in the code object.
// (the gzip instance keeps the header's and the trailers' state beside the decoder's: at four waves per SIMD, 128 vector registers,
// it spilled six of them -- 28 bytes of scratch per lane; three waves per SIMD, 168 registers, and nothing is spilled)
#ifndef PZG_RES_GZIP_WAVES_PER_SIMD
#define PZG_RES_GZIP_WAVES_PER_SIMD 3
#endif
__global__ __launch_bounds__(64, RES_RING == 15 ? 1 : PZG_RES_GZIP_WAVES_PER_SIMD) void resume_gzip_kernel(ResumeArgs a)
{
    typedef Decoder<RES_RING, true, true> Dec;
    PZG_RESUME_WAVE(Dec);
}
__global__ __launch_bounds__(64, RES_RING == 15 ? 1 : PZG_RES_WAVES_PER_SIMD) void resume_raw_kernel(ResumeArgs a)
{
    typedef Decoder<RES_RING, false, true, true> Dec;
    PZG_RESUME_WAVE(Dec);
}

static_assert(Decoder<RES_RING, true, true>::STRIP_WORDS == Decoder<RES_RING, false, true>::STRIP_WORDS &&
              Decoder<RES_RING, false, true, true>::STRIP_WORDS == Decoder<RES_RING, false, true>::STRIP_WORDS, "one slice size for the three kernels");
size_t resume_scalar_bytes() { return sizeof(ResumeState); }
size_t resume_state_bytes() { return ResumeSlot<RES_RING>::BYTES; }

static uint32_t resume_launch_waves_of(int num_cus, uint32_t n, uint32_t per_simd);
size_t resume_strip_wave_bytes() { return (size_t)Decoder<RES_RING, false, true>::STRIP_WORDS * sizeof(uint32_t); }
uint32_t resume_launch_waves(int num_cus, uint32_t n) { return resume_launch_waves_of(num_cus, n, PZG_RES_WAVES_PER_SIMD); }
static uint32_t resume_launch_waves_of(int num_cus, uint32_t n, uint32_t per_simd)
{
    constexpr uint32_t by_lds = (160u * 1024u) / (uint32_t)((sizeof(WaveLds<RES_RING>) + 511u) / 512u * 512u);
    const uint32_t by_vgpr = RES_RING == 15 ? 4u : 4u * per_simd;
    const uint32_t waves = (uint32_t)num_cus * (by_lds < by_vgpr ? by_lds : by_vgpr);
    return waves > n ? n : waves;
}

hipError_t launch_resume(const ResumeArgs &a, uint32_t format, int num_cus, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.counter, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(resume_launch_waves_of(num_cus, a.n, format == RESUME_FORMAT_GZIP ? PZG_RES_GZIP_WAVES_PER_SIMD : PZG_RES_WAVES_PER_SIMD)), block(64);
    if (format == RESUME_FORMAT_ZLIB)
        hipLaunchKernelGGL(inflate_resume_kernel, grid, block, 0, stream, a);
    else if (format == RESUME_FORMAT_GZIP)
        hipLaunchKernelGGL(resume_gzip_kernel, grid, block, 0, stream, a);
    else if (format == RESUME_FORMAT_RAW)
        hipLaunchKernelGGL(resume_raw_kernel, grid, block, 0, stream, a);
    else
        return hipErrorInvalidValue;
    e = hipGetLastError();
    if (e != hipSuccess || format != RESUME_FORMAT_GZIP) return e;
    return launch_resume_crc(a, num_cus, stream);  // the running CRC-32, before anything is downloaded
}

}  // namespace pzg
