// model_scan_many.cpp -- TEST INFRASTRUCTURE: the three passes of pzg_index_scan_many as a one-lane host program, through the code the
// kernels call (pure_zlib_amd/csrc/scan_core.h: ScanMany::locate / find / decode / resolve over Scan's passes), the way model_scan.cpp
// runs one stream.  Every buffer the core is handed has 64 guard bytes on both sides; a guard that changed is the call's return
// value.  Never linked into libpzg.so; the product has no CPU path.
// With -DPZSM_MAIN it is a program of its own (for a sanitizer build): model_scan_many BATCH scans the batch of that file (written
// by tests/scanmanycheck.py write_batch) at chunks 256 and 1024, spans 1 and 4096, and prints every stream's result.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/scan_core.h"

namespace {

constexpr size_t GUARD = 64;

struct Guarded {
    uint8_t *base = nullptr;
    size_t n = 0;
    explicit Guarded(size_t bytes) : n(bytes)
    {
        const size_t all = (2 * GUARD + n + 63u) & ~(size_t)63u;
        base = (uint8_t *)aligned_alloc(64, all);
        for (size_t i = 0; i < GUARD; ++i) base[i] = base[GUARD + n + i] = (uint8_t)(0x40u + i);
        memset(base + GUARD, 0xA5, n);  // device memory is not zeroed either
    }
    Guarded(const Guarded &) = delete;
    ~Guarded() { free(base); }
    uint8_t *p() const { return base + GUARD; }
    bool ok() const
    {
        for (size_t i = 0; i < GUARD; ++i)
            if (base[i] != (uint8_t)(0x40u + i) || base[GUARD + n + i] != (uint8_t)(0x40u + i)) return false;
        return true;
    }
};

}  // namespace

struct pzsm_result {
    int32_t status;
    uint32_t d0, d1, npoints;
    uint64_t out_len, in_used;
};

extern "C" {

uint32_t pzsm_chunks(uint64_t in_len, uint64_t chunk) { return in_len ? (uint32_t)((in_len + chunk - 1u) / chunk) : 1u; }

uint32_t pzsm_locate(const uint32_t *first_chunk, uint32_t n, uint32_t g) { return pzg::ScanMany::locate(first_chunk, n, g); }

// The whole scan of n streams packed in `in` (in_base is dword-aligned here: stream s lies in_off[s] & 3 bytes past a boundary).
// points (point_off[n] pairs) and windows (point_off[n] x 32768 bytes, or null) go in as the caller filled them and come back as the
// passes left them, every slot.  cand / next / count / endbit: the entries of all streams' chunks, stream after stream; may be null.
// Returns 0, or 1 + the number of the buffer whose guard changed.
int pzsm_scan_many(const uint8_t *in, uint64_t in_bytes, const uint64_t *in_off, const uint64_t *in_len, uint32_t n, uint64_t chunk, uint64_t span,
                   uint64_t *points, const uint32_t *point_off, uint8_t *windows, pzsm_result *results, uint64_t *cand_out, uint32_t *next_out,
                   uint64_t *count_out, uint64_t *endbit_out)
{
    using pzg::Scan;
    using pzg::ScanMany;
    std::vector<uint32_t> first(n + 1u);
    uint32_t total = 0;
    for (uint32_t s = 0; s < n; ++s) {
        first[s] = total;
        total += pzsm_chunks(in_len[s], chunk);
    }
    first[n] = total;
    const size_t slots = point_off[n];
    Guarded inp(in_bytes), lds(sizeof(pzg::ScanLds)), cand(8 * (size_t)total), next(4 * (size_t)total), count(8 * (size_t)total), endbit(8 * (size_t)total);
    Guarded rings(2 * (size_t)Scan::RING * total), wbuf(2 * (size_t)Scan::RING * n), pts(16 * slots), win(windows ? (size_t)Scan::RING * slots : 0);
    Guarded res(sizeof(pzg::ScanResult) * (size_t)n), streams(sizeof(pzg::ScanStream) * (size_t)n), fc(4 * ((size_t)n + 1u));
    if (in_bytes) memcpy(inp.p(), in, in_bytes);
    if (slots) memcpy(pts.p(), points, 16 * slots);
    if (windows && slots) memcpy(win.p(), windows, (size_t)Scan::RING * slots);
    memcpy(fc.p(), first.data(), 4 * ((size_t)n + 1u));
    pzg::ScanStream *st = (pzg::ScanStream *)(void *)streams.p();
    for (uint32_t s = 0; s < n; ++s) st[s] = pzg::ScanStream{in_off[s], in_len[s], point_off[s], point_off[s + 1] - point_off[s], 0u};
    pzg::ScanLds &L = *(pzg::ScanLds *)(void *)lds.p();
    const uint32_t *fcp = (const uint32_t *)(const void *)fc.p();
    uint64_t *cd = (uint64_t *)(void *)cand.p(), *ct = (uint64_t *)(void *)count.p(), *eb = (uint64_t *)(void *)endbit.p();
    uint32_t *nx = (uint32_t *)(void *)next.p();
    uint16_t *rg = (uint16_t *)(void *)rings.p();
    for (uint32_t g = 0; g < total; ++g) ScanMany::find(L, inp.p(), st, fcp, n, chunk, g, cd);
    for (uint32_t g = 0; g < total; ++g) ScanMany::decode(L, inp.p(), st, fcp, n, g, cd, rg, nx, ct, eb);
    for (uint32_t s = 0; s < n; ++s)
        ScanMany::resolve(0u, 1u, st, fcp, s, cd, nx, ct, eb, rg, span, wbuf.p(), (uint64_t *)(void *)pts.p(), windows ? win.p() : nullptr,
                          (pzg::ScanResult *)(void *)res.p());
    const Guarded *all[] = {&inp, &lds, &cand, &next, &count, &endbit, &rings, &wbuf, &pts, &win, &res, &streams, &fc};
    for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i)
        if (!all[i]->ok()) return 1 + (int)i;
    if (memcmp(inp.p(), in, in_bytes) != 0 || memcmp(fc.p(), first.data(), 4 * ((size_t)n + 1u)) != 0) return 100;  // (the passes' inputs)
    memcpy(results, res.p(), sizeof(pzsm_result) * (size_t)n);
    if (slots) memcpy(points, pts.p(), 16 * slots);
    if (windows && slots) memcpy(windows, win.p(), (size_t)Scan::RING * slots);
    if (cand_out) memcpy(cand_out, cand.p(), cand.n);
    if (next_out) memcpy(next_out, next.p(), next.n);
    if (count_out) memcpy(count_out, count.p(), count.n);
    if (endbit_out) memcpy(endbit_out, endbit.p(), endbit.n);
    return 0;
}
}

#ifdef PZSM_MAIN
// BATCH: little-endian uint64 n, in_bytes, in_off[n], in_len[n], point_off[n + 1]; then the in_bytes of input
int main(int argc, char **argv)
{
    static_assert(sizeof(pzsm_result) == sizeof(pzg::ScanResult), "the result block");
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
    fclose(f);
    if (d.size() < 16) return 2;
    uint64_t head[2];
    memcpy(head, d.data(), 16);
    const uint32_t n = (uint32_t)head[0];
    const size_t words = 2 + 3 * (size_t)n + 1;
    if (d.size() != 8 * words + head[1]) return 2;
    std::vector<uint64_t> w(words);
    memcpy(w.data(), d.data(), 8 * words);
    const uint64_t *in_off = w.data() + 2, *in_len = in_off + n;
    std::vector<uint32_t> point_off(n + 1u);
    for (uint32_t s = 0; s <= n; ++s) point_off[s] = (uint32_t)in_len[n + s];
    const uint64_t chunks[] = {256, 1024}, spans[] = {1, 4096};
    for (uint64_t chunk : chunks)
        for (uint64_t span : spans) {
            std::vector<uint64_t> pts(2 * (size_t)point_off[n], 0xCDCDCDCDCDCDCDCDull);
            std::vector<uint8_t> win((size_t)32768 * point_off[n], 0xCD);
            std::vector<pzsm_result> r(n);
            const int rc = pzsm_scan_many(d.data() + 8 * words, head[1], in_off, in_len, n, chunk, span, pts.data(), point_off.data(), win.data(), r.data(),
                                          nullptr, nullptr, nullptr, nullptr);
            if (rc) {
                printf("chunk %llu span %llu: rc %d\n", (unsigned long long)chunk, (unsigned long long)span, rc);
                return 1;
            }
            for (uint32_t s = 0; s < n; ++s)
                printf("chunk %llu span %llu stream %u: status %d d0 %u d1 %u npoints %u out_len %llu in_used %llu\n", (unsigned long long)chunk,
                       (unsigned long long)span, s, r[s].status, r[s].d0, r[s].d1, r[s].npoints, (unsigned long long)r[s].out_len,
                       (unsigned long long)r[s].in_used);
        }
    return 0;
}
#endif
