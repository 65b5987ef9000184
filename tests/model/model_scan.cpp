// model_scan.cpp -- TEST INFRASTRUCTURE: the three passes of pzg_index_scan (pure_zlib_amd/csrc/scan_core.h: block finder, marker
// pass, chain walk) as a one-lane host program, the way model_seg.cpp builds the segment decoder, so that the CPU suite can check
// them against system zlib without a GPU.  Every buffer the core is handed has 64 guard bytes on both sides; a guard that changed
// is the call's return value.  Never linked into libpzg.so; the product has no CPU path.
// With -DPZS_MAIN it is a program of its own (for a sanitizer build): model_scan FILE... scans every file at three chunk sizes.
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

// the input at `mis` bytes past a dword boundary, as a device pointer may be
struct Input {
    Guarded g;
    const uint32_t *src;
    uint64_t ndw, end_bit;
    uint32_t mis_bits;
    Input(const uint8_t *in, uint64_t in_len, uint32_t mis) : g(4 + in_len + 4)
    {
        mis &= 3u;
        if (in_len) memcpy(g.p() + mis, in, in_len);
        src = (const uint32_t *)(const void *)g.p();
        ndw = (mis + in_len + 3u) >> 2;
        end_bit = 8u * (mis + in_len);
        mis_bits = 8u * mis;
    }
};

}  // namespace

struct pzs_result {
    int32_t status;
    uint32_t d0, d1, npoints;
    uint64_t out_len, in_used;
};

extern "C" {

uint32_t pzs_chunks(uint64_t in_len, uint64_t chunk) { return in_len ? (uint32_t)((in_len + chunk - 1u) / chunk) : 1u; }

// The whole scan.  cand / next / count / endbit (nchunks entries each) and rings (nchunks x 32768 symbols, circular as the core keeps
// them) may be null.  Returns 0, or 1 + the number of the buffer whose guard changed.
int pzs_scan(const uint8_t *in, uint64_t in_len, uint32_t mis, uint64_t chunk, uint64_t span, uint64_t *points, uint32_t max_points,
             uint8_t *windows, pzs_result *r, uint64_t *cand_out, uint32_t *next_out, uint64_t *count_out, uint64_t *endbit_out,
             uint16_t *rings_out)
{
    using pzg::Scan;
    const uint32_t n = pzs_chunks(in_len, chunk);
    Input inp(in, in_len, mis);
    Guarded lds(sizeof(pzg::ScanLds)), cand(8 * (size_t)n), next(4 * (size_t)n), count(8 * (size_t)n), endbit(8 * (size_t)n);
    Guarded rings(2 * (size_t)Scan::RING * n), wbuf(2 * Scan::RING), pts(16 * (size_t)max_points), win(windows ? (size_t)Scan::RING * max_points : 0);
    Guarded res(sizeof(pzg::ScanResult));
    if (windows && max_points) memcpy(win.p(), windows, (size_t)Scan::RING * max_points);  // (what the call leaves as it was)
    pzg::ScanLds &L = *(pzg::ScanLds *)(void *)lds.p();
    uint64_t *cd = (uint64_t *)(void *)cand.p();
    cd[0] = 0;
    for (uint32_t k = 1; k < n; ++k) {
        const uint64_t from = 8u * k * chunk, to = 8u * (k + 1u) * chunk < 8u * in_len ? 8u * (k + 1u) * chunk : 8u * in_len;
        const uint64_t q = Scan::find(L, inp.src, inp.ndw, inp.end_bit, from + inp.mis_bits, to + inp.mis_bits);
        cd[k] = q == Scan::NONE ? Scan::NONE : q - inp.mis_bits;
    }
    for (uint32_t k = 0; k < n; ++k)
        Scan::decode(L, inp.src, inp.ndw, inp.mis_bits, inp.end_bit, cd, n, k, (uint16_t *)(void *)rings.p() + (size_t)k * Scan::RING,
                     (uint32_t *)(void *)next.p(), (uint64_t *)(void *)count.p(), (uint64_t *)(void *)endbit.p());
    Scan::resolve(0u, 1u, cd, (const uint32_t *)(const void *)next.p(), (const uint64_t *)(const void *)count.p(),
                  (const uint64_t *)(const void *)endbit.p(), (const uint16_t *)(const void *)rings.p(), n, span, wbuf.p(),
                  (uint64_t *)(void *)pts.p(), max_points, windows ? win.p() : nullptr, (pzg::ScanResult *)(void *)res.p());
    const Guarded *all[] = {&inp.g, &lds, &cand, &next, &count, &endbit, &rings, &wbuf, &pts, &win, &res};
    for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i)
        if (!all[i]->ok()) return 1 + (int)i;
    memcpy(r, res.p(), sizeof(*r));
    const uint32_t stored = r->npoints < max_points ? r->npoints : max_points;
    if (stored) memcpy(points, pts.p(), 16 * (size_t)stored);
    if (windows && stored) memcpy(windows, win.p(), (size_t)Scan::RING * stored);
    if (cand_out) memcpy(cand_out, cand.p(), cand.n);
    if (next_out) memcpy(next_out, next.p(), next.n);
    if (count_out) memcpy(count_out, count.p(), count.n);
    if (endbit_out) memcpy(endbit_out, endbit.p(), endbit.n);
    if (rings_out) memcpy(rings_out, rings.p(), rings.n);
    return 0;
}

// the finder alone: the smallest candidate position in [from_bit, to_bit) of the stream, or ~0
uint64_t pzs_find(const uint8_t *in, uint64_t in_len, uint32_t mis, uint64_t from_bit, uint64_t to_bit)
{
    Input inp(in, in_len, mis);
    Guarded lds(sizeof(pzg::ScanLds));
    const uint64_t q = pzg::Scan::find(*(pzg::ScanLds *)(void *)lds.p(), inp.src, inp.ndw, inp.end_bit, from_bit + inp.mis_bits, to_bit + inp.mis_bits);
    if (!inp.g.ok() || !lds.ok()) abort();
    return q == pzg::Scan::NONE ? q : q - inp.mis_bits;
}
}

#ifdef PZS_MAIN
int main(int argc, char **argv)
{
    static_assert(sizeof(pzs_result) == sizeof(pzg::ScanResult), "the result block");
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
        fclose(f);
        const uint64_t chunks[] = {256, 1024, 4096};
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t room = 64;
            std::vector<uint64_t> pts(2 * room);
            std::vector<uint8_t> win((size_t)32768 * room);
            pzs_result r{};
            const int rc = pzs_scan(d.data(), d.size(), (uint32_t)a + c, chunks[c], 4096, pts.data(), room, win.data(), &r, nullptr, nullptr, nullptr,
                                    nullptr, nullptr);
            printf("%s chunk %llu: rc %d status %d points %u out_len %llu\n", argv[a], (unsigned long long)chunks[c], rc, r.status, r.npoints,
                   (unsigned long long)r.out_len);
            if (rc) return 1;
        }
    }
    return 0;
}
#endif
