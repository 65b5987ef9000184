// model_members.cpp -- TEST INFRASTRUCTURE: the member finder and the layout of pzg_gzip_find_members / pzg_gzip_layout
// (pure_zlib_amd/csrc/member_core.h) as a one-lane host program, the way model_scan.cpp builds the index scan, so that the CPU
// suite can check them against a plain-Python finder without a GPU.  Every buffer the core is handed has 64 guard bytes on both
// sides -- the input none at all beyond the aligned dwords that hold it -- and a guard that changed is the call's return value.
// Never linked into libpzg.so; the product has no CPU path.
// Built with AddressSanitizer (tests/test_sanitized_cores.py builds it so with tests/cxx/san_members.cpp and runs the files of
// tests/memberscheck.py) every such buffer is instead a heap block of exactly its bytes: the sanitizer is the guard then, for reads
// as well as writes.
// With -DPZM_MAIN it is a program of its own: model_members FILE... at three chunk sizes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/member_core.h"

namespace {

constexpr size_t GUARD = 64;

#if defined(__SANITIZE_ADDRESS__)
struct Guarded {
    uint8_t *base = nullptr, *at = nullptr;
    size_t n = 0;
    explicit Guarded(size_t bytes) : n(bytes)
    {
        base = (uint8_t *)malloc(n ? n : 16);  // (no bytes: the address behind a block, where nothing may be touched)
        memset(base, 0xA5, n ? n : 16);
        at = n ? base : base + 16;
    }
    Guarded(const Guarded &) = delete;
    ~Guarded() { free(base); }
    uint8_t *p() const { return at; }
    bool ok() const { return true; }
};
#else
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
#endif

// The input at `mis` bytes past a dword boundary, as a device pointer may be, in a heap block of exactly the aligned dwords that
// hold it: a sanitizer build sees any read outside them.
struct Input {
    std::vector<uint32_t> dwords;
    const uint8_t *in;
    Input(const uint8_t *d, uint64_t in_len, uint32_t mis) : dwords((size_t)(((mis & 3u) + in_len + 3u) >> 2), 0xA5A5A5A5u)
    {
        if (dwords.empty()) dwords.resize(1);
        in = (const uint8_t *)dwords.data() + (mis & 3u);
        if (in_len) memcpy((uint8_t *)dwords.data() + (mis & 3u), d, in_len);
    }
};

}  // namespace

extern "C" {

uint64_t pzm_chunks(uint64_t in_len, uint64_t chunk) { return in_len ? (in_len + chunk - 1u) / chunk : 1u; }

// The finder: count pass, prefix sums, write pass.  starts / bsize: max_members entries.  Returns 0, or 1 + the number of the
// buffer whose guard changed.
int pzm_find(const uint8_t *in, uint64_t in_len, uint32_t mis, uint64_t chunk, uint64_t *starts, uint32_t *bsize, uint32_t max_members,
             uint64_t *nmembers)
{
    using pzg::Members;
    const uint64_t n = pzm_chunks(in_len, chunk), nt = Members::tiles(n);
    Input inp(in, in_len, mis);
    Guarded counts(8 * (size_t)n), part(8 * (size_t)nt), total(8), st(8 * (size_t)max_members), bs(4 * (size_t)max_members);
    memcpy(st.p(), starts, st.n);  // (what the call leaves as it was)
    memcpy(bs.p(), bsize, bs.n);
    uint64_t *c = (uint64_t *)(void *)counts.p(), *pt = (uint64_t *)(void *)part.p(), *tot = (uint64_t *)(void *)total.p();
    for (uint64_t k = 0; k < n; ++k) c[k] = Members::chunk_sweep<false>(inp.in, in_len, chunk, k, 0u, nullptr, nullptr, 0u);
    for (uint64_t t = 0; t < nt; ++t) Members::tile_sum(c, n, t, pt);
    Members::tile_offsets(pt, nt, 0u, tot);
    for (uint64_t t = 0; t < nt; ++t) Members::tile_scan(c, n, t, pt, c);
    for (uint64_t k = 0; k < n; ++k)
        Members::chunk_sweep<true>(inp.in, in_len, chunk, k, c[k], (uint64_t *)(void *)st.p(), (uint32_t *)(void *)bs.p(), max_members);
    const Guarded *all[] = {&counts, &part, &total, &st, &bs};
    for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i)
        if (!all[i]->ok()) return 1 + (int)i;
    *nmembers = *tot;
    memcpy(starts, st.p(), st.n);
    memcpy(bsize, bs.p(), bs.n);
    return 0;
}

// The layout of m starts: four arrays of m entries and the total.
int pzm_layout(const uint8_t *in, uint64_t in_len, uint32_t mis, const uint64_t *starts, uint64_t m, uint64_t out_base_off, uint64_t *in_off,
               uint64_t *in_lenv, uint64_t *out_off, uint64_t *out_cap, uint64_t *total)
{
    using pzg::Members;
    const uint64_t nt = Members::tiles(m);
    Input inp(in, in_len, mis);
    Guarded io(8 * (size_t)m), il(8 * (size_t)m), oo(8 * (size_t)m), oc(8 * (size_t)m), part(8 * (size_t)nt), tot(8);
    Members::Input I;
    I.init(inp.in, in_len);
    uint64_t *cap = (uint64_t *)(void *)oc.p(), *pt = (uint64_t *)(void *)part.p();
    for (uint64_t j = 0; j < m; ++j) Members::member(I, starts, m, j, (uint64_t *)(void *)io.p(), (uint64_t *)(void *)il.p(), cap);
    for (uint64_t t = 0; t < nt; ++t) Members::tile_sum(cap, m, t, pt);
    Members::tile_offsets(pt, nt, out_base_off, (uint64_t *)(void *)tot.p());
    for (uint64_t t = 0; t < nt; ++t) Members::tile_scan(cap, m, t, pt, (uint64_t *)(void *)oo.p());
    const Guarded *all[] = {&io, &il, &oo, &oc, &part, &tot};
    for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i)
        if (!all[i]->ok()) return 1 + (int)i;
    memcpy(in_off, io.p(), io.n);
    memcpy(in_lenv, il.p(), il.n);
    memcpy(out_off, oo.p(), oo.n);
    memcpy(out_cap, oc.p(), oc.n);
    memcpy(total, tot.p(), 8);
    return 0;
}
}

#ifdef PZM_MAIN
int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
        fclose(f);
        const uint64_t chunks[] = {64, 256, 4096};
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t room = 4096;
            std::vector<uint64_t> st(room), io(room), il(room), oo(room), oc(room);
            std::vector<uint32_t> bs(room);
            uint64_t n = 0, total = 0;
            int rc = pzm_find(d.data(), d.size(), (uint32_t)a + c, chunks[c], st.data(), bs.data(), room, &n);
            const uint64_t m = n < room ? n : room;
            if (!rc) rc = pzm_layout(d.data(), d.size(), (uint32_t)a + c, st.data(), m, 0, io.data(), il.data(), oo.data(), oc.data(), &total);
            printf("%s chunk %llu: rc %d members %llu total %llu\n", argv[a], (unsigned long long)chunks[c], rc, (unsigned long long)n,
                   (unsigned long long)total);
            if (rc) return 1;
        }
    }
    return 0;
}
#endif
