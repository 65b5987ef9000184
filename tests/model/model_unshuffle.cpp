// model_unshuffle.cpp -- TEST INFRASTRUCTURE: the byte-plane stage of pzg_unshuffle_many (pure_zlib_amd/csrc/unshuffle_core.h) as a host
// program, the way model_unpredict.cpp builds the Predictor 2 stage, so that the CPU suite can check it against a plain-numpy reference
// (tests/fpcases.py) without a GPU: the 64 lanes are a loop here, the waves that share a job's rows -- the grid's second dimension --
// another around it, in either order.  The destination has 64 guard bytes on both sides, the source is a heap block of exactly the
// aligned dwords that hold the bytes the job may read, and a guard that changed is the call's return value.  Never linked into
// libpzg.so; the product has no CPU path.
// Built with AddressSanitizer (tests/test_sanitized_unshuffle.py builds it so with tests/cxx/san_unshuffle.cpp) the destination is
// instead a heap block of exactly the window's bytes -- from its first row's first byte to its last row's last -- behind the
// dst_off & 15 bytes that give it its alignment: the sanitizer is the guard then, for reads as well as writes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/unshuffle_core.h"

namespace {

using U = pzg::Unshuffle;
static_assert(sizeof(U::Desc) == 64, "pzg_unshuffle_desc");

constexpr size_t GUARD = 64;

struct Guarded {
    uint8_t *base = nullptr;
    size_t n = 0;
    explicit Guarded(size_t bytes) : n(bytes)
    {
        const size_t all = (2 * GUARD + n + 63u) & ~(size_t)63u;
        base = (uint8_t *)aligned_alloc(64, all);
        for (size_t i = 0; i < GUARD; ++i) base[i] = base[GUARD + n + i] = (uint8_t)(0x40u + i);
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

// The source at `mis` bytes past a dword boundary in a heap block of exactly the aligned dwords that hold it.  Without a byte it is
// the address just behind another block: nothing at all may be read.
struct Input {
    std::vector<uint32_t> dwords;
    const uint8_t *in;
    Input(const uint8_t *d, uint64_t len, uint32_t mis) : dwords(len ? (size_t)(((mis & 3u) + len + 3u) >> 2) : 1u, 0xA5A5A5A5u)
    {
        in = len ? (const uint8_t *)dwords.data() + (mis & 3u) : (const uint8_t *)(dwords.data() + 1);
        if (len) memcpy((uint8_t *)dwords.data() + (mis & 3u), d, len);
    }
};

}  // namespace

extern "C" {

// the elements of a lane's run, and so the elements of a row a wave reaches at once (64 times as many)
uint32_t pzs_run(void) { return U::E; }

// One job: desc, 64 bytes (its src_off is not looked at: the source given here is the job's own); src_bytes bytes of source -- what
// the job may read, min(src_len, rows * src_row_bytes), or 0 where nothing may be read -- at misalignment mis; src_len: what the call
// is told the source holds; dst: dst_bytes of the caller's, the window at desc.dst_off in them (the block they are copied into is
// 64-byte aligned, so dst_off is the destination's alignment too).  The job's rows are run as `slices` waves, the last first where
// `descending`.  sd: status, detail[0], detail[1] as the waves left them (-1: nobody wrote them).
// Returns 0, 1 when a guard changed, 2 when the status was not written exactly once.
int pzs_unshuffle(const void *desc, const uint8_t *src, uint64_t src_bytes, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint32_t slices,
                  int descending, int32_t *sd)
{
    U::Desc D;
    memcpy(&D, desc, sizeof D);
    const uint64_t dst_off = D.dst_off;
    D.src_off = D.dst_off = 0u;
    Input inp(src, src_bytes, mis);
    int32_t status = -1;
    uint32_t detail[2] = {0xffffffffu, 0xffffffffu};
    int writes = 0;
    auto run = [&](uint8_t *at) {
        for (uint32_t t = 0; t < slices; ++t) {
            const uint32_t s = descending ? slices - 1u - t : t;
            int32_t st = -77;
            uint32_t d[2] = {0u, 0u};
            const U::Desc Du = U::fetch(&D);
            U::job(inp.in, src_len, at, Du, s, slices, &st, d);
            if (st != -77) {
                ++writes;
                status = st;
                detail[0] = d[0];
                detail[1] = d[1];
            }
        }
    };
#if defined(__SANITIZE_ADDRESS__)
    const bool legal = !U::empty(D) && U::geometry_ok(D);
    const uint64_t extent = legal ? (uint64_t)(D.win_rows - 1u) * D.dst_stride + D.win_bytes : 0u;
    const size_t k = (size_t)(dst_off & 15u);
    uint8_t *block = nullptr;  // (posix_memalign: 16-byte aligned whatever the size, and exactly that size)
    if (posix_memalign((void **)&block, 16, extent ? k + (size_t)extent : 16)) return 3;
    uint8_t *at = extent ? block + k : block + 16;
    if (extent) memcpy(block, dst + dst_off - k, k + (size_t)extent);
    run(at);
    if (extent) memcpy(dst + dst_off - k, block, k + (size_t)extent);
    free(block);
    const bool ok = true;
#else
    Guarded out((size_t)dst_bytes);
    if (dst_bytes) memcpy(out.p(), dst, (size_t)dst_bytes);
    run(out.p() + dst_off);
    const bool ok = out.ok();
    if (ok && dst_bytes) memcpy(dst, out.p(), (size_t)dst_bytes);
#endif
    sd[0] = status;
    sd[1] = (int32_t)detail[0];
    sd[2] = (int32_t)detail[1];
    return !ok ? 1 : writes != 1 ? 2 : 0;
}
}
