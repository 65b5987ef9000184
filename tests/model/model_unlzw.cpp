// model_unlzw.cpp -- TEST INFRASTRUCTURE: the LZW decoder of pzg_unlzw_many (pure_zlib_amd/csrc/unlzw_core.h) as a host program, the way
// model_unshuffle.cpp builds the byte-plane stage, so that the CPU suite can check it against a table decoder written from the header's
// rules (tests/lzwcases.py) without a GPU: the 64 lanes are loops here and the wave's table is a plain struct.  The destination has 64
// guard bytes on both sides, the source is a heap block of exactly the aligned dwords that hold the stream, and a guard that changed
// is the call's return value.  Never linked into libpzg.so; the product has no CPU path.
// Built with AddressSanitizer (tests/test_sanitized_unlzw.py builds it so with tests/cxx/san_unlzw.cpp) the stream's output is instead
// a heap block of exactly out_cap bytes behind the out_off & 15 bytes that give it its alignment: the sanitizer is the guard then,
// for reads as well as writes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/unlzw_core.h"

namespace {

using Z = pzg::Unlzw;

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

// The stream at `mis` bytes past a dword boundary in a heap block of exactly the aligned dwords that hold it.  Without a byte it is
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

uint32_t pzs_unlzw_starts(void) { return Z::STARTS; }

// One stream: in_len bytes at misalignment mis; dst: dst_bytes of the caller's, the stream's output at out_off in them with room for
// out_cap (the block they are copied into is 64-byte aligned, so out_off is the output's alignment too).  res: status, out_len,
// detail[0], detail[1].  Returns 0, or 1 when a guard changed.
int pzs_unlzw(const uint8_t *in, uint64_t in_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t out_off, uint64_t out_cap, uint32_t early_change,
              int64_t *res)
{
    Input inp(in, in_len, mis);
    static Z::Table T;
    for (uint32_t i = 0; i < Z::STARTS; ++i) T.start[i] = 0xDEADBEEFu;  // (LDS is not zeroed at launch)
    Z::Result r;
#if defined(__SANITIZE_ADDRESS__)
    const size_t k = (size_t)(out_off & 15u);
    uint8_t *block = nullptr;  // (posix_memalign: 16-byte aligned whatever the size, and exactly that size)
    if (posix_memalign((void **)&block, 16, out_cap ? k + (size_t)out_cap : 16)) return 3;
    uint8_t *at = out_cap ? block + k : block + 16;
    if (out_cap) memcpy(block, dst + out_off - k, k + (size_t)out_cap);
    r = Z::stream(inp.in, in_len, at, out_cap, early_change, T);
    if (out_cap) memcpy(dst + out_off - k, block, k + (size_t)out_cap);
    free(block);
    const bool ok = true;
#else
    Guarded out((size_t)dst_bytes);
    if (dst_bytes) memcpy(out.p(), dst, (size_t)dst_bytes);
    r = Z::stream(inp.in, in_len, out.p() + out_off, out_cap, early_change, T);
    const bool ok = out.ok();
    if (ok && dst_bytes) memcpy(dst, out.p(), (size_t)dst_bytes);
#endif
    res[0] = r.status;
    res[1] = r.out_len;
    res[2] = r.d0;
    res[3] = r.d1;
    return ok ? 0 : 1;
}
}
