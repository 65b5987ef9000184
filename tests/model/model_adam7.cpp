// model_adam7.cpp -- TEST INFRASTRUCTURE: the Adam7 gather of pzg_adam7_many (pure_zlib_amd/csrc/adam7_core.h) as a host program, the
// way model_unfilter.cpp builds the unfilter, so that the CPU suite can check it against a plain-Python Adam7 (tests/adam7cases.py)
// without a GPU: the 64 lanes are a loop here, the waves that share an image's rows -- the grid's second dimension -- another around
// it.  The destination has 64 guard bytes on both sides, the source is a heap block of exactly the aligned dwords that hold the
// image's extent, and a guard that changed is the call's return value.  Never linked into libpzg.so; the product has no CPU path.
// Built with AddressSanitizer (tests/test_sanitized_adam7.py builds it so with tests/cxx/san_adam7.cpp) the destination is instead a
// heap block of exactly the image's bytes -- from its first row's first byte to its last row's last -- behind the dst_off & 3 bytes
// that give it its alignment: the sanitizer is the guard then, for reads as well as writes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/adam7_core.h"

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

uint32_t pza_slices(void) { return pzg::Adam7::SLICES; }

uint64_t pza_src_extent(uint32_t width, uint32_t height, uint32_t bits) { return pzg::Adam7::src_extent(width, height, bits); }

// One image: src_len bytes -- its source extent, or 0 where nothing may be read -- at misalignment mis; dst: dst_bytes of the caller's,
// the image at dst_off in them (the block they are copied into is 64-byte aligned, so dst_off is the destination's alignment too).
// The image's rows are run as `slices` waves.  sd: status, detail[0], detail[1] (every wave must give the same: -2 where not).
// Returns 0, or 1 when a guard changed.
int pza_adam7(const uint8_t *src, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t dst_off, uint64_t stride, uint32_t width,
              uint32_t height, uint32_t bits, uint32_t slices, int32_t *sd)
{
    Input inp(src, src_len, mis);
    int32_t status = -1;
    uint32_t d0 = 0, d1 = 0;
    bool same = true;
    auto run = [&](uint8_t *at) {
        for (uint32_t s = 0; s < slices; ++s) {
            int32_t st = -1;
            uint32_t e0 = 0, e1 = 0;
            pzg::Adam7::image(inp.in, at, stride, width, height, bits, s, slices, &st, &e0, &e1);
            if (s == 0u) {
                status = st;
                d0 = e0;
                d1 = e1;
            } else if (st != status || e0 != d0 || e1 != d1) {
                same = false;
            }
        }
    };
#if defined(__SANITIZE_ADDRESS__)
    const bool legal = width && height && pzg::Adam7::geometry_ok(stride, width, height, bits);
    const uint64_t extent = legal ? (uint64_t)(height - 1u) * stride + pzg::Adam7::bytes_of(width, bits) : 0u;
    const size_t k = (size_t)(dst_off & 3u);
    uint8_t *block = (uint8_t *)malloc(extent ? k + (size_t)extent : 16), *at = extent ? block + k : block + 16;  // (malloc: 16-byte aligned)
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
    sd[0] = same ? status : -2;
    sd[1] = (int32_t)d0;
    sd[2] = (int32_t)d1;
    return ok ? 0 : 1;
}
}
