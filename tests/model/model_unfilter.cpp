// model_unfilter.cpp -- TEST INFRASTRUCTURE: the scanline unfilter of pzg_unfilter_many (pure_zlib_amd/csrc/unfilter_core.h) as a host
// program, the way model_members.cpp builds the member finder, so that the CPU suite can check it against a plain-Python unfilter
// without a GPU: the 64 lanes of a group are an array here, a step a loop over them.  The destination has 64 guard bytes on both
// sides, the input none at all beyond the aligned dwords that hold it, and a guard that changed is the call's return value.
// Never linked into libpzg.so; the product has no CPU path.
// Built with AddressSanitizer (tests/test_sanitized_cores.py builds it so with tests/cxx/san_unfilter.cpp and runs every case of
// tests/pngcases.py) the destination is instead a heap block of exactly the aligned dwords that hold the image's extent, which the
// core may read whole: the sanitizer is the guard then, for reads as well as writes.
// With -DPZU_MAIN it is a program of its own: model_unfilter [SEED] runs seeded images of every bpp at the edge shapes against a
// byte-by-byte unfilter of its own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pure_zlib_amd/csrc/unfilter_core.h"

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

// One image: src_len bytes at misalignment mis; dst: dst_bytes of the caller's, the image at dst_off in them (the block they are
// copied into is 64-byte aligned, so dst_off is the destination's alignment too).  sd: status, detail[0], detail[1].  Returns 0, or
// 1 when a guard changed.
int pzu_unfilter(const uint8_t *src, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t dst_off, uint64_t stride,
                 uint32_t row_bytes, uint32_t height, uint32_t bpp, int32_t *sd)
{
    Input inp(src, src_len, mis);
    int32_t status = -1;
    uint32_t d0 = 0, d1 = 0;
#if defined(__SANITIZE_ADDRESS__)
    // [lo, hi) of the caller's bytes: the aligned dwords that hold [dst_off, dst_off + (height - 1) stride + row_bytes), cut to what
    // the caller has (an illegal stride: nothing may be touched, whatever the extent would be)
    const uint64_t extent = height && row_bytes && stride >= row_bytes ? (uint64_t)(height - 1u) * stride + row_bytes : 0u;
    const uint64_t lo = dst_off & ~(uint64_t)3u, end = (dst_off + extent + 3u) & ~(uint64_t)3u, hi = !extent ? lo : end < dst_bytes ? end : dst_bytes;
    uint8_t *block = (uint8_t *)malloc(hi > lo ? (size_t)(hi - lo) : 16), *at = hi > lo ? block : block + 16;  // (malloc: 16-byte aligned)
    if (hi > lo) memcpy(at, dst + lo, (size_t)(hi - lo));
    pzg::Unfilter::image(inp.in, src_len, at + (dst_off - lo), stride, row_bytes, height, bpp, &status, &d0, &d1);
    if (hi > lo) memcpy(dst + lo, at, (size_t)(hi - lo));
    free(block);
    const bool ok = true;
#else
    Guarded out((size_t)dst_bytes);
    if (dst_bytes) memcpy(out.p(), dst, (size_t)dst_bytes);
    pzg::Unfilter::image(inp.in, src_len, out.p() + dst_off, stride, row_bytes, height, bpp, &status, &d0, &d1);
    const bool ok = out.ok();
    if (ok && dst_bytes) memcpy(dst, out.p(), (size_t)dst_bytes);
#endif
    sd[0] = status;
    sd[1] = (int32_t)d0;
    sd[2] = (int32_t)d1;
    return ok ? 0 : 1;
}
}

#ifdef PZU_MAIN
namespace {
uint32_t rng_state = 1;
uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
}  // namespace

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
    const uint32_t bpps[] = {1, 2, 3, 4, 6, 8}, heights[] = {1, 2, 63, 64, 65, 129};
    int bad = 0, runs = 0;
    for (uint32_t bpp : bpps) {
        const uint32_t rbs[] = {bpp - 1, bpp, bpp + 1, 63, 64, 65, 257};
        for (uint32_t rb : rbs)
            for (uint32_t h : heights) {
                if (!rb) continue;
                const uint32_t mis = rnd() & 3u, off = rnd() % 19u, stride = rb + rnd() % 7u;
                std::vector<uint8_t> src((size_t)h * (1 + rb)), want((size_t)h * rb), dst(off + (size_t)h * stride + 9, 0xCD);
                for (auto &b : src) b = (uint8_t)(rnd() % 3u ? rnd() : rnd() & 3u);
                for (uint32_t y = 0; y < h; ++y) src[(size_t)y * (1 + rb)] = (uint8_t)(rnd() % 5u);
                for (uint32_t y = 0; y < h; ++y)
                    for (uint32_t j = 0; j < rb; ++j) {
                        const int ft = src[(size_t)y * (1 + rb)], x = src[(size_t)y * (1 + rb) + 1 + j];
                        const int a = j >= bpp ? want[(size_t)y * rb + j - bpp] : 0, b = y ? want[(size_t)(y - 1) * rb + j] : 0;
                        const int c = j >= bpp && y ? want[(size_t)(y - 1) * rb + j - bpp] : 0;
                        const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
                        want[(size_t)y * rb + j] = (uint8_t)(x + pred);
                    }
                int32_t sd[3];
                const int rc = pzu_unfilter(src.data(), src.size(), mis, dst.data(), dst.size(), off, stride, rb, h, bpp, sd);
                bool same = rc == 0 && sd[0] == 0;
                for (size_t i = 0; same && i < dst.size(); ++i) {
                    const size_t rel = i - off, y = rel / stride, j = rel % stride;
                    const bool in = i >= off && y < h && j < rb;
                    same = dst[i] == (in ? want[y * rb + j] : 0xCD);
                }
                ++runs;
                if (!same) {
                    ++bad;
                    printf("bpp %u row_bytes %u height %u: rc %d status %d\n", bpp, rb, h, rc, sd[0]);
                }
            }
    }
    printf("%d images, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
