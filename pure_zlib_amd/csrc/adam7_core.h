// adam7_core.h -- Adam7 deinterlacing (PNG specification section 8.2) of many images in one launch (pzg_adam7_many): the seven
// reduced images of an image, unfiltered, dense and back to back in pass order, woven into the image.  Pass p holds the pixels
// (x0 + i dx, y0 + j dy):
//   pass  1  2  3  4  5  6  7          ph = ceil((height - y0) / dy) rows of prb = ceil(pw * pixel_bits / 8) bytes,
//   x0    0  4  0  2  0  1  0          pw = ceil((width - x0) / dx); a pass without pixels takes no bytes.
//   y0    0  0  4  0  2  0  1          Below 8 bits the pixels are packed, the leftmost in the high bits, in every pass row and
//   dx    8  8  4  4  2  2  1          in every row of the image.
//   dy    8  8  8  4  4  2  2
//   the gather     every byte of the image is produced exactly once, by one lane, from the source bytes that hold its pixels:
//                  nothing is read, modified and written back, so two lanes never meet in a byte, whatever the depth.  A lane
//                  takes one ALIGNED dword of a destination row at a time (lane k the dwords k, k + 64, ...) and stores it as a
//                  dword where it lies wholly inside [0, row_bytes) of the row; the dwords at the row's two ends go as single
//                  bytes, those inside only.  Nothing else is written.
//   the rows       an odd row is one row of pass 7, whole: its inner dwords are a copy, two aligned source dwords funnelled by
//                  the misalignment between the two sides.  An even row mixes the passes 6 | 5 | 4, 3 | 2, 1 by the trailing zero
//                  bits of x -- how many of them count is the row's (R.cap: 0 for an odd row) -- so a pixel's pass row and its
//                  place in it are a select among at most four wave-uniform row bases and a shift of x.
//   the bits       below 8 bits a destination byte is put together pixel by pixel; the padding bits of a row's last byte are 0,
//                  whatever the pass rows have in theirs.
//   the reads      a source byte is read as the aligned dword that holds it: nothing is read but the aligned dwords that hold
//                  bytes of the image's source extent, which is a function of (width, height, pixel_bits) alone.
//   the split      the rows of an image go to `slices` waves, wave s taking the rows s, s + slices, ...: a large image alone is
//                  spread over the grid's second dimension, and in a batch of small ones the waves without a row leave at once.
// Geometry that is not legal -- a pixel_bits outside {1, 2, 4, 8, 16, 24, 32, 48, 64}, a stride below the row's bytes, a width or
// height of 2^31 or more -- is ST_FILTER with detail {BAD_ARGS, pixel_bits}; nothing of that image is read or written.
// The same source compiles as a host program for the CPU model (tests/model/model_adam7.cpp): there the 64 lanes are a loop.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct Adam7 {
    static constexpr uint32_t LANES = 64u;
    static constexpr uint32_t SLICES = 16u;  // the grid's second dimension (pzg_adam7_kernel.h)
    static constexpr int32_t ST_OK = 0, ST_FILTER = 23;  // (PZG_OK, PZG_E_FILTER: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t BAD_ARGS = 0xffffffffu;

    // one image, wave-uniform
    struct Job {
        const uint32_t *src;  // the aligned dwords that hold the passes: source byte q is byte (q + mis) & 3 of src[(q + mis) >> 2]
        uint32_t mis;
        uint8_t *dst;
        uint64_t stride, rb;  // rb: the bytes of a row of the image
        uint32_t width;
        uint64_t off[7], prb[7];  // pass p + 1: where it starts in the source, the bytes of a row of it
    };

    // one row of the image, wave-uniform: a pixel whose x has t trailing zero bits is pixel x >> shiftL of the pass row at
    // baseL, L = min(t, cap)
    struct Row {
        uint64_t base0, base1, base2, base3;
        uint32_t shift0, shift1, shift2, shift3, cap;
    };

    PZG_FN static bool bits_ok(uint32_t b) { return b == 1u || b == 2u || b == 4u || b == 8u || b == 16u || b == 24u || b == 32u || b == 48u || b == 64u; }

    // ceil((size - first) / (1 << lstep)), 0 where size <= first (first < 1 << lstep, size < 2^31)
    PZG_FN static uint32_t pass_dim(uint32_t size, uint32_t first, uint32_t lstep) { return (size + ((1u << lstep) - 1u - first)) >> lstep; }

    PZG_FN static uint64_t bytes_of(uint32_t pixels, uint32_t bits) { return ((uint64_t)pixels * bits + 7u) >> 3; }

    PZG_FN static bool geometry_ok(uint64_t stride, uint32_t width, uint32_t height, uint32_t bits)
    {
        return bits_ok(bits) && !(width >> 31) && !(height >> 31) && stride >= bytes_of(width, bits);
    }

    // pass p of the layout: it starts at `at`; returns where the next one does
    PZG_FN static uint64_t pass_put(uint64_t *off, uint64_t *prb, uint32_t p, uint64_t at, uint32_t width, uint32_t height, uint32_t bits, uint32_t x0,
                                    uint32_t ldx, uint32_t y0, uint32_t ldy)
    {
        off[p] = at;
        prb[p] = bytes_of(pass_dim(width, x0, ldx), bits);
        return at + pass_dim(height, y0, ldy) * prb[p];
    }

    // off[p], prb[p] of the seven passes; returns the bytes of all of them, the image's source extent.  (Written out: every index is
    // a constant, so that the fourteen values are registers on the device.)
    PZG_FN static uint64_t layout(uint32_t width, uint32_t height, uint32_t bits, uint64_t *off, uint64_t *prb)
    {
        uint64_t at = 0;
        at = pass_put(off, prb, 0u, at, width, height, bits, 0u, 3u, 0u, 3u);
        at = pass_put(off, prb, 1u, at, width, height, bits, 4u, 3u, 0u, 3u);
        at = pass_put(off, prb, 2u, at, width, height, bits, 0u, 2u, 4u, 3u);
        at = pass_put(off, prb, 3u, at, width, height, bits, 2u, 2u, 0u, 2u);
        at = pass_put(off, prb, 4u, at, width, height, bits, 0u, 1u, 2u, 2u);
        at = pass_put(off, prb, 5u, at, width, height, bits, 1u, 1u, 0u, 1u);
        return pass_put(off, prb, 6u, at, width, height, bits, 0u, 0u, 1u, 1u);
    }

    PZG_FN static uint64_t src_extent(uint32_t width, uint32_t height, uint32_t bits)
    {
        uint64_t off[7], prb[7];
        return layout(width, height, bits, off, prb);
    }

    PZG_FN static void row_begin(const Job &J, uint32_t y, Row &R)
    {
        const uint64_t r1 = y >> 1, r2 = y >> 2, r3 = y >> 3;
        R.base1 = R.base2 = R.base3 = 0u;
        R.shift1 = R.shift2 = R.shift3 = 0u;
        if (y & 1u) {
            R.cap = 0u;
            R.base0 = J.off[6] + r1 * J.prb[6];
            R.shift0 = 0u;
            return;
        }
        R.base0 = J.off[5] + r1 * J.prb[5];
        R.shift0 = 1u;
        if (y & 2u) {
            R.cap = 1u;
            R.base1 = J.off[4] + r2 * J.prb[4];
            R.shift1 = 1u;
        } else if (y & 4u) {
            R.cap = 2u;
            R.base1 = J.off[3] + r2 * J.prb[3];
            R.shift1 = 2u;
            R.base2 = J.off[2] + r3 * J.prb[2];
            R.shift2 = 2u;
        } else {
            R.cap = 3u;
            R.base1 = J.off[3] + r2 * J.prb[3];
            R.shift1 = 2u;
            R.base2 = J.off[1] + r3 * J.prb[1];
            R.shift2 = 3u;
            R.base3 = J.off[0] + r3 * J.prb[0];
            R.shift3 = 3u;
        }
    }

    // aL of four values (taken by value: a conditional between members would choose between their ADDRESSES, and the row would
    // live in memory to have some)
    template <class T>
    PZG_FN static T pick(uint32_t L, T a0, T a1, T a2, T a3)
    {
        const T lo = L == 0u ? a0 : a1, hi = L == 2u ? a2 : a3;
        return L < 2u ? lo : hi;
    }

    // pixel x of the row: the start of its pass row in the source, and its number in that row
    PZG_FN static void locate(const Row &R, uint32_t x, uint64_t *base, uint32_t *sx)
    {
        const uint32_t t = (uint32_t)__builtin_ctz(x | 8u), L = t < R.cap ? t : R.cap;
        *base = pick<uint64_t>(L, R.base0, R.base1, R.base2, R.base3);
        *sx = x >> pick<uint32_t>(L, R.shift0, R.shift1, R.shift2, R.shift3);
    }

    PZG_FN static uint32_t src_byte(const Job &J, uint64_t q)
    {
        q += J.mis;
        return (J.src[q >> 2] >> (8u * ((uint32_t)q & 3u))) & 0xffu;
    }

    // the bytes [j0, j1) of the row (j1 - j0 <= 4), byte j at bits 8 (j - lo) of the result
    template <uint32_t BITS>
    PZG_FN static uint32_t gather(const Job &J, const Row &R, int64_t lo, uint64_t j0, uint64_t j1)
    {
        uint32_t o = 0u;
        if (BITS >= 8u) {
            constexpr uint32_t B = BITS >= 8u ? BITS / 8u : 1u;
            uint32_t x = (uint32_t)(j0 / B), k = (uint32_t)(j0 - (uint64_t)x * B);
            for (uint64_t j = j0; j < j1; ++j) {
                uint64_t base;
                uint32_t sx;
                locate(R, x, &base, &sx);
                o |= src_byte(J, base + (uint64_t)sx * B + k) << (8u * (uint32_t)((int64_t)j - lo));
                if (++k == B) {
                    k = 0u;
                    ++x;
                }
            }
        } else {
            constexpr uint32_t PPB = BITS >= 8u ? 1u : 8u / BITS;  // pixels of a byte
            for (uint64_t j = j0; j < j1; ++j) {
                uint32_t v = 0u;
#pragma unroll
                for (uint32_t i = 0; i < PPB; ++i) {
                    const uint32_t x = (uint32_t)j * PPB + i;  // (j < 2^28: the row of a width below 2^31)
                    if (x < J.width) {
                        uint64_t base;
                        uint32_t sx;
                        locate(R, x, &base, &sx);
                        const uint64_t bit = (uint64_t)sx * BITS;
                        const uint32_t pix = (src_byte(J, base + (bit >> 3)) >> (8u - BITS - ((uint32_t)bit & 7u))) & ((1u << BITS) - 1u);
                        v |= pix << (8u - BITS - i * BITS);
                    }
                }
                o |= v << (8u * (uint32_t)((int64_t)j - lo));
            }
        }
        return o;
    }

    // Dword u of the aligned destination of the row at `at`: it holds the row's bytes lo .. lo + 3, lo = 4 u - wal.
    template <uint32_t BITS>
    PZG_FN static void dword(const Job &J, const Row &R, uint8_t *at, uint32_t wal, uint64_t u)
    {
        const int64_t lo = 4ll * (int64_t)u - wal;
        uint32_t *out = (uint32_t *)(void *)(at - wal) + u;
        if (lo >= 0 && (uint64_t)lo + 4u <= J.rb) {
            uint32_t o;
            if (R.cap == 0u) {  // a row of pass 7: the copy
                const uint64_t q = R.base0 + (uint64_t)lo + J.mis;
                const uint32_t m = (uint32_t)q & 3u, a = J.src[q >> 2], b = m ? J.src[(q >> 2) + 1u] : 0u;  // (m != 0: byte lo + 3 lies in that dword)
                o = funnel(b, a, 8u * m);
                if (BITS < 8u && (uint64_t)lo + 4u == J.rb) {
                    const uint32_t used = (uint32_t)(((uint64_t)J.width * BITS) & 7u);  // bits of the row's last byte that hold pixels (0: all)
                    if (used) o &= 0x00ffffffu | (((0xff00u >> used) & 0xffu) << 24);
                }
            } else {
                o = gather<BITS>(J, R, lo, (uint64_t)lo, (uint64_t)lo + 4u);
            }
            *out = o;
        } else {
            const uint64_t j0 = lo < 0 ? 0u : (uint64_t)lo, j1 = (uint64_t)(lo + 4) < J.rb ? (uint64_t)(lo + 4) : J.rb;
            const uint32_t o = gather<BITS>(J, R, lo, j0, j1);
            uint8_t *p = (uint8_t *)(void *)out;
            for (uint64_t j = j0; j < j1; ++j) p[(int64_t)j - lo] = (uint8_t)(o >> (8u * (uint32_t)((int64_t)j - lo)));
        }
    }

    // the rows slice, slice + slices, ... of the image
    template <uint32_t BITS>
    PZG_FN static void rows(const Job &J, uint32_t height, uint32_t slice, uint32_t slices)
    {
        for (uint32_t y = slice; y < height; y += slices) {
            Row R;
            row_begin(J, y, R);
            uint8_t *at = J.dst + (uint64_t)y * J.stride;
            const uint32_t wal = (uint32_t)((uintptr_t)at & 3u);
            const uint64_t nd = (wal + J.rb + 3u) >> 2;
            PZG_LANES_BEGIN(k)
            for (uint64_t u = k; u < nd; u += LANES) dword<BITS>(J, R, at, wal, u);
            PZG_LANES_END
        }
    }

    // One image's share of a wave: its status and detail (every wave of the image, every lane, returns the same).
    PZG_FN static void image(const uint8_t *src, uint8_t *dst, uint64_t stride, uint32_t width, uint32_t height, uint32_t bits, uint32_t slice,
                             uint32_t slices, int32_t *status, uint32_t *d0, uint32_t *d1)
    {
        *status = ST_OK;
        *d0 = *d1 = 0u;
        if (width == 0u || height == 0u) return;
        if (!geometry_ok(stride, width, height, bits)) {
            *status = ST_FILTER;
            *d0 = BAD_ARGS;
            *d1 = bits;
            return;
        }
        Job J;
        J.mis = (uint32_t)((uintptr_t)src & 3u);
        J.src = (const uint32_t *)(const void *)(src - J.mis);
        J.dst = dst;
        J.stride = stride;
        J.rb = bytes_of(width, bits);
        J.width = width;
        layout(width, height, bits, J.off, J.prb);
        switch (bits) {
        case 1u: rows<1u>(J, height, slice, slices); break;
        case 2u: rows<2u>(J, height, slice, slices); break;
        case 4u: rows<4u>(J, height, slice, slices); break;
        case 8u: rows<8u>(J, height, slice, slices); break;
        case 16u: rows<16u>(J, height, slice, slices); break;
        case 24u: rows<24u>(J, height, slice, slices); break;
        case 32u: rows<32u>(J, height, slice, slices); break;
        case 48u: rows<48u>(J, height, slice, slices); break;
        default: rows<64u>(J, height, slice, slices); break;
        }
    }
};

}  // namespace pzg
