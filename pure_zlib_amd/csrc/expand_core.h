// expand_core.h -- pixel expansion of many images in one launch (pzg_expand_many): the rows of an image as PNG stores them -- packed
// 1/2/4-bit samples, palette indices, big-endian 16-bit samples, with or without a tRNS colour key -- written as rows of 8-bit RGBA
// (R, G, B, A) or RGB pixels.  Nothing in it knows of PNG's chunks: rows of samples in, rows of 8-bit pixels out.
//   the samples    below 8 bits the pixels are packed, the leftmost in the high bits; gray is scaled by bit replication (x 255, x 85,
//                  x 17), a palette index is not.  A 16-bit sample gives its HIGH byte (libpng's strip_16, OpenCV).  Gray fans out to
//                  R = G = B; the alpha of types 4 and 6 is copied, reduced the same way; a pixel of type 0 or 2 whose samples ALL
//                  equal the colour key -- compared at the source depth, all 16 bits of a 16-bit sample -- gets alpha 0, every other
//                  255.  A palette entry is a dword whose bytes in memory order are R, G, B, A.  RGB8 drops alpha.
//   the gather     every destination byte is produced exactly once, by one lane, from the source bytes that hold its pixel.  A lane
//                  takes one ALIGNED 16-byte unit of a destination row at a time (lane k the units k, k + 64, ...): four RGBA
//                  pixels where the row is aligned, five and a third RGB ones -- a dword of the unit is put together from the two
//                  pixels it overlaps.  A unit that lies wholly inside [0, row_bytes) of the row is ONE 16-byte store; of the units
//                  at the row's two ends, a dword wholly inside goes as a dword and the others as single bytes, those inside only.
//                  Nothing else is written.
//   the reads      a source byte is read as the aligned dword that holds it (a pixel as the one, two or three that hold it, funnelled
//                  by the misalignment): nothing is read but the aligned dwords that hold bytes of the image's source rows, and the
//                  palette entries [pal_off, pal_off + pal_len).  The padding bits of a packed row's last byte belong to no pixel and
//                  are never interpreted.
//   the palette    a wave that has rows of a palette image copies the image's pal_len entries into its workgroup's 1 KiB of LDS
//                  once and looks every pixel up there (plain dwords: an index is data, so nothing about the banks can be arranged).
//   the split      the rows of an image go to `slices` waves, wave s taking the rows s, s + slices, ... (adam7_core.h).
//   a bad index    a pixel of a palette image whose index is >= pal_len: the image is ST_PALETTE with detail {row, x} of the FIRST
//                  such pixel in row-major order.  Every lane keeps the smallest key (row << 32 | x) it met, the wave reduces them,
//                  and one lane raises the image's word in the launch's scratch -- the complement of the key, so that zeroed memory
//                  is "none" -- with one atomic max; then it counts itself in.  The last of the image's `slices` waves to arrive
//                  (a fence before the count, one behind it) reads the word and writes status and detail.  Images of the other
//                  types, empty ones and illegal ones have the same answer in every wave: the wave of slice 0 writes it.
// Geometry that is not legal -- a (color_type, bit_depth) that is no PNG image type, an unknown format, a destination stride below
// width * bytes per pixel, a source stride below the row's bytes, a pal_len of 0 or above 256 for type 3, a width or height of 2^31
// or more -- is ST_FILTER with detail {BAD_ARGS, color_type << 8 | bit_depth}; nothing of that image is read or written.
// The same source compiles as a host program for the CPU model (tests/model/model_expand.cpp): there the 64 lanes are a loop and the
// waves of an image run one after the other.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct Expand {
    static constexpr uint32_t LANES = 64u;
    static constexpr uint32_t SLICES = 16u;  // the grid's second dimension (pzg_expand_kernel.h)
    static constexpr uint32_t UNIT = 16u;    // the bytes of a destination row a lane owns at a time
    static constexpr int32_t ST_OK = 0, ST_FILTER = 23, ST_PALETTE = 24;  // (PZG_OK, PZG_E_FILTER, PZG_E_PALETTE: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t BAD_ARGS = 0xffffffffu;
    static constexpr uint32_t RGBA8 = 0u, RGB8 = 1u;  // (PZG_PIX_RGBA8, PZG_PIX_RGB8)
    static constexpr uint64_t NONE = ~0ull;           // no bad index: smaller than no key (a row is below 2^31)

    // pzg_expand_desc of include/pzg.h, field for field (pzg_api.cpp holds the two against each other)
    struct Desc {
        uint64_t src_off, src_stride, dst_off, dst_stride;
        uint32_t width, height, pal_off;
        uint16_t pal_len, key[3];
        uint8_t color_type, bit_depth, out_format, has_key;
        uint32_t reserved[2];
    };

    // one image, wave-uniform
    struct Job {
        const uint32_t *src;  // the aligned dwords that hold the rows: byte q of row y is byte (q' & 3) of src[q' >> 2], q' = y * sstride + q + mis
        uint32_t mis;
        uint64_t sstride;
        uint8_t *dst;
        uint64_t dstride, orb;  // orb: the bytes of a delivered row
        uint32_t width;
        const uint32_t *pal;    // the image's entries, in LDS
        uint32_t pal_len, has_key, key0, key1, key2;
    };

    struct alignas(16) Quad {
        uint32_t a, b, c, d;
    };

    PZG_FN static uint32_t channels(uint32_t ct) { return ct == 0u || ct == 3u ? 1u : ct == 2u ? 3u : ct == 4u ? 2u : 4u; }

    PZG_FN static bool type_ok(uint32_t ct, uint32_t depth)
    {
        const bool sub = depth == 1u || depth == 2u || depth == 4u;
        if (ct == 0u) return sub || depth == 8u || depth == 16u;
        if (ct == 3u) return sub || depth == 8u;
        return (ct == 2u || ct == 4u || ct == 6u) && (depth == 8u || depth == 16u);
    }

    // the bytes of a source row, of a delivered one (width < 2^31)
    PZG_FN static uint64_t src_row_bytes(uint32_t width, uint32_t ct, uint32_t depth) { return ((uint64_t)width * (channels(ct) * depth) + 7u) >> 3; }
    PZG_FN static uint64_t dst_row_bytes(uint32_t width, uint32_t fmt) { return (uint64_t)width * (fmt == RGBA8 ? 4u : 3u); }

    PZG_FN static bool geometry_ok(const Desc &D)
    {
        if (!type_ok(D.color_type, D.bit_depth) || D.out_format > RGB8 || (D.width >> 31) || (D.height >> 31)) return false;
        if (D.color_type == 3u && (D.pal_len == 0u || D.pal_len > 256u)) return false;
        return D.dst_stride >= dst_row_bytes(D.width, D.out_format) && D.src_stride >= src_row_bytes(D.width, D.color_type, D.bit_depth);
    }

    // an image's descriptor, every field wave-uniform
    PZG_FN static Desc fetch(const Desc *p)
    {
        Desc D;
        D.src_off = uni64(p->src_off);
        D.src_stride = uni64(p->src_stride);
        D.dst_off = uni64(p->dst_off);
        D.dst_stride = uni64(p->dst_stride);
        D.width = uni(p->width);
        D.height = uni(p->height);
        D.pal_off = uni(p->pal_off);
        D.pal_len = (uint16_t)uni(p->pal_len);
        D.key[0] = (uint16_t)uni(p->key[0]);
        D.key[1] = (uint16_t)uni(p->key[1]);
        D.key[2] = (uint16_t)uni(p->key[2]);
        D.color_type = (uint8_t)uni(p->color_type);
        D.bit_depth = (uint8_t)uni(p->bit_depth);
        D.out_format = (uint8_t)uni(p->out_format);
        D.has_key = (uint8_t)uni(p->has_key);
        D.reserved[0] = D.reserved[1] = 0u;
        return D;
    }

    PZG_FN static uint32_t swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }  // a big-endian sample in the low half of v

    // the palette entry of index s, or 0 and the pixel's key where the image has no such entry
    PZG_FN static uint32_t lookup(const Job &J, uint32_t s, uint32_t x, uint32_t y, uint64_t &bad)
    {
        if (s >= J.pal_len) {
            const uint64_t key = ((uint64_t)y << 32) | x;
            bad = key < bad ? key : bad;
            return 0u;
        }
        return J.pal[s];
    }

    // Pixel x (< width) of the row whose first byte is byte rowq of the source dwords, as R | G << 8 | B << 16 | A << 24.
    template <uint32_t CT, uint32_t DEPTH>
    PZG_FN static uint32_t pixel(const Job &J, uint64_t rowq, uint32_t x, uint32_t y, uint64_t &bad)
    {
        if constexpr (DEPTH < 8u) {
            const uint64_t bit = (uint64_t)x * DEPTH, q = rowq + (bit >> 3);
            const uint32_t byte = (J.src[q >> 2] >> (8u * ((uint32_t)q & 3u))) & 0xffu;
            const uint32_t s = (byte >> (8u - DEPTH - ((uint32_t)bit & 7u))) & ((1u << DEPTH) - 1u);
            if constexpr (CT == 3u) return lookup(J, s, x, y, bad);
            const uint32_t a = J.has_key && s == J.key0 ? 0u : 255u;
            return s * (255u / ((1u << DEPTH) - 1u)) * 0x010101u | (a << 24);
        } else {
            constexpr uint32_t SB = (CT == 0u || CT == 3u ? 1u : CT == 2u ? 3u : CT == 4u ? 2u : 4u) * DEPTH / 8u;  // the bytes of a pixel
            const uint64_t q = rowq + (uint64_t)x * SB;
            const uint32_t m = (uint32_t)q & 3u;
            const uint32_t *p = J.src + (q >> 2);
            const uint32_t a = p[0], b = m + SB > 4u ? p[1] : 0u;  // (read only where the pixel's bytes reach it)
            const uint32_t w0 = funnel(b, a, 8u * m);               // the pixel's bytes 0 .. 3
            uint32_t w1 = 0u;                                       // ... and 4 .. 7
            if constexpr (SB > 4u) {
                const uint32_t c = m + SB > 8u ? p[2] : 0u;
                w1 = funnel(c, b, 8u * m);
            }
            if constexpr (CT == 3u) return lookup(J, w0 & 0xffu, x, y, bad);
            if constexpr (CT == 0u && DEPTH == 8u) {
                const uint32_t s = w0 & 0xffu, al = J.has_key && s == J.key0 ? 0u : 255u;
                return s * 0x010101u | (al << 24);
            }
            if constexpr (CT == 0u && DEPTH == 16u) {
                const uint32_t al = J.has_key && swap16(w0) == J.key0 ? 0u : 255u;
                return (w0 & 0xffu) * 0x010101u | (al << 24);
            }
            if constexpr (CT == 2u && DEPTH == 8u) {
                const bool hit = J.has_key && (w0 & 0xffu) == J.key0 && ((w0 >> 8) & 0xffu) == J.key1 && ((w0 >> 16) & 0xffu) == J.key2;
                return (w0 & 0x00ffffffu) | (hit ? 0u : 0xff000000u);
            }
            if constexpr (CT == 2u && DEPTH == 16u) {
                const bool hit = J.has_key && swap16(w0) == J.key0 && swap16(w0 >> 16) == J.key1 && swap16(w1) == J.key2;
                return (w0 & 0xffu) | ((w0 >> 8) & 0xff00u) | ((w1 & 0xffu) << 16) | (hit ? 0u : 0xff000000u);
            }
            if constexpr (CT == 4u && DEPTH == 8u) return (w0 & 0xffu) * 0x010101u | ((w0 & 0xff00u) << 16);
            if constexpr (CT == 4u && DEPTH == 16u) return (w0 & 0xffu) * 0x010101u | ((w0 & 0xff0000u) << 8);
            if constexpr (CT == 6u && DEPTH == 8u) return w0;
            if constexpr (CT == 6u && DEPTH == 16u) return (w0 & 0xffu) | ((w0 >> 8) & 0xff00u) | ((w1 & 0xffu) << 16) | ((w1 & 0xff0000u) << 8);
            return 0u;
        }
    }

    // The bytes [j0, j1) of the delivered row (lo <= j0 < j1 <= lo + 4, j1 <= orb), byte j at bits 8 (j - lo) of the result: at most
    // two pixels hold them.  (Bits above byte j1 - 1 may hold anything.)
    template <uint32_t CT, uint32_t DEPTH, uint32_t FMT>
    PZG_FN static uint32_t gather(const Job &J, uint64_t rowq, uint32_t y, int64_t lo, uint64_t j0, uint64_t j1, uint64_t &bad)
    {
        constexpr uint32_t OB = FMT == RGBA8 ? 4u : 3u;
        constexpr uint32_t KEEP = FMT == RGBA8 ? 0xffffffffu : 0x00ffffffu;
        const uint32_t x0 = (uint32_t)(j0 / OB), ph = (uint32_t)(j0 - (uint64_t)x0 * OB);
        uint64_t v = pixel<CT, DEPTH>(J, rowq, x0, y, bad) & KEEP;
        if (ph + (uint32_t)(j1 - j0) > OB)  // (x0 + 1 < width: byte j1 - 1 is one of its bytes)
            v |= (uint64_t)(pixel<CT, DEPTH>(J, rowq, x0 + 1u, y, bad) & KEEP) << (8u * OB);
        return (uint32_t)(v >> (8u * ph)) << (8u * (uint32_t)((int64_t)j0 - lo));
    }

    // Dword `out` of the aligned destination: it holds the row's bytes lo .. lo + 3, some of them inside the row.
    template <uint32_t CT, uint32_t DEPTH, uint32_t FMT>
    PZG_FN static void edge_dword(const Job &J, uint64_t rowq, uint32_t y, uint8_t *out, int64_t lo, uint64_t &bad)
    {
        if (lo >= 0 && (uint64_t)lo + 4u <= J.orb) {
            *(uint32_t *)(void *)out = gather<CT, DEPTH, FMT>(J, rowq, y, lo, (uint64_t)lo, (uint64_t)lo + 4u, bad);
        } else {
            const uint64_t j0 = lo < 0 ? 0u : (uint64_t)lo, j1 = (uint64_t)(lo + 4) < J.orb ? (uint64_t)(lo + 4) : J.orb;
            const uint32_t o = gather<CT, DEPTH, FMT>(J, rowq, y, lo, j0, j1, bad);
            for (uint64_t j = j0; j < j1; ++j) out[(int64_t)j - lo] = (uint8_t)(o >> (8u * (uint32_t)((int64_t)j - lo)));
        }
    }

    // Unit u of the aligned destination of the row at `at`: it holds the row's bytes lo .. lo + 15, lo = 16 u - wal.
    template <uint32_t CT, uint32_t DEPTH, uint32_t FMT>
    PZG_FN static void unit(const Job &J, uint64_t rowq, uint32_t y, uint8_t *at, uint32_t wal, uint64_t u, uint64_t &bad)
    {
        const int64_t lo = (int64_t)(UNIT * u) - (int64_t)wal;
        uint8_t *out = at + lo;  // (16-byte aligned; in front of the row where lo < 0: those bytes are not touched)
        if (lo >= 0 && (uint64_t)lo + UNIT <= J.orb) {
            Quad o;
            o.a = gather<CT, DEPTH, FMT>(J, rowq, y, lo, (uint64_t)lo, (uint64_t)lo + 4u, bad);
            o.b = gather<CT, DEPTH, FMT>(J, rowq, y, lo + 4, (uint64_t)lo + 4u, (uint64_t)lo + 8u, bad);
            o.c = gather<CT, DEPTH, FMT>(J, rowq, y, lo + 8, (uint64_t)lo + 8u, (uint64_t)lo + 12u, bad);
            o.d = gather<CT, DEPTH, FMT>(J, rowq, y, lo + 12, (uint64_t)lo + 12u, (uint64_t)lo + 16u, bad);
            *(Quad *)(void *)out = o;
        } else {
            for (int64_t d = 0; d < (int64_t)UNIT; d += 4)
                if (lo + d + 4 > 0 && lo + d < (int64_t)J.orb) edge_dword<CT, DEPTH, FMT>(J, rowq, y, out + d, lo + d, bad);
        }
    }

    // the smallest of the lanes' values, wave-uniform
    PZG_FN static uint64_t lanes_min64(const LaneVec<uint64_t> &x)
    {
#if PZG_DEVICE_PASS
        uint64_t v = x.v;
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t yl = (uint32_t)__shfl_xor((int)(uint32_t)v, o), yh = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
            const uint64_t y = ((uint64_t)yh << 32) | yl;
            v = y < v ? y : v;
        }
        return uni64(v);
#else
        uint64_t v = x.v[0];
        for (uint32_t k = 1; k < LANES; ++k) v = x.v[k] < v ? x.v[k] : v;
        return v;
#endif
    }

    // the rows slice, slice + slices, ... of the image; returns the smallest key of a bad palette index among them, or NONE
    template <uint32_t CT, uint32_t DEPTH, uint32_t FMT>
    PZG_FN static uint64_t rows(const Job &J, uint32_t height, uint32_t slice, uint32_t slices)
    {
        LaneVec<uint64_t> bad;
        PZG_LANES_BEGIN(k)
        PZG_LV(bad, k) = NONE;
        PZG_LANES_END
        for (uint32_t y = slice; y < height; y += slices) {
            const uint64_t rowq = (uint64_t)y * J.sstride + J.mis;
            uint8_t *at = J.dst + (uint64_t)y * J.dstride;
            const uint32_t wal = (uint32_t)((uintptr_t)at & (UNIT - 1u));
            const uint64_t nu = (wal + J.orb + (UNIT - 1u)) / UNIT;
            PZG_LANES_BEGIN(k)
            uint64_t b = PZG_LV(bad, k);
            for (uint64_t u = k; u < nu; u += LANES) unit<CT, DEPTH, FMT>(J, rowq, y, at, wal, u, b);
            PZG_LV(bad, k) = b;
            PZG_LANES_END
        }
        if constexpr (CT == 3u) return lanes_min64(bad);
        return NONE;
    }

    template <uint32_t CT, uint32_t DEPTH>
    PZG_FN static uint64_t rows_fmt(const Job &J, uint32_t fmt, uint32_t height, uint32_t slice, uint32_t slices)
    {
        return fmt == RGBA8 ? rows<CT, DEPTH, RGBA8>(J, height, slice, slices) : rows<CT, DEPTH, RGB8>(J, height, slice, slices);
    }

    PZG_FN static uint64_t rows_of(const Job &J, uint32_t ct, uint32_t depth, uint32_t fmt, uint32_t height, uint32_t slice, uint32_t slices)
    {
        switch (ct << 8 | depth) {
        case 0x0001u: return rows_fmt<0u, 1u>(J, fmt, height, slice, slices);
        case 0x0002u: return rows_fmt<0u, 2u>(J, fmt, height, slice, slices);
        case 0x0004u: return rows_fmt<0u, 4u>(J, fmt, height, slice, slices);
        case 0x0008u: return rows_fmt<0u, 8u>(J, fmt, height, slice, slices);
        case 0x0010u: return rows_fmt<0u, 16u>(J, fmt, height, slice, slices);
        case 0x0208u: return rows_fmt<2u, 8u>(J, fmt, height, slice, slices);
        case 0x0210u: return rows_fmt<2u, 16u>(J, fmt, height, slice, slices);
        case 0x0301u: return rows_fmt<3u, 1u>(J, fmt, height, slice, slices);
        case 0x0302u: return rows_fmt<3u, 2u>(J, fmt, height, slice, slices);
        case 0x0304u: return rows_fmt<3u, 4u>(J, fmt, height, slice, slices);
        case 0x0308u: return rows_fmt<3u, 8u>(J, fmt, height, slice, slices);
        case 0x0408u: return rows_fmt<4u, 8u>(J, fmt, height, slice, slices);
        case 0x0410u: return rows_fmt<4u, 16u>(J, fmt, height, slice, slices);
        case 0x0608u: return rows_fmt<6u, 8u>(J, fmt, height, slice, slices);
        default: return rows_fmt<6u, 16u>(J, fmt, height, slice, slices);
        }
    }

    // the image's entries into the wave's LDS (the lookups of the image before are over)
    PZG_FN static void load_palette(uint32_t *pal, const uint32_t *entries, uint32_t len)
    {
        wave_sync();
        PZG_LANES_BEGIN(k)
        for (uint32_t e = k; e < len; e += LANES) pal[e] = entries[e];
        PZG_LANES_END
        wave_sync();
    }

    PZG_FN static void answer(int32_t *status, uint32_t *detail, int32_t st, uint32_t d0, uint32_t d1)
    {
        if (lane_id() != 0u) return;
        *status = st;
        if (detail) {
            detail[0] = d0;
            detail[1] = d1;
        }
    }

    // A wave of a palette image has done its rows.  scr[0]: the complement of the smallest key so far (0: none); scr[1]: the waves
    // that have arrived.  The last of the image's `slices` waves writes the answer.
    PZG_FN static void arrive(uint64_t *scr, uint32_t slices, uint64_t bad, int32_t *status, uint32_t *detail)
    {
        if (lane_id() != 0u) return;
#if PZG_DEVICE_PASS
        unsigned long long *w = (unsigned long long *)(void *)scr;
        if (bad != NONE) atomicMax(w, (unsigned long long)~bad);
        __threadfence();  // the key is out before the count says so
        if (atomicAdd(w + 1, 1ull) + 1ull != slices) return;
        __threadfence();
        const uint64_t inv = atomicMax(w, 0ull);  // (reads the word where the other waves' atomics went)
#else
        if (bad != NONE && ~bad > scr[0]) scr[0] = ~bad;
        if (++scr[1] != slices) return;
        const uint64_t inv = scr[0];
#endif
        if (inv == 0u) {
            answer(status, detail, ST_OK, 0u, 0u);
        } else {
            answer(status, detail, ST_PALETTE, (uint32_t)(~inv >> 32), (uint32_t)~inv);
        }
    }

    // One image's share of a wave.  pal: 256 dwords of the wave's own (LDS); scr: the image's two words of the launch's scratch, zero
    // before the launch; status, detail: the image's (detail may be null).
    PZG_FN static void image(const uint8_t *src_base, uint8_t *dst_base, const uint32_t *palette_base, const Desc &D, uint32_t *pal, uint32_t slice,
                             uint32_t slices, uint64_t *scr, int32_t *status, uint32_t *detail)
    {
        if (D.width == 0u || D.height == 0u) {
            if (slice == 0u) answer(status, detail, ST_OK, 0u, 0u);
            return;
        }
        if (!geometry_ok(D)) {
            if (slice == 0u) answer(status, detail, ST_FILTER, BAD_ARGS, (uint32_t)D.color_type << 8 | D.bit_depth);
            return;
        }
        const uint8_t *src = src_base + D.src_off;
        Job J;
        J.mis = (uint32_t)((uintptr_t)src & 3u);
        J.src = (const uint32_t *)(const void *)(src - J.mis);
        J.sstride = D.src_stride;
        J.dst = dst_base + D.dst_off;
        J.dstride = D.dst_stride;
        J.orb = dst_row_bytes(D.width, D.out_format);
        J.width = D.width;
        J.pal = pal;
        J.pal_len = D.pal_len;
        J.has_key = D.has_key;
        J.key0 = D.key[0];
        J.key1 = D.key[1];
        J.key2 = D.key[2];
        if (D.color_type == 3u && slice < D.height) load_palette(pal, palette_base + D.pal_off, D.pal_len);
        const uint64_t bad = rows_of(J, D.color_type, D.bit_depth, D.out_format, D.height, slice, slices);
        if (D.color_type == 3u) {
            arrive(scr, slices, bad, status, detail);
        } else if (slice == 0u) {
            answer(status, detail, ST_OK, 0u, 0u);
        }
    }
};

}  // namespace pzg
