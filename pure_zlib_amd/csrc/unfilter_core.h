// unfilter_core.h -- scanline unfiltering (PNG specification section 9; PDF FlateDecode Predictor 10-15) of many images in one
// launch, a wavefront per image (pzg_unfilter_many).  Nothing here knows of PNG: an image is `height` rows of one filter byte and
// row_bytes filtered bytes, delivered without the filter bytes at a stride of the caller's.
//
// Sub, Average and Paeth are recurrences along the row, Up, Average and Paeth down the image: byte j of row y needs byte j - bpp of
// its own row (a), byte j of row y - 1 (b) and byte j - bpp of row y - 1 (c), all reconstructed.  Rows are taken in groups of 64 as
// a skewed diagonal:
//   the diagonal   lane k owns row 64 g + k and runs ONE STEP behind lane k - 1.  A step is four bytes of the row -- a dword, not a
//                  filter unit: whatever bpp is, a step then costs a lane one aligned load and one aligned store, and a group takes
//                  ceil(row_bytes / 4) + 63 steps (bpp 3, the common RGB: 3/4 of the steps the unit would take; bpp 8: twice as many
//                  of half the work).  The dword lane k - 1 finished one step ago is lane k's b: ONE cross-lane shift (DPP
//                  wave_shr:1) a step.  c is a window of bpp bytes back over the last three b dwords the lane received, a the same
//                  window over its own last results (bpp <= 4: a 32-bit shift register, because a then lies inside the dword under
//                  way): registers, no memory.  bpp is a template parameter: every window is a funnel shift by a constant.
//                  All five filters run in the same loop, chosen per lane by selects.
//   the hand-over  lane 0 of group g + 1 reads row 64 g + 63 back from dst.  (LDS cannot hold a row: row_bytes is 32 bits wide.)
//                  It is ordered because loader and storer are the SAME wave: the group ends with s_waitcnt vmcnt(0) behind its
//                  last store -- every store of the wave has been acknowledged by its L1, which is the L1 lane 0's loads then go
//                  through -- and a wavefront observes its own vector memory operations in order.  No other wave writes the image.
//   the fetch      a row starts 1 + row_bytes behind its predecessor, so at any of four misalignments.  A lane reads the aligned
//                  dwords that hold its row one a step, four steps ahead of their use (AHEAD), and funnels each with the one before
//                  it by its row's misalignment.  The dword behind the last one that holds a byte of the image's src_len is never
//                  read (it counts as 0), nor anything in front of the first.  Lane 0's reads of the row above: the same, over the
//                  aligned dwords that hold bytes of that row.
//   the stores     a lane gathers four bytes a step and stores them as ONE aligned dword: where the row's destination is not
//                  dword-aligned, the step's result is funnelled with the step's before it.  The dwords that would reach outside
//                  [0, row_bytes) of the row -- its first and its last at most, and one more behind it -- go as single bytes, those
//                  inside only.  Nothing else is written.
// Errors: the filter bytes of a group are read before any of its rows; the first row of a bad one (> 4) ends the image there, the
// rows in front of it delivered, nothing of it or behind it written.  Rows that do not lie wholly inside src_len are not looked at.
// The same source compiles as a host program for the CPU model (tests/model/model_unfilter.cpp): there the 64 lanes are an array
// and a loop, the shift a copy taken before the step.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct Unfilter {
    static constexpr uint32_t LANES = 64u;  // rows of a group (the device's wave; the host model's array)
    static constexpr uint32_t AHEAD = 4u;   // steps between a dword's load and its use
    static constexpr int32_t ST_OK = 0, ST_TRUNCATED = 1, ST_FILTER = 23;  // (PZG_OK, PZG_E_TRUNCATED, PZG_E_FILTER: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t BAD_ARGS = 0xffffffffu;  // detail[0] of an image whose bpp or stride is not legal

    // one image, wave-uniform
    struct Job {
        const uint32_t *src;  // the aligned dwords that hold the image: input byte q is byte (q + mis) & 3 of src[(q + mis) >> 2]
        uint64_t ndw;         // ... as many as hold a byte of src_len
        uint32_t mis;
        uint8_t *dst;
        uint64_t stride, rowlen;  // rowlen: 1 + row_bytes
        uint32_t rb, nd;          // row_bytes; dwords of a row
    };

    // one row of the group under way, per lane
    struct Row {
        uint32_t active, ft;
        uint64_t xd;               // the aligned dword that holds the row's first filtered byte
        uint32_t m8, xprev;        // 8 * that byte's place in it; the dword in front of the one the step loads
        uint32_t r1, r2, b1, b2;   // the last two results; the last two b dwords
        uint32_t cur;              // the last result, as the next lane takes it
        uint32_t *out;             // the aligned dword that holds the row's first delivered byte
        uint32_t wal;              // ... and that byte's place in it
        const uint32_t *up;        // lane 0 of a group behind the first: the same of the row above, in dst
        uint32_t reads_up, um, upprev;
        uint32_t xs[AHEAD], us[AHEAD];
    };

    PZG_FN static bool bpp_ok(uint32_t bpp) { return bpp == 1u || bpp == 2u || bpp == 3u || bpp == 4u || bpp == 6u || bpp == 8u; }

    // the four bytes that start BPP bytes in front of h0, of the twelve h2 h1 h0
    template <uint32_t BPP>
    PZG_FN static uint32_t window(uint32_t h2, uint32_t h1, uint32_t h0)
    {
        constexpr uint32_t off = 8u - BPP;
        if (off == 0u) return h2;
        if (off == 4u) return h1;
        return off > 4u ? funnel(h0, h1, 8u * (off - 4u)) : funnel(h1, h2, 8u * off);
    }

    // PNG 9.2, 9.4: one byte
    PZG_FN static uint32_t recon(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
    {
        const int32_t pa = (int32_t)b - (int32_t)c, pb = (int32_t)a - (int32_t)c, pc = pa + pb;
        const uint32_t ua = (uint32_t)(pa < 0 ? -pa : pa), ub = (uint32_t)(pb < 0 ? -pb : pb), uc = (uint32_t)(pc < 0 ? -pc : pc);
        const uint32_t paeth = (ua <= ub && ua <= uc) ? a : ub <= uc ? b : c;
        const uint32_t lin = ((ft & 1u ? a : 0u) + (ft & 2u ? b : 0u)) >> (ft == 3u ? 1u : 0u);  // None, Sub, Up, Average (9 bits before the shift)
        return (x + (ft == 4u ? paeth : lin)) & 0xffu;
    }

    // a step's dword: x filtered, b the dword above
    template <uint32_t BPP>
    PZG_FN static uint32_t recon_dword(const Row &R, uint32_t x, uint32_t b)
    {
        const uint32_t cwin = window<BPP>(R.b2, R.b1, b);
        const uint32_t awin = BPP > 4u ? window<BPP>(R.r2, R.r1, 0u) : 0u;
        uint32_t hist = R.r1, rec = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t a = BPP > 4u ? (awin >> (8u * i)) & 0xffu : (hist >> (8u * (4u - (BPP > 4u ? 4u : BPP)))) & 0xffu;
            const uint32_t r = recon(R.ft, (x >> (8u * i)) & 0xffu, a, (b >> (8u * i)) & 0xffu, (cwin >> (8u * i)) & 0xffu);
            rec |= r << (8u * i);
            hist = (hist >> 8) | (r << 24);
        }
        return rec;
    }

    // Row 64 g + k of the image, its filter byte read; rows: those that lie wholly inside src_len.
    PZG_FN static void row_begin(const Job &J, Row &R, uint32_t g, uint32_t k, uint32_t rows)
    {
        const uint64_t r = (uint64_t)LANES * g + k;
        R.active = r < rows ? 1u : 0u;
        R.ft = 0u;
        R.xd = 0u;
        R.m8 = R.xprev = R.r1 = R.r2 = R.b1 = R.b2 = R.cur = 0u;
        R.out = nullptr;
        R.up = nullptr;
        R.wal = R.reads_up = R.um = R.upprev = 0u;
#pragma unroll
        for (uint32_t s = 0; s < AHEAD; ++s) R.xs[s] = R.us[s] = 0u;
        if (!R.active) return;
        const uint64_t q = J.mis + r * J.rowlen;
        R.ft = (J.src[q >> 2] >> (8u * ((uint32_t)q & 3u))) & 0xffu;
        R.xd = (q + 1u) >> 2;
        R.m8 = 8u * ((uint32_t)(q + 1u) & 3u);
        R.xprev = J.src[R.xd];  // (row_bytes >= 1: it holds a byte of the row)
        uint8_t *at = J.dst + r * J.stride;
        R.wal = (uint32_t)((uintptr_t)at & 3u);
        R.out = (uint32_t *)(void *)(at - R.wal);
        if (k == 0u && g != 0u) {
            const uint8_t *above = at - J.stride;
            R.reads_up = 1u;
            R.um = (uint32_t)((uintptr_t)above & 3u);
            R.up = (const uint32_t *)(const void *)(above - R.um);
            R.upprev = R.up[0];
        }
    }

    // the loads of step t into slot t % AHEAD
    PZG_FN static void fetch(const Job &J, Row &R, uint32_t k, uint32_t t, uint32_t s)
    {
        const uint32_t u = t - k;  // (t < k: wraps to a value that is no dword of the row)
        const bool on = R.active && t >= k && u < J.nd;
        R.xs[s] = on && R.xd + u + 1u < J.ndw ? J.src[R.xd + u + 1u] : 0u;
        // dword u + 1 of the row above holds its bytes 4 (u + 1) - um and on
        R.us[s] = on && R.reads_up && 4ull * (u + 1u) < (uint64_t)J.rb + R.um ? R.up[u + 1u] : 0u;
    }

    // Step t of lane k: dword t - k of its row, where the row has one.  shifted: lane k - 1's `cur` as the step found it.
    template <uint32_t BPP>
    PZG_FN static void step(const Job &J, Row &R, uint32_t k, uint32_t t, uint32_t s, uint32_t shifted)
    {
        const uint32_t u = t - k;
        if (!(R.active && t >= k && u < J.nd)) return;
        const uint32_t x = funnel(R.xs[s], R.xprev, R.m8);
        R.xprev = R.xs[s];
        uint32_t b = k ? shifted : 0u;
        if (R.reads_up) {
            b = funnel(R.us[s], R.upprev, 8u * R.um);
            R.upprev = R.us[s];
        }
        const uint32_t rec = recon_dword<BPP>(R, x, b);
        // dword u of the aligned destination holds the row's bytes lo .. lo + 3
        const uint32_t o = R.wal ? funnel(rec, R.r1, 32u - 8u * R.wal) : rec;
        const int64_t lo = 4ll * u - R.wal;
        if (lo >= 0 && lo + 4 <= (int64_t)J.rb) {
            R.out[u] = o;
        } else {
            uint8_t *p = (uint8_t *)(void *)(R.out + u);
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if (lo + j >= 0 && lo + j < (int64_t)J.rb) p[j] = (uint8_t)(o >> (8u * j));
        }
        if (u + 1u == J.nd && R.wal) {  // what the last result still holds: the row's bytes 4 nd - wal and on
            const uint32_t o2 = rec >> (32u - 8u * R.wal);
            uint8_t *p = (uint8_t *)(void *)(R.out + u + 1u);
            const int64_t lo2 = 4ll * J.nd - R.wal;
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j)
                if (j < R.wal && lo2 + j < (int64_t)J.rb) p[j] = (uint8_t)(o2 >> (8u * j));
        }
        R.b2 = R.b1;
        R.b1 = b;
        R.r2 = R.r1;
        R.r1 = rec;
        R.cur = rec;
    }

    // lane k - 1's value of v (lane 0: anything)
    PZG_FN static uint32_t from_lane_above(uint32_t v)
    {
#if PZG_DEVICE_PASS
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
#else
        return v;
#endif
    }

    // One group of one image, by a wave.  n_on: its rows (1 .. 64).  Returns the first lane whose filter byte is bad (its rows in
    // front of that one are delivered), LANES where none is; *bad_ft: that byte.
    template <uint32_t BPP>
    PZG_FN static uint32_t group(const Job &J, uint32_t g, uint32_t rows, uint32_t *bad_ft)
    {
        const uint64_t left = rows - (uint64_t)LANES * g;
        uint32_t n_on = left < LANES ? (uint32_t)left : LANES;
#if PZG_DEVICE_PASS
        const uint32_t k = lane_id();
        Row R;
        row_begin(J, R, g, k, rows);
        const uint64_t bad = ballot(R.active && R.ft > 4u);
        uint32_t first = LANES;
        if (bad) {
            first = ctz64(bad);
            *bad_ft = uni(read_lane(R.ft, first));
            if (k >= first) R.active = 0u;
            n_on = first;
        }
        if (n_on) {
            const uint32_t steps = J.nd + n_on - 1u;
#pragma unroll
            for (uint32_t s = 0; s < AHEAD; ++s) fetch(J, R, k, s, s);
            for (uint32_t t0 = 0; t0 < steps; t0 += AHEAD) {
#pragma unroll
                for (uint32_t s = 0; s < AHEAD; ++s) {
                    const uint32_t shifted = from_lane_above(R.cur);
                    step<BPP>(J, R, k, t0 + s, s, shifted);
                    fetch(J, R, k, t0 + s + AHEAD, s);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the hand-over: the group's stores have landed before the next group's lane 0 loads
        return first;
#else
        Row R[LANES];
        uint32_t first = LANES;
        for (uint32_t k = 0; k < LANES; ++k) {
            row_begin(J, R[k], g, k, rows);
            if (first == LANES && R[k].active && R[k].ft > 4u) {
                first = k;
                *bad_ft = R[k].ft;
            }
        }
        if (first != LANES) {
            for (uint32_t k = first; k < LANES; ++k) R[k].active = 0u;
            n_on = first;
        }
        if (n_on) {
            const uint32_t steps = J.nd + n_on - 1u;
            for (uint32_t k = 0; k < LANES; ++k)
                for (uint32_t s = 0; s < AHEAD; ++s) fetch(J, R[k], k, s, s);
            for (uint32_t t0 = 0; t0 < steps; t0 += AHEAD)
                for (uint32_t s = 0; s < AHEAD; ++s) {
                    uint32_t shifted[LANES];
                    for (uint32_t k = 0; k < LANES; ++k) shifted[k] = k ? R[k - 1u].cur : 0u;
                    for (uint32_t k = 0; k < LANES; ++k) {
                        step<BPP>(J, R[k], k, t0 + s, s, shifted[k]);
                        fetch(J, R[k], k, t0 + s + AHEAD, s);
                    }
                }
        }
        return first;
#endif
    }

    template <uint32_t BPP>
    PZG_FN static void groups(const Job &J, uint32_t rows, uint32_t height, int32_t *status, uint32_t *d0, uint32_t *d1)
    {
        const uint32_t ngroups = (uint32_t)(((uint64_t)rows + LANES - 1u) / LANES);
        for (uint32_t g = 0; g < ngroups; ++g) {
            uint32_t ft = 0;
            const uint32_t first = group<BPP>(J, g, rows, &ft);
            if (first != LANES) {
                *status = ST_FILTER;
                *d0 = LANES * g + first;
                *d1 = ft;
                return;
            }
        }
        if (rows < height) {
            *status = ST_TRUNCATED;
            *d0 = rows;
        }
    }

    // One image, by a wave: its status and detail (every lane returns the same).
    PZG_FN static void image(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t stride, uint32_t row_bytes, uint32_t height, uint32_t bpp,
                             int32_t *status, uint32_t *d0, uint32_t *d1)
    {
        *status = ST_OK;
        *d0 = *d1 = 0u;
        if (row_bytes == 0u || height == 0u) return;
        if (!bpp_ok(bpp) || stride < row_bytes) {
            *status = ST_FILTER;
            *d0 = BAD_ARGS;
            *d1 = bpp;
            return;
        }
        Job J;
        J.mis = (uint32_t)((uintptr_t)src & 3u);
        J.src = (const uint32_t *)(const void *)(src - J.mis);
        J.ndw = (J.mis + src_len + 3u) >> 2;
        J.dst = dst;
        J.stride = stride;
        J.rowlen = 1ull + row_bytes;
        J.rb = row_bytes;
        J.nd = (uint32_t)(((uint64_t)row_bytes + 3u) >> 2);
        const uint64_t whole = src_len / J.rowlen;
        const uint32_t rows = whole < height ? (uint32_t)whole : height;
        switch (bpp) {
        case 1u: groups<1u>(J, rows, height, status, d0, d1); break;
        case 2u: groups<2u>(J, rows, height, status, d0, d1); break;
        case 3u: groups<3u>(J, rows, height, status, d0, d1); break;
        case 4u: groups<4u>(J, rows, height, status, d0, d1); break;
        case 6u: groups<6u>(J, rows, height, status, d0, d1); break;
        default: groups<8u>(J, rows, height, status, d0, d1); break;
        }
    }
};

}  // namespace pzg
