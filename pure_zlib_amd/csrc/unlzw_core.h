// unlzw_core.h -- LZW as TIFF (Compression 5) and PDF (LZWDecode) pack it, decoded by one wavefront per stream (pzg_unlzw_many).
// The contract is the comment of pzg_unlzw_many in include/pzg.h; this is how the wave keeps it.
//   positions       between two Clear codes the width of the j-th code is a function of j alone (rel_bits, width), so the 64 lanes of a
//                   STEP fetch the codes j0 .. j0 + 63 side by side: two aligned dwords a lane, byte-swapped (the codes are packed most
//                   significant bit first), nothing outside the dwords that hold bytes of the stream.  A ballot cuts the step at the
//                   first lane whose code is a Clear, an EOI, incomplete or illegal; the lanes in front of it are the step's codes.
//   no table        entry 258 + m is the string of code m since the Clear plus the first byte of code m + 1: the delivered output from
//                   start[m] to start[m + 1] inclusive.  The "table" is start[]: one output position per code since the last Clear,
//                   3,840 dwords of LDS (Table; start[0 .. min(j0, 3838)] hold at the top of a step).  Its length is
//                   start[m + 1] - start[m] + 1.
//   lengths         a code that names an entry of an earlier step has its length from start[].  One that names an entry made inside
//                   the step -- code m = j0 + q, lane q in front of it -- is one longer than lane q's string: a link (q, +1).  Links are
//                   resolved by pointer jumping through the crossbar, at most six rounds, and as few as the deepest chain needs (none in
//                   most steps of ordinary data; all six where every code is the one just made, as in a run of equal bytes).  The
//                   jumping leaves every lane its ROOT -- the literal or earlier entry its chain ends in -- and its depth.
//   offsets         an inclusive wave scan of the lengths; the ends are the step's entries of start[].
//   the copies      string(k) = string(link) + first byte of string(link + 1), so a string is its root's string and then one first
//                   byte per link of its chain.  First bytes need no output of this step: a lane's is its root's, a literal or one byte
//                   of earlier output (one gather of loads).  Every lane copies its root's string from earlier output to its own place
//                   -- up to 64 bytes by itself in dwords, a longer one by the whole wave, 256 bytes a round -- and walks its chain once,
//                   storing one byte per link.  So NO copy of a step reads what the step wrote, the copies need no order among
//                   themselves, and a step costs one wait for its stores (the top of the next step: s_waitcnt vmcnt(0), as the
//                   stream-waves of inflate_core.h order their far reads), however deep its chains.  The entry made by the last code
//                   of the step in front ends one byte inside this step's output: that byte is lane 0's first byte, from a register.
//   the capacity    every store is held against out_cap; the step in which the output reaches it ends the stream with PZG_OK.
// NOT built: staging of the output in LDS (the strings of a step are copied global to global); a second wave for a long stream;
// codes packed least significant bit first (GIF) and a variable minimum code size.
// The same source compiles as a host program for the CPU model (tests/model/model_unlzw.cpp) and the sanitized program
// (tests/cxx/san_unlzw.cpp): there the 64 lanes are arrays and loops.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "wave.h"

namespace pzg {

struct Unlzw {
    static constexpr uint32_t LANES = 64u, CLEAR = 256u, EOI = 257u, FIRST = 258u, FULL = 4096u;
    static constexpr uint32_t STARTS = 3840u;  // start[0 .. 3838] are used: entry 4095 is code 3837's
    static constexpr uint32_t LONG = 64u;      // a root string longer than this is copied by the whole wave
    static constexpr int32_t ST_OK = 0, ST_TRUNCATED = 1, ST_LZW = 25;  // (PZG_OK, PZG_E_TRUNCATED, PZG_E_LZW: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t ORDINARY = 0u, AT_CLEAR = 1u, AT_EOI = 2u, AT_END = 3u, AT_BAD = 4u;  // what a lane's code is

    struct Table {
        uint32_t start[STARTS];
    };

    struct Result {
        int32_t status;
        uint32_t out_len, d0, d1;
    };

    // the bits in front of code j since the Clear; n9 = 255 - early_change codes have 9 bits, 512 have 10, 1,024 have 11
    PZG_FN static uint64_t rel_bits(uint64_t j, uint32_t n9)
    {
        if (j <= n9) return 9u * j;
        if (j <= n9 + 512u) return 9u * n9 + 10u * (j - n9);
        if (j <= n9 + 1536u) return 9u * n9 + 5120u + 11u * (j - n9 - 512u);
        return 9u * n9 + 16384u + 12u * (j - n9 - 1536u);
    }

    PZG_FN static uint32_t width(uint64_t j, uint32_t n9) { return j < n9 ? 9u : j < n9 + 512u ? 10u : j < n9 + 1536u ? 11u : 12u; }

    PZG_FN static uint32_t load4(const uint8_t *p)
    {
        uint32_t x;
        __builtin_memcpy(&x, p, 4);
        return x;
    }
    PZG_FN static void store4(uint8_t *p, uint32_t x) { __builtin_memcpy(p, &x, 4); }

    // this wave's stores have landed before its later loads are issued
    PZG_FN static void store_fence()
    {
#if PZG_DEVICE_PASS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    }

    // lane k's share of a copy of n bytes by the whole wave: the bytes 4 k .. 4 k + 3 of every 256
    PZG_FN static void wave_copy_lane(uint8_t *d, const uint8_t *s, uint32_t n, uint32_t k)
    {
        for (uint32_t q = 4u * k; q < n; q += 4u * LANES) {
            if (n - q >= 4u) {
                store4(d + q, load4(s + q));
            } else {
                for (uint32_t i = q; i < n; ++i) d[i] = s[i];
            }
        }
    }

    // One stream.  in: its first byte (any alignment; not looked at where in_len is 0); out: where its output goes; T: the wave's table.
    PZG_FN static Result stream(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint32_t early_change, Table &T)
    {
        const uint32_t cap = out_cap > 0xffffffffull ? 0xffffffffu : (uint32_t)out_cap;
        const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);
        const uint32_t *src = (const uint32_t *)(const void *)(in - mis);
        const uint64_t end_byte = mis + in_len, end_bit = 8u * end_byte;
        const uint32_t n9 = 255u - (early_change ? 1u : 0u);
        uint64_t base = 8u * (uint64_t)mis;  // where code 0 since the Clear starts, in bits from src
        uint64_t j0 = 0u;                    // the codes since the Clear in front of this step
        uint32_t pos = 0u;                   // the bytes delivered
        for (;;) {
            if (pos >= cap) return Result{ST_OK, cap, 0u, 0u};
            if (j0 < STARTS && lane_id() == 0u) T.start[j0] = pos;
            wave_sync();
            // the codes, and what each of them is
            LaneVec<uint32_t> code, what, stopv;
            PZG_LANES_BEGIN(k)
            const uint64_t j = j0 + k, P = base + rel_bits(j, n9);
            const uint32_t w = width(j, n9);
            const bool complete = P + w <= end_bit;
            const uint64_t d = P >> 5;
            const uint32_t w0 = complete ? src[d] : 0u, w1 = complete && ((d + 1u) << 2) < end_byte ? src[d + 1u] : 0u;
            const uint64_t x = (uint64_t)__builtin_bswap32(w0) << 32 | __builtin_bswap32(w1);
            const uint32_t c = (uint32_t)(x >> (64u - ((uint32_t)P & 31u) - w)) & ((1u << w) - 1u);
            const uint32_t f = j == 0u ? FIRST : j - 1u < FULL - FIRST ? FIRST + (uint32_t)(j - 1u) : FULL;  // the next free entry
            uint32_t kind = !complete ? AT_END : c == CLEAR ? AT_CLEAR : c == EOI ? AT_EOI : ORDINARY;
            if (kind == ORDINARY && c > EOI && !(c < f || (c == f && j != 0u))) kind = AT_BAD;
            PZG_LV(code, k) = c;
            PZG_LV(what, k) = kind;
            PZG_LV(stopv, k) = kind != ORDINARY ? 1u : 0u;
            PZG_LANES_END
            const uint64_t stops = lanes_ballot(stopv);
            const uint32_t t = stops ? ctz64(stops) : LANES;  // the step's codes are those of the lanes in front of t

            // lengths: known (res), or one more than another lane's (link)
            LaneVec<uint32_t> val, res, link, par, srcv, flags;
            PZG_LANES_BEGIN(k)
            const uint32_t c = PZG_LV(code, k);
            uint32_t v = 0u, r = 1u, l = k, s = 0u, fl = 0u;  // fl: 1 a literal, 2 the entry that ends inside this step
            if (k < t) {
                if (c < CLEAR) {
                    v = 1u;
                    fl = 1u;
                } else {
                    const uint32_t m = c - FIRST;
                    if (m < j0) {
                        s = T.start[m];
                        v = T.start[m + 1u] - s + 1u;
                        fl = m + 1u == j0 ? 2u : 0u;
                    } else {
                        v = 1u;
                        r = 0u;
                        l = m - (uint32_t)j0;
                    }
                }
            }
            PZG_LV(val, k) = v;
            PZG_LV(res, k) = r;
            PZG_LV(link, k) = l;
            PZG_LV(par, k) = l;
            PZG_LV(srcv, k) = s;
            PZG_LV(flags, k) = fl;
            PZG_LANES_END
            for (;;) {
                LaneVec<uint32_t> open;
                PZG_LANES_BEGIN(k)
                PZG_LV(open, k) = PZG_LV(res, k) ^ 1u;
                PZG_LANES_END
                if (lanes_ballot(open) == 0ull) break;
                LaneVec<uint32_t> tv, tr, tl;
                lanes_gather(tv, val, link);
                lanes_gather(tr, res, link);
                lanes_gather(tl, link, link);
                PZG_LANES_BEGIN(k)
                if (!PZG_LV(res, k)) {
                    PZG_LV(val, k) += PZG_LV(tv, k);
                    PZG_LV(res, k) = PZG_LV(tr, k);
                    PZG_LV(link, k) = PZG_LV(tl, k);
                }
                PZG_LANES_END
            }
            // val: the lengths; link: the roots.  Offsets, and the step's entries of start[]
            LaneVec<uint32_t> incl = val, rlen, rsrc, rfl;
            lanes_iscan_add(incl);
            const uint32_t total = lane_get(incl, LANES - 1u);
            lanes_gather(rlen, val, link);
            lanes_gather(rsrc, srcv, link);
            lanes_gather(rfl, flags, link);
            PZG_LANES_BEGIN(k)
            if (k < t && j0 + k + 1u < STARTS) T.start[j0 + k + 1u] = pos + PZG_LV(incl, k);
            PZG_LANES_END
            // first bytes: a root's own, everybody's from its root
            store_fence();
            LaneVec<uint32_t> own, fb;
            PZG_LANES_BEGIN(k)
            uint32_t b = PZG_LV(code, k);
            if (k < t && PZG_LV(link, k) == k && !(PZG_LV(flags, k) & 1u)) b = out[PZG_LV(srcv, k)];
            PZG_LV(own, k) = b;
            PZG_LANES_END
            lanes_gather(fb, own, link);
            const uint32_t fb0 = lane_get(fb, 0u);
            // the roots' strings
            const uint32_t remaining = cap - pos;
            LaneVec<uint32_t> room, ncopy, isl;
            PZG_LANES_BEGIN(k)
            const uint32_t excl = PZG_LV(incl, k) - PZG_LV(val, k);
            const uint32_t rm = k < t && excl < remaining ? remaining - excl : 0u;
            uint32_t n = PZG_LV(rfl, k) & 1u ? 0u : PZG_LV(rlen, k) - (PZG_LV(rfl, k) >> 1);
            n = n < rm ? n : rm;
            uint8_t *d = out + pos + excl;
            if ((PZG_LV(rfl, k) & 1u) && rm) d[0] = (uint8_t)PZG_LV(fb, k);
            if ((PZG_LV(rfl, k) & 2u) && PZG_LV(rlen, k) - 1u < rm) d[PZG_LV(rlen, k) - 1u] = (uint8_t)fb0;
            PZG_LV(room, k) = rm;
            PZG_LV(ncopy, k) = n;
            PZG_LV(isl, k) = n > LONG ? 1u : 0u;
            PZG_LANES_END
            for (uint32_t i = 0u;; i += 4u) {
                LaneVec<uint32_t> more;
                PZG_LANES_BEGIN(k)
                PZG_LV(more, k) = !PZG_LV(isl, k) && i < PZG_LV(ncopy, k) ? 1u : 0u;
                PZG_LANES_END
                if (lanes_ballot(more) == 0ull) break;
                PZG_LANES_BEGIN(k)
                if (PZG_LV(more, k)) {
                    const uint8_t *s = out + PZG_LV(rsrc, k) + i;
                    uint8_t *d = out + pos + (PZG_LV(incl, k) - PZG_LV(val, k)) + i;
                    const uint32_t rem = PZG_LV(ncopy, k) - i;
                    if (rem >= 4u) {
                        store4(d, load4(s));
                    } else {
                        for (uint32_t q = 0u; q < rem; ++q) d[q] = s[q];
                    }
                }
                PZG_LANES_END
            }
            for (uint64_t lm = lanes_ballot(isl); lm != 0ull; lm &= lm - 1ull) {
                const uint32_t L = ctz64(lm);
                const uint8_t *s = out + lane_get(rsrc, L);
                uint8_t *d = out + pos + (lane_get(incl, L) - lane_get(val, L));
                const uint32_t n = lane_get(ncopy, L);
                PZG_LANES_BEGIN(k)
                wave_copy_lane(d, s, n, k);
                PZG_LANES_END
            }
            // the chains: one byte per link, the first byte of the string behind the one linked to
            LaneVec<uint32_t> info, cur;
            PZG_LANES_BEGIN(k)
            PZG_LV(info, k) = PZG_LV(val, k) | PZG_LV(par, k) << 16 | (PZG_LV(link, k) != k ? 1u << 22 : 0u);
            PZG_LV(cur, k) = PZG_LV(info, k);
            PZG_LANES_END
            for (;;) {
                LaneVec<uint32_t> on, nxt, to, g;
                PZG_LANES_BEGIN(k)
                PZG_LV(on, k) = PZG_LV(cur, k) >> 22;
                PZG_LV(to, k) = (PZG_LV(cur, k) >> 16) & 63u;
                PZG_LV(nxt, k) = PZG_LV(to, k) + 1u;
                PZG_LANES_END
                if (lanes_ballot(on) == 0ull) break;
                lanes_gather(g, fb, nxt);
                PZG_LANES_BEGIN(k)
                const uint32_t off = (PZG_LV(cur, k) & 0xffffu) - 1u;
                if (PZG_LV(on, k) && off < PZG_LV(room, k)) out[pos + (PZG_LV(incl, k) - PZG_LV(val, k)) + off] = (uint8_t)PZG_LV(g, k);
                PZG_LANES_END
                lanes_gather(cur, info, to);
            }
            // where the step ends
            if (total >= remaining) return Result{ST_OK, cap, 0u, 0u};
            pos += total;
            if (t == LANES) {
                j0 += LANES;
                continue;
            }
            const uint32_t kind = lane_get(what, t), c = lane_get(code, t);
            if (kind == AT_CLEAR) {
                base += rel_bits(j0 + t, n9) + width(j0 + t, n9);
                j0 = 0u;
                continue;
            }
            if (kind == AT_EOI) return Result{ST_OK, pos, 0u, 0u};
            if (kind == AT_END) return Result{ST_TRUNCATED, pos, 0u, 0u};
            return Result{ST_LZW, pos, c, pos};
        }
    }
};

}  // namespace pzg
