// scan_core.h -- the access points of ONE large raw DEFLATE stream, found in parallel (pzg_index_scan): the block finder plus
// marker window scheme of pugz and rapidgzip.
//
// pzg_index_build finds the points with one sequential decode by one wavefront.  Here the compressed body is cut into chunks and
//   find      one wave per chunk k >= 1 finds the first bit of its chunk at which a dynamic block's header MAY start (find());
//             chunk 0 starts at bit 0, a true block start by definition;
//   decode    one wave per candidate inflates from there over 16-bit SYMBOLS -- a value below 256 is a byte, MARK + j stands for
//             byte j of the 32 KiB in front of the candidate, which the wave does not know -- until a block ends exactly at a later
//             candidate (or the final block ends, or an error).  Nothing is stored but the ring of the last 32 Ki symbols, a
//             64-bit count of the symbols produced and the bit reached;
//   resolve   one workgroup walks the chain 0 -> next[0] -> next[next[0]] ... : the window of the segment reached is the last
//             32768 entries of window(k) ++ ring_k with ring_k's markers looked up in window(k).  Links that lie `span` or more
//             output bytes past the last point become the points, exactly pzg_index_build's rule and layout.
// A wave started at a false candidate decodes garbage; nothing follows from it unless the true chain lands on it, and the chain
// only ever lands on block ends of the true decode.  The points are checked by what uses them: the segments' decode and the
// checksum over it (pure_zlib_amd/indexed.py build_parallel).
//
// The token loop is sequential and wave-uniform (every lane computes the same scalars); the wave works as one in the refills
// of the input window, the table builds and the match copies.  The ring lives in the wave's own 64 KiB slot of device memory
// (L2), not in LDS: 64 KiB of LDS per wave would leave two waves to a CU, and a chunk per wave wants thousands resident.  The slot
// holds the ring as it was written, circularly: the symbol of output position p of the segment at entry p & 32767.
// The same source compiles as a host program for the CPU model tests (wave.h); inflate_core.h is not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct ScanResult {
    int32_t status;       // 0, or S_SCAN (PZG_E_SCAN)
    uint32_t d0, d1, npoints;
    uint64_t out_len, in_used;
};

struct ScanLds {
    static constexpr uint32_t IN_DW = 512u, IN_BLK = 256u;  // the input window: 2 KiB, refilled by halves
    static constexpr uint32_t PB_LIT = 10u, PB_DIST = 8u, PB_CL = 7u;
    uint32_t in[IN_DW];
    uint16_t lit_pri[1u << PB_LIT], dist_pri[1u << PB_DIST];  // codes up to PB bits: symbol | length << 9 (0: longer, or none)
    uint16_t lit_sym[288], dist_sym[32];                      // the symbols sorted by (length, symbol), the same entries
    uint16_t lit_cnt[16], lit_first[16], lit_start[16];       // per length: codes, the first code, where they start in *_sym
    uint16_t dist_cnt[16], dist_first[16], dist_start[16];
    uint8_t lens[320];
};

struct Scan {
    static constexpr uint32_t RING = 32768u, RMASK = RING - 1u, MARK = 32768u;
    static constexpr uint64_t NONE = ~0ull;               // cand[k]: the chunk has no candidate
    static constexpr uint32_t NEXT_FINAL = 0xffffffffu;   // next[k]: the segment ended with the final block
    static constexpr uint32_t NEXT_FAIL = 0x80000000u;    // next[k] = NEXT_FAIL | status (status 0: a dead wave, or no candidate)
    // A wave that started at a false candidate decodes garbage, and garbage can go on for long.  A true segment ends at the first
    // candidate that is a block end of the true decode; it passes a candidate only when that one is false (the finder keeps ONE per
    // chunk, the first, so a false one in front of a true block start hides that start).  How often the predicate lets a position of
    // arbitrary bits through has not been measured: the estimate is one in some 10^7 (the first three rules alone pass about one
    // in 10^3, the complete literal/length code is the strict one), and on the streams of the tests no true segment passes more
    // than a few.  Eight in a row would fail a sound stream's scan (PZG_E_SCAN): the caller's sequential decode then takes over.
    // The bound counts candidates, not chunks, because a true segment may span any number of chunks without one (a run of stored or
    // fixed blocks; a stream of those alone is ONE segment).  So a false wave with only candidate-free chunks behind it is not
    // stopped by this bound: it ends where garbage ends, at an impossible code, length or distance symbol, a bad stored length or
    // the end of the input -- in the worst case the rest of the input, once, by one wave.  Chunk 0's wave is true by definition
    // and never stopped.
    static constexpr uint32_t DEAD_AFTER = 8u;
    // statuses (the numbers of include/pzg.h)
    enum : uint32_t { S_OK = 0, S_TRUNCATED = 1, S_LEN_NLEN = 5, S_BTYPE = 6, S_HUFF_BUILD = 7, S_EMPTY_BRANCH = 9, S_BAD_LITLEN = 12,
                      S_BAD_DIST = 13, S_SCAN = 22 };

    struct Code {
        uint16_t *pri;
        uint32_t pb;
        uint16_t *sym, *cnt, *first, *start;
    };
    PZG_FN static Code lit_code(ScanLds &L) { return Code{L.lit_pri, ScanLds::PB_LIT, L.lit_sym, L.lit_cnt, L.lit_first, L.lit_start}; }
    PZG_FN static Code dist_code(ScanLds &L) { return Code{L.dist_pri, ScanLds::PB_DIST, L.dist_sym, L.dist_cnt, L.dist_first, L.dist_start}; }
    // (the code-length code is done with before the distance code is built: it borrows that one's arrays)
    PZG_FN static Code cl_code(ScanLds &L) { return Code{L.dist_pri, ScanLds::PB_CL, L.dist_sym, L.dist_cnt, L.dist_first, L.dist_start}; }

    // ---- the input: aligned dwords through a window in LDS, a 64-bit holder in front of it --------------------------------------
    // Bit positions of the reader count from bit 0 of src[0]; dwords from ndw on read as zeros (callers compare bitpos() with the
    // end of the input).  All of it is wave-uniform.
    struct Reader {
        uint32_t *win;
        const uint32_t *src;
        uint64_t ndw, lo, hi, next, hold;
        uint32_t cnt, tail;  // tail: the bits of the last dword that are input (what follows them in it reads as zeros too)

        PZG_FN void init(uint32_t *w, const uint32_t *s, uint64_t n, uint64_t end_bit)
        {
            win = w; src = s; ndw = n; lo = hi = next = hold = 0; cnt = 0;
            const uint32_t keep = n ? (uint32_t)(end_bit - 32u * (n - 1u)) : 32u;
            tail = keep >= 32u ? ~0u : (1u << keep) - 1u;
        }
        PZG_FN void load_block()
        {
            wave_sync();
            for (uint32_t j = lane_id(); j < ScanLds::IN_BLK; j += PZG_WAVE) {
                const uint64_t d = hi + j;
                win[d & (ScanLds::IN_DW - 1u)] = d + 1u < ndw ? src[d] : d + 1u == ndw ? src[d] & tail : 0u;
            }
            hi += ScanLds::IN_BLK;
            if (hi - lo > ScanLds::IN_DW) lo = hi - ScanLds::IN_DW;
            wave_sync();
        }
        // dwords dlo .. dhi (dhi - dlo < IN_BLK) are in the window afterwards
        PZG_FN void want(uint64_t dlo, uint64_t dhi)
        {
            if (dlo < lo || dlo >= hi) lo = hi = dlo & ~(uint64_t)(ScanLds::IN_BLK - 1u);
            while (hi <= dhi) load_block();
        }
        PZG_FN void refill()
        {
            if (cnt <= 32u) {
                want(next, next);
                hold |= (uint64_t)uni(win[next & (ScanLds::IN_DW - 1u)]) << cnt;
                cnt += 32u;
                ++next;
            }
        }
        PZG_FN void drop(uint32_t n) { hold >>= n; cnt -= n; }
        // n <= 16 bits (after refill(): 32 or more are there)
        PZG_FN uint32_t get(uint32_t n)
        {
            const uint32_t v = (uint32_t)hold & ((1u << n) - 1u);
            drop(n);
            return v;
        }
        PZG_FN uint64_t bitpos() const { return 32u * next - cnt; }
        PZG_FN void seek(uint64_t bit)
        {
            next = bit >> 5;
            hold = 0;
            cnt = 0;
            refill();
            drop((uint32_t)bit & 31u);
        }
    };

    // ---- canonical codes ---------------------------------------------------------------------------------------------------------
    // The tables of the code with lengths lens[0..n): returns 2^15 - the Kraft sum in units of 2^-15 (0: complete, below: over-
    // subscribed, above: incomplete); ncodes: the symbols that have a code.  The wave sorts the symbols length by length (a ballot
    // gives every symbol its rank) and then fills the primary table, a symbol to a lane.
    PZG_FN static int32_t build_code(const uint8_t *lens, uint32_t n, const Code &c, uint32_t &ncodes)
    {
        const uint32_t lane = lane_id();
        wave_sync();
        for (uint32_t j = lane; j < (1u << c.pb); j += PZG_WAVE) c.pri[j] = 0;
        uint32_t idx = 0, code = 0;
        int32_t left = 1;
        for (uint32_t l = 1; l <= 15u; ++l) {
            const uint32_t start = idx;
            for (uint32_t s0 = 0; s0 < n; s0 += PZG_WAVE) {
                const uint32_t s = s0 + lane;
                const bool has = s < n && lens[s] == l;
                const uint64_t m = ballot(has);
                if (has) c.sym[idx + mbcnt_k(m, lane)] = (uint16_t)(s | (l << 9));
                idx += popc64(m);
            }
            const uint32_t cn = idx - start;
            left = left * 2 - (int32_t)cn;
            if (lane == 0) {
                c.cnt[l] = (uint16_t)cn;
                c.first[l] = (uint16_t)code;
                c.start[l] = (uint16_t)start;
            }
            code = (code + cn) << 1;
        }
        wave_sync();
        ncodes = idx;
        if (left < 0) return left;  // (its codes are no codes: the caller gives up on the block)
        for (uint32_t i = lane; i < idx; i += PZG_WAVE) {
            const uint32_t e = c.sym[i], l = e >> 9;
            if (l <= c.pb) {
                const uint32_t cd = (uint32_t)c.first[l] + i - (uint32_t)c.start[l];
                for (uint32_t j = bitrev32(cd) >> (32u - l); j < (1u << c.pb); j += 1u << l) c.pri[j] = (uint16_t)e;
            }
        }
        wave_sync();
        return left;
    }

    // the next symbol of code c (r refilled); false: the bits are no code of it
    PZG_FN static bool decode_sym(Reader &r, const Code &c, uint32_t &sym)
    {
        const uint32_t e = uni(c.pri[(uint32_t)r.hold & ((1u << c.pb) - 1u)]);
        if (e) {
            r.drop(e >> 9);
            sym = e & 511u;
            return true;
        }
        uint32_t code = 0;
        for (uint32_t l = 1; l <= 15u; ++l) {
            code = (code << 1) | ((uint32_t)(r.hold >> (l - 1u)) & 1u);
            const uint32_t d = code - uni(c.first[l]);
            if (d < uni(c.cnt[l])) {
                sym = uni(c.sym[uni(c.start[l]) + d]) & 511u;
                r.drop(l);
                return true;
            }
        }
        return false;
    }

    // HCLEN's order of the code-length code's lengths (RFC 1951 3.2.7), five bits each
    PZG_FN static uint32_t cl_order(uint32_t i)
    {
        // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
        const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                           11ull << 50 | 4ull << 55;
        const uint64_t b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        return (uint32_t)((i < 12u ? a >> (5u * i) : b >> (5u * (i - 12u))) & 31u);
    }

    // A dynamic block's header from HLIT on (RFC 1951 3.2.7), by the rules of zlib's inflate: both codes built, or a status.
    // lit_complete: the literal/length code is complete (it may also be ONE code of length 1).
    PZG_FN static uint32_t read_dynamic(Reader &r, ScanLds &L, uint64_t end_bit, bool &lit_complete)
    {
        const uint32_t lane = lane_id();
        lit_complete = false;
        r.refill();
        const uint32_t hlit = r.get(5), hdist = r.get(5), hclen = r.get(4) + 4u;
        if (hlit > 29u || hdist > 29u) return S_HUFF_BUILD;
        wave_sync();
        for (uint32_t j = lane; j < 19u; j += PZG_WAVE) L.lens[j] = 0;
        wave_sync();
        for (uint32_t i = 0; i < hclen; ++i) {
            r.refill();
            const uint32_t v = r.get(3);
            if (lane == 0) L.lens[cl_order(i)] = (uint8_t)v;
        }
        uint32_t nc;
        const Code cl = cl_code(L);
        if (build_code(L.lens, 19u, cl, nc) != 0) return S_HUFF_BUILD;
        const uint32_t total = hlit + 257u + hdist + 1u;
        uint32_t i = 0, prev = 0;
        while (i < total) {
            uint32_t s;
            r.refill();
            if (!decode_sym(r, cl, s)) return S_EMPTY_BRANCH;
            if (s < 16u) {
                if (lane == 0) L.lens[i] = (uint8_t)s;
                prev = s;
                ++i;
                continue;
            }
            uint32_t rep, v = 0;
            if (s == 16u) {
                if (i == 0) return S_HUFF_BUILD;
                rep = 3u + r.get(2);
                v = prev;
            } else if (s == 17u) {
                rep = 3u + r.get(3);
            } else {
                rep = 11u + r.get(7);
            }
            if (i + rep > total) return S_HUFF_BUILD;
            for (uint32_t j = lane; j < rep; j += PZG_WAVE) L.lens[i + j] = (uint8_t)v;
            i += rep;
            prev = v;
        }
        if (r.bitpos() > end_bit) return S_TRUNCATED;
        wave_sync();
        if (uni(L.lens[256]) == 0u) return S_HUFF_BUILD;
        const Code lc = lit_code(L), dc = dist_code(L);
        int32_t left = build_code(L.lens, hlit + 257u, lc, nc);
        if (left < 0 || (left > 0 && !(nc == 1u && uni(lc.cnt[1]) == 1u))) return S_HUFF_BUILD;
        lit_complete = left == 0;
        left = build_code(L.lens + hlit + 257u, hdist + 1u, dc, nc);
        if (left < 0 || (left > 0 && !(nc == 0u || (nc == 1u && uni(dc.cnt[1]) == 1u)))) return S_HUFF_BUILD;
        return S_OK;
    }

    PZG_FN static void build_fixed(ScanLds &L)
    {
        wave_sync();
        for (uint32_t j = lane_id(); j < 320u; j += PZG_WAVE) L.lens[j] = (uint8_t)(j < 144u ? 8u : j < 256u ? 9u : j < 280u ? 7u : j < 288u ? 8u : 5u);
        wave_sync();
        uint32_t nc;
        build_code(L.lens, 288u, lit_code(L), nc);
        build_code(L.lens + 288u, 32u, dist_code(L), nc);
    }

    // ---- (a) the finder ------------------------------------------------------------------------------------------------------------
    // The cheap part of the candidate predicate, a position to a lane: w0..w3 are the four dwords from the one that holds the
    // position's bit, sh that bit's place in w0.  BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, and the HCLEN + 4 lengths of
    // the code-length code are a complete code.
    PZG_FN static bool cheap(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t sh)
    {
        const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
        const uint64_t x = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;  // bits 0 .. 63 from the position
        if ((x & 7u) != 4u) return false;
        if (((x >> 3) & 31u) > 29u || ((x >> 8) & 31u) > 29u) return false;
        const uint32_t hclen = (uint32_t)((x >> 13) & 15u) + 4u;
        const uint64_t z = x >> 17;                                       // lengths 0 .. 14
        const uint32_t t = (uint32_t)(x >> 62) | ((uint32_t)(hi >> sh) << 2);  // lengths 15 .. 18
        uint32_t sum = 0;
        for (uint32_t i = 0; i < 19u; ++i) {
            const uint32_t l = i < 15u ? (uint32_t)(z >> (3u * i)) & 7u : (t >> (3u * (i - 15u))) & 7u;
            if (i < hclen && l) sum += 128u >> l;
        }
        return sum == 128u;
    }

    // The smallest candidate position in [from, to), reader bits, or NONE.  A candidate: cheap() holds, the header reads by
    // read_dynamic() without a status and inside the input, and its literal/length code is complete.
    PZG_FN static uint64_t find(ScanLds &L, const uint32_t *src, uint64_t ndw, uint64_t end_bit, uint64_t from, uint64_t to)
    {
        Reader r;
        r.init(L.in, src, ndw, end_bit);
        const uint32_t lane = lane_id();
        for (uint64_t b = from; b < to; b += PZG_WAVE) {
            const uint64_t p = b + lane, d = p >> 5;
            r.want(b >> 5, (b >> 5) + 5u);
            const uint32_t w0 = L.in[d & (ScanLds::IN_DW - 1u)], w1 = L.in[(d + 1u) & (ScanLds::IN_DW - 1u)];
            const uint32_t w2 = L.in[(d + 2u) & (ScanLds::IN_DW - 1u)], w3 = L.in[(d + 3u) & (ScanLds::IN_DW - 1u)];
            uint64_t m = ballot(p < to && cheap(w0, w1, w2, w3, (uint32_t)p & 31u));
            while (m) {
                const uint64_t q = b + ctz64(m);
                m &= m - 1u;
                bool complete;
                r.seek(q);
                r.refill();
                r.drop(3);
                if (read_dynamic(r, L, end_bit, complete) == S_OK && complete) return q;
            }
        }
        return NONE;
    }

    // ---- (b) the marker pass -----------------------------------------------------------------------------------------------------
    // Segment k: from cand[k] to the first block end that is a later candidate.  mis_bits: the reader's bit of the stream's bit 0.
    PZG_FN static void decode(ScanLds &L, const uint32_t *src, uint64_t ndw, uint32_t mis_bits, uint64_t end_bit, const uint64_t *cand,
                              uint32_t n, uint32_t k, uint16_t *ring, uint32_t *next_out, uint64_t *count_out, uint64_t *endbit_out)
    {
        const uint32_t lane = lane_id();
        const uint64_t start = uni64(cand[k]);
        uint32_t next = NEXT_FAIL;
        uint64_t count = 0, reached = 0;
        if (start != NONE) {
            for (uint32_t j = lane; j < RING; j += PZG_WAVE) ring[j] = (uint16_t)(MARK + j);
            Reader r;
            r.init(L.in, src, ndw, end_bit);
            r.seek(start + mis_bits);
            const Code lc = lit_code(L), dc = dist_code(L);
            uint32_t cur = k + 1u, passed = 0, st = S_OK;
            for (;;) {
                r.refill();
                const uint32_t bfinal = r.get(1), btype = r.get(2);
                if (btype == 3u) {
                    st = S_BTYPE;
                } else if (btype == 0u) {
                    r.drop((8u - ((uint32_t)r.bitpos() & 7u)) & 7u);
                    r.refill();
                    const uint32_t len = r.get(16);
                    r.refill();
                    const uint32_t nlen = r.get(16);
                    if (r.bitpos() > end_bit) st = S_TRUNCATED;
                    else if ((len ^ nlen) != 0xffffu) st = S_LEN_NLEN;
                    else if (r.bitpos() + 8ull * len > end_bit) st = S_TRUNCATED;
                    else {
                        for (uint32_t i = 0; i < len; ++i) {
                            r.refill();
                            const uint32_t v = r.get(8);
                            if (lane == 0) ring[(uint32_t)(count + i) & RMASK] = (uint16_t)v;
                        }
                        count += len;
                    }
                } else {
                    bool complete;
                    if (btype == 1u) build_fixed(L);
                    else st = read_dynamic(r, L, end_bit, complete);
                    while (st == S_OK) {
                        uint32_t sym;
                        r.refill();
                        if (!decode_sym(r, lc, sym)) { st = S_EMPTY_BRANCH; break; }
                        if (r.bitpos() > end_bit) { st = S_TRUNCATED; break; }
                        if (sym < 256u) {
                            if (lane == 0) ring[(uint32_t)count & RMASK] = (uint16_t)sym;
                            ++count;
                            continue;
                        }
                        if (sym == 256u) break;
                        if (sym > 285u) { st = S_BAD_LITLEN; break; }
                        uint32_t len;
                        if (sym < 265u) len = sym - 254u;
                        else if (sym == 285u) len = 258u;
                        else {
                            const uint32_t e = (sym - 261u) >> 2;
                            len = 3u + ((4u + ((sym - 265u) & 3u)) << e) + r.get(e);
                        }
                        uint32_t ds;
                        r.refill();
                        if (!decode_sym(r, dc, ds)) { st = S_EMPTY_BRANCH; break; }
                        if (ds > 29u) { st = S_BAD_DIST; break; }
                        uint32_t dist;
                        if (ds < 4u) dist = ds + 1u;
                        else {
                            const uint32_t e = (ds >> 1) - 1u;
                            dist = 1u + ((2u + (ds & 1u)) << e) + r.get(e);
                        }
                        if (r.bitpos() > end_bit) { st = S_TRUNCATED; break; }
                        // the copy: element i comes from i % dist of the `dist` symbols in front of the match -- all of them older
                        // than the match, so the lanes need not wait for one another.  (A distance within `len` of the ring's size
                        // makes a lane's source the entry a LATER element overwrites: every round loads before it stores.)
                        wave_sync();  // the stores so far, lane 0's literals among them, are visible to every lane
                        const uint32_t from = (uint32_t)count - dist;
                        for (uint32_t i0 = 0; i0 < len; i0 += PZG_WAVE) {
                            const uint32_t i = i0 + lane;
                            if (i < len) {
                                const uint32_t o = dist >= len ? i : i % dist;
                                const uint16_t v = ring[(from + o) & RMASK];
                                ring[((uint32_t)count + i) & RMASK] = v;
                            }
                        }
                        count += len;
                    }
                }
                reached = r.bitpos() - mis_bits;
                if (st != S_OK) {
                    next = NEXT_FAIL | st;
                    break;
                }
                if (bfinal) {
                    next = NEXT_FINAL;
                    break;
                }
                // the block ended at `reached`: the cursor moves up to the first candidate that is not in front of it
                while (cur < n) {
                    const uint64_t c = uni64(cand[cur]);
                    if (c != NONE && c >= reached) break;
                    if (c != NONE) ++passed;
                    ++cur;
                }
                if (cur < n && uni64(cand[cur]) == reached) {
                    next = cur;
                    break;
                }
                if (k != 0u && passed >= DEAD_AFTER) break;  // dead: NEXT_FAIL | 0
            }
        }
        if (lane == 0) {
            next_out[k] = next;
            count_out[k] = count;
            endbit_out[k] = reached;
        }
    }

    // ---- (c) the chain walk --------------------------------------------------------------------------------------------------------
    // One workgroup of nt threads (the host model: one).  wbuf: 2 x 32768 bytes, the window of the segment reached and the one
    // being made: entry j is the byte at output position out_pos - 32768 + j, 0 where that lies in front of the stream.
    PZG_FN static void resolve(uint32_t tid, uint32_t nt, const uint64_t *cand, const uint32_t *next, const uint64_t *count,
                               const uint64_t *endbit, const uint16_t *rings, uint32_t n, uint64_t span, uint8_t *wbuf, uint64_t *points,
                               uint32_t max_points, uint8_t *windows, ScanResult *res)
    {
        uint8_t *wo = wbuf, *wn = wbuf + RING;
        for (uint32_t j = tid; j < RING; j += nt) wo[j] = 0;
        wave_sync();
        uint32_t k = 0, np = 0, d0 = 0;
        uint64_t out_pos = 0, last = 0;
        for (uint32_t step = 0; step < n; ++step) {
            const uint32_t nx = next[k];
            const uint64_t cnt = count[k];
            if (nx == NEXT_FINAL) {
                if (tid == 0) *res = ScanResult{(int32_t)S_OK, 0u, 0u, np, out_pos + cnt, (endbit[k] + 7u) >> 3};
                return;
            }
            if ((nx & NEXT_FAIL) || nx <= k || nx >= n) {
                d0 = (nx & NEXT_FAIL) ? nx & ~NEXT_FAIL : 0u;
                break;
            }
            const uint16_t *ring = rings + (size_t)k * RING;
            for (uint32_t j = tid; j < RING; j += nt) {
                uint32_t b;
                if (cnt + j < RING) {
                    b = wo[(uint32_t)cnt + j];
                } else {
                    const uint32_t s = ring[((uint32_t)cnt + j) & RMASK];  // (cnt - 32768 + j modulo the ring)
                    b = s >= MARK ? wo[s - MARK] : s;
                }
                wn[j] = (uint8_t)b;
            }
            wave_sync();
            out_pos += cnt;
            if (out_pos - last >= span) {
                if (np < max_points) {
                    if (tid == 0) {
                        points[2 * (size_t)np] = cand[nx];
                        points[2 * (size_t)np + 1] = out_pos;
                    }
                    if (windows) {
                        const uint32_t w = out_pos < RING ? (uint32_t)out_pos : RING;
                        for (uint32_t j = RING - w + tid; j < RING; j += nt) windows[(size_t)np * RING + j] = wn[j];
                    }
                }
                ++np;
                last = out_pos;
            }
            uint8_t *t = wo;
            wo = wn;
            wn = t;
            k = nx;
        }
        if (tid == 0) *res = ScanResult{(int32_t)S_SCAN, d0, (uint32_t)cand[k], np, out_pos, 0u};
    }
};

// ---- many streams in one launch (pzg_index_scan_many) ----------------------------------------------------------------------------
// The chunks of all streams form ONE list, stream after stream: stream s owns entries first_chunk[s] .. first_chunk[s + 1] of cand,
// next, count, endbit and rings, cut from its own first byte, and slot s of the walk's windows and of the results.  A wave (find,
// decode) or a workgroup (resolve) finds its stream and hands that stream's slices to Scan's three passes as they are: to them
// every stream is the only one.
struct ScanStream {
    uint64_t in_off, in_len;         // the stream: in_base + in_off .. + in_len
    uint32_t point_off, max_points;  // its slots of points and windows: point_off .. + max_points
    uint64_t reserved;
};

struct ScanMany {
    // The stream that owns entry g of the list: the last s with first_chunk[s] <= g.  first_chunk: n + 1 entries, ascending,
    // first_chunk[0] = 0 and g < first_chunk[n]; a stream without chunks (two equal entries) owns nothing.  Wave-uniform.
    PZG_FN static uint32_t locate(const uint32_t *first_chunk, uint32_t n, uint32_t g)
    {
        uint32_t lo = 0, hi = n;  // first_chunk[lo] <= g < first_chunk[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (uni(first_chunk[mid]) <= g) lo = mid;
            else hi = mid;
        }
        return lo;
    }

    // the input of one stream as Scan reads it: the aligned dwords that hold its bytes, the stream's bit 0 at bit mis_bits of src[0]
    struct Input {
        const uint32_t *src;
        uint64_t ndw, end_bit, in_len;
        uint32_t mis_bits;
    };
    PZG_FN static Input input(const uint8_t *in_base, const ScanStream &st)
    {
        const uint8_t *in = in_base + uni64(st.in_off);
        const uint32_t mis = (uint32_t)((uintptr_t)in & 3u);
        Input I;
        I.in_len = uni64(st.in_len);
        I.src = (const uint32_t *)(const void *)(in - mis);
        I.ndw = (mis + I.in_len + 3u) >> 2;
        I.mis_bits = 8u * mis;
        I.end_bit = 8u * (mis + I.in_len);
        return I;
    }

    // entry g of the list: the candidate of that chunk of its stream (its chunk 0: bit 0)
    PZG_FN static void find(ScanLds &L, const uint8_t *in_base, const ScanStream *streams, const uint32_t *first_chunk, uint32_t n,
                            uint64_t chunk, uint32_t g, uint64_t *cand)
    {
        const uint32_t s = locate(first_chunk, n, g), k = g - uni(first_chunk[s]);
        uint64_t q = 0;
        if (k) {
            const Input I = input(in_base, streams[s]);
            const uint64_t from = 8u * (uint64_t)k * chunk, all = 8u * I.in_len;
            const uint64_t to = from + 8u * chunk < all ? from + 8u * chunk : all;
            q = Scan::find(L, I.src, I.ndw, I.end_bit, from + I.mis_bits, to + I.mis_bits);
            if (q != Scan::NONE) q -= I.mis_bits;
        }
        if (lane_id() == 0) cand[g] = q;
    }

    // entry g of the list: the segment from that chunk's candidate, over its stream's candidates alone
    PZG_FN static void decode(ScanLds &L, const uint8_t *in_base, const ScanStream *streams, const uint32_t *first_chunk, uint32_t n,
                              uint32_t g, const uint64_t *cand, uint16_t *rings, uint32_t *next, uint64_t *count, uint64_t *endbit)
    {
        const uint32_t s = locate(first_chunk, n, g), base = uni(first_chunk[s]), nk = uni(first_chunk[s + 1u]) - base;
        const Input I = input(in_base, streams[s]);
        Scan::decode(L, I.src, I.ndw, I.mis_bits, I.end_bit, cand + base, nk, g - base, rings + (size_t)g * Scan::RING, next + base,
                     count + base, endbit + base);
    }

    // stream s: its chain, its points and windows into its own slots, its result.  wbufs: 2 x 32768 bytes per stream.
    PZG_FN static void resolve(uint32_t tid, uint32_t nt, const ScanStream *streams, const uint32_t *first_chunk, uint32_t s,
                               const uint64_t *cand, const uint32_t *next, const uint64_t *count, const uint64_t *endbit,
                               const uint16_t *rings, uint64_t span, uint8_t *wbufs, uint64_t *points, uint8_t *windows, ScanResult *results)
    {
        const uint32_t base = first_chunk[s], nk = first_chunk[s + 1u] - base;
        const size_t slot = streams[s].point_off;
        Scan::resolve(tid, nt, cand + base, next + base, count + base, endbit + base, rings + (size_t)base * Scan::RING, nk, span,
                      wbufs + (size_t)s * 2u * Scan::RING, points + 2u * slot, streams[s].max_points,
                      windows ? windows + slot * Scan::RING : nullptr, results + s);
    }
};

}  // namespace pzg
