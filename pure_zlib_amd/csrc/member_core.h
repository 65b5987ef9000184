// member_core.h -- the members of a gzip FILE (RFC 1952 2.2: a series of members), found and laid out on the device so that the
// flagship kernel decodes them one wavefront per member in one launch (pzg_gzip_find_members, pzg_gzip_layout).
//
// A member starts with an empty window: unlike the segments of one stream (scan_core.h) members need no marker pass and no
// windows, they only have to be found, sized and laid out.
//   find      the input is cut into chunks, one wave per chunk.  A step takes STEP dwords per lane, coalesced; a lane looks at the
//             four byte positions of each of its dwords, with the bytes behind them from the next lane's dword (the last lane:
//             from the dword that follows the wave's).  Where 1f 8b 08 stands the lane reads on (rare: the rest of the predicate,
//             and the BGZF subfield).  Pass one counts a chunk's candidates, an exclusive scan over the chunks places them, pass
//             two runs the same sweep again and writes the positions, ascending.  Position 0 is entry 0 whatever its bytes.
//   layout    member j is starts[j] .. starts[j + 1] (the last: the end of the input); its room is its ISIZE, the last dword of
//             that extent, capped at DEFLATE's maximum expansion; the output offsets are the exclusive prefix sum of the rooms.
//   scan      the prefix sums are 64-bit and in a fixed order (tiles of TILE entries: a wave sums each, one wave scans the tiles'
//             sums, a wave scans each tile from its tile's sum on): the same result from run to run.
// A candidate is no proof of a member: a false one is found by what uses the list, the decode (pure_zlib_amd/gzfile.py).  Nothing
// is read but the aligned dwords that hold input bytes.  The same source compiles as a one-lane host program for the CPU model
// tests (wave.h); inflate_core.h is not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct Members {
    static constexpr uint32_t STEP = 4u;             // dwords per lane per step of the sweep
    static constexpr uint32_t TILE = 4096u;          // entries per tile of the prefix sums
    static constexpr uint64_t MIN_MEMBER = 18u;      // header (10) + trailer (8): a shorter extent has no ISIZE
    static constexpr uint64_t MAX_EXPANSION = 1032u; // DEFLATE's maximum expansion (zlib's technical notes): the cap of a member's room

    // The input as aligned dwords: input position q is byte (q + mis) & 3 of src[(q + mis) >> 2].
    struct Input {
        const uint32_t *src;
        uint64_t ndw, in_len;
        uint32_t mis;

        PZG_FN void init(const uint8_t *in, uint64_t len)
        {
            mis = (uint32_t)((uintptr_t)in & 3u);
            src = (const uint32_t *)(const void *)(in - mis);
            ndw = (mis + len + 3u) >> 2;
            in_len = len;
        }
        PZG_FN uint32_t dword(uint64_t d) const { return d < ndw ? src[d] : 0u; }
        // q < in_len
        PZG_FN uint32_t byte(uint64_t q) const
        {
            const uint64_t r = q + mis;
            return (src[r >> 2] >> (8u * ((uint32_t)r & 3u))) & 0xffu;
        }
        // the little-endian dword at q (q + 4 <= in_len)
        PZG_FN uint32_t dword_at(uint64_t q) const
        {
            const uint64_t r = q + mis;
            const uint32_t sh = 8u * ((uint32_t)r & 3u), lo = src[r >> 2];
            return sh ? (lo >> sh) | (src[(r >> 2) + 1u] << (32u - sh)) : lo;
        }
    };

    // ---- (a) the member finder ---------------------------------------------------------------------------------------------------
    // Stricter than the decoder's gzip_header(): a member start this misses is decoded by its predecessor's wave, which walks on
    // into it; a false hit costs a repair.
    PZG_FN static bool candidate(const Input &I, uint64_t q)
    {
        if (q + 10u > I.in_len) return false;
        if (I.byte(q) != 0x1fu || I.byte(q + 1u) != 0x8bu || I.byte(q + 2u) != 8u) return false;
        if (I.byte(q + 3u) & 0xe0u) return false;  // FLG: the reserved bits
        const uint32_t xfl = I.byte(q + 8u), os = I.byte(q + 9u);
        return (xfl == 0u || xfl == 2u || xfl == 4u) && (os <= 13u || os == 255u);
    }

    // A candidate's BGZF block size: FEXTRA, and in it a subfield 'B' 'C' of two bytes that lies wholly inside XLEN and inside
    // the input -- its value plus one; else 0.
    PZG_FN static uint32_t block_size(const Input &I, uint64_t q)
    {
        if (!(I.byte(q + 3u) & 4u) || q + 12u > I.in_len) return 0u;
        const uint32_t xlen = I.byte(q + 10u) | (I.byte(q + 11u) << 8);
        const uint64_t x = q + 12u;
        for (uint32_t pos = 0; pos + 4u <= xlen && x + pos + 4u <= I.in_len;) {
            const uint32_t slen = I.byte(x + pos + 2u) | (I.byte(x + pos + 3u) << 8);
            if (I.byte(x + pos) == 66u && I.byte(x + pos + 1u) == 67u && slen == 2u) {
                if (pos + 6u > xlen || x + pos + 6u > I.in_len) return 0u;
                return (I.byte(x + pos + 4u) | (I.byte(x + pos + 5u) << 8)) + 1u;
            }
            pos += 4u + slen;
        }
        return 0u;
    }

    // the next lane's value of v; the last lane: the first lane's value of `after`
    PZG_FN static uint32_t next_lane(uint32_t v, uint32_t after, uint32_t lane)
    {
#if PZG_DEVICE_PASS
        const uint32_t up = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane + 1u) & 63u) << 2), (int)v);
        const uint32_t first = uni(after);
        return lane == 63u ? first : up;
#else
        (void)v;
        (void)lane;
        return after;
#endif
    }

    // Which of the four byte positions of dword d (w0; w1 follows it) are candidates of the chunk [from, to), position 0 apart.
    PZG_FN static uint32_t hits(const Input &I, uint64_t d, uint32_t w0, uint32_t w1, uint64_t from, uint64_t to)
    {
        uint32_t m = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t x = b ? funnel(w1, w0, 8u * b) : w0;
            if ((x & 0xffffffu) == 0x088b1fu) {
                const uint64_t r = 4u * d + b;
                if (r > I.mis) {  // (in front of the input, or position 0)
                    const uint64_t q = r - I.mis;
                    if (q >= from && q < to && candidate(I, q)) m |= 1u << b;
                }
            }
        }
        return m;
    }

    // One chunk: the candidates of [from, to) -- and, first of all, position 0 for the chunk that starts there -- counted; WRITE:
    // and stored from slot `at` on, ascending, as far as there is room.
    template <bool WRITE>
    PZG_FN static uint64_t sweep(const Input &I, uint64_t from, uint64_t to, uint64_t at, uint64_t *starts, uint32_t *bsize, uint64_t room)
    {
        const uint32_t lane = lane_id();
        uint64_t n = 0;
        if (from == 0u) {
            if (WRITE && lane == 0u && at < room) {
                starts[at] = 0u;
                bsize[at] = candidate(I, 0u) ? block_size(I, 0u) : 0u;
            }
            n = 1u;
        }
        if (from >= to) return n;
        const uint64_t d_lo = (from + I.mis) >> 2, d_hi = (to - 1u + I.mis) >> 2;
        for (uint64_t base = d_lo; base <= d_hi; base += STEP * PZG_WAVE) {
            uint32_t v[STEP + 1u];
#pragma unroll
            for (uint32_t u = 0; u < STEP; ++u) v[u] = I.dword(base + u * PZG_WAVE + lane);
            v[STEP] = I.dword(base + STEP * PZG_WAVE);
#pragma unroll
            for (uint32_t u = 0; u < STEP; ++u) {
                const uint64_t d = base + u * PZG_WAVE + lane;
                const uint32_t w1 = next_lane(v[u], v[u + 1u], lane);
                const uint32_t m = d <= d_hi ? hits(I, d, v[u], w1, from, to) : 0u;
                if (ballot(m != 0u) == 0ull) continue;
                const uint32_t c = (uint32_t)__builtin_popcount(m), inc = wave_iscan_add(c);
                if (WRITE) {
                    uint64_t slot = at + n + inc - c;
                    for (uint32_t b = 0; b < 4u; ++b)
                        if ((m >> b) & 1u) {
                            const uint64_t q = 4u * d + b - I.mis;
                            if (slot < room) {
                                starts[slot] = q;
                                bsize[slot] = block_size(I, q);
                            }
                            ++slot;
                        }
                }
                n += uni(read_lane(inc, PZG_WAVE - 1u));
            }
        }
        return n;
    }

    // chunk k of the input
    template <bool WRITE>
    PZG_FN static uint64_t chunk_sweep(const uint8_t *in, uint64_t in_len, uint64_t chunk, uint64_t k, uint64_t at, uint64_t *starts,
                                       uint32_t *bsize, uint64_t room)
    {
        Input I;
        I.init(in, in_len);
        const uint64_t from = k * chunk, to = in_len - from > chunk ? from + chunk : in_len;
        return sweep<WRITE>(I, from, to, at, starts, bsize, room);
    }

    // ---- the prefix sums -------------------------------------------------------------------------------------------------------------
    PZG_FN static uint64_t wave_iscan_add64(uint64_t x, uint32_t lane)
    {
#if PZG_DEVICE_PASS
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t from = ((lane - o) & 63u) << 2;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)from, (int)(uint32_t)x);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)from, (int)(uint32_t)(x >> 32));
            if (lane >= o) x += ((uint64_t)hi << 32) | lo;
        }
#else
        (void)lane;
#endif
        return x;
    }
    PZG_FN static uint64_t last_lane64(uint64_t x)
    {
        return (uint64_t)uni(read_lane((uint32_t)x, PZG_WAVE - 1u)) | ((uint64_t)uni(read_lane((uint32_t)(x >> 32), PZG_WAVE - 1u)) << 32);
    }

    // By one wave: carry + x[lo] + ... + x[hi - 1]; out (null: none; x itself: in place): out[i] = carry + x[lo] + ... + x[i - 1].
    PZG_FN static uint64_t scan_range(const uint64_t *x, uint64_t lo, uint64_t hi, uint64_t carry, uint64_t *out)
    {
        const uint32_t lane = lane_id();
        for (uint64_t i0 = lo; i0 < hi; i0 += PZG_WAVE) {
            const uint64_t i = i0 + lane;
            const uint64_t v = i < hi ? x[i] : 0u;
            const uint64_t inc = wave_iscan_add64(v, lane);
            if (out && i < hi) out[i] = carry + inc - v;
            carry += last_lane64(inc);
        }
        return carry;
    }
    PZG_FN static uint64_t tiles(uint64_t n) { return (n + TILE - 1u) / TILE; }
    // tile t of x[0 .. n): its sum
    PZG_FN static void tile_sum(const uint64_t *x, uint64_t n, uint64_t t, uint64_t *part)
    {
        const uint64_t lo = t * TILE, hi = n - lo > TILE ? lo + TILE : n;
        const uint64_t s = scan_range(x, lo, hi, 0u, nullptr);
        if (lane_id() == 0u) part[t] = s;
    }
    // the tiles' sums become the tiles' offsets, from `base` on; *total: the sum of them all
    PZG_FN static void tile_offsets(uint64_t *part, uint64_t ntiles, uint64_t base, uint64_t *total)
    {
        const uint64_t s = scan_range(part, 0u, ntiles, base, part);
        if (lane_id() == 0u) *total = s - base;
    }
    // tile t: out[i] = the sum of everything in front of x[i], plus the base (out may be x)
    PZG_FN static void tile_scan(const uint64_t *x, uint64_t n, uint64_t t, const uint64_t *part, uint64_t *out)
    {
        const uint64_t lo = t * TILE, hi = n - lo > TILE ? lo + TILE : n;
        scan_range(x, lo, hi, uni64(part[t]), out);
    }

    // ---- (b) the layout ----------------------------------------------------------------------------------------------------------------
    // Member j of m: its extent and its room.  (A start beyond the input, or in front of its predecessor, is taken as the nearest
    // position that is neither: whatever the list holds, the extents lie inside the input.)
    PZG_FN static void member(const Input &I, const uint64_t *starts, uint64_t m, uint64_t j, uint64_t *in_off, uint64_t *in_lenv, uint64_t *out_cap)
    {
        uint64_t s = starts[j], e = j + 1u < m ? starts[j + 1u] : I.in_len;
        if (s > I.in_len) s = I.in_len;
        if (e > I.in_len) e = I.in_len;
        if (e < s) e = s;
        const uint64_t len = e - s;
        uint64_t cap = 0;
        if (len >= MIN_MEMBER) {
            const uint64_t isize = I.dword_at(e - 4u), most = MAX_EXPANSION * len;
            cap = isize < most ? isize : most;
        }
        in_off[j] = s;
        in_lenv[j] = len;
        out_cap[j] = cap;
    }
};

}  // namespace pzg
