// unshuffle_core.h -- the byte-plane transpose ("shuffle") undone, with or without a byte-wise running sum in front of it, and the
// clipping of the result to a window, of many jobs in one launch (pzg_unshuffle_many).  With the sum it is TIFF's floating-point
// predictor (Predictor 3; TIFF Technical Note 3), without it the shuffle filter that HDF5, Zarr and Blosc put in front of zlib.
// Nothing here knows of TIFF's tags: a job is `rows` stored rows of src_row_bytes = n * B bytes, dense, B = elem_bytes; of them the
// window -- rows [win_row, win_row + win_rows), of each the bytes [win_byte, win_byte + win_bytes) of the RECONSTRUCTED row, which
// may start or end inside an element -- is delivered at a stride of the caller's.
//   the rule        1. t[k] = stored[k] + t[k - S] modulo 256 over ALL n * B bytes of the row, S = sum_stride (S = 0: t = stored);
//                   2. t is B planes of n bytes; byte j of output element i is t[j * n + i] (reverse: t[(B - 1 - j) * n + i]).
//                   n is a multiple of S, so byte i of every plane is of channel i mod S, and the value at byte i of plane p is the
//                   channel's total over the planes 0 .. p-1 plus its inclusive sum inside plane p.
//   the runs        a lane owns E = 8 consecutive elements: it reads its 8 bytes from each of the B planes -- the three aligned dwords
//                   that hold them, funnelled by that plane's own misalignment -- and stores 8 B contiguous bytes.  B and S are
//                   template parameters: every register index is a constant.  `reverse` is not: the elements are built with plane j
//                   as byte j and reversed by ONE v_perm_b32 a dword with a wave-uniform selector (and a swap of the two dwords of
//                   an 8-byte element).
//   the sums        a lane's bytes of a plane are summed per slot (position modulo S in the run: two v_dot4 with constant weights),
//                   the slot totals become channel totals by the run's phase (its first element modulo S: not 0 where S = 3, and
//                   then a select between three registers, no dynamic index), and the channel totals modulo 256 go two to a dword
//                   (16-bit fields: 64 x 255 < 2^16) through the wave's inclusive prefix sum (wave.h): B * ceil(S / 2) scans a
//                   chunk.  The scan gives a lane what the lanes in front of it in its row sum to, and the row its total.  The lane
//                   then runs over its bytes again, plane by plane, starting from plane start + lanes in front, and puts each sum
//                   at its place in the output dwords.
//   the planes      the start of plane p is the total of the planes in front of it.  A row of at most 64 runs (512 elements) is
//                   ONE chunk: the scans' totals are the planes' totals, and the row is read once.  A longer row is read twice: a
//                   first pass over its chunks adds up every plane's channel totals (per lane, one reduction per plane and field
//                   pair at the end), a second pass goes chunk by chunk as above and carries every plane's running sum on.  The
//                   carries live in registers (B * ceil(S / 2) of them), nothing in LDS.
//   LDS             the alternative -- staging the summed row in LDS and transposing out of it -- was NOT built: the workgroup is one
//                   wave, so a row of 8,192 float32 (32 KiB) would leave five waves to a CU where the register plan leaves the
//                   occupancy to the registers alone, a row longer than the reservation needs the chunked plan anyway, and the
//                   short rows that fit (a 256-pixel tile row is 1 KiB) are read once by the register plan too.
//   several rows    a row that fills fewer than 33 lanes shares the wave with others (unpredict_core.h): with lpr lanes to the row a
//                   wave takes 64 / lpr rows at once; a lane subtracts what the scan had reached at the last lane of the row in
//                   front and takes its row's total from the row's last lane (two crossbar gathers).
//   what is read    with a sum, every element of a processed row (the sum of the last plane needs all of it).  Without, only the
//                   elements that hold the window's bytes, from each plane.  Nothing but aligned dwords that hold such bytes.
//   the stores      those of unpredict_core.h: where a row's destination is not dword-aligned a lane's dwords are funnelled with the
//                   last dword of the lane in front (one crossbar gather), so that every lane stores ALIGNED dwords: 16-byte stores
//                   where its run lies wholly inside the window at a 16-byte boundary, dwords otherwise; a dword that reaches outside
//                   the window goes as single bytes, those inside only.  Nothing else is written.
//   the split       the rows of the window go to `slices` waves in groups of 64 / lpr, wave s taking the groups s, s + slices, ...
// Rows that do not lie wholly inside src_len are not looked at: the job is ST_TRUNCATED with detail {rows wholly inside, 0}, and
// those of them that fall in the window are delivered.  Illegal geometry (geometry_ok) is ST_FILTER with detail {BAD_ARGS,
// elem_bytes << 16 | sum_stride << 8 | reverse}; nothing of that job is read or written.  Every wave of a job computes the same
// answer: the wave of slice 0 writes it.
// The same source compiles as a host program for the CPU model (tests/model/model_unshuffle.cpp) and the sanitized program
// (tests/cxx/san_unshuffle.cpp): there the 64 lanes are arrays and loops, and the waves of a job run one after the other.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

struct Unshuffle {
    static constexpr uint32_t LANES = 64u, E = 8u;                             // E: the elements of a lane's run
    static constexpr int32_t ST_OK = 0, ST_TRUNCATED = 1, ST_FILTER = 23;  // (PZG_OK, PZG_E_TRUNCATED, PZG_E_FILTER: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t BAD_ARGS = 0xffffffffu;
    static constexpr uint32_t FIELDS = 0x00ff00ffu;                                                         // two sums modulo 256 in a dword
    static constexpr uint32_t SEL_KEEP = 0x03020100u, SEL_SWAP16 = 0x02030001u, SEL_SWAP32 = 0x00010203u;  // v_perm_b32 selectors

    // pzg_unshuffle_desc of include/pzg.h, field for field (pzg_api.cpp holds the two against each other)
    struct Desc {
        uint64_t src_off, dst_off, dst_stride;
        uint32_t src_row_bytes, rows, win_row, win_rows, win_byte, win_bytes;
        uint8_t elem_bytes, sum_stride, reverse, reserved0;
        uint32_t reserved[3];
    };

    // one job, wave-uniform
    struct Job {
        const uint32_t *src;  // the aligned dwords that hold the rows: byte q of stored row r is byte (q' & 3) of src[q' >> 2], q' = mis + r * srb + q
        uint32_t mis;
        uint64_t srb, n;      // a stored row's bytes, and its elements: a plane's bytes
        uint8_t *dst;         // window row 0
        uint64_t dstride;
        uint64_t row0, nrows;  // the first stored row of the window; the window's rows that are processed
        uint64_t wb0, wb1;     // the window's bytes of a row: [wb0, wb1)
        uint64_t e0, e1;       // the elements of a row that are processed: [e0, e1)
        uint32_t sel;          // the byte swap of a dword that reverses its elements (SEL_*)
        uint32_t rev;
    };

    struct alignas(16) Quad {
        uint32_t a, b, c, d;
    };

    template <uint32_t NW>
    struct Run {
        uint32_t y[NW];
    };

    // a lane's bytes of every plane
    template <uint32_t B>
    struct Planes {
        uint32_t lo[B], hi[B];
    };

    PZG_FN static bool empty(const Desc &D) { return D.rows == 0u || D.src_row_bytes == 0u || D.win_rows == 0u || D.win_bytes == 0u; }

    PZG_FN static bool geometry_ok(const Desc &D)
    {
        if (D.elem_bytes != 2u && D.elem_bytes != 4u && D.elem_bytes != 8u) return false;
        if (D.sum_stride > 4u || D.reverse > 1u) return false;
        if (D.src_row_bytes % D.elem_bytes != 0u) return false;
        if (D.sum_stride != 0u && (D.src_row_bytes / D.elem_bytes) % D.sum_stride != 0u) return false;
        if ((uint64_t)D.win_row + D.win_rows > D.rows || (uint64_t)D.win_byte + D.win_bytes > D.src_row_bytes) return false;
        return D.dst_stride >= D.win_bytes;
    }

    // the stored rows that lie wholly inside src_len (src_row_bytes != 0)
    PZG_FN static uint64_t rows_inside(const Desc &D, uint64_t src_len)
    {
        const uint64_t whole = src_len / D.src_row_bytes;
        return whole < D.rows ? whole : D.rows;
    }

    // a job's descriptor, every field wave-uniform
    PZG_FN static Desc fetch(const Desc *p)
    {
        Desc D;
        D.src_off = uni64(p->src_off);
        D.dst_off = uni64(p->dst_off);
        D.dst_stride = uni64(p->dst_stride);
        D.src_row_bytes = uni(p->src_row_bytes);
        D.rows = uni(p->rows);
        D.win_row = uni(p->win_row);
        D.win_rows = uni(p->win_rows);
        D.win_byte = uni(p->win_byte);
        D.win_bytes = uni(p->win_bytes);
        D.elem_bytes = (uint8_t)uni(p->elem_bytes);
        D.sum_stride = (uint8_t)uni(p->sum_stride);
        D.reverse = (uint8_t)uni(p->reverse);
        D.reserved0 = 0u;
        D.reserved[0] = D.reserved[1] = D.reserved[2] = 0u;
        return D;
    }

    // byte j of the result is byte (sel >> 8 j) & 3 of x
    PZG_FN static uint32_t bytes_perm(uint32_t x, uint32_t sel)
    {
#if PZG_DEVICE_PASS
        return __builtin_amdgcn_perm(0u, x, sel);
#else
        uint32_t r = 0;
        for (uint32_t j = 0; j < 4u; ++j) r |= ((x >> (8u * ((sel >> (8u * j)) & 3u))) & 0xffu) << (8u * j);
        return r;
#endif
    }

    // the weights that pick, of the bytes 4 half .. 4 half + 3 of a run, those of a slot (their position modulo S)
    PZG_FN static constexpr uint32_t slot_weights(uint32_t S, uint32_t slot, uint32_t half)
    {
        uint32_t w = 0u;
        for (uint32_t j = 0; j < 4u; ++j)
            if ((4u * half + j) % S == slot) w |= 1u << (8u * j);
        return w;
    }

    // the first element of run r of a row, modulo S: 0 but where S is 3 (E is a multiple of 1, 2 and 4)
    template <uint32_t S>
    PZG_FN static uint32_t phase(uint32_t r)
    {
        if constexpr (S == 3u) return (r % 3u) * (E % 3u) % 3u;
        return 0u;
    }

    // The `valid` first bytes of the run of a plane that starts at byte q of J.src (the rest 0); need: where the plane's processed
    // bytes end.  Only dwords that hold bytes of [q, need) are read.
    PZG_FN static void load_run(const Job &J, uint64_t q, uint64_t need, bool live, uint32_t valid, uint32_t &lo, uint32_t &hi)
    {
        const uint32_t *p = J.src + (q >> 2);
        uint32_t w[3];
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) w[i] = live && (((q >> 2) + i) << 2) < need ? p[i] : 0u;
        const uint32_t sh = 8u * ((uint32_t)q & 3u);
        lo = funnel(w[1], w[0], sh);
        hi = funnel(w[2], w[1], sh);
        if (valid < 8u) {
            lo &= valid >= 4u ? 0xffffffffu : (1u << (8u * valid)) - 1u;
            hi &= valid <= 4u ? 0u : (1u << (8u * (valid - 4u))) - 1u;
        }
    }

    // The channel totals modulo 256 of a run's bytes, two to a dword; ph: the run's first element modulo S.
    template <uint32_t S, uint32_t NP>
    PZG_FN static void run_totals(uint32_t lo, uint32_t hi, uint32_t ph, uint32_t (&pair)[NP])
    {
        uint32_t st[S], ct[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) st[s] = dot4(lo, slot_weights(S, s, 0u), dot4(hi, slot_weights(S, s, 1u), 0u)) & 0xffu;
        if constexpr (S == 3u) {
            ct[0] = ph == 0u ? st[0] : ph == 1u ? st[2] : st[1];
            ct[1] = ph == 0u ? st[1] : ph == 1u ? st[0] : st[2];
            ct[2] = ph == 0u ? st[2] : ph == 1u ? st[1] : st[0];
        } else {
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) ct[s] = st[s];
        }
#pragma unroll
        for (uint32_t q = 0; q < NP; ++q) pair[q] = 2u * q + 1u < S ? ct[2u * q] | (ct[2u * q + 1u] << 16) : ct[2u * q];
    }

    // x: two 16-bit sums per lane; afterwards those of the lanes in front of it IN ITS ROW, and in tot its row's.  row: the lane's row of
    // the wave's; seg: the last lane of the row in front; endl: the last lane of its own; several: the wave has more than one row.
    PZG_FN static void row_scan(LaneVec<uint32_t> &x, LaneVec<uint32_t> &tot, const LaneVec<uint32_t> &row, const LaneVec<uint32_t> &seg,
                                const LaneVec<uint32_t> &endl, bool several)
    {
        LaneVec<uint32_t> inc = x;
        lanes_iscan_add(inc);
        LaneVec<uint32_t> base = inc, end;
        if (several) lanes_gather(base, inc, seg);
        lanes_gather(end, inc, endl);
        PZG_LANES_BEGIN(k)
        const uint32_t b = several && PZG_LV(row, k) ? PZG_LV(base, k) : 0u;
        PZG_LV(x, k) = PZG_LV(inc, k) - PZG_LV(x, k) - b;
        PZG_LV(tot, k) = PZG_LV(end, k) - b;
        PZG_LANES_END
    }

    // One dword of the aligned destination: it holds the row's bytes lo .. lo + 3; `at` is where byte wb0 of the row goes.
    PZG_FN static void put_dword(const Job &J, uint8_t *at, int64_t lo, uint32_t o)
    {
        uint8_t *out = at + (lo - (int64_t)J.wb0);
        if (lo >= (int64_t)J.wb0 && lo + 4 <= (int64_t)J.wb1) {
            *(uint32_t *)(void *)out = o;
        } else {
#pragma unroll
            for (int64_t j = 0; j < 4; ++j)
                if (lo + j >= (int64_t)J.wb0 && lo + j < (int64_t)J.wb1) out[j] = (uint8_t)(o >> (8u * (uint32_t)j));
        }
    }

    // The groups slice, slice + slices, ... of the job's rows.  B: the bytes of an element; S: the stride of the sum, 0 for none.
    template <uint32_t B, uint32_t S>
    PZG_FN static void groups(const Job &J, uint32_t slice, uint32_t slices)
    {
        constexpr uint32_t RUN = E * B, NW = RUN / 4u, NP = S ? (S + 1u) / 2u : 1u, SS = S ? S : 1u;
        const uint64_t runs = (J.e1 - J.e0 + E - 1u) / E;                    // the runs of a row
        const uint32_t lpr = runs < LANES ? (uint32_t)runs : LANES;          // the lanes a row takes of a wave
        const uint32_t rpw = LANES / lpr;                                    // the rows a wave takes at once
        const uint32_t nch = (uint32_t)((runs + LANES - 1u) / LANES);        // the chunks of a row (rpw == 1 where there are several)
        const uint64_t ngroups = (J.nrows + rpw - 1u) / rpw;
        const bool several = rpw > 1u;
        LaneVec<uint32_t> row, pos, seg, endl;
        PZG_LANES_BEGIN(k)
        const uint32_t j = k / lpr;
        PZG_LV(row, k) = j;
        PZG_LV(pos, k) = k - j * lpr;
        PZG_LV(seg, k) = (j * lpr - 1u) & (LANES - 1u);
        PZG_LV(endl, k) = (j * lpr + lpr - 1u) & (LANES - 1u);
        PZG_LANES_END
        for (uint64_t g = slice; g < ngroups; g += slices) {
            // the sum at the start of this chunk's part of plane p (rows of several chunks: one row to the wave)
            LaneVec<uint32_t> carry[B][NP];
            if constexpr (S != 0u) {
                PZG_LANES_BEGIN(k)
#pragma unroll
                for (uint32_t p = 0; p < B; ++p)
#pragma unroll
                    for (uint32_t q = 0; q < NP; ++q) PZG_LV(carry[p][q], k) = 0u;
                PZG_LANES_END
                if (nch > 1u) {
                    // the first pass: every plane's channel totals
                    LaneVec<uint32_t> pt[B][NP];
                    PZG_LANES_BEGIN(k)
#pragma unroll
                    for (uint32_t p = 0; p < B; ++p)
#pragma unroll
                        for (uint32_t q = 0; q < NP; ++q) PZG_LV(pt[p][q], k) = 0u;
                    PZG_LANES_END
                    for (uint32_t ch = 0; ch < nch; ++ch) {
                        PZG_LANES_BEGIN(k)
                        const uint64_t es = J.e0 + ((uint64_t)ch * LANES + k) * E;
                        const bool live = es < J.e1;
                        const uint32_t valid = live && J.e1 - es < E ? (uint32_t)(J.e1 - es) : E;
                        const uint64_t rq = J.mis + (J.row0 + g) * J.srb;
#pragma unroll
                        for (uint32_t p = 0; p + 1u < B; ++p) {
                            uint32_t lo, hi, pair[NP];
                            load_run(J, rq + p * J.n + es, rq + p * J.n + J.e1, live, valid, lo, hi);
                            run_totals<SS, NP>(lo, hi, phase<S>(ch * LANES + k), pair);
#pragma unroll
                            for (uint32_t q = 0; q < NP; ++q) PZG_LV(pt[p][q], k) = (PZG_LV(pt[p][q], k) + pair[q]) & FIELDS;
                        }
                        PZG_LANES_END
                    }
#pragma unroll
                    for (uint32_t p = 0; p + 1u < B; ++p)
#pragma unroll
                        for (uint32_t q = 0; q < NP; ++q) {
                            lanes_iscan_add(pt[p][q]);
                            const uint32_t total = lane_get(pt[p][q], LANES - 1u);
                            PZG_LANES_BEGIN(k)
                            PZG_LV(carry[p + 1u][q], k) = (PZG_LV(carry[p][q], k) + total) & FIELDS;
                            PZG_LANES_END
                        }
                }
            }
            uint32_t tail = 0u;  // the last dword of the chunk in front
            for (uint32_t ch = 0; ch < nch; ++ch) {
                LaneVec<Planes<B>> X;
                LaneVec<Run<NW>> R;
                LaneVec<uint32_t> on;
                LaneVec<uint32_t> ex[B][NP], tot[B][NP];
                // the fetch, and the run's totals per plane and channel
                PZG_LANES_BEGIN(k)
                const uint64_t wr = g * rpw + PZG_LV(row, k), es = J.e0 + ((uint64_t)ch * LANES + PZG_LV(pos, k)) * E;
                const bool live = PZG_LV(row, k) < rpw && wr < J.nrows && es < J.e1;
                PZG_LV(on, k) = live ? 1u : 0u;
                const uint32_t valid = live && J.e1 - es < E ? (uint32_t)(J.e1 - es) : E;
                const uint64_t rq = J.mis + (J.row0 + wr) * J.srb;
#pragma unroll
                for (uint32_t p = 0; p < B; ++p) {
                    load_run(J, rq + p * J.n + es, rq + p * J.n + J.e1, live, valid, PZG_LV(X, k).lo[p], PZG_LV(X, k).hi[p]);
                    if constexpr (S != 0u) {
                        uint32_t pair[NP];
                        run_totals<SS, NP>(PZG_LV(X, k).lo[p], PZG_LV(X, k).hi[p], phase<S>(ch * LANES + PZG_LV(pos, k)), pair);
#pragma unroll
                        for (uint32_t q = 0; q < NP; ++q) PZG_LV(ex[p][q], k) = pair[q];
                    }
                }
                PZG_LANES_END
                // what the lanes in front of a lane in its row sum to, and the row's total, per plane and channel
                if constexpr (S != 0u) {
#pragma unroll
                    for (uint32_t p = 0; p < B; ++p)
#pragma unroll
                        for (uint32_t q = 0; q < NP; ++q) row_scan(ex[p][q], tot[p][q], row, seg, endl, several);
                }
                // the run again from there, every sum to its place in the output
                LaneVec<uint32_t> last, prev, idx;
                PZG_LANES_BEGIN(k)
                uint32_t(&y)[NW] = PZG_LV(R, k).y;
#pragma unroll
                for (uint32_t i = 0; i < NW; ++i) y[i] = 0u;
                [[maybe_unused]] const uint32_t ph = phase<S>(ch * LANES + PZG_LV(pos, k));
                [[maybe_unused]] uint32_t running[NP];
#pragma unroll
                for (uint32_t q = 0; q < NP; ++q) running[q] = 0u;
#pragma unroll
                for (uint32_t p = 0; p < B; ++p) {
                    uint32_t acc[SS];
                    if constexpr (S != 0u) {
                        uint32_t cv[SS];
#pragma unroll
                        for (uint32_t q = 0; q < NP; ++q) {
                            const uint32_t start = (nch == 1u ? running[q] : PZG_LV(carry[p][q], k)) + PZG_LV(ex[p][q], k);
                            cv[2u * q] = start & 0xffffu;
                            if (2u * q + 1u < SS) cv[(2u * q + 1u) % SS] = start >> 16;
                            running[q] = (running[q] + PZG_LV(tot[p][q], k)) & FIELDS;
                            PZG_LV(carry[p][q], k) = (PZG_LV(carry[p][q], k) + PZG_LV(tot[p][q], k)) & FIELDS;
                        }
                        if constexpr (S == 3u) {
                            acc[0] = ph == 0u ? cv[0] : ph == 1u ? cv[1] : cv[2];
                            acc[1] = ph == 0u ? cv[1] : ph == 1u ? cv[2] : cv[0];
                            acc[2] = ph == 0u ? cv[2] : ph == 1u ? cv[0] : cv[1];
                        } else {
#pragma unroll
                            for (uint32_t s = 0; s < SS; ++s) acc[s] = cv[s];
                        }
                    } else {
                        acc[0] = 0u;
                    }
#pragma unroll
                    for (uint32_t i = 0; i < E; ++i) {
                        const uint32_t b = ((i < 4u ? PZG_LV(X, k).lo[p] : PZG_LV(X, k).hi[p]) >> (8u * (i & 3u))) & 0xffu;
                        uint32_t v = b;
                        if constexpr (S != 0u) {
                            acc[i % SS] += b;
                            v = acc[i % SS] & 0xffu;
                        }
                        y[(i * B + p) >> 2] |= v << (8u * ((i * B + p) & 3u));
                    }
                }
                // plane j is byte j of the element so far
                if constexpr (B == 8u) {
#pragma unroll
                    for (uint32_t i = 0; i < NW; i += 2u) {
                        const uint32_t a = bytes_perm(J.rev ? y[i + 1u] : y[i], J.sel), b = bytes_perm(J.rev ? y[i] : y[i + 1u], J.sel);
                        y[i] = a;
                        y[i + 1u] = b;
                    }
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < NW; ++i) y[i] = bytes_perm(y[i], J.sel);
                }
                PZG_LV(last, k) = y[NW - 1u];
                PZG_LV(idx, k) = (k - 1u) & (LANES - 1u);
                PZG_LANES_END
                lanes_gather(prev, last, idx);
                const uint32_t next_tail = lane_get(last, LANES - 1u);
                // the stores
                PZG_LANES_BEGIN(k)
                if (PZG_LV(on, k)) {
                    const uint32_t(&y)[NW] = PZG_LV(R, k).y;
                    const uint64_t wr = g * rpw + PZG_LV(row, k), b0 = (J.e0 + ((uint64_t)ch * LANES + PZG_LV(pos, k)) * E) * B;
                    uint8_t *at = J.dst + wr * J.dstride;  // byte wb0 of the row
                    // (every run starts a multiple of 16 bytes behind element e0: where that one goes decides for all of them)
                    const uint32_t sh = (uint32_t)((uintptr_t)at - (uintptr_t)J.wb0 + (uintptr_t)(J.e0 * B)) & 3u;
                    const uint32_t before = PZG_LV(pos, k) ? PZG_LV(prev, k) : tail;
                    uint32_t o[NW];
#pragma unroll
                    for (uint32_t i = 0; i < NW; ++i) o[i] = sh ? funnel(y[i], i ? y[i - 1u] : before, 32u - 8u * sh) : y[i];
                    const int64_t lo = (int64_t)b0 - (int64_t)sh;  // o[i] holds the row's bytes lo + 4 i .. + 3
                    if (lo >= (int64_t)J.wb0 && lo + (int64_t)RUN <= (int64_t)J.wb1) {
                        uint8_t *out = at + (lo - (int64_t)J.wb0);
                        if (((uintptr_t)out & 15u) == 0u) {
#pragma unroll
                            for (uint32_t i = 0; i < NW; i += 4u) {
                                Quad v;
                                v.a = o[i];
                                v.b = o[i + 1u];
                                v.c = o[i + 2u];
                                v.d = o[i + 3u];
                                *(Quad *)(void *)(out + 4u * i) = v;
                            }
                        } else {
#pragma unroll
                            for (uint32_t i = 0; i < NW; ++i) *(uint32_t *)(void *)(out + 4u * i) = o[i];
                        }
                    } else {
#pragma unroll
                        for (uint32_t i = 0; i < NW; ++i)
                            if (lo + 4 * (int64_t)i + 4 > (int64_t)J.wb0 && lo + 4 * (int64_t)i < (int64_t)J.wb1) put_dword(J, at, lo + 4 * (int64_t)i, o[i]);
                    }
                    // what the row's last run still holds: its last sh bytes
                    if (sh && b0 + RUN >= J.wb1 && lo + (int64_t)RUN < (int64_t)J.wb1) put_dword(J, at, lo + (int64_t)RUN, y[NW - 1u] >> (32u - 8u * sh));
                }
                PZG_LANES_END
                tail = next_tail;
            }
        }
    }

    template <uint32_t B>
    PZG_FN static void groups_of(const Job &J, uint32_t sum_stride, uint32_t slice, uint32_t slices)
    {
        switch (sum_stride) {
        case 0u: groups<B, 0u>(J, slice, slices); break;
        case 1u: groups<B, 1u>(J, slice, slices); break;
        case 2u: groups<B, 2u>(J, slice, slices); break;
        case 3u: groups<B, 3u>(J, slice, slices); break;
        default: groups<B, 4u>(J, slice, slices); break;
        }
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

    // One job's share of a wave.  status, detail: the job's (detail may be null).
    PZG_FN static void job(const uint8_t *src_base, uint64_t src_len, uint8_t *dst_base, const Desc &D, uint32_t slice, uint32_t slices, int32_t *status,
                           uint32_t *detail)
    {
        if (empty(D)) {
            if (slice == 0u) answer(status, detail, ST_OK, 0u, 0u);
            return;
        }
        if (!geometry_ok(D)) {
            if (slice == 0u) answer(status, detail, ST_FILTER, BAD_ARGS, (uint32_t)D.elem_bytes << 16 | (uint32_t)D.sum_stride << 8 | D.reverse);
            return;
        }
        const uint64_t inside = rows_inside(D, src_len);
        if (slice == 0u) answer(status, detail, inside < D.rows ? ST_TRUNCATED : ST_OK, inside < D.rows ? (uint32_t)inside : 0u, 0u);
        const uint64_t end = (uint64_t)D.win_row + D.win_rows < inside ? (uint64_t)D.win_row + D.win_rows : inside;
        if (end <= D.win_row) return;
        const uint8_t *src = src_base + D.src_off;
        Job J;
        J.mis = (uint32_t)((uintptr_t)src & 3u);
        J.src = (const uint32_t *)(const void *)(src - J.mis);
        J.srb = D.src_row_bytes;
        J.n = D.src_row_bytes / D.elem_bytes;
        J.dst = dst_base + D.dst_off;
        J.dstride = D.dst_stride;
        J.row0 = D.win_row;
        J.nrows = end - D.win_row;
        J.wb0 = D.win_byte;
        J.wb1 = (uint64_t)D.win_byte + D.win_bytes;
        J.e0 = D.sum_stride ? 0u : J.wb0 / D.elem_bytes;
        J.e1 = D.sum_stride ? J.n : (J.wb1 + D.elem_bytes - 1u) / D.elem_bytes;
        J.rev = D.reverse ? 1u : 0u;
        J.sel = !J.rev ? SEL_KEEP : D.elem_bytes == 2u ? SEL_SWAP16 : SEL_SWAP32;
        switch (D.elem_bytes) {
        case 2u: groups_of<2u>(J, D.sum_stride, slice, slices); break;
        case 4u: groups_of<4u>(J, D.sum_stride, slice, slices); break;
        default: groups_of<8u>(J, D.sum_stride, slice, slices); break;
        }
    }
};

}  // namespace pzg
