// unpredict_core.h -- TIFF horizontal differencing undone (TIFF 6.0 section 14, Predictor 2), and the clipping of a strip or tile to a
// window, of many jobs in one launch (pzg_unpredict_many).  Nothing here knows of TIFF's tags: a job is `rows` stored rows of
// src_row_bytes bytes, dense; of them the window -- rows [win_row, win_row + win_rows), of each the bytes [win_byte, win_byte +
// win_bytes) of the RECONSTRUCTED row -- is delivered at a stride of the caller's.
//   the recurrence  sample k of a row is stored[k] + actual[k - samples] modulo 2^(8 sample_bytes), in the file's byte order: rows are
//                   independent of each other, and along the row it is `samples` interleaved prefix sums.  It starts at byte 0 of
//                   the stored row whatever the window: a row is processed up to the sample that holds the window's last byte, nothing
//                   behind it.
//   the runs        a lane owns RUN contiguous bytes of a row, RUN = lcm(16, samples * sample_bytes): whole pixels, whole 16-byte
//                   units (16 bytes; 48 where the pixel has a factor 3, 32 for four 8-byte samples).  It sums its run per channel
//                   in registers; the lanes' per-channel totals go through the wave's inclusive prefix sum (wave.h), one scan per
//                   channel (three, over 22-bit limbs, for an 8-byte sample: the scan is 32 bits wide); the lane then runs over
//                   its samples again, starting from what the lanes in front of it sum to.  samples and sample_bytes are template
//                   parameters: every register index is a constant.  The byte order is not: a big-endian file's dwords are byte-
//                   swapped by ONE v_perm_b32 with a wave-uniform selector behind the load and again in front of the store.
//   several rows    a row that fills fewer than 33 lanes shares the wave with others: with lpr lanes to the row a wave takes
//                   64 / lpr rows at once (a tile row of 256 RGB8 pixels is 16 lanes: four rows).  The scan still runs over all
//                   64 lanes; a lane subtracts what the scan had reached at the last lane of the row in front (one crossbar
//                   gather): sums modulo 2^32 make that exact.  This is the only variant built.
//   long rows       a row longer than 64 runs goes in chunks of 64 runs, the per-channel sums (and the last dword, below) carried
//                   on in wave-uniform registers.
//   the fetch       a lane reads the aligned dwords that hold its run, RUN / 4 + 1 of them, and funnels them by the row's
//                   misalignment.  Nothing is read but dwords that hold bytes of the rows processed, and of those only up to the
//                   sample that holds the window's last byte.
//   the stores      where a row's destination is not dword-aligned a lane's dwords are funnelled with the last dword of the lane
//                   in front of it (one crossbar gather), so that every lane stores ALIGNED dwords: as 16-byte stores where its
//                   run lies wholly inside the window at a 16-byte boundary, as dwords otherwise; a dword that reaches outside
//                   the window goes as single bytes, those inside only.  Nothing else is written.
//   the split       the rows of the window go to `slices` waves in groups of 64 / lpr, wave s taking the groups s, s + slices, ...
//                   (adam7_core.h, expand_core.h): a strip can be a whole image.
// Predictor 1 is the same loop with the sums left out: a clipped copy.
// Rows that do not lie wholly inside src_len are not looked at: the job is ST_TRUNCATED with detail {rows wholly inside, 0}, and
// those of them that fall in the window are delivered.  Illegal geometry (geometry_ok) is ST_FILTER with detail {BAD_ARGS,
// predictor << 16 | sample_bytes << 8 | samples}; nothing of that job is read or written.  Every wave of a job computes the same
// answer: the wave of slice 0 writes it.
// The same source compiles as a host program for the CPU model (tests/model/model_unpredict.cpp): there the 64 lanes are arrays
// and loops, and the waves of a job run one after the other.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.h"

namespace pzg {

// what a sum of samples of SB bytes is held in
template <uint32_t SB>
struct UnpredictSum {
    using T = uint32_t;
};
template <>
struct UnpredictSum<8u> {
    using T = uint64_t;
};

struct Unpredict {
    static constexpr uint32_t LANES = 64u;
    static constexpr int32_t ST_OK = 0, ST_TRUNCATED = 1, ST_FILTER = 23;  // (PZG_OK, PZG_E_TRUNCATED, PZG_E_FILTER: pzg_api.cpp holds them against include/pzg.h)
    static constexpr uint32_t BAD_ARGS = 0xffffffffu;
    static constexpr uint32_t SEL_KEEP = 0x03020100u, SEL_SWAP16 = 0x02030001u, SEL_SWAP32 = 0x00010203u;  // v_perm_b32 selectors

    // pzg_unpredict_desc of include/pzg.h, field for field (pzg_api.cpp holds the two against each other)
    struct Desc {
        uint64_t src_off, dst_off, dst_stride;
        uint32_t src_row_bytes, rows, win_row, win_rows, win_byte, win_bytes;
        uint8_t predictor, sample_bytes, samples, big_endian;
        uint32_t reserved[3];
    };

    // one job, wave-uniform
    struct Job {
        const uint32_t *src;  // the aligned dwords that hold the rows: byte q of stored row r is byte (q' & 3) of src[q' >> 2], q' = mis + r * srb + q
        uint32_t mis;
        uint64_t srb;
        uint8_t *dst;         // window row 0
        uint64_t dstride;
        uint64_t row0, nrows;  // the first stored row of the window; the window's rows that are processed
        uint64_t wb0, wb1;     // the window's bytes of a row: [wb0, wb1)
        uint64_t pe;           // a row is processed up to here: wb1, rounded up to a whole sample (its first byte takes the carry of its last)
        uint32_t sel;          // the byte swap of a dword that makes its samples little-endian (SEL_*)
        uint32_t be;
    };

    struct alignas(16) Quad {
        uint32_t a, b, c, d;
    };

    template <uint32_t NW>
    struct Run {
        uint32_t y[NW];
    };

    // the bytes of a lane's run for a pixel of p bytes: lcm(16, p)
    PZG_FN static constexpr uint32_t run_bytes(uint32_t p) { return p % 3u == 0u ? 48u : p > 16u ? 32u : 16u; }

    PZG_FN static bool empty(const Desc &D) { return D.rows == 0u || D.src_row_bytes == 0u || D.win_rows == 0u || D.win_bytes == 0u; }

    PZG_FN static bool geometry_ok(const Desc &D)
    {
        if (D.predictor != 1u && D.predictor != 2u) return false;
        if (D.sample_bytes != 1u && D.sample_bytes != 2u && D.sample_bytes != 4u && D.sample_bytes != 8u) return false;
        if (D.samples < 1u || D.samples > 4u) return false;
        if (D.predictor == 2u && D.src_row_bytes % ((uint32_t)D.samples * D.sample_bytes) != 0u) return false;
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
        D.predictor = (uint8_t)uni(p->predictor);
        D.sample_bytes = (uint8_t)uni(p->sample_bytes);
        D.samples = (uint8_t)uni(p->samples);
        D.big_endian = (uint8_t)uni(p->big_endian);
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

    // sample i of a run whose dwords hold little-endian samples (8-byte samples: dword-swapped where the file is big-endian)
    template <uint32_t SB, uint32_t NW>
    PZG_FN static uint64_t sample_get(const uint32_t (&x)[NW], uint32_t i, uint32_t be)
    {
        if constexpr (SB == 1u) return (x[i >> 2] >> (8u * (i & 3u))) & 0xffu;
        if constexpr (SB == 2u) return (x[i >> 1] >> (16u * (i & 1u))) & 0xffffu;
        if constexpr (SB == 4u) return x[i];
        if constexpr (SB == 8u) {
            const uint32_t lo = be ? x[2u * i + 1u] : x[2u * i], hi = be ? x[2u * i] : x[2u * i + 1u];
            return ((uint64_t)hi << 32) | lo;
        }
        return 0u;
    }

    template <uint32_t SB, uint32_t NW>
    PZG_FN static void sample_put(uint32_t (&y)[NW], uint32_t i, uint64_t v, uint32_t be)
    {
        if constexpr (SB == 1u) y[i >> 2] |= ((uint32_t)v & 0xffu) << (8u * (i & 3u));
        if constexpr (SB == 2u) y[i >> 1] |= ((uint32_t)v & 0xffffu) << (16u * (i & 1u));
        if constexpr (SB == 4u) y[i] = (uint32_t)v;
        if constexpr (SB == 8u) {
            y[2u * i] = be ? (uint32_t)(v >> 32) : (uint32_t)v;
            y[2u * i + 1u] = be ? (uint32_t)v : (uint32_t)(v >> 32);
        }
    }

    // x: a value per lane; afterwards the sum of the values of the lanes in front of it IN ITS ROW.  row: the lane's row of the wave's;
    // seg: the last lane of the row in front; several: the wave has more than one row.  Returns the sum over the wave.
    PZG_FN static uint32_t row_exclusive(LaneVec<uint32_t> &x, const LaneVec<uint32_t> &row, const LaneVec<uint32_t> &seg, bool several)
    {
        LaneVec<uint32_t> inc = x;
        lanes_iscan_add(inc);
        const uint32_t total = lane_get(inc, LANES - 1u);
        LaneVec<uint32_t> base = inc;
        if (several) lanes_gather(base, inc, seg);
        PZG_LANES_BEGIN(k)
        const uint32_t b = several && PZG_LV(row, k) ? PZG_LV(base, k) : 0u;
        PZG_LV(x, k) = PZG_LV(inc, k) - PZG_LV(x, k) - b;
        PZG_LANES_END
        return total;
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

    // The groups slice, slice + slices, ... of the job's rows.  SB, S: the bytes of a sample, the samples of a pixel; SUM: predictor 2.
    template <uint32_t SB, uint32_t S, bool SUM>
    PZG_FN static void groups(const Job &J, uint32_t slice, uint32_t slices)
    {
        constexpr uint32_t RUN = run_bytes(SB * S), NW = RUN / 4u, NS = RUN / SB;
        using V = typename UnpredictSum<SB>::T;
        const uint64_t runs = (J.pe + RUN - 1u) / RUN;                      // the runs of a row
        const uint32_t lpr = runs < LANES ? (uint32_t)runs : LANES;          // the lanes a row takes of a wave
        const uint32_t rpw = LANES / lpr;                                    // the rows a wave takes at once
        const uint32_t nch = (uint32_t)((runs + LANES - 1u) / LANES);        // the chunks of a row (rpw == 1 where there are several)
        const uint64_t ngroups = (J.nrows + rpw - 1u) / rpw;
        const bool several = rpw > 1u;
        LaneVec<uint32_t> row, pos, seg;
        PZG_LANES_BEGIN(k)
        const uint32_t j = k / lpr;
        PZG_LV(row, k) = j;
        PZG_LV(pos, k) = k - j * lpr;
        PZG_LV(seg, k) = (j * lpr - 1u) & (LANES - 1u);
        PZG_LANES_END
        for (uint64_t g = slice; g < ngroups; g += slices) {
            V carry[S];
#pragma unroll
            for (uint32_t c = 0; c < S; ++c) carry[c] = 0u;
            uint32_t tail = 0u;  // the last dword of the chunk in front
            for (uint32_t ch = 0; ch < nch; ++ch) {
                LaneVec<Run<NW>> R;
                LaneVec<uint32_t> on;
                LaneVec<V> tot[S];
                // the fetch, and the run's sum per channel
                PZG_LANES_BEGIN(k)
                const uint64_t wr = g * rpw + PZG_LV(row, k), b0 = ((uint64_t)ch * LANES + PZG_LV(pos, k)) * RUN;
                const bool live = PZG_LV(row, k) < rpw && wr < J.nrows && b0 < J.pe;
                PZG_LV(on, k) = live ? 1u : 0u;
                const uint64_t rq = J.mis + (J.row0 + wr) * J.srb, q = rq + b0, need = rq + J.pe;
                const uint32_t *p = J.src + (q >> 2);
                uint32_t w[NW + 1u];
#pragma unroll
                for (uint32_t i = 0; i <= NW; ++i) w[i] = live && (((q >> 2) + i) << 2) < need ? p[i] : 0u;
                uint32_t(&x)[NW] = PZG_LV(R, k).y;
#pragma unroll
                for (uint32_t i = 0; i < NW; ++i) x[i] = funnel(w[i + 1u], w[i], 8u * ((uint32_t)q & 3u));
                if constexpr (SUM) {
                    if constexpr (SB > 1u) {
#pragma unroll
                        for (uint32_t i = 0; i < NW; ++i) x[i] = bytes_perm(x[i], J.sel);
                    }
                    V t[S];
#pragma unroll
                    for (uint32_t c = 0; c < S; ++c) t[c] = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < NS; ++i) t[i % S] += (V)sample_get<SB, NW>(x, i, J.be);
#pragma unroll
                    for (uint32_t c = 0; c < S; ++c) PZG_LV(tot[c], k) = live ? t[c] : 0u;
                }
                PZG_LANES_END
                // what the lanes in front of a lane in its row sum to, per channel
                if constexpr (SUM) {
#pragma unroll
                    for (uint32_t c = 0; c < S; ++c) {
                        if constexpr (SB < 8u) {
                            LaneVec<uint32_t> v;
                            PZG_LANES_BEGIN(k)
                            PZG_LV(v, k) = (uint32_t)PZG_LV(tot[c], k);
                            PZG_LANES_END
                            const uint32_t total = row_exclusive(v, row, seg, several);
                            PZG_LANES_BEGIN(k)
                            PZG_LV(tot[c], k) = (V)(carry[c] + PZG_LV(v, k));
                            PZG_LANES_END
                            carry[c] += (V)total;
                        } else {
                            // 64 lanes of 22 bits sum to 28: three scans that lose no carry
                            LaneVec<uint32_t> v0, v1, v2;
                            PZG_LANES_BEGIN(k)
                            const uint64_t t = PZG_LV(tot[c], k);
                            PZG_LV(v0, k) = (uint32_t)t & 0x3fffffu;
                            PZG_LV(v1, k) = (uint32_t)(t >> 22) & 0x3fffffu;
                            PZG_LV(v2, k) = (uint32_t)(t >> 44);
                            PZG_LANES_END
                            const uint64_t t0 = row_exclusive(v0, row, seg, several), t1 = row_exclusive(v1, row, seg, several),
                                           t2 = row_exclusive(v2, row, seg, several);
                            PZG_LANES_BEGIN(k)
                            PZG_LV(tot[c], k) = (V)(carry[c] + PZG_LV(v0, k) + ((uint64_t)PZG_LV(v1, k) << 22) + ((uint64_t)PZG_LV(v2, k) << 44));
                            PZG_LANES_END
                            carry[c] += (V)(t0 + (t1 << 22) + (t2 << 44));
                        }
                    }
                }
                // the run again, from there
                LaneVec<uint32_t> last, prev, idx;
                PZG_LANES_BEGIN(k)
                uint32_t(&x)[NW] = PZG_LV(R, k).y;
                if constexpr (SUM) {
                    V acc[S];
#pragma unroll
                    for (uint32_t c = 0; c < S; ++c) acc[c] = PZG_LV(tot[c], k);
                    uint32_t y[NW];
#pragma unroll
                    for (uint32_t i = 0; i < NW; ++i) y[i] = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < NS; ++i) {
                        acc[i % S] += (V)sample_get<SB, NW>(x, i, J.be);
                        sample_put<SB, NW>(y, i, acc[i % S], J.be);
                    }
#pragma unroll
                    for (uint32_t i = 0; i < NW; ++i) x[i] = SB > 1u ? bytes_perm(y[i], J.sel) : y[i];
                }
                PZG_LV(last, k) = x[NW - 1u];
                PZG_LV(idx, k) = (k - 1u) & (LANES - 1u);
                PZG_LANES_END
                lanes_gather(prev, last, idx);
                const uint32_t next_tail = lane_get(last, LANES - 1u);
                // the stores
                PZG_LANES_BEGIN(k)
                if (PZG_LV(on, k)) {
                    const uint32_t(&y)[NW] = PZG_LV(R, k).y;
                    const uint64_t wr = g * rpw + PZG_LV(row, k), b0 = ((uint64_t)ch * LANES + PZG_LV(pos, k)) * RUN;
                    uint8_t *at = J.dst + wr * J.dstride;  // byte wb0 of the row
                    const uint32_t sh = (uint32_t)((uintptr_t)at - (uintptr_t)J.wb0) & 3u;
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

    template <uint32_t SB>
    PZG_FN static void groups_of(const Job &J, uint32_t samples, uint32_t slice, uint32_t slices)
    {
        switch (samples) {
        case 1u: groups<SB, 1u, true>(J, slice, slices); break;
        case 2u: groups<SB, 2u, true>(J, slice, slices); break;
        case 3u: groups<SB, 3u, true>(J, slice, slices); break;
        default: groups<SB, 4u, true>(J, slice, slices); break;
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
            if (slice == 0u) answer(status, detail, ST_FILTER, BAD_ARGS, (uint32_t)D.predictor << 16 | (uint32_t)D.sample_bytes << 8 | D.samples);
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
        J.dst = dst_base + D.dst_off;
        J.dstride = D.dst_stride;
        J.row0 = D.win_row;
        J.nrows = end - D.win_row;
        J.wb0 = D.win_byte;
        J.wb1 = (uint64_t)D.win_byte + D.win_bytes;
        J.pe = D.predictor == 2u ? (J.wb1 + D.sample_bytes - 1u) / D.sample_bytes * D.sample_bytes : J.wb1;
        J.be = D.big_endian ? 1u : 0u;
        J.sel = !J.be || D.sample_bytes == 1u ? SEL_KEEP : D.sample_bytes == 2u ? SEL_SWAP16 : SEL_SWAP32;
        if (D.predictor == 1u) {
            groups<1u, 1u, false>(J, slice, slices);
            return;
        }
        switch (D.sample_bytes) {
        case 1u: groups_of<1u>(J, D.samples, slice, slices); break;
        case 2u: groups_of<2u>(J, D.samples, slice, slices); break;
        case 4u: groups_of<4u>(J, D.samples, slice, slices); break;
        default: groups_of<8u>(J, D.samples, slice, slices); break;
        }
    }
};

}  // namespace pzg
