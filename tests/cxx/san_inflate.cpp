// san_inflate.cpp -- TEST INFRASTRUCTURE: the instances of the kernel source (pure_zlib_amd/csrc/inflate_core.h) that the host models
// build, under ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_cores.py writes from the shared case lists.
// Built once per model file, with the model file, because the models reuse each other's names:
//   -DSAN_RAW      tests/model/model_raw.cpp          entry 0
//   -DSAN_HARNESS  tests/model/model_harness.cpp      entries 1 and 2, and 4 with format 0
//   -DSAN_SEG      tests/model/model_seg.cpp          entry 3
//   -DSAN_FMT      tests/model/model_resume_fmt.cpp   entry 4 with formats 4 and 32
// Every buffer a model is handed is a heap block of exactly its bytes: the dictionary dict_len, the output cap (of a resumable
// call: its room), the points max_points, a resume slot what the model says a slot takes.  The input is made exactly the aligned
// dwords that cover it by the model (tests/model/model_input.h), and every case runs twice: with the stream at the end of its
// block, and at the block's start behind 0 to 3 bytes (the case's number modulo 4).
//   usage: san_inflate CASEFILE
//   a case: 0 name, 1 entry, 2 input, 3 dictionary (a segment: its window), 4 cap, 5 ring, 6 what is compared (bits, below),
//           7 status, 8 detail0, 9 detail1, 10 out_len, 11 in_used, 12 checksum, 13 the delivered bytes,
//           entry 3: 14 start_bit, 15 end_bit, 16 span, 17 max_points, 18 the count of points, 19 the points stored (2 x uint64 each)
//           entry 4: 14 format (0 zlib, 4 gzip, 32 raw), 15 bytes per feed (0: all at once), 16 whether the last feed says it is,
//                    17 the room of a call: 4096 bytes, or less.  include/pzg.h asks for 4096 bytes at least (the decoders
//                    deliver whole 16-byte groups, and what the last flush of a stream cannot store is counted and lost), so a
//                    smaller room is a PROBE: every call is first made with that room on a copy of the slot, also of exactly
//                    its bytes, for the sanitizers alone to judge, and then with 4096 bytes on the slot itself
//   entries: 0 raw (pzm_raw_decompress), 1 gzip (pzm_decompress_gzip), 2 zlib with FDICT (pzm_decompress_dict), 3 a segment or an
//   index build (pzm_seg_decompress), 4 a resumable decoder fed piece by piece: out_len, in_used and the bytes are the sums over
//   its calls, the status is the last call's, the checksum of a gzip decoder the CRC-32 of all it delivered, which must be the
//   one its trailers state (what resume_crc_kernel does on the device)
//   status is always compared; bits of field 6: 1 detail0, 2 detail1, 4 out_len, 8 in_used, 16 checksum, 32 bytes
#include "san_cases.h"

struct pzm_result {
    int32_t status;
    uint32_t detail0, detail1, adler;
    uint64_t out_len, in_used;
};
extern "C" {
int pzm_raw_decompress(const uint8_t *in, uint64_t in_len, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t cap, int ring_bits,
                       pzm_result *r);
int pzm_decompress_gzip(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, int ring_bits, pzm_result *r);
int pzm_decompress_dict(const uint8_t *in, uint64_t in_len, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t cap, pzm_result *r);
int pzm_seg_decompress(const uint8_t *in, uint64_t in_len, uint32_t start_bit, uint64_t end_bit, const uint8_t *dict, uint32_t dict_len, uint8_t *out,
                       uint64_t cap, uint64_t span, uint64_t *points, uint32_t max_points, uint32_t *npoints, pzm_result *r);
uint32_t pzm_resume_state_bytes_rb(int rb);
int pzm_resume_feed_rb(int rb, uint8_t *state, const uint8_t *in, uint64_t in_len, uint32_t final_input, uint8_t *out, uint64_t cap, pzm_result *r,
                       uint32_t *chunks);
uint32_t pzm_fmt_state_bytes(void);
int pzm_fmt_resume_feed(uint32_t format, uint8_t *state, const uint8_t *in, uint64_t in_len, uint32_t final_input, uint8_t *out, uint64_t cap,
                        pzm_result *r, uint32_t *chunks, uint32_t *gz_expect);
}

enum { CMP_D0 = 1, CMP_D1 = 2, CMP_OUT_LEN = 4, CMP_IN_USED = 8, CMP_SUM = 16, CMP_BYTES = 32 };

struct Got {
    pzm_result r;
    std::vector<uint8_t> bytes;  // what was delivered (below the capacity)
    uint32_t npoints = 0;
    std::vector<uint8_t> points;
    bool failed = false;  // the program itself could not go on
};

static void one_shot(const san::Case &c, Got &g)
{
    const std::vector<uint8_t> &in = c.b(2);
    const san::Block dict(c.b(3));
    const uint64_t cap = c.u(4);
    const int ring = (int)c.u(5);
    san::Block out((size_t)cap);
    memset(&g.r, 0xEE, sizeof(g.r));
    int rc = -2;
    switch (c.u(1)) {
#ifdef SAN_RAW
    case 0: rc = pzm_raw_decompress(in.data(), in.size(), dict.p, (uint32_t)dict.n, out.p, cap, ring, &g.r); break;
#endif
#ifdef SAN_HARNESS
    case 1: rc = pzm_decompress_gzip(in.data(), in.size(), out.p, cap, ring, &g.r); break;
    case 2: rc = pzm_decompress_dict(in.data(), in.size(), dict.p, (uint32_t)dict.n, out.p, cap, &g.r); break;
#endif
#ifdef SAN_SEG
    case 3: {
        const uint32_t max_points = (uint32_t)c.u(17);
        san::Block points(16 * (size_t)max_points);
        rc = pzm_seg_decompress(in.data(), in.size(), (uint32_t)c.u(14), c.u(15), dict.p, (uint32_t)dict.n, out.p, cap, c.u(16), points.as<uint64_t>(),
                                max_points, &g.npoints, &g.r);
        const size_t stored = g.npoints < max_points ? g.npoints : max_points;
        g.points.assign(points.p, points.p + 16 * stored);
        for (size_t i = 16 * stored; i < points.n; ++i) g.failed |= points.p[i] != 0xA5;  // nothing is stored past the count
        break;
    }
#endif
    default: break;
    }
    (void)ring;
    g.failed |= rc != 0;
    const uint64_t m = g.r.out_len < cap ? g.r.out_len : cap;
    g.bytes.assign(out.p, out.p + m);
}

#if defined(SAN_FMT) || defined(SAN_HARNESS)
enum { NEED_INPUT = 101, OUT_FULL = 102 };

// zlib's CRC-32, a bit at a time (nothing of the code under test)
static uint32_t crc32_bits(uint32_t crc, const uint8_t *p, size_t n)
{
    uint32_t reg = ~crc;
    for (size_t i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (0xedb88320u & (0u - (reg & 1u)));
    }
    return ~reg;
}

// One decoder through all its feeds, the way tests/resume_fmt_cases.py's Driver feeds one: what a call does not consume goes in
// front of the next piece, a call that ran out of room is repeated with the rest, and when every piece is in and the decoder
// still wants input, the end is signalled with a feed of what is left.
static void resumed(const san::Case &c, Got &g)
{
    const std::vector<uint8_t> &s = c.b(2);
    const int ring = (int)c.u(5);
    const uint32_t format = (uint32_t)c.u(14);
    const size_t step = c.u(15) ? (size_t)c.u(15) : s.size() + 1;
    const bool final_said = c.u(16) != 0;
    const uint64_t rooms = c.u(17);
#ifdef SAN_FMT
    san::Block state(pzm_fmt_state_bytes(), 0);
#else
    san::Block state(pzm_resume_state_bytes_rb(ring), 0);
#endif
    std::vector<uint8_t> data;  // what the next call gets
    size_t pos = 0;
    uint32_t fin = 0, crc = 0, chunks_seen = 0;
    bool pending = false;
    uint64_t out_sum = 0, in_sum = 0, idle = 0;
    memset(&g.r, 0, sizeof(g.r));
    for (;;) {
        if (!pending) {
            if (pos < s.size()) {
                const size_t n = s.size() - pos < step ? s.size() - pos : step;
                data.insert(data.end(), s.begin() + pos, s.begin() + pos + n);
                pos += n;
                fin = final_said && pos == s.size() ? 1u : 0u;
            } else
                fin = 1u;
        }
        if (rooms < 4096u) {  // the probe: this very call with the small room, on a copy of the slot
            san::Block probe(state.n, 0), small((size_t)rooms);
            memcpy(probe.p, state.p, state.n);
            pzm_result pr;
            uint32_t pc = 0, pe = 0;
            (void)pe;
#ifdef SAN_FMT
            const int prc = pzm_fmt_resume_feed(format, probe.p, data.data(), data.size(), fin, small.p, rooms, &pr, &pc, &pe);
#else
            const int prc = pzm_resume_feed_rb(ring, probe.p, data.data(), data.size(), fin, small.p, rooms, &pr, &pc);
#endif
            if (prc != 0 || pr.in_used > data.size()) g.failed = true;
        }
        const uint64_t room = 4096u;
        san::Block out((size_t)room);
        pzm_result r;
        memset(&r, 0xEE, sizeof(r));
        uint32_t chunks = 0, expect = 0;
#ifdef SAN_FMT
        const int rc = pzm_fmt_resume_feed(format, state.p, data.data(), data.size(), fin, out.p, room, &r, &chunks, &expect);
#else
        const int rc = pzm_resume_feed_rb(ring, state.p, data.data(), data.size(), fin, out.p, room, &r, &chunks);
#endif
        idle = r.status != OUT_FULL || r.out_len || r.in_used ? 0 : idle + 1;  // out of room in 4096 bytes, and nothing done
        if (rc != 0 || r.out_len > room || r.in_used > data.size() || chunks < chunks_seen || idle > 4) {  // (or it goes round in circles)
            g.failed = true;
            break;
        }
        chunks_seen = chunks;
        g.bytes.insert(g.bytes.end(), out.p, out.p + r.out_len);
        crc = crc32_bits(crc, out.p, (size_t)r.out_len);
        out_sum += r.out_len;
        in_sum += r.in_used;
        data.erase(data.begin(), data.begin() + (size_t)r.in_used);
        g.r = r;
        if (format == 4u) {
            g.r.adler = crc;
            if ((r.status == 0 || r.status == 19) && crc != expect) g.r.status = 10;  // PZG_E_CHECKSUM, as the CRC pass reports it
        }
        pending = r.status == OUT_FULL;
        if (pending) continue;
        if (r.status != NEED_INPUT) break;
        if (fin) {  // input wanted after the end was signalled
            g.failed = true;
            break;
        }
    }
    g.r.out_len = out_sum;
    g.r.in_used = in_sum;
}
#else
static void resumed(const san::Case &, Got &g) { g.failed = true; }
#endif

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        const std::string name = c.s(0);
        const char place[2][3] = {"e", {'s', (char)('0' + t.cases % 4), 0}};
        ++t.cases;
        for (int p = 0; p < 2; ++p) {
            setenv("PZM_TIGHT_INPUT", place[p], 1);
            Got g;
            if (c.u(1) == 4)
                resumed(c, g);
            else
                one_shot(c, g);
            const std::string what = name + " (" + place[p] + ")";
            const uint64_t cmp = c.u(6);
            if (g.failed) t.miss(what, "the run failed, went round in circles or stored a point past the count:", 1, 0);
            if (g.r.status != (int32_t)c.u(7)) t.miss(what, "status", g.r.status, (int32_t)c.u(7));
            if ((cmp & CMP_D0) && g.r.detail0 != (uint32_t)c.u(8)) t.miss(what, "detail0", g.r.detail0, (uint32_t)c.u(8));
            if ((cmp & CMP_D1) && g.r.detail1 != (uint32_t)c.u(9)) t.miss(what, "detail1", g.r.detail1, (uint32_t)c.u(9));
            if ((cmp & CMP_OUT_LEN) && g.r.out_len != c.u(10)) t.miss(what, "out_len", (long long)g.r.out_len, (long long)c.u(10));
            if ((cmp & CMP_IN_USED) && g.r.in_used != c.u(11)) t.miss(what, "in_used", (long long)g.r.in_used, (long long)c.u(11));
            if ((cmp & CMP_SUM) && g.r.adler != (uint32_t)c.u(12)) t.miss(what, "checksum", g.r.adler, (uint32_t)c.u(12));
            if ((cmp & CMP_BYTES) && g.bytes != c.b(13)) {
                const std::vector<uint8_t> &want = c.b(13);
                size_t at = 0;
                while (at < g.bytes.size() && at < want.size() && g.bytes[at] == want[at]) ++at;
                if (g.bytes.size() != want.size()) t.miss(what, "delivered bytes: length", (long long)g.bytes.size(), (long long)want.size());
                if (at < g.bytes.size() && at < want.size()) t.miss(what + " byte " + std::to_string(at), "value", g.bytes[at], want[at]);
            }
            if (c.u(1) == 3) {
                if (g.npoints != (uint32_t)c.u(18)) t.miss(what, "points", g.npoints, (uint32_t)c.u(18));
                if (g.points != c.b(19)) t.miss(what, "stored points: bytes", (long long)g.points.size(), (long long)c.b(19).size());
            }
        }
    }
    return t.done();
}
