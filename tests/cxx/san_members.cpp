// san_members.cpp -- TEST INFRASTRUCTURE: the member finder and the layout (pure_zlib_amd/csrc/member_core.h through
// tests/model/model_members.cpp) under ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_cores.py writes from
// tests/memberscheck.py.  The input is exactly the aligned dwords that hold it, starts / bsize have exactly max_members entries and
// the layout's arrays exactly m (model_members.cpp).
//   usage: san_members CASEFILE
//   a finder case: 0 name, 1 the number 0, 2 input, 3 mis, 4 chunk (0: 64 KiB, as pzg_gzip_find_members takes it), 5 max_members,
//                  6 the count, 7 the starts stored (uint64 each), 8 their block sizes (uint32 each)
//   a layout case: 0 name, 1 the number 1, 2 input, 3 mis, 4 the starts (uint64 each), 5 out_base_off, 6 in_off, 7 in_len, 8 out_off,
//                  9 out_cap (uint64 each), 10 the total
#include "san_cases.h"

extern "C" int pzm_find(const uint8_t *in, uint64_t in_len, uint32_t mis, uint64_t chunk, uint64_t *starts, uint32_t *bsize, uint32_t max_members,
                        uint64_t *nmembers);
extern "C" int pzm_layout(const uint8_t *in, uint64_t in_len, uint32_t mis, const uint64_t *starts, uint64_t m, uint64_t out_base_off, uint64_t *in_off,
                          uint64_t *in_lenv, uint64_t *out_off, uint64_t *out_cap, uint64_t *total);

static bool same(const san::Block &got, const std::vector<uint8_t> &want) { return got.n == want.size() && (!got.n || !memcmp(got.p, want.data(), got.n)); }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const std::vector<uint8_t> &in = c.b(2);
        const uint32_t mis = (uint32_t)c.u(3);
        if (c.u(1) == 0) {
            const uint64_t chunk = c.u(4) ? c.u(4) : 65536u;
            const uint32_t room = (uint32_t)c.u(5);
            san::Block starts(8 * (size_t)room), bsize(4 * (size_t)room);
            uint64_t n = ~0ull;
            const int rc = pzm_find(in.data(), in.size(), mis, chunk, starts.as<uint64_t>(), bsize.as<uint32_t>(), room, &n);
            if (rc) t.miss(name, "return value", rc, 0);
            if (n != c.u(6)) t.miss(name, "count", (long long)n, (long long)c.u(6));
            // what is stored, and behind it the entries the call must leave as they were
            std::vector<uint8_t> ws = c.b(7), wb = c.b(8);
            ws.resize(8 * (size_t)room, 0xA5);
            wb.resize(4 * (size_t)room, 0xA5);
            if (!same(starts, ws)) t.miss(name, "starts", 0, 1);
            if (!same(bsize, wb)) t.miss(name, "bsize", 0, 1);
        } else {
            const san::Block starts(c.b(4));
            const uint64_t m = starts.n / 8;
            san::Block io(8 * (size_t)m), il(8 * (size_t)m), oo(8 * (size_t)m), oc(8 * (size_t)m);
            uint64_t total = ~0ull;
            const int rc = pzm_layout(in.data(), in.size(), mis, starts.as<const uint64_t>(), m, c.u(5), io.as<uint64_t>(), il.as<uint64_t>(),
                                      oo.as<uint64_t>(), oc.as<uint64_t>(), &total);
            if (rc) t.miss(name, "return value", rc, 0);
            if (!same(io, c.b(6))) t.miss(name, "in_off", 0, 1);
            if (!same(il, c.b(7))) t.miss(name, "in_len", 0, 1);
            if (!same(oo, c.b(8))) t.miss(name, "out_off", 0, 1);
            if (!same(oc, c.b(9))) t.miss(name, "out_cap", 0, 1);
            if (total != c.u(10)) t.miss(name, "total", (long long)total, (long long)c.u(10));
        }
    }
    return t.done();
}
