// san_unlzw.cpp -- TEST INFRASTRUCTURE: the LZW decoder (pure_zlib_amd/csrc/unlzw_core.h through tests/model/model_unlzw.cpp) under
// ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_unlzw.py writes from tests/lzwcases.py.  The source is exactly
// the aligned dwords that hold the stream, the stream's output exactly out_cap bytes (model_unlzw.cpp).
//   usage: san_unlzw CASEFILE
//   a case: 0 name, 1 the stream, 2 mis, 3 out_off, 4 out_cap, 5 early change, 6 status, 7 out_len, 8 detail0, 9 detail1,
//           10 the whole destination as it must be afterwards (it starts as bytes of 0xCD)
#include "san_cases.h"

extern "C" int pzs_unlzw(const uint8_t *in, uint64_t in_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t out_off, uint64_t out_cap,
                         uint32_t early_change, int64_t *res);

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const std::vector<uint8_t> &in = c.b(1), &want = c.b(10);
        std::vector<uint8_t> dst(want.size(), 0xCD);
        int64_t res[4] = {-1, -1, -1, -1};
        const int rc = pzs_unlzw(in.data(), in.size(), (uint32_t)c.u(2), dst.data(), dst.size(), c.u(3), c.u(4), (uint32_t)c.u(5), res);
        if (rc) t.miss(name, "return value", rc, 0);
        if (res[0] != (int64_t)c.u(6)) t.miss(name, "status", res[0], (int64_t)c.u(6));
        if (res[1] != (int64_t)c.u(7)) t.miss(name, "out_len", res[1], (int64_t)c.u(7));
        if (res[2] != (int64_t)c.u(8)) t.miss(name, "detail0", res[2], (int64_t)c.u(8));
        if (res[3] != (int64_t)c.u(9)) t.miss(name, "detail1", res[3], (int64_t)c.u(9));
        for (size_t i = 0; i < dst.size(); ++i)
            if (dst[i] != want[i]) {
                t.miss(name + " byte " + std::to_string(i), "value", dst[i], want[i]);
                break;
            }
    }
    return t.done();
}
