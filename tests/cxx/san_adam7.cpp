// san_adam7.cpp -- TEST INFRASTRUCTURE: the Adam7 gather (pure_zlib_amd/csrc/adam7_core.h through tests/model/model_adam7.cpp) under
// ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_adam7.py writes from tests/adam7cases.py.  The source is
// exactly the aligned dwords that hold its extent, the destination exactly the image's bytes (model_adam7.cpp).
//   usage: san_adam7 CASEFILE
//   a case: 0 name, 1 src, 2 mis, 3 dst_off, 4 stride, 5 width, 6 height, 7 pixel_bits, 8 row slices, 9 status, 10 detail0, 11 detail1,
//           12 the whole destination as it must be afterwards (it starts as bytes of 0xCD)
#include "san_cases.h"

extern "C" int pza_adam7(const uint8_t *src, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t dst_off, uint64_t stride,
                         uint32_t width, uint32_t height, uint32_t bits, uint32_t slices, int32_t *sd);

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const std::vector<uint8_t> &src = c.b(1), &want = c.b(12);
        std::vector<uint8_t> dst(want.size(), 0xCD);
        int32_t sd[3] = {-1, -1, -1};
        const int rc = pza_adam7(src.data(), src.size(), (uint32_t)c.u(2), dst.data(), dst.size(), c.u(3), c.u(4), (uint32_t)c.u(5), (uint32_t)c.u(6),
                                 (uint32_t)c.u(7), (uint32_t)c.u(8), sd);
        if (rc) t.miss(name, "return value", rc, 0);
        if (sd[0] != (int32_t)c.u(9)) t.miss(name, "status", sd[0], (int32_t)c.u(9));
        if ((uint32_t)sd[1] != (uint32_t)c.u(10)) t.miss(name, "detail0", (uint32_t)sd[1], (uint32_t)c.u(10));
        if ((uint32_t)sd[2] != (uint32_t)c.u(11)) t.miss(name, "detail1", (uint32_t)sd[2], (uint32_t)c.u(11));
        for (size_t i = 0; i < dst.size(); ++i)
            if (dst[i] != want[i]) {
                t.miss(name + " byte " + std::to_string(i), "value", dst[i], want[i]);
                break;
            }
    }
    return t.done();
}
