// san_unfilter.cpp -- TEST INFRASTRUCTURE: the scanline unfilter (pure_zlib_amd/csrc/unfilter_core.h through
// tests/model/model_unfilter.cpp) under ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_cores.py writes from
// tests/pngcases.py.  The source is exactly the aligned dwords that hold it, the destination exactly those that hold the image's
// extent (model_unfilter.cpp).
//   usage: san_unfilter CASEFILE
//   a case: 0 name, 1 src, 2 mis, 3 dst_off, 4 stride, 5 row_bytes, 6 height, 7 bpp, 8 status, 9 detail0, 10 detail1,
//           11 the whole destination as it must be afterwards (it starts as bytes of 0xCD)
#include "san_cases.h"

extern "C" int pzu_unfilter(const uint8_t *src, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes, uint64_t dst_off, uint64_t stride,
                            uint32_t row_bytes, uint32_t height, uint32_t bpp, int32_t *sd);

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const std::vector<uint8_t> &src = c.b(1), &want = c.b(11);
        std::vector<uint8_t> dst(want.size(), 0xCD);
        int32_t sd[3] = {-1, -1, -1};
        const int rc = pzu_unfilter(src.data(), src.size(), (uint32_t)c.u(2), dst.data(), dst.size(), c.u(3), c.u(4), (uint32_t)c.u(5), (uint32_t)c.u(6),
                                    (uint32_t)c.u(7), sd);
        if (rc) t.miss(name, "return value", rc, 0);
        if (sd[0] != (int32_t)c.u(8)) t.miss(name, "status", sd[0], (int32_t)c.u(8));
        if ((uint32_t)sd[1] != (uint32_t)c.u(9)) t.miss(name, "detail0", (uint32_t)sd[1], (uint32_t)c.u(9));
        if ((uint32_t)sd[2] != (uint32_t)c.u(10)) t.miss(name, "detail1", (uint32_t)sd[2], (uint32_t)c.u(10));
        for (size_t i = 0; i < dst.size(); ++i)
            if (dst[i] != want[i]) {
                t.miss(name + " byte " + std::to_string(i), "value", dst[i], want[i]);
                break;
            }
    }
    return t.done();
}
