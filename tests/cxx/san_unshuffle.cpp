// san_unshuffle.cpp -- TEST INFRASTRUCTURE: the byte-plane stage (pure_zlib_amd/csrc/unshuffle_core.h through
// tests/model/model_unshuffle.cpp) under ASan + UBSan over a case file (san_cases.h) that tests/test_sanitized_unshuffle.py writes from
// tests/fpcases.py.  The source is exactly the aligned dwords that hold the bytes the job may read, the destination exactly the
// window's bytes (model_unshuffle.cpp).
//   usage: san_unshuffle CASEFILE
//   a case: 0 name, 1 the descriptor (64 bytes), 2 the source bytes the job may read, 3 src_len, 4 mis, 5 row slices, 6 the last wave
//           first, 7 status, 8 detail0, 9 detail1, 10 the whole destination as it must be afterwards (it starts as bytes of 0xCD)
#include "san_cases.h"

extern "C" int pzs_unshuffle(const void *desc, const uint8_t *src, uint64_t src_bytes, uint64_t src_len, uint32_t mis, uint8_t *dst, uint64_t dst_bytes,
                             uint32_t slices, int descending, int32_t *sd);

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const std::vector<uint8_t> &desc = c.b(1), &src = c.b(2), &want = c.b(10);
        if (desc.size() != 64) return 2;
        std::vector<uint8_t> dst(want.size(), 0xCD);
        int32_t sd[3] = {-1, -1, -1};
        const int rc = pzs_unshuffle(desc.data(), src.data(), src.size(), c.u(3), (uint32_t)c.u(4), dst.data(), dst.size(), (uint32_t)c.u(5), (int)c.u(6), sd);
        if (rc) t.miss(name, "return value", rc, 0);
        if (sd[0] != (int32_t)c.u(7)) t.miss(name, "status", sd[0], (int32_t)c.u(7));
        if ((uint32_t)sd[1] != (uint32_t)c.u(8)) t.miss(name, "detail0", (uint32_t)sd[1], (uint32_t)c.u(8));
        if ((uint32_t)sd[2] != (uint32_t)c.u(9)) t.miss(name, "detail1", (uint32_t)sd[2], (uint32_t)c.u(9));
        for (size_t i = 0; i < dst.size(); ++i)
            if (dst[i] != want[i]) {
                t.miss(name + " byte " + std::to_string(i), "value", dst[i], want[i]);
                break;
            }
    }
    return t.done();
}
