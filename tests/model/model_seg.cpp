// model_seg.cpp -- TEST INFRASTRUCTURE: the segment instance of the kernel source, Decoder<15, false, false, true, true> (pieces of one
// indexed raw stream: pzg_index_build / pzg_decompress_many_segments), as a one-lane host program -- the way model_raw.cpp builds the
// raw instances -- so that the CPU suite can check it against system zlib without a GPU.  Never linked into libpzg.so; the product
// has no CPU path.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../pure_zlib_amd/csrc/inflate_core.h"
#include "model_input.h"

struct pzm_result {
    int32_t status;
    uint32_t detail0, detail1, adler;
    uint64_t out_len, in_used;
};

extern "C" {

// One segment (or, with span != 0, one index build: start_bit = end_bit = 0 then, and *npoints gets the points the stream has).  The
// input is allocated as exactly the aligned dwords that cover it, as the kernel reads it (model_input.h: at the end of the block, or
// where PZM_TIGHT_INPUT says; under ASan + UBSan in tests/test_sanitized_cores.py); no scratch: the windows alone, as the kernel.
int pzm_seg_decompress(const uint8_t *in, uint64_t in_len, uint32_t start_bit, uint64_t end_bit, const uint8_t *dict, uint32_t dict_len,
                       uint8_t *out, uint64_t cap, uint64_t span, uint64_t *points, uint32_t max_points, uint32_t *npoints, pzm_result *r)
{
    typedef pzg::Decoder<15, false, false, true, true> SegDecoder;
    static_assert(sizeof(pzg::IndexPoint) == 16, "two 64-bit words per point");
    auto *lds = (pzg::WaveLds<15> *)aligned_alloc(16, (sizeof(pzg::WaveLds<15>) + 15u) & ~(size_t)15u);
    memset(lds, 0xA5, sizeof(*lds));  // LDS is not zero-initialised on the device either
    const ModelInput ib = model_input(in, in_len, 0, true);
    SegDecoder dec(*lds);
    dec.seg_start = start_bit;
    dec.seg_end = end_bit;
    dec.idx_points = (pzg::IndexPoint *)points;
    dec.idx_cap = max_points;
    dec.idx_span = span;
    pzg::StreamResult sr;
    dec.run(ib.stream, in_len, out, cap, &sr, dict_len ? dict : nullptr, dict_len);
    if (npoints) *npoints = dec.idx_n;
    r->status = sr.status;
    r->detail0 = sr.detail0;
    r->detail1 = sr.detail1;
    r->adler = sr.adler;
    r->out_len = sr.out_len;
    r->in_used = sr.in_used;
    free(ib.buf);
    free(lds);
    return 0;
}
}
