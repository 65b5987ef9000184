// model_raw.cpp -- TEST INFRASTRUCTURE: the raw instance of the kernel source, Decoder<RB, false, false, true> (PZG_RAW: bare
// RFC 1951 streams), as a one-lane host program -- the way model_harness.cpp builds the zlib and gzip instances -- so that the CPU
// suite can check it against system zlib and the oracle without a GPU.  Never linked into libpzg.so; the product has no CPU path.
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

// the scratch a model "wave" keeps from one stream to the next (its profile is in it), one per ring
template <int RB>
static uint32_t *&kept_scratch()
{
    static uint32_t *kept = nullptr;
    return kept;
}

// One stream.  The input is padded on both sides with 8 bytes of 0xEE (the bit reader loads whole aligned dwords), or with
// PZM_TIGHT_INPUT in the environment allocated as exactly the aligned dwords that cover it (model_input.h; under ASan + UBSan in
// tests/test_sanitized_cores.py, which hands over a dictionary of exactly dict_len bytes and an output of exactly cap);
// PZM_NO_STRIPS=1: no scratch, the windows alone.
template <int RB>
static void run_one(const uint8_t *in, uint64_t in_len, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t cap, pzm_result *r)
{
    typedef pzg::Decoder<RB, false, false, true> RawDecoder;
    auto *lds = (pzg::WaveLds<RB> *)aligned_alloc(16, (sizeof(pzg::WaveLds<RB>) + 15u) & ~(size_t)15u);
    memset(lds, 0xA5, sizeof(*lds));  // LDS is not zero-initialised on the device either
    const ModelInput ib = model_input(in, in_len);
    RawDecoder dec(*lds);
    uint32_t *&kept = kept_scratch<RB>();
    if (!getenv("PZM_NO_STRIPS")) {
        if (!kept) {
            kept = (uint32_t *)malloc(sizeof(uint32_t) * RawDecoder::STRIP_WORDS);
            memset(kept, 0xC3, sizeof(uint32_t) * RawDecoder::STRIP_WORDS);
        }
        dec.strip = kept;
    }
    pzg::StreamResult sr;
    dec.run(ib.stream, in_len, out, cap, &sr, dict_len ? dict : nullptr, dict_len);
    r->status = sr.status;
    r->detail0 = sr.detail0;
    r->detail1 = sr.detail1;
    r->adler = sr.adler;
    r->out_len = sr.out_len;
    r->in_used = sr.in_used;
    free(ib.buf);
    free(lds);
}

extern "C" {

// dict_len = 0: none.  What the launch does: the ring's instance, then the 32 KiB-ring pass for the streams it handed back.
int pzm_raw_decompress(const uint8_t *in, uint64_t in_len, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t cap, int ring_bits,
                       pzm_result *r)
{
    if (ring_bits == 15) run_one<15>(in, in_len, dict, dict_len, out, cap, r);
    else if (ring_bits == 14) run_one<14>(in, in_len, dict, dict_len, out, cap, r);
    else if (ring_bits == 13) run_one<13>(in, in_len, dict, dict_len, out, cap, r);
    else if (ring_bits == 12) run_one<12>(in, in_len, dict, dict_len, out, cap, r);
    else if (ring_bits == 11) run_one<11>(in, in_len, dict, dict_len, out, cap, r);
    else return -1;
    if (r->status == pzg::ST_RETRY_FULL_RING) run_one<15>(in, in_len, dict, dict_len, out, cap, r);
    return 0;
}
}
