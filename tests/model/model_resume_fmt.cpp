// model_resume_fmt.cpp -- TEST INFRASTRUCTURE: the resumable gzip and raw instances of the kernel source (inflate_core.h),
// Decoder<12, true, true> and Decoder<12, false, true, true>, as a one-lane host program (PZG_WAVE == 1), so that the CPU suite can
// check their header / trailer phases and suspension rules without a GPU (tests/test_model_resume_formats.py).  What
// resume_crc_kernel does behind the decode kernel is modelled by the test itself (the CRC-32 of each call's delivery, appended with
// pzm_crc32_append -- inflate_core.h's crc32_append -- to the running value).  Never linked into libpzg.so; the product has no CPU path.
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

constexpr int RB = 12;  // the ring the resumable kernels are built for (pzg_kernels_b.hip PZG_RES_RING)

// one call on a decoder whose slot the caller keeps in `state` (pzm_fmt_state_bytes() bytes, zeroed for a fresh decoder)
template <bool GZ, bool RAW>
static void feed(uint8_t *state, const uint8_t *in, uint64_t in_len, uint32_t final_input, uint8_t *out, uint64_t cap, pzm_result *r, uint32_t *chunks,
                 uint32_t *gz_expect)
{
    typedef pzg::Decoder<RB, GZ, true, RAW> Dec;
    auto *lds = (pzg::WaveLds<RB> *)aligned_alloc(16, (sizeof(pzg::WaveLds<RB>) + 15u) & ~(size_t)15u);
    memset(lds, 0xA5, sizeof(*lds));  // LDS is not zero-initialised on the device either
    const ModelInput ib = model_input(in, in_len);  // (padded, or as PZM_TIGHT_INPUT says)
    Dec dec(*lds);
    pzg::StreamResult sr;
    // the wave's scratch (strips); PZM_NO_STRIPS=1 in the environment: the windows alone
    uint32_t *strip = getenv("PZM_NO_STRIPS") ? nullptr : (uint32_t *)malloc(sizeof(uint32_t) * Dec::STRIP_WORDS);
    if (strip) memset(strip, 0xC3, sizeof(uint32_t) * Dec::STRIP_WORDS);
    dec.strip = strip;
    dec.run_resume((pzg::ResumeState *)state, (uint32_t *)(state + pzg::ResumeSlot<RB>::IMAGE_OFF), state + pzg::ResumeSlot<RB>::HIST_OFF, ib.stream, in_len,
                   out, cap, final_input, &sr, chunks);
    r->status = sr.status;
    r->detail0 = sr.detail0;
    r->detail1 = sr.detail1;
    r->adler = sr.adler;
    r->out_len = sr.out_len;
    r->in_used = sr.in_used;
    *gz_expect = sr.gz_crc;
    free(strip);
    free(ib.buf);
    free(lds);
}

extern "C" {

uint32_t pzm_fmt_state_bytes(void) { return (uint32_t)pzg::ResumeSlot<RB>::BYTES; }
uint32_t pzm_fmt_scalar_bytes(void) { return (uint32_t)sizeof(pzg::ResumeState); }

// format: 4 (PZG_GZIP) or 32 (PZG_RAW); *gz_expect: gzip -- the CRC-32 the output so far must have by the trailers read
int pzm_fmt_resume_feed(uint32_t format, uint8_t *state, const uint8_t *in, uint64_t in_len, uint32_t final_input, uint8_t *out, uint64_t cap,
                        pzm_result *r, uint32_t *chunks, uint32_t *gz_expect)
{
    if (format == 4u) feed<true, false>(state, in, in_len, final_input, out, cap, r, chunks, gz_expect);
    else if (format == 32u) feed<false, true>(state, in, in_len, final_input, out, cap, r, chunks, gz_expect);
    else return -1;
    return 0;
}

uint32_t pzm_crc32_append(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return pzg::crc32_append(crc_a, crc_b, len_b); }
}
