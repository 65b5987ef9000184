// model_input.h -- TEST INFRASTRUCTURE: the input buffer of the one-lane host models of inflate_core.h.  The bit reader loads whole
// aligned dwords, so a stream is handed over in one of three ways, chosen by PZM_TIGHT_INPUT in the environment (read at every
// call, so a program may change it from one call to the next):
//   unset        padded with 8 bytes of 0xEE on both sides (`front` more in front: every alignment of the first byte);
//                `tight_default`: as "1"
//   "1", "end"   a heap block of exactly the aligned dwords that cover the stream, which ENDS at the block's end (it starts
//                -len mod 4 bytes into it)
//   "s0".."s3"   such a block with the stream 0 to 3 bytes behind its START (its last dword ends the block)
// so that under AddressSanitizer a read outside those dwords is caught on either side (tests/test_sanitized_cores.py).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

struct ModelInput {
    uint8_t *buf;  // to be freed
    const uint8_t *stream;
};
static inline ModelInput model_input(const uint8_t *in, uint64_t in_len, uint32_t front = 0, bool tight_default = false)
{
    ModelInput b;
    {
        const char *how = getenv("PZM_TIGHT_INPUT");
        if (!how && tight_default) how = "end";
        if (how) {
            const uint64_t mis = how[0] == 's' ? (uint64_t)(how[1] - '0') & 3u : (4u - (in_len & 3u)) & 3u;
            const uint64_t all = (mis + in_len + 3u) & ~(uint64_t)3u;
            b.buf = (uint8_t *)malloc(all ? all : 1);
            memset(b.buf, 0xEE, all);
            if (in_len) memcpy(b.buf + mis, in, in_len);
            b.stream = b.buf + mis;
        } else {
            b.buf = (uint8_t *)malloc(in_len + 16 + front);
            memset(b.buf, 0xEE, in_len + 16 + front);
            if (in_len) memcpy(b.buf + 8 + front, in, in_len);
            b.stream = b.buf + 8 + front;
        }
    }
    return b;
}
