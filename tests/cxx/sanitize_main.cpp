// sanitize_main.cpp -- TEST INFRASTRUCTURE: runs the oracle and the kernel host model (inflate_core.h
// compiled for the host) over the streams named on the command line under ASan + UBSan.
// GPU AddressSanitizer is not available on this pool; the kernel's indexing logic is the same source.
//   usage: sanitize_main <capacity> <ring_bits> file.z [file.z ...]
//   (PZM_TIGHT_INPUT=1: the model reads each stream from an allocation that ends with it -- tests/model/model_harness.cpp;
//   PZM_SAN_BUNDLES=1: the streams go through the bundles too)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../oracle/pz_oracle.h"

struct pzm_result {
    int32_t status;
    uint32_t detail0, detail1, adler;
    uint64_t out_len, in_used;
};
extern "C" int pzm_decompress(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, int ring_bits, pzm_result *r);
extern "C" int pzm_bundle(const uint8_t *const *ins, const uint64_t *in_lens, uint8_t *const *outs, const uint64_t *caps, uint32_t n,
                          pzm_result *r);

// PZM_SAN_BUNDLES=1: the streams also go through the bundles, 64 at a time; a lane that comes back clean must have the oracle's status
static int bundles(const std::vector<std::vector<uint8_t>> &zs, uint64_t cap)
{
    int bad = 0;
    for (size_t b0 = 0; b0 < zs.size(); b0 += 64) {
        const uint32_t n = (uint32_t)(zs.size() - b0 < 64 ? zs.size() - b0 : 64);
        std::vector<const uint8_t *> ins(n);
        std::vector<uint64_t> lens(n), caps(n, cap);
        std::vector<std::vector<uint8_t>> outs(n, std::vector<uint8_t>(cap ? cap : 1));
        std::vector<uint8_t *> op(n);
        std::vector<pzm_result> r(n);
        for (uint32_t k = 0; k < n; ++k) {
            ins[k] = zs[b0 + k].data();
            lens[k] = zs[b0 + k].size();
            op[k] = outs[k].data();
        }
        if (pzm_bundle(ins.data(), lens.data(), op.data(), caps.data(), n, r.data()) != 0) return 1;
        for (uint32_t k = 0; k < n; ++k) {
            if (r[k].status == 103) continue;  // handed back to the ordinary kernel
            std::vector<uint8_t> o(cap ? cap : 1);
            pzo_result ro;
            pzo_decompress(zs[b0 + k].data(), zs[b0 + k].size(), o.data(), cap, &ro);
            if (ro.status != r[k].status) {
                printf("BUNDLE MISMATCH stream %zu: oracle %d bundle %d\n", b0 + k, ro.status, r[k].status);
                bad++;
            }
        }
    }
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const uint64_t cap = strtoull(argv[1], nullptr, 10);
    const int rb = atoi(argv[2]);
    int bad = 0;
    std::vector<std::vector<uint8_t>> all;
    for (int i = 3; i < argc; ++i) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<uint8_t> z;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) z.insert(z.end(), buf, buf + n);
        fclose(f);
        all.push_back(z);
        std::vector<uint8_t> o1(cap ? cap : 1), o2(cap ? cap : 1);
        pzo_result ro;
        pzm_result rm;
        pzo_decompress(z.data(), z.size(), o1.data(), cap, &ro);
        pzm_decompress(z.data(), z.size(), o2.data(), cap, rb, &rm);
        const uint64_t m = ro.out_len < cap ? ro.out_len : cap;
        if (ro.status != rm.status || (ro.status == 0 && (ro.out_len != rm.out_len || memcmp(o1.data(), o2.data(), m) != 0))) {
            printf("MISMATCH %s: oracle %d model %d\n", argv[i], ro.status, rm.status);
            bad++;
        }
    }
    if (getenv("PZM_SAN_BUNDLES")) bad += bundles(all, cap);
    printf("checked %d streams, %d mismatches\n", argc - 3, bad);
    return bad ? 1 : 0;
}
