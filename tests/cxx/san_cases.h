// san_cases.h -- TEST INFRASTRUCTURE: what the case-file programs (san_*.cpp; tests/sancases.py writes their files) share.
//
// THE CASE FILE: cases one behind the other up to the end of the file.  A case is a little-endian uint32 -- the number of its
// fields -- and then each field as a little-endian uint64 length and that many bytes.  A field is either bytes as they are or an
// integer, which is a field of eight bytes, little-endian.  What field k of a case means is said at the top of each program.
//
// Block: a heap block of EXACTLY n bytes, so that under AddressSanitizer an access one byte outside it is reported; n == 0 gives
// the address just behind another block, where nothing at all may be touched.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace san {

struct Case {
    std::vector<std::vector<uint8_t>> f;
    uint64_t u(size_t k) const
    {
        if (k >= f.size() || f[k].size() != 8) {
            fprintf(stderr, "case file: field %zu is no integer\n", k);
            exit(2);
        }
        uint64_t v;
        memcpy(&v, f[k].data(), 8);
        return v;
    }
    const std::vector<uint8_t> &b(size_t k) const
    {
        if (k >= f.size()) {
            fprintf(stderr, "case file: no field %zu\n", k);
            exit(2);
        }
        return f[k];
    }
    std::string s(size_t k) const { return std::string(b(k).begin(), b(k).end()); }
};

inline std::vector<Case> read_cases(const char *path)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<Case> all;
    uint32_t nf;
    while (fread(&nf, 4, 1, fp) == 1) {
        Case c;
        for (uint32_t k = 0; k < nf; ++k) {
            uint64_t len;
            if (fread(&len, 8, 1, fp) != 1) exit(2);
            std::vector<uint8_t> v((size_t)len);
            if (len && fread(v.data(), 1, (size_t)len, fp) != (size_t)len) exit(2);
            c.f.push_back(std::move(v));
        }
        all.push_back(std::move(c));
    }
    fclose(fp);
    return all;
}

struct Block {
    uint8_t *base, *p;
    size_t n;
    explicit Block(size_t bytes, int fill = 0xA5) : n(bytes)
    {
        base = (uint8_t *)malloc(n ? n : 16);
        memset(base, fill, n ? n : 16);
        p = n ? base : base + 16;
    }
    Block(const std::vector<uint8_t> &v) : Block(v.size())
    {
        if (n) memcpy(p, v.data(), n);
    }
    Block(const Block &) = delete;
    ~Block() { free(base); }
    template <class T>
    T *as() const
    {
        return (T *)(void *)p;
    }
};

// one line per mismatch, and the count
struct Tally {
    int cases = 0, bad = 0;
    void miss(const std::string &name, const char *what, long long got, long long want)
    {
        printf("MISMATCH %s: %s %lld, expected %lld\n", name.c_str(), what, got, want);
        ++bad;
    }
    int done() const
    {
        printf("%d cases, %d mismatches\n", cases, bad);
        return bad ? 1 : 0;
    }
};

}  // namespace san
