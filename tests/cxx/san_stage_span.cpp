// san_stage_span.cpp -- TEST INFRASTRUCTURE: the staging arithmetic of the image stages' host-pointer form
// (pure_zlib_amd/csrc/pzg_stage_span.h, nothing else of the library) under ASan + UBSan over a case file (san_cases.h) that
// tests/test_sanitized_stage_span.py writes.  The staged source span, the staged destination span, the caller's destination and the
// metadata block are heap blocks of exactly the computed sizes, so an offset one byte outside is a report.  The caller's base
// pointers lie `mis` bytes into 16-byte aligned blocks.  The program paints every byte of the staged destination span -- the byte
// that belongs at the caller's offset k is pattern(k) --, copies back the rows the case says were delivered, and compares.
//   usage: san_stage_span CASEFILE
//   a case: 0 name, 1 n; 2 - 9 n 64-bit words each: src_off, src_len, dst_off, dst_stride, row_bytes, rows, empty, delivered rows;
//           10 src mis, 11 dst mis; expected: 12 nothing but empty images, 13 s_lo, 14 s_hi (normalised), 15 d_lo, 16 d_hi, 17 s_skew,
//           18 d_skew, 19 n words src_at, 20 n words dst_at, 21 the caller's destination as it must be afterwards (it starts as 0xCD);
//           the block: 22 pairs of words (element size, count) to take, 23 a word per take: its offset, 24 m_in, 25 m_all
#include "../../pure_zlib_amd/csrc/pzg_stage_span.h"
#include "san_cases.h"

static uint8_t pattern(uint64_t k)
{
    const uint8_t v = (uint8_t)(k * 31u + 7u);
    return v == 0xCD ? 0x11 : v;
}

static std::vector<uint64_t> words(const std::vector<uint8_t> &b)
{
    std::vector<uint64_t> w(b.size() / 8);
    if (!w.empty()) memcpy(w.data(), b.data(), 8 * w.size());
    return w;
}

struct Desc64 {
    uint8_t b[64];
};

template <class T>
static size_t take_and_touch(pzg::MetaCursor &c, size_t count, uint8_t *block)
{
    const pzg::MetaPiece<T> p = c.take<T>(count);
    if (block && count) {  // the piece's first and last element
        memset(&p.in(block)[0], 0x5A, sizeof(T));
        memset(&p.in(block)[count - 1], 0x5A, sizeof(T));
    }
    return p.off;
}

static size_t take_sized(pzg::MetaCursor &c, uint64_t size, size_t count, uint8_t *block)
{
    switch (size) {
    case 1: return take_and_touch<uint8_t>(c, count, block);
    case 4: return take_and_touch<uint32_t>(c, count, block);
    case 8: return take_and_touch<uint64_t>(c, count, block);
    case 64: return take_and_touch<Desc64>(c, count, block);
    }
    fprintf(stderr, "case file: no element of %llu bytes\n", (unsigned long long)size);
    exit(2);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    san::Tally t;
    for (const san::Case &c : san::read_cases(argv[1])) {
        ++t.cases;
        const std::string name = c.s(0);
        const size_t n = (size_t)c.u(1);
        std::vector<uint64_t> f[8];
        for (int k = 0; k < 8; ++k) f[k] = words(c.b(2 + k));
        std::vector<pzg::StageExtent> ext(n);
        for (size_t i = 0; i < n; ++i) ext[i] = pzg::StageExtent{f[0][i], f[1][i], f[2][i], f[3][i], f[4][i], (uint32_t)f[5][i], f[6][i] != 0};
        const std::vector<uint64_t> delivered = f[7], src_at = words(c.b(19)), dst_at = words(c.b(20));
        const std::vector<uint8_t> &want = c.b(21);

        // the spans
        pzg::StageSpans sp;
        for (size_t i = 0; i < n; ++i) sp.add(ext[i]);
        if (sp.nothing() != (c.u(12) != 0)) t.miss(name, "nothing", sp.nothing(), (long long)c.u(12));
        sp.s.normalise();
        if (sp.s.lo != c.u(13)) t.miss(name, "s_lo", (long long)sp.s.lo, (long long)c.u(13));
        if (sp.s.hi != c.u(14)) t.miss(name, "s_hi", (long long)sp.s.hi, (long long)c.u(14));
        if (!sp.nothing()) {
            if (sp.d.lo != c.u(15)) t.miss(name, "d_lo", (long long)sp.d.lo, (long long)c.u(15));
            if (sp.d.hi != c.u(16)) t.miss(name, "d_hi", (long long)sp.d.hi, (long long)c.u(16));
        }

        // the base pointers and their skews
        const size_t s_mis = (size_t)c.u(10), d_mis = (size_t)c.u(11);
        san::Block src_caller(s_mis + 1), dst_caller(d_mis + want.size(), 0xCD);
        if (((uintptr_t)src_caller.p | (uintptr_t)dst_caller.p) & 15u) {
            fprintf(stderr, "the allocator gave a block off the 16-byte boundary\n");
            return 2;
        }
        uint8_t *dst_base = dst_caller.p + d_mis;
        if (!sp.nothing()) {
            if (sp.s.skew(src_caller.p + s_mis) != c.u(17)) t.miss(name, "s_skew", (long long)sp.s.skew(src_caller.p + s_mis), (long long)c.u(17));
            if (sp.d.skew(dst_base) != c.u(18)) t.miss(name, "d_skew", (long long)sp.d.skew(dst_base), (long long)c.u(18));
        }

        // the staged spans: every rebased offset with its extent inside them (the first and the last byte are touched)
        if (!sp.nothing()) {
            san::Block s_staged(sp.s.size()), d_staged(sp.d.size());
            for (size_t k = 0; k < d_staged.n; ++k) d_staged.p[k] = pattern(sp.d.lo + k);
            unsigned sum = 0;
            for (size_t i = 0; i < n; ++i) {
                const pzg::StageExtent &e = ext[i];
                const uint64_t sa = sp.src_at(e), da = sp.dst_at(e);
                if (sa != src_at[i]) t.miss(name + " image " + std::to_string(i), "src_at", (long long)sa, (long long)src_at[i]);
                if (da != dst_at[i]) t.miss(name + " image " + std::to_string(i), "dst_at", (long long)da, (long long)dst_at[i]);
                if (e.empty) continue;
                if (e.src_len) sum += s_staged.p[sa] + s_staged.p[sa + e.src_len - 1];
                sum += d_staged.p[da] + d_staged.p[da + (uint64_t)(e.rows - 1u) * e.dst_stride + e.row_bytes - 1];
            }
            if (sum == 0xffffffffu) printf("(%u)\n", sum);  // (the reads are used)
            for (size_t i = 0; i < n; ++i) sp.copy_back(ext[i], (uint32_t)delivered[i], d_staged.p, dst_base);
        }
        for (size_t k = 0; k < d_mis; ++k)
            if (dst_caller.p[k] != 0xCD) {
                t.miss(name + " byte " + std::to_string(k) + " in front of dst_base", "value", dst_caller.p[k], 0xCD);
                break;
            }
        for (size_t k = 0; k < want.size(); ++k)
            if (dst_base[k] != want[k]) {
                t.miss(name + " byte " + std::to_string(k), "value", dst_base[k], want[k]);
                break;
            }

        // the metadata block
        const std::vector<uint64_t> takes = words(c.b(22)), offs = words(c.b(23));
        pzg::MetaCursor sizing;
        for (size_t k = 0; k < offs.size(); ++k) take_sized(sizing, takes[2 * k], (size_t)takes[2 * k + 1], nullptr);
        const pzg::MetaResults m(sizing, n);
        if (m.m_in != c.u(24)) t.miss(name, "m_in", (long long)m.m_in, (long long)c.u(24));
        if (m.m_all != c.u(25)) t.miss(name, "m_all", (long long)m.m_all, (long long)c.u(25));
        san::Block block(m.m_all);
        pzg::MetaCursor cur;
        for (size_t k = 0; k < offs.size(); ++k) {
            const size_t off = take_sized(cur, takes[2 * k], (size_t)takes[2 * k + 1], block.p);
            if (off != offs[k]) t.miss(name + " take " + std::to_string(k), "offset", (long long)off, (long long)offs[k]);
        }
        if (n) {
            m.status.in(block.p)[0] = m.status.in(block.p)[n - 1] = 1;
            m.detail.in(block.p)[0] = m.detail.in(block.p)[2 * n - 1] = 1;
        }
        if (m.status.off != m.m_in || (size_t)((uint8_t *)m.detail.in(block.p) - block.p) != m.m_in + (4 * n + 255) / 256 * 256)
            t.miss(name, "status / detail offsets", (long long)m.status.off, (long long)m.m_in);
    }
    return t.done();
}
