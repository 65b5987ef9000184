// pzg_stage_span.h -- the arithmetic of the image stages' host-pointer form (pzg_api.cpp image_stage_host): which bytes of the
// caller's src and dst travel, where an image lies in what travelled, how the metadata block is cut up, and which rows come back.
// Plain C++17 on host arrays, no HIP: tests/cxx/san_stage_span.cpp runs it under ASan + UBSan on blocks of exactly these sizes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

namespace pzg {

inline size_t pad256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// One image as the host path sees it.  An empty image (no pixels) is not read, not written, and its offsets are not looked at;
// src_len == 0 is an image with pixels that reads no source byte (its src_off is not looked at either).
struct StageExtent {
    uint64_t src_off = 0, src_len = 0;
    uint64_t dst_off = 0, dst_stride = 0, row_bytes = 0;  // row r: row_bytes bytes at dst_off + r * dst_stride
    uint32_t rows = 0;
    bool empty = true;
};

// [lo, hi) of an array: the bytes (or entries) its users name.  Nothing added yet: lo > hi.
struct Span {
    uint64_t lo = ~0ull, hi = 0;
    void add(uint64_t off, uint64_t len)
    {
        lo = std::min(lo, off);
        hi = std::max(hi, off + len);
    }
    bool unused() const { return lo > hi; }
    void normalise() { if (unused()) lo = hi = 0; }  // an unused span travels as no bytes from offset 0
    size_t size() const { return (size_t)(hi - lo); }
    uint64_t rebased(uint64_t off, bool used) const { return used ? off - lo : 0u; }
    // the span keeps its place modulo 16: a row is fetched and stored at the alignment the caller gave it
    size_t skew(const void *base) const { return (size_t)(((uintptr_t)base + lo) & 15u); }
};

// The spans of src and dst that a call's images cover.
struct StageSpans {
    Span s, d;
    void add(const StageExtent &e)
    {
        if (e.empty) return;
        d.add(e.dst_off, (uint64_t)(e.rows - 1u) * e.dst_stride + e.row_bytes);
        if (e.src_len) s.add(e.src_off, e.src_len);
    }
    bool nothing() const { return d.unused(); }  // nothing but empty images
    uint64_t src_at(const StageExtent &e) const { return s.rebased(e.src_off, !e.empty && e.src_len != 0u); }
    uint64_t dst_at(const StageExtent &e) const { return d.rebased(e.dst_off, !e.empty); }
    // rows [0, min(rows, e.rows)) of the image, from the staged span of dst (its byte 0 is the caller's byte d.lo) into the caller's dst
    void copy_back(const StageExtent &e, uint32_t rows, const uint8_t *staged, uint8_t *dst_base) const
    {
        if (e.empty) return;
        rows = std::min(rows, e.rows);
        for (uint32_t r = 0; r < rows; ++r) {
            const uint64_t at = e.dst_off + (uint64_t)r * e.dst_stride;
            memcpy(dst_base + at, staged + (at - d.lo), e.row_bytes);
        }
    }
};

// A piece of the metadata block: the same offset in the host's copy and in the device's.
template <class T>
struct MetaPiece {
    size_t off = 0;
    T *in(uint8_t *block) const { return (T *)(void *)(block + off); }
};

// Cuts the block into pad256-rounded pieces, in the order they are asked for.  `at` is the size of what was handed out so far.
struct MetaCursor {
    size_t at = 0;
    template <class T>
    MetaPiece<T> take(size_t count)
    {
        const MetaPiece<T> p{at};
        at += pad256(sizeof(T) * count);
        return p;
    }
};

// What every stage's block ends with, behind the m_in bytes of what goes up: the statuses and details that come down.  m_all: all of it.
struct MetaResults {
    size_t m_in, m_all;
    MetaPiece<int32_t> status;
    MetaPiece<uint32_t> detail;
    MetaResults(MetaCursor c, size_t n) : m_in(c.at), status(c.take<int32_t>(n)), detail(c.take<uint32_t>(2 * n)) { m_all = c.at; }
};

}  // namespace pzg
