// pzg_launch.h -- kernel argument block and launcher prototypes shared by pzg_kernels.hip and pzg_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pzg {

struct InflateArgs {
    const uint8_t *in_base;
    const uint64_t *in_off;   // n
    const uint64_t *in_len;   // n
    uint8_t *out_base;
    const uint64_t *out_off;  // n
    const uint64_t *out_cap;  // n
    uint64_t *out_len;        // n
    int32_t *status;          // n
    uint32_t *detail;         // 2n or null
    uint64_t *in_used;        // n or null
    uint32_t *adler;          // n or null
    const uint32_t *order;    // optional launch permutation (n) or null
    uint32_t *counter;        // device word the persistent waves draw stream indices from (zeroed per launch)
    uint64_t *prof_out;       // diagnostic builds only (-DPZG_PROFILE): 12 counters per stream, else null
    uint32_t n;
    uint32_t gzip;            // 0: zlib streams (RFC 1950, the reference's format); 1: gzip members (RFC 1952, an extension)
    uint32_t *gz_expect;      // gzip only: 2n words of device scratch: the CRC-32 the output must have (from the member trailers)
    // extension (PZG_FDICT): preset dictionaries, dict_base + dict_off[i] .. + dict_len[i] (0: none for stream i); null: none at all
    const uint8_t *dict_base;
    const uint64_t *dict_off;
    const uint64_t *dict_len;
    // token scratch of the launch's stream-waves (inflate_core.h strip_span): inflate_strip_bytes() bytes, or null -- the
    // kernels then decode by windows alone.  Must not be shared with a launch that may run at the same time.
    uint32_t *strip;
    uint32_t strip_waves;     // stream-waves (workgroups 0 .. strip_waves - 1) that own a slice of it; the others decode by windows alone
    // bundles (round 6; pzg_bundle_kernel.h): nonzero -- the launch's small streams of the fixed code are decoded 64 to a wave, one
    // lane per stream, before the ordinary kernel takes what is left.  zlib streams without dictionaries only.
    uint32_t bundle;
    uint32_t *bundle_report;  // null, or a word of page-locked HOST memory: the launch's last kernel leaves 1 + the streams the bundles decoded there
    // extension (PZG_RAW): 1 -- bare RFC 1951 streams, no header, no trailer, nothing checked (dictionaries apply unconditionally);
    // 2 -- and adler[] gets the CRC-32 of the bytes delivered instead of their Adler-32 (PZG_CRC32: one more pass over the output)
    uint32_t raw;
    // extension (indexed streams; raw != 0): nonzero -- the streams are SEGMENTS of a raw stream (pzg_kernels_b.hip inflate_seg_kernel, the
    // 32 KiB ring whatever the launch's ring): stream i starts at bit seg_start_bit[i] (0..7) of its first byte and ends with the block
    // that ends at bit seg_end_bit[i], counted from that byte's bit 0 (0: with the final block); either array may be null (all zeros)
    uint32_t seg;
    const uint8_t *seg_start_bit;  // n or null
    const uint64_t *seg_end_bit;   // n or null
    // ... and, idx_span != 0 (n = 1: the index build), the access points of the stream: {in_bit, out_pos} pairs, the first idx_cap of
    // them stored, all of them counted in *idx_count
    uint64_t *idx_points;
    uint32_t *idx_count;
    uint64_t idx_span;
    uint32_t idx_cap;
};

// one batched call of the resumable decoder (decompressIncremental): decoder i continues from its ResumeState
struct ResumeArgs {
    uint8_t *state_base;      // n slots of state_stride bytes: ResumeState + the LDS image (zeroed = a fresh decoder)
    uint64_t state_stride;
    const uint8_t *in_base;
    const uint64_t *in_off;   // n: the unconsumed tail of the last call followed by the new input
    const uint64_t *in_len;   // n
    const uint8_t *final_in;  // n or null: nonzero = no more input will follow (running out is an error then)
    uint8_t *out_base;
    const uint64_t *out_off;  // n: this call's output room
    const uint64_t *out_cap;  // n (>= 4096)
    uint64_t *out_len;        // n: bytes delivered by this call
    int32_t *status;          // n: PZG_DEC_NEED_INPUT / PZG_DEC_OUT_FULL / PZG_OK (done) / PZG_E_*
    uint32_t *detail;         // 2n or null
    uint64_t *in_used;        // n: input bytes the decoder is done with
    uint32_t *adler;          // n or null
    uint32_t *chunks;         // n: 32 KiB chunks the reference would have published so far (cumulative)
    uint32_t *counter;
    uint32_t n;
    // optional (null: off): every decoder also packs what it delivered behind the others' -- dense + dense_region + 16 * (the value
    // of *dense_cursor it drew), reported in dense_off[i] -- so that the host fetches one linear span instead of mostly empty rooms
    uint8_t *dense;
    uint64_t dense_region;
    uint32_t *dense_cursor;  // zeroed by the launcher's caller; counts 16-byte units
    uint64_t *dense_off;     // n
    // the stream-waves' scratch (inflate_core.h strip_span), resume_strip_wave_bytes() per wave, or null: workgroups 0 .. strip_waves - 1
    // own a slice, the others -- and all of them without it -- decode by windows alone.  Not shared with a launch that may run at the same time.
    uint32_t *strip;
    uint32_t strip_waves;
};
// format: RESUME_FORMAT_ZLIB -- zlib decoders (inflate_resume_kernel); RESUME_FORMAT_GZIP (PZG_GZIP) -- gzip decoders: resume_gzip_kernel,
// then resume_crc_kernel over what they delivered; RESUME_FORMAT_RAW (PZG_RAW) -- raw decoders (resume_raw_kernel)
constexpr uint32_t RESUME_FORMAT_ZLIB = 0u, RESUME_FORMAT_GZIP = 4u, RESUME_FORMAT_RAW = 32u;  // (pzg_api.cpp holds them against include/pzg.h)
hipError_t launch_resume(const ResumeArgs &a, uint32_t format, int num_cus, hipStream_t stream);
hipError_t launch_resume_crc(const ResumeArgs &a, int num_cus, hipStream_t stream);  // (pzg_kernels.hip, beside the batch CRC passes)
size_t resume_state_bytes();   // one decoder's slot: ResumeState + LDS image
size_t resume_scalar_bytes();  // ... its ResumeState part (zeroing it makes the decoder fresh)
size_t resume_strip_wave_bytes();                      // one stream-wave's slice of ResumeArgs::strip
uint32_t resume_launch_waves(int num_cus, uint32_t n);  // workgroups of a launch over n decoders

hipError_t launch_inflate(const InflateArgs &a, int ring_bits, int num_cus, hipStream_t stream);
size_t inflate_strip_bytes(int ring_bits, int num_cus, uint32_t n, uint32_t gzip);  // what InflateArgs::strip holds when every stream-wave of that launch owns a slice
size_t inflate_strip_wave_bytes();  // ... one stream-wave's slice
// the profiles of `waves` stream-wave slices of a strips' scratch switched off (no stream consults or counts down its wave's profile
// from then on) or on again (inflate_core.h strip_profile_layout: the words behind the quantiles)
hipError_t launch_profile_switch(uint32_t *strip, uint32_t waves, bool off, hipStream_t stream);
// the gzip instances (pzg_kernels_b.hip): `waves` workgroups of the ring's kernel, or of the fixup pass
hipError_t launch_inflate_gzip(const InflateArgs &a, int ring_bits, bool fixup, uint32_t waves, hipStream_t stream);
// the raw instances: the same
hipError_t launch_inflate_raw(const InflateArgs &a, int ring_bits, bool fixup, uint32_t waves, hipStream_t stream);

// the segment instance (pzg_kernels_b.hip): `waves` workgroups of the 32 KiB ring's kernel
hipError_t launch_inflate_seg(const InflateArgs &a, uint32_t waves, hipStream_t stream);
// the 32 KiB of output in front of every stored point of an index build, min(*count, cap) of them, into the END of slot k of `windows`
// (cap x 32768 bytes; a point below 32768 has that much less, the front of its slot is left as it is).  Nothing is copied unless
// *status is 0 and the point lies inside out_cap.
hipError_t launch_index_windows(const uint8_t *out, const uint64_t *out_cap, const uint64_t *points, const uint32_t *count, uint32_t cap,
                                const int32_t *status, uint8_t *windows, hipStream_t stream);

// the parallel index scan (pzg_kernels_b.hip, scan_core.h).  The caller fills in what is above the line; launch_scan() lays the rest
// out in `scratch` (scan_scratch_bytes(nchunks) bytes of device memory, 256-byte aligned) and enqueues the three kernels.
struct ScanResult;
struct ScanArgs {
    const uint8_t *in;
    uint64_t in_len, chunk, span;
    uint32_t nchunks, max_points;
    uint64_t *points;    // max_points {in_bit, out_pos} pairs
    uint8_t *windows;    // max_points x 32768 bytes, or null
    ScanResult *result;  // 32 bytes: status, d0, d1, npoints, out_len, in_used
    // ----
    uint64_t *cand, *count, *endbit;
    uint32_t *next;
    uint16_t *rings;
    uint8_t *wbuf;
};
size_t scan_scratch_bytes(uint32_t nchunks);
hipError_t launch_scan(ScanArgs a, uint8_t *scratch, hipStream_t stream);

// ... of many streams in one launch (pzg_index_scan_many): a wave per chunk of ALL streams, a workgroup per stream for the walk.
// scan_many_layout() lays out what is below the line in `scratch` (scan_many_scratch_bytes(n, nchunks) bytes, 256-byte aligned).
// The caller then copies the n stream entries and, behind them, the n + 1 entries of first_chunk to a.streams in one piece
// (scan_many_table_bytes(n) bytes) on the stream it launches on; launch_scan_many() enqueues the three kernels; the results are at
// a.results.
struct ScanStream;
struct ScanManyArgs {
    const uint8_t *in_base;
    uint64_t chunk, span;
    uint32_t n, nchunks;  // streams; chunks of all of them
    uint64_t *points;     // {in_bit, out_pos} pairs: stream s at its point_off
    uint8_t *windows;     // 32768 bytes per point slot, or null
    // ----
    ScanStream *streams;
    uint32_t *first_chunk;
    ScanResult *results;
    uint64_t *cand, *count, *endbit;
    uint32_t *next;
    uint16_t *rings;
    uint8_t *wbuf;
};
size_t scan_many_scratch_bytes(uint32_t n, uint32_t nchunks);
size_t scan_many_table_bytes(uint32_t n);
void scan_many_layout(ScanManyArgs &a, uint8_t *scratch);
hipError_t launch_scan_many(const ScanManyArgs &a, hipStream_t stream);

// the members of a gzip file (pzg_kernels_b.hip, member_core.h).  The caller fills in what is above the line; `scratch`:
// members_find_scratch_bytes(nchunks) bytes of device memory, 8-byte aligned; the count of candidates lands at members_find_total().
struct MemberArgs {
    const uint8_t *in;
    uint64_t in_len, chunk, nchunks;
    uint64_t *starts;      // max_members
    uint32_t *bsize;       // max_members
    uint64_t max_members;
    // ----
    uint64_t *counts, *total;
};
size_t members_find_scratch_bytes(uint64_t nchunks);
hipError_t launch_members_find(MemberArgs a, uint8_t *scratch, hipStream_t stream);
const uint64_t *members_find_total(uint64_t nchunks, const uint8_t *scratch);
// ... and their layout: m entries each; scratch: members_layout_scratch_bytes(m) bytes, the sum of the rooms at members_layout_total()
struct LayoutArgs {
    const uint8_t *in;
    uint64_t in_len, m, out_base_off;
    const uint64_t *starts;
    uint64_t *in_off, *in_lenv, *out_off, *out_cap;
};
size_t members_layout_scratch_bytes(uint64_t m);
hipError_t launch_members_layout(const LayoutArgs &a, uint8_t *scratch, hipStream_t stream);
const uint64_t *members_layout_total(uint64_t m, const uint8_t *scratch);

// scanline unfiltering (pzg_unfilter_kernel.h, unfilter_core.h; compiled with pzg_api.cpp): a wave per image.  Every pointer is device memory.
struct UnfilterArgs {
    const uint8_t *src_base;
    const uint64_t *src_off, *src_len;  // n
    uint8_t *dst_base;
    const uint64_t *dst_off, *dst_stride;  // n
    const uint32_t *row_bytes, *height;    // n
    const uint8_t *bpp;                    // n
    int32_t *status;                       // n
    uint32_t *detail;                      // 2n or null
    uint32_t n;
};

// Adam7 deinterlacing (pzg_adam7_kernel.h, adam7_core.h; compiled with pzg_api.cpp): the rows of an image over the grid's y.  Every
// pointer is device memory.
struct Adam7Args {
    const uint8_t *src_base;
    const uint64_t *src_off;  // n
    uint8_t *dst_base;
    const uint64_t *dst_off, *dst_stride;  // n
    const uint32_t *width, *height;        // n
    const uint8_t *pixel_bits;             // n
    int32_t *status;                       // n
    uint32_t *detail;                      // 2n or null
    uint32_t n;
};

// pixel expansion (pzg_expand_kernel.h, expand_core.h; compiled with pzg_api.cpp): the rows of an image over the grid's y.  Every pointer
// is device memory.  desc: n descriptors of 64 bytes, pzg_expand_desc as the core sees it (Expand::Desc); scratch: two zeroed 64-bit
// words per image (expand_scratch_bytes), where the waves of a palette image meet.
struct ExpandArgs {
    const uint8_t *src_base;
    uint8_t *dst_base;
    const uint32_t *palette_base;  // may be null where no image has a palette
    const void *desc;              // n
    uint64_t *scratch;             // 2n, zero
    int32_t *status;               // n
    uint32_t *detail;              // 2n or null
    uint32_t n;
};
inline size_t expand_scratch_bytes(uint32_t n) { return 16 * (size_t)n; }

// TIFF Predictor 2 and window clipping (pzg_unpredict_kernel.h, unpredict_core.h; compiled with pzg_api.cpp): the rows of a job over the
// grid's y.  Every pointer is device memory.  desc: n descriptors of 64 bytes, pzg_unpredict_desc as the core sees it (Unpredict::Desc).
struct UnpredictArgs {
    const uint8_t *src_base;
    const uint64_t *src_len;  // n
    uint8_t *dst_base;
    const void *desc;         // n
    int32_t *status;          // n
    uint32_t *detail;         // 2n or null
    uint32_t n;
};

// The byte-plane transpose and TIFF Predictor 3 (pzg_unshuffle_kernel.h, unshuffle_core.h; compiled with pzg_api.cpp): the rows of a job
// over the grid's y.  Every pointer is device memory.  desc: n descriptors of 64 bytes, pzg_unshuffle_desc as the core sees it
// (Unshuffle::Desc).
struct UnshuffleArgs {
    const uint8_t *src_base;
    const uint64_t *src_len;  // n
    uint8_t *dst_base;
    const void *desc;         // n
    int32_t *status;          // n
    uint32_t *detail;         // 2n or null
    uint32_t n;
};

// LZW (pzg_unlzw_kernel.h, unlzw_core.h; compiled with pzg_api.cpp): one wave a stream, the arrays those of InflateArgs.  Every
// pointer is device memory.
struct UnlzwArgs {
    const uint8_t *in_base;
    const uint64_t *in_off, *in_len;    // n
    uint8_t *out_base;
    const uint64_t *out_off, *out_cap;  // n
    uint64_t *out_len;                  // n
    int32_t *status;                    // n
    uint32_t *detail;                   // 2n or null
    uint32_t n, early_change;
};

// partials: 3 * 4 * ceil(max_waves / 4) uint32 of device scratch
hipError_t launch_adler32(const uint8_t *buf, uint64_t len, uint32_t init, uint32_t *partials, uint32_t max_waves,
                          uint32_t *out, hipStream_t stream);

// Adler-32 of n buffers base + off[i] .. + len[i] (device memory), one wave per buffer
hipError_t launch_adler32_many(const uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t *out, uint32_t n, int num_cus,
                               hipStream_t stream);

// order[0..n): stream indices, longest (by out_cap) first; scratch: 128 uint32 of device memory
hipError_t launch_order(const uint64_t *out_cap, uint32_t n, uint32_t *order, uint32_t *scratch, hipStream_t stream);

}  // namespace pzg
