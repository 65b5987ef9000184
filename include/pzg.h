/*
 * pzg.h -- C ABI of the MI355X-native batched zlib/DEFLATE decompressor.
 *
 * This is the drop-in boundary for the one hot path of GaloisInc/pure-zlib:
 *
 *     Codec.Compression.Zlib.decompress :: L.ByteString -> Either DecompressionError L.ByteString
 *         (reference: src/Codec/Compression/Zlib.hs:32-51)
 *
 * The reference is pure Haskell with no FFI of its own; these entry points are
 * what a `foreign import ccall safe` in a replacement Codec.Compression.Zlib
 * module binds (the binding a maintainer would add is shown in INTEGRATION.md).
 * Plain pointers and sizes only; no C++/torch/HIP types cross the boundary.
 *
 * There is NO CPU backend: every entry point that computes runs hand-written
 * HIP kernels on a gfx950 device and fails loudly (negative return code) when no
 * device is usable.
 *
 * Threading: a pzg_ctx may be shared by threads.  Host-pointer calls take one of the context's
 * independent pipelines (HIP streams + staging) each and overlap; device-pointer launches are
 * enqueued on the context's stream in call order, each with its own work counter.
 * Ownership: the caller allocates and owns every buffer; the library retains no
 * caller pointer past return (except with PZG_ASYNC, until pzg_sync()).
 * No exception crosses the boundary.
 *
 * Lifetimes: the reference's ZlibDecoder is a garbage-collected closure (Monad.hs:163-167,185-197): it can be dropped
 * at any time, in any order, and cannot dangle.  The same holds here.  A pzg_ctx is reference counted: the handle
 * pzg_init returns is one reference, every live pzg_decoder holds another.  pzg_shutdown() waits for the work
 * enqueued through the handle, drops the caller's reference and invalidates the handle (every later call on it fails
 * with PZG_RC_BAD_ARG instead of touching freed memory, for as long as a decoder keeps the context alive; after that
 * the handle is dangling like any freed pointer).  Decoders created from it stay fully usable after pzg_shutdown --
 * pzg_decoder_feed / _reset / _destroy in any order -- and the device resources go with the last
 * pzg_decoder_destroy().  pzg_shutdown() then pzg_decoder_destroy(), or the reverse, are both correct; finalisers
 * (GHC ForeignPtr, Python __del__, C++ shared_ptr) may therefore run in whatever order the collector picks.
 */
#ifndef PZG_H
#define PZG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define PZG_API __attribute__((visibility("default")))
#else
#define PZG_API
#endif

#define PZG_VERSION_MAJOR 0
#define PZG_VERSION_MINOR 5

/* ---- call-level return codes (the int every function returns) ---------------- */
#define PZG_RC_OK            0
#define PZG_RC_BAD_ARG      (-1)
#define PZG_RC_NO_DEVICE    (-2)  /* no gfx950 device / HIP runtime unusable: there is no CPU fallback */
#define PZG_RC_HIP_ERROR    (-3)  /* a HIP call failed; pzg_last_error() has the text */
#define PZG_RC_NO_MEMORY    (-4)

/* ---- per-stream status codes --------------------------------------------------
 * One per reference outcome.  `show` strings are those of
 * src/Codec/Compression/Zlib/Monad.hs:95-102 plus the raise site quoted. */
#define PZG_OK                    0  /* Right bytes                                              Zlib.hs:46-47  */
#define PZG_E_TRUNCATED           1  /* DecompressionError "Ran out of data mid-decompression 2." Zlib.hs:38-39  */
#define PZG_E_HDR_FCHECK          2  /* HeaderError "Header checksum failed"                      Zlib.hs:62-63  */
#define PZG_E_HDR_METHOD          3  /* HeaderError "Bad compression method: <d0>"                Zlib.hs:64-65  */
#define PZG_E_HDR_WINDOW          4  /* HeaderError "Window size too big: <d0>"                   Zlib.hs:66-67  */
#define PZG_E_FMT_LEN_NLEN        5  /* FormatError "Len/nlen mismatch in uncompressed block."    Deflate.hs:75-76 */
#define PZG_E_FMT_BTYPE           6  /* FormatError "Unacceptable BTYPE: 3"                       Deflate.hs:102-104 */
#define PZG_E_HUFF_BUILD          7  /* HuffmanTreeError <insert message>; d0 = tree id, d1 = bit offset of the block header
                                        modulo 2^32 (pzg_error_message re-derives the exact text from it: exact for streams
                                        with less than 512 MiB of compressed data in front of the block)  HuffmanTree.hs:55-63 */
#define PZG_E_HUFF_EMPTY_TREE     8  /* HuffmanTreeError "Tried to advance empty tree!"           HuffmanTree.hs:76 */
#define PZG_E_HUFF_EMPTY_BRANCH   9  /* HuffmanTreeError "Advanced to empty tree!"                HuffmanTree.hs:80 */
#define PZG_E_CHECKSUM           10  /* ChecksumError "checksum mismatch: <hex d0> != <hex d1>"   Deflate.hs:56-63 */
#define PZG_E_BAD_DISTANCE       11  /* reference THROWS (OutputWindow.hs:87 slice bounds); d0 = distance, d1 = bytes produced */
#define PZG_E_BAD_LITLEN_SYMBOL  12  /* reference THROWS (Deflate.hs:160-166 array index); d0 = symbol 286/287 */
#define PZG_E_BAD_DIST_SYMBOL    13  /* reference THROWS (Deflate.hs:199-205 array index); d0 = symbol >= 30 */
#define PZG_E_OUT_TOO_SMALL      14  /* not a reference outcome: out_len[i] holds the size needed */
#define PZG_E_DATA_REMAINING     15  /* DecompressionError "Finished with data remaining." -- produced by the host
                                        mirror from in_used[] and the caller's chunking (Zlib.hs:48-49), never by the kernel */
/* PZG_GZIP only (extension, no reference counterpart): */
#define PZG_E_GZIP_HEADER        18  /* "Header error: gzip: ..."; d0 = 1 bad magic, 2 method != 8, 3 reserved flag bits, 4 header CRC16 */
#define PZG_E_GZIP_ISIZE         19  /* "Checksum error: gzip: length mismatch: <d0> != <d1>" (ISIZE vs bytes produced mod 2^32);
                                      * a CRC-32 mismatch is PZG_E_CHECKSUM.  Not checked for PZG_E_OUT_TOO_SMALL streams. */

/* pzg_decompress_many_dict only (extension): */
#define PZG_E_DICT               20  /* "Header error: preset dictionary mismatch: <hex d0> != <hex d1>": the stream's DICTID (d0) is
                                      * not the Adler-32 of the dictionary supplied for it (d1) */
#define PZG_E_SEGMENT 21  /* segments only: the blocks do not end at end_bit. d0 = 1 final block came first, 2 a block ran past; d1 = bit reached */
#define PZG_E_FILTER 23  /* (0.5) pzg_unfilter_many only: row d0 has filter byte d1 (> 4).  d0 = 0xffffffff: the image's bpp (d1) or its
                            stride is not legal -- device arrays only, the host-pointer form refuses the call.  pzg_adam7_many: only
                            the latter, d1 = the image's pixel_bits; pzg_expand_many: only the latter, d1 = color_type << 8 | bit_depth */
#define PZG_E_PALETTE 24  /* (0.5) pzg_expand_many only: a pixel of a palette image has an index >= pal_len; d0 = its row, d1 = its x: the
                             first such pixel in row-major order */
#define PZG_E_LZW 25  /* (0.5) pzg_unlzw_many only: a code that is neither a literal, an entry made so far, nor the next free entry behind
                         a previous code; d0 = the code, d1 = the bytes produced so far */
#define PZG_E_SCAN 22  /* pzg_index_scan only: the chain of blocks did not reach the final block.
                          d0 = the status the chain's last segment met (0: a dead wave),
                          d1 = low 32 bits of that segment's start bit.
                          Decode sequentially for the stream's own error. */
/* Reference raise sites that have NO status because they cannot fire (here or in the reference):
 *   Deflate.hs:150-151  DecompressionError "Unexpected code: <n>" -- getCodeLengths' fall-through for a code-length symbol outside
 *                       0..18; the code-length alphabet has exactly 19 symbols (Deflate.hs:87-88 builds its tree from 19 lengths),
 *                       so nextCode can only return 0..18.
 *   HuffmanTree.hs:77   HuffmanTreeError "Tried to advance value!" -- advanceTree on a leaf; nextCode (Monad.hs:295-302) restarts
 *                       from the root as soon as advanceTree returns a value, so a leaf is never advanced.
 *   Monad.hs:277        FormatError "Can't get a block on a non-byte boundary." -- nextBlock with bits pending; its only caller
 *                       (Deflate.hs:70-72) runs advanceToByte first.
 * The oracle keeps the first two as dead code for fidelity; no input reaches them. */
/* pzg_decoder_feed only: a decoder that is not finished */
#define PZG_DEC_NEED_INPUT      101  /* NeedMore (Monad.hs:164): every complete element of the input has been decoded */
#define PZG_DEC_OUT_FULL        102  /* this call's output room is used up: call again with the rest of the input */

/* tree ids in detail[2*i] of PZG_E_HUFF_BUILD */
#define PZG_TREE_CODELEN 0
#define PZG_TREE_LITLEN  1
#define PZG_TREE_DIST    2

/* ---- flags ------------------------------------------------------------------- */
#define PZG_DEVICE_PTRS  1u  /* every pointer argument is device memory on the context's device */
#define PZG_ASYNC        2u  /* enqueue only (requires PZG_DEVICE_PTRS); caller calls pzg_sync().  Launches enqueued on different
                              * streams (pzg_set_stream in between) may run at the same time, two at most: a third waits, on its own
                              * stream, for the first's token scratch (see pzg_init) */
#define PZG_GZIP         4u  /* EXTENSION (the reference has no gzip: README.md:42-50 TODO): every stream is
                              * one RFC 1952 member (gzip header, deflate, CRC-32 + ISIZE); adler[] then holds the CRC-32 */
#define PZG_LPT_ORDER    8u  /* device-pointer batches of mixed sizes: launch the longest streams (largest out_cap[]) first; the
                              * permutation is built on the device.  Host-pointer batches are always launched that way. */
#define PZG_HOST_PINNED 16u  /* host-pointer batches whose in_base / out_base arenas are PAGE-LOCKED (pzg_host_alloc, or hipHostMalloc /
                              * hipHostRegister by the caller): the copy engines read and write them directly -- no packing into
                              * staging, no copy-out; this is the path the module mirrors (`decompress` / `decompressMany`) take.
                              * Requirements: extents in ascending order on both sides (in_off[i] + in_len[i] <= in_off[i+1], the same for
                              * out_off / out_cap; PZG_RC_BAD_ARG otherwise); the whole span of the output arena from the first extent
                              * to the end of the last is written (bytes in gaps BETWEEN extents, and the bytes of an extent past its
                              * stream's out_len[i] -- a stream that failed or came out short -- are unspecified afterwards: they may
                              * hold what an earlier batch of this context decoded; bytes outside the span are untouched.  The staged
                              * path, without this flag, writes out_len[i] bytes per extent and nothing else); gaps of the input arena travel over the link, so pack tightly
                              * (16-byte aligned extents keep the wide store path).  Pageable memory under this flag is still
                              * correct, only slower.  Not combined with preset dictionaries. */
#define PZG_RAW         32u  /* (0.5) EXTENSION: every stream is a bare RFC 1951 stream -- what a deflated member of a .zip / .jar / .whl
                              * holds, system zlib's wbits = -15: no header, no trailer, no checksum check.  Everything else means what
                              * it means for zlib streams:
                              *   in_used[i]  the input bytes up to and including the byte that holds the last bit of the final block;
                              *               what follows is left alone
                              *   adler[i]    the Adler-32 of the decoded bytes, reported and not checked (failed and over-capacity
                              *               streams: the rules of pzg_decompress_many below)
                              *   status[i]   PZG_E_HDR_*, PZG_E_CHECKSUM and PZG_E_DICT cannot occur; input that runs out before the
                              *               final block ends (in_len[i] = 0 too) is PZG_E_TRUNCATED; the bit offset in detail[1] of
                              *               PZG_E_HUFF_BUILD counts from the first bit of the raw stream, so that pzg_error_message
                              *               over the raw bytes gives the text
                              * With pzg_decompress_many_dict a stream with dict_len[i] > 0 decodes with that dictionary as the history
                              * in front of its output, unconditionally -- there is no FDICT bit and no DICTID (zlib's raw
                              * inflateSetDictionary); dict_len[i] = 0: plain raw.  Not combined with PZG_GZIP (PZG_RC_BAD_ARG).
                              * Raw launches do not use the bundles (PZG_OPT_BUNDLES).  Resumable raw decoders: pzg_decoder_create_format. */
#define PZG_CRC32       64u  /* (0.5) only together with PZG_RAW (PZG_RC_BAD_ARG otherwise): adler[i] holds the CRC-32 (RFC 1952 section 8)
                              * of the bytes delivered instead of their Adler-32 -- computed on the device in one more pass over the
                              * output, 0 when out_len[i] > out_cap[i].  Nothing is verified: the caller owns the expected value (a ZIP
                              * central directory, say). */

typedef struct pzg_ctx pzg_ctx;

/* Create a context on HIP device `device` (0-based).  One HIP stream + grow-only device
 * arenas for the host-pointer path.  Returns PZG_RC_NO_DEVICE when HIP has no usable device.
 * Device memory the library takes for itself, grow-only until pzg_shutdown: the kernels' scratch -- 64.8 KiB per stream-wave
 * of a launch (one wave per stream, at most the residency of the chip: 6,656 waves = 421 MiB on an MI355X), two such arenas per
 * device for PZG_DEVICE_PTRS launches and one per host-path pipeline in use (four at the most: 2.5 GiB per device in the worst
 * case; PZG_OPT_SCRATCH_BYTES bounds it) -- beside the host path's staging arenas.  A launch whose scratch cannot be allocated,
 * or only in part, still decodes: the stream-waves without a slice take the slower path that needs none. */
PZG_API int  pzg_init(int device, pzg_ctx **out);
/* decompressMany over SEVERAL devices of one node (API of Zlib.hs:32-35, batched): bit d of `device_mask`
 * selects HIP device d, 0 selects every visible device.  One call of pzg_decompress_many() with HOST pointers then
 * partitions the streams over the devices (longest-processing-time-first by capacity), one host thread, HIP stream set
 * and staging arenas per device, and every result lands in the caller's own out_off[] / status[] slots: the streams
 * are independent, so nothing crosses between devices (no collective).  PZG_DEVICE_PTRS calls of pzg_decompress_many need a
 * one-device context; data that already lives on several devices goes through pzg_decompress_many_sharded(). */
PZG_API int  pzg_init_mask(uint32_t device_mask, pzg_ctx **out);
/* The same with the devices named one by one: one shard per entry, in that order (shard k of
 * pzg_decompress_many_sharded = devices[k]).  A device may be named more than once -- several shards then share it, each
 * with its own streams, arenas and host thread (a way to keep more batches in flight on one device, and how the
 * multi-shard code is exercised on a one-GPU box). */
PZG_API int  pzg_init_devices(const int32_t *devices, uint32_t ndevices, pzg_ctx **out);
PZG_API int  pzg_device_count(pzg_ctx *ctx);  /* devices (shards) of the context */
/* Drop the caller's reference (see "Lifetimes" above): synchronises, invalidates the handle, frees everything unless
 * decoders are still alive -- then the last pzg_decoder_destroy() frees it.  NULL is ignored. */
PZG_API void pzg_shutdown(pzg_ctx *ctx);

/* Make the context launch on an existing HIP stream (e.g. a framework's current stream) instead of
 * its own.  `hip_stream` is a hipStream_t passed as void*; NULL means HIP's default (null) stream.
 * pzg_reset_stream() goes back to the context's own non-blocking stream. */
PZG_API int  pzg_set_stream(pzg_ctx *ctx, void *hip_stream);
PZG_API int  pzg_reset_stream(pzg_ctx *ctx);
PZG_API int  pzg_sync(pzg_ctx *ctx);

/* Tuning options.
 * PZG_OPT_RING_BITS: log2 of the LDS ring each stream-wave keeps of its most recent output.
 *   15  the whole 32 KiB DEFLATE window lives in LDS (OutputWindow.hs as a pure LDS ring): 4 stream-waves per CU
 *   11-14  a smaller near ring; back-references older than it are read from the stream's own, already
 *       flushed output in HBM/L2.  More stream-waves per CU; the kernel is latency-bound and scales with them.
 *   Results are bit-identical for every value.  Default: PZG_DEFAULT_RING_BITS. */
#define PZG_OPT_RING_BITS 1
#define PZG_DEFAULT_RING_BITS 11
/* PZG_OPT_HOST_THREADS: helper threads (1..256) that pack / copy out the STAGED host-pointer path and the decoders' feeds
 *   (default: the machine's hardware threads, at most 24).  Set it while no host-pointer call is running. */
#define PZG_OPT_HOST_THREADS 2
/* PZG_OPT_SCRATCH_BYTES: upper bound, per SHARD of the context, on the scratch memory the LIBRARY allocates for its inflate kernels
 *   (0, the default: no bound).  A shard is one entry of the device list the context was made with: pzg_init / pzg_init_mask name
 *   every device once, so that there the bound is per device; a pzg_init_devices list that names one physical device k times
 *   makes k shards of it, each with its own arenas -- the ceiling on that device is k x the bound -- and every pzg_decoder object
 *   adds one arena of one share (bound / 6) on top: with d decoders alive the ceiling is (k + d / 6) x the bound.  A launch's stream-waves decode long runs of input through a scratch of 64.8 KiB each -- 421 MiB for a
 *   launch that fills an MI355X (6,656 stream-waves) -- and a context keeps up to six such arenas per device, grow-only: two for
 *   device-pointer launches (overlapping launches must not share one) and one per host-path pipeline (four), 2.5 GiB at the
 *   most; a pzg_decoder object keeps one more for its feeds (at most 4,096 stream-waves: 259 MiB).  With a bound every arena gets an even share (bound / 6): only as many stream-waves as fit own a slice, the others
 *   decode by the slower path that needs no scratch; below 64.8 KiB per arena all of them do.  Results never depend on it.
 *   Takes effect launch by launch (an arena larger than its share is released when it is next used). */
#define PZG_OPT_SCRATCH_BYTES 3
/* PZG_OPT_BUNDLES (0.5): 1 (default) -- a PZG_DEVICE_PTRS launch of 32,768 or more zlib streams first takes its streams of the
 *   FIXED code (what `compressobj(1, ..., Z_FIXED)` and level-1 encoders make of short records) 64 to a wavefront, one lane per
 *   stream; every other stream, and every stream that is not plain (another block type, any error, a stream or capacity of a MiB or
 *   more), is decoded by the ordinary one-stream-per-wavefront kernel as before; a launch in which no stream turned out to be one for
 *   the bundles lets the next 2, 6, 14 ... 64 launches of the context go without looking (the look costs such a launch ~1 %).
 *   2 -- launches of any size, always looking.  0 -- off.  Results never depend on it; it needs no scratch memory.
 *   Setting the option (to the value it already has, too) ends the launches a context is going without looking. */
#define PZG_OPT_BUNDLES 4
/* PZG_OPT_PROFILE (0.5): 1 (default) -- a stream-wave of a PZG_DEVICE_PTRS launch remembers where the tokens of the last stream it
 *   decoded lay and cuts the next stream's input into pieces of equal WORK there (checked against the stream itself before it is
 *   trusted); 0 -- pieces of equal length, always.  Results never depend on it: it is there to be measured (bench.py's
 *   hetero_variant reports both).  Takes effect launch by launch. */
#define PZG_OPT_PROFILE 5
PZG_API int  pzg_set_option(pzg_ctx *ctx, int option, int64_t value);
/* The only environment variable the library reads is PZG_RING_BITS (11..15): the default of PZG_OPT_RING_BITS for
 * contexts created afterwards. */

/* Page-locked host memory for PZG_HOST_PINNED arenas (hipHostMalloc, portable across the node's devices).  NULL when the
 * system will not lock that much.  Free with pzg_host_free (NULL is ignored).  No context is needed. */
PZG_API void *pzg_host_alloc(size_t bytes);
PZG_API void  pzg_host_free(void *p);

/*
 * decompressMany: decode n independent zlib (RFC 1950) streams, one wavefront per stream.
 * Replaces n calls of Codec.Compression.Zlib.decompress (Zlib.hs:32-51) on single-chunk inputs.
 *
 *   in_base, in_off[n], in_len[n]    stream i is in_base[in_off[i] .. in_off[i]+in_len[i])
 *   out_base, out_off[n], out_cap[n] stream i may write out_base[out_off[i] .. out_off[i]+out_cap[i])
 *   out_len[n]             bytes the stream decodes to (may exceed the capacity: PZG_E_OUT_TOO_SMALL)
 *   status[n]              PZG_OK or PZG_E_*
 *   detail[2n]             two detail words per stream (see the status table); may be NULL
 *   in_used[n]             input bytes consumed incl. the Adler trailer; may be NULL
 *   adler[n]               Adler-32 computed over the decoded bytes; may be NULL.  With PZG_GZIP: the CRC-32 of them.
 *                          0 for PZG_E_OUT_TOO_SMALL: nothing of such a stream is delivered.
 * (PZG_RAW: bare RFC 1951 streams instead, see the flag; with PZG_CRC32 adler[] holds their CRC-32.)
 *
 * A stream that FAILED (status neither PZG_OK nor PZG_E_OUT_TOO_SMALL) delivers what the reference had emitted before the error:
 *   out_len[i]   those bytes -- nothing of a stored block whose bytes run out (Deflate.hs:77: nextBlock reads the block whole
 *                before emitBlock emits it)
 *   extent       bytes [0, min(out_len[i], out_cap[i])) are those bytes, on every path (device pointers, staged, PZG_HOST_PINNED,
 *                sharded); nothing is written past out_cap[i]
 *   adler[i]     the Adler-32 of those bytes, 0 if out_len[i] > out_cap[i] (what lies past the capacity is not stored).  With
 *                PZG_GZIP: their CRC-32, or 0 if out_len[i] > out_cap[i]; a member whose CRC-32 or ISIZE is wrong but whose
 *                output outgrew the capacity reports PZG_E_OUT_TOO_SMALL (nothing stored to check)
 *   in_used[i]   unspecified
 *
 * Extents may be laid out with gaps (aligned arenas) and in any order; they must not overlap on the
 * output side.  One compressed stream may be up to 16 GiB (longer ones report PZG_E_TRUNCATED); the decoded size is
 * not limited.  A 16-byte aligned out_base+out_off[i] takes the wide (16 B/lane) store path.
 *
 * Without PZG_DEVICE_PTRS all pointers are host memory and the call stages through the
 * context's device arenas (H2D, kernel, D2H) and returns when results are in host memory.
 * Return value: PZG_RC_* for the call as a whole; per-stream results are in status[].
 */
PZG_API int pzg_decompress_many(pzg_ctx *ctx,
                        const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len,
                        uint8_t *out_base, const uint64_t *out_off, const uint64_t *out_cap,
                        uint64_t *out_len, int32_t *status, uint32_t *detail,
                        uint64_t *in_used, uint32_t *adler,
                        uint32_t n, uint32_t flags);

/*
 * decompressMany over several devices with the data ALREADY on them: a context from
 * pzg_init_mask() has one shard per device; batch b names its shard (0 .. pzg_device_count()-1) and carries pointers that
 * are all device memory of THAT shard's device, with the meaning they have in pzg_decompress_many().  Every batch is
 * enqueued on its own device's stream -- nothing crosses PCIe or xGMI, no collective: the streams are independent -- and
 * the call returns when all of them have finished (with PZG_ASYNC: at once; pzg_sync() waits for every device).
 * Several batches may name the same shard (they run one after the other on its stream).  flags: PZG_ASYNC, PZG_GZIP,
 * PZG_LPT_ORDER, PZG_RAW, PZG_CRC32 (PZG_DEVICE_PTRS is implied).
 */
typedef struct pzg_device_batch {
    uint32_t shard;  /* which device of the context the pointers below live on */
    uint32_t n;      /* streams in this batch */
    const uint8_t *in_base; const uint64_t *in_off, *in_len;
    uint8_t *out_base;      const uint64_t *out_off, *out_cap;
    uint64_t *out_len; int32_t *status;
    uint32_t *detail;   /* 2n or NULL */
    uint64_t *in_used;  /* n or NULL */
    uint32_t *adler;    /* n or NULL */
} pzg_device_batch;
PZG_API int pzg_decompress_many_sharded(pzg_ctx *ctx, const pzg_device_batch *batches, uint32_t nbatches, uint32_t flags);

/*
 * EXTENSION -- preset dictionaries (RFC 1950 FDICT).  The reference skips DICTID and decodes with an empty history
 * (Zlib.hs:68, a FIXME there); pzg_decompress_many does exactly that.  This entry point is the same call plus one
 * dictionary extent per stream (dict_len[i] = 0: none): a stream whose header has FDICT set and that has a
 * dictionary checks DICTID against the dictionary's Adler-32 (PZG_E_DICT) and decodes with the dictionary as the
 * history in front of its output; every other stream behaves as in pzg_decompress_many.  dict_* may be NULL.
 * With PZG_RAW (0.5) the dictionary of a stream that has one is its history unconditionally: see the flag.
 */
PZG_API int pzg_decompress_many_dict(pzg_ctx *ctx,
                             const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len,
                             const uint8_t *dict_base, const uint64_t *dict_off, const uint64_t *dict_len,
                             uint8_t *out_base, const uint64_t *out_off, const uint64_t *out_cap,
                             uint64_t *out_len, int32_t *status, uint32_t *detail,
                             uint64_t *in_used, uint32_t *adler,
                             uint32_t n, uint32_t flags);

/*
 * EXTENSION -- one LARGE stream, indexed (the zran / indexed_gzip scheme).  A stream is decoded by one wavefront; an index of
 * access points cuts it into segments that are independent pieces of work, so that the whole stream decodes with a wavefront per
 * segment and any byte range is read without decoding what is in front of it.  An access point is a block boundary: the block
 * that starts at bit in_bit of the raw stream (counted from bit 0 of its first byte) produces output byte out_pos first; with the
 * 32768 bytes of output in front of out_pos (its window) it is all a decoder needs to start there.
 *
 * pzg_index_build: one sequential decode of ONE raw (RFC 1951) stream -- out, out_len, status, detail, in_used and adler are exactly
 * what pzg_decompress_many gives with PZG_RAW, which is implied -- that also records the points.  The rule: the end of a non-final
 * block is a point when out_pos is `span` bytes or more past the last point's out_pos (past 0 for the first point); span 0 means
 * 1 MiB.  *npoints is the number of points the stream HAS at this span: if it exceeds max_points only the first max_points were
 * stored (their windows too) and the caller repeats with more room or a larger span.  The points (and windows) are valid only
 * when *status == PZG_OK.  windows (max_points x 32768 bytes, or NULL): slot k receives the window of point k at its END -- the
 * last min(out_pos, 32768) bytes of the slot; what lies in front of them in the slot is left as it was.
 * flags: 0 -- in, out, points and windows are host memory; PZG_DEVICE_PTRS -- they are device memory.  npoints, out_len, status,
 * detail, in_used and adler are host memory in both forms, and the call returns when they are filled in: it runs on a stream of
 * the library's own, NOT the one given to pzg_set_stream, and is ordered against the caller's other work only by returning -- work
 * the caller has enqueued on a stream of its own that writes `in` must have finished before the call.  PZG_GZIP, PZG_HOST_PINNED,
 * any other flag, and a context of several devices are PZG_RC_BAD_ARG.
 *
 * pzg_decompress_many_segments: pzg_decompress_many_dict over PZG_RAW (implied) pieces that begin and end inside a stream.  Segment i
 * is the bytes in_off[i] .. + in_len[i]; its first block's header starts at bit start_bit[i] (0..7) of the first of them, and it ends
 * with the block that ends at bit end_bit[i], counted from bit 0 of that same byte -- whatever that block's BFINAL says -- or, with
 * end_bit[i] = 0, with the final block, as a raw stream does.  Bit offsets reported for the segment (end_bit, detail[1] of
 * PZG_E_HUFF_BUILD) count the same way.  No trailer is read; in_used[i] is the byte that holds bit end_bit[i] - 1, plus one.
 * dict_* (required) is the window of each segment (dict_len[i] = 0: none, for the segment at the start of the stream).
 *   status[i]   PZG_E_SEGMENT: a block ended past end_bit[i] (d0 = 2), or the final block ended before it (d0 = 1); d1 = the bit reached.
 *               A segment cannot tell a wrong window from the right one: the caller checks the checksums.
 *   failed and over-capacity segments follow the rules of pzg_decompress_many: out_len, the bytes delivered, the checksum, nothing
 *   written past out_cap[i].  adler[i] covers the segment's own bytes, starting from 1 (PZG_CRC32: their CRC-32) -- combine them
 *   with adler32_combine / crc32_combine.
 * Segments always decode on the 32 KiB ring (a window is history on that ring only), whatever PZG_OPT_RING_BITS says.
 * flags: PZG_DEVICE_PTRS, PZG_ASYNC, PZG_LPT_ORDER, PZG_CRC32.  PZG_GZIP, PZG_HOST_PINNED and a context of several devices are
 * PZG_RC_BAD_ARG; so, with host pointers, are start_bit[i] > 7 and end_bit[i] > 8 * in_len[i] (device arrays are not read by the host:
 * such a segment simply starts where it is told and fails where its input ends).
 */
typedef struct pzg_index_point { uint64_t in_bit, out_pos; } pzg_index_point;

PZG_API int pzg_index_build(pzg_ctx *ctx, const uint8_t *in, uint64_t in_len,
        uint8_t *out, uint64_t out_cap, uint64_t span,          /* span 0: 1 MiB */
        pzg_index_point *points, uint32_t max_points, uint32_t *npoints,
        uint8_t *windows,                                       /* max_points x 32768 bytes, or NULL */
        uint64_t *out_len, int32_t *status, uint32_t detail[2], uint64_t *in_used, uint32_t *adler,
        uint32_t flags);                                        /* PZG_DEVICE_PTRS or 0; PZG_RAW implied */

/*
 * pzg_index_scan: the access points of ONE raw (RFC 1951) stream found IN PARALLEL, without the sequential decode of pzg_index_build
 * (the block finder plus marker window scheme of pugz and rapidgzip).  The input is cut into chunks of `chunk` compressed bytes;
 *   1. a wavefront per chunk k >= 1 finds the smallest bit position of its chunk at which a CANDIDATE block header starts (chunk 0
 *      starts at bit 0, a block start by definition).  A candidate, exactly: BFINAL = 0 and BTYPE = 2; HLIT <= 29 and HDIST <= 29; the
 *      HCLEN + 4 lengths of the code-length code form a complete prefix code (Kraft sum exactly 1); the run-length expansion yields
 *      exactly HLIT + 257 + HDIST + 1 lengths, with no repeat-previous (16) at position 0 and no run crossing the end; symbol 256 has a
 *      nonzero length; the literal/length code is complete; the distance code is complete, or has exactly one code of length 1, or
 *      has no codes at all; the whole header lies inside the input.  Fixed and stored blocks are not looked for: a stream made only
 *      of those has no candidates and is one segment (a limit, not an error);
 *   2. a wavefront per candidate decodes from there with the 32 KiB in front of it as MARKERS instead of bytes, until a block ends
 *      exactly at a later candidate, or the final block ends, or an error (a wave that passes 8 candidates without landing on one is
 *      given up as started at a false candidate);
 *   3. one workgroup walks the chain of segments from bit 0, resolves each segment's last 32 KiB against the window in front of it,
 *      and applies pzg_index_build's rule: a link of the chain is a point when its out_pos is `span` or more past the last point's.
 * points, max_points, npoints (the count the stream HAS at this span and chunk: more than max_points means only the first max_points
 * were stored), windows (the window at the END of its slot), in_used, the host / device pointer forms (npoints, out_len, status,
 * detail and in_used are host memory in both), the one-device context, the rejected flags and the stream of the library's own are
 * those of pzg_index_build.  No output bytes and no checksum are produced: *out_len is the decoded size.  The points are a subset of
 * the stream's block boundaries, in general not the ones pzg_index_build picks; nothing but the segments' decode
 * (pzg_decompress_many_segments) and the checksum over it proves them, so verify before trusting them (the Python mirror's
 * Index.build_parallel does).
 *   *status   PZG_OK, or PZG_E_SCAN: the chain ended in an error or in a dead wave (a broken stream; or, in principle, eight false
 *             candidates in a row).  pzg_index_build or pzg_decompress_many then gives the stream's own error.
 *   chunk     compressed bytes per chunk; 0: 128 KiB; below 256: PZG_RC_BAD_ARG.  span 0: 1 MiB.
 * Device memory: 64 KiB + 32 bytes per chunk (in_len / chunk of them) plus 64.25 KiB, allocated for the call and freed before it
 * returns -- 2,048 chunks of 128 KiB, a 256 MiB input: 128 MiB; PZG_RC_NO_MEMORY when the device does not have it.
 */
PZG_API int pzg_index_scan(pzg_ctx *ctx, const uint8_t *in, uint64_t in_len,
        uint64_t chunk,   /* compressed bytes per chunk; 0: 128 KiB; below 256: PZG_RC_BAD_ARG */
        uint64_t span,    /* 0: 1 MiB */
        pzg_index_point *points, uint32_t max_points, uint32_t *npoints, uint8_t *windows,
        uint64_t *out_len, int32_t *status, uint32_t detail[2], uint64_t *in_used,
        uint32_t flags);  /* 0 or PZG_DEVICE_PTRS */

/*
 * pzg_index_scan_many (0.5): pzg_index_scan over n raw streams in ONE call -- the large members of a gzip file or a ZIP archive, each
 * too few chunks to fill the chip alone.  The chunks of all streams form one list: a wavefront per chunk finds and decodes as above
 * (it finds its stream by a binary search over the streams' first chunks), a workgroup per stream walks that stream's chain.
 * Stream s is in_base + in_off[s] .. + in_len[s]; it owns the point and window slots point_off[s] .. point_off[s + 1] (point_off:
 * n + 1 entries, ascending; windows: point_off[n] x 32768 bytes, or NULL).  For every stream, points, windows (the window at the END
 * of its slot, the front of the slot untouched), npoints[s] (the count the stream HAS), out_len[s], in_used[s], status[s] (PZG_OK or
 * PZG_E_SCAN) and detail[2s], detail[2s + 1] are exactly what pzg_index_scan gives for that stream alone with the same chunk and span
 * and max_points = point_off[s + 1] - point_off[s]: chunks are cut per stream from the stream's own first byte, and a broken stream
 * changes nothing in its neighbours' results or slots.
 * flags: 0 -- in_base, points and windows are host memory; PZG_DEVICE_PTRS -- they are device memory.  in_off, in_len, point_off and
 * every result array are host memory in both forms (the host sizes the grid by the chunk counts), and the call returns when the
 * results are in place: it runs on a stream of the library's own.  PZG_RC_BAD_ARG: n == 0; any other flag (PZG_RAW is implied); a
 * context of several devices; chunk non-zero and below 256; an in_len[s] of 2^34 or more; an in_off[s] above 2^62; descending
 * point_off; more than 2^32 - 1 chunks in total.  Nothing is read but the aligned dwords that hold a stream's bytes.
 * Device memory: 64 KiB + 32 bytes per chunk plus 64 KiB + 256 bytes per stream, allocated for the call and freed before it returns;
 * PZG_RC_NO_MEMORY when the device does not have it.  The host-pointer form also stages the input -- from the first stream's first
 * byte to the last one's last, in one piece -- and the slots in the context's arenas.
 */
PZG_API int pzg_index_scan_many(pzg_ctx *ctx,
        const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
        uint64_t chunk, uint64_t span,                           /* as for pzg_index_scan */
        pzg_index_point *points, const uint32_t *point_off,      /* n + 1, ascending */
        uint32_t *npoints,                                       /* n */
        uint8_t *windows,                                        /* point_off[n] x 32768 bytes, or NULL */
        uint64_t *out_len, int32_t *status, uint32_t *detail,    /* detail: 2n, or NULL */
        uint64_t *in_used,                                       /* n, or NULL */
        uint32_t flags);                                         /* 0 or PZG_DEVICE_PTRS */

PZG_API int pzg_decompress_many_segments(pzg_ctx *ctx,
        const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len,
        const uint8_t *start_bit, const uint64_t *end_bit,
        const uint8_t *dict_base, const uint64_t *dict_off, const uint64_t *dict_len,
        uint8_t *out_base, const uint64_t *out_off, const uint64_t *out_cap,
        uint64_t *out_len, int32_t *status, uint32_t *detail, uint64_t *in_used, uint32_t *adler,
        uint32_t n, uint32_t flags);   /* PZG_DEVICE_PTRS, PZG_ASYNC, PZG_LPT_ORDER, PZG_CRC32; PZG_RAW implied */

/*
 * EXTENSION -- a gzip FILE of many members (RFC 1952 2.2; BGZF, WARC, rotated logs, `cat a.gz b.gz`), a wavefront per member.  A
 * member starts with an empty window, so members need no index: they are found, sized and laid out on the device, and the four
 * arrays of pzg_gzip_layout go straight into pzg_decompress_many(..., PZG_GZIP | PZG_DEVICE_PTRS), one launch for the whole file.
 *
 * pzg_gzip_find_members: the input is cut into chunks of `chunk` bytes, a wavefront per chunk.  Position p is a CANDIDATE exactly
 * when p + 10 <= in_len; the bytes at p, p + 1, p + 2 are 1f 8b 08; FLG & 0xe0 == 0; XFL is 0, 2 or 4; OS <= 13 or OS == 255.  That
 * is stricter than the decoder's own header check on purpose: a member start the finder misses is decoded by its predecessor's
 * wavefront, which walks on into it (slower, still correct); a candidate that is no member start (the bytes occur inside
 * compressed data about once in 2^37 positions, and inside stored blocks whenever the data holds them) is for the caller to find by
 * decoding: the Python mirror's decompress_gzip_file does.  Position 0 is always entry 0, whatever its bytes.
 *   starts[]    the candidates, ascending;  bsize[]  parallel to it: 0, or -- FEXTRA set and a subfield SI1 = 66, SI2 = 67, SLEN = 2
 *               wholly inside XLEN and inside the input -- that subfield's value plus 1, the BGZF total block size
 *   *nmembers   the count the input HAS: if it exceeds max_members only the first max_members are stored and nothing behind them
 *               is touched; the caller repeats with more room
 *   chunk       bytes per chunk; 0: 64 KiB; below 64: PZG_RC_BAD_ARG.  The result does not depend on it, and is the same from run to run.
 * pzg_gzip_layout: for the m accepted starts (ascending), member j is in_off[j] = starts[j], in_len[j] = starts[j + 1] - starts[j]
 * (the last: to the end of the input); out_cap[j] = min(ISIZE, 1032 * in_len[j]) with ISIZE the little-endian dword at the end of
 * that extent (0 for an extent below 18 bytes; 1032 : 1 is DEFLATE's maximum expansion, so a false start's garbage cannot ask for
 * gigabytes); out_off[j] = out_base_off + out_cap[0] + ... + out_cap[j - 1], packed without alignment: the output is the members'
 * concatenation; *total = the sum of all out_cap.  The sums are 64-bit, made on the device in a fixed order.
 * flags: 0 -- in and the arrays are host memory; PZG_DEVICE_PTRS -- they are device memory.  nmembers and total are host memory in
 * both forms and the calls return when they are filled: they run on a stream of the library's own, as pzg_index_scan does.  Any
 * other flag, a context of several devices, m == 0 and in_len of 2^40 or more are PZG_RC_BAD_ARG; so, with host pointers, are
 * descending starts and a start beyond in_len (device arrays are not read by the host: there such a start is taken as the
 * nearest position that is neither, so that every extent lies inside the input).  Neither call reads anything but the aligned
 * dwords that hold input bytes.
 * Device memory, allocated for the call and freed before it returns: find -- 8 bytes per chunk (+ 8 per 4,096 chunks); layout -- 8
 * bytes per 4,096 members.  The host-pointer forms also stage the input and the arrays in the context's arenas (in_len + 12 bytes
 * per max_members; in_len + 40 bytes per member), which the context keeps.  PZG_RC_NO_MEMORY when the device does not have it.
 * A single member is one wavefront's work in these calls: a caller splits the large ones with pzg_index_scan_many and decodes their
 * segments with pzg_decompress_many_segments (the Python mirror's decompress_gzip_file and read_zip do).
 */
PZG_API int pzg_gzip_find_members(pzg_ctx *ctx, const uint8_t *in, uint64_t in_len,
        uint64_t chunk,                  /* 0: 64 KiB; below 64: PZG_RC_BAD_ARG */
        uint64_t *starts, uint32_t *bsize, uint32_t max_members,
        uint32_t *nmembers, uint32_t flags);
PZG_API int pzg_gzip_layout(pzg_ctx *ctx, const uint8_t *in, uint64_t in_len,
        const uint64_t *starts, uint32_t m, uint64_t out_base_off,
        uint64_t *in_off, uint64_t *in_lenv, uint64_t *out_off,
        uint64_t *out_cap, uint64_t *total, uint32_t flags);

/*
 * pzg_unfilter_many (0.5): EXTENSION -- scanline unfiltering, the second half of a PNG decode (PNG specification section 9) and of a
 * PDF FlateDecode stream with Predictor 10-15; a wavefront per image, all n in one launch.  Nothing in it knows of PNG:
 *   image i     height[i] rows of 1 + row_bytes[i] bytes at src_base + src_off[i]: a filter byte (0 None, 1 Sub, 2 Up, 3 Average,
 *               4 Paeth) and the filtered bytes.  bpp[i] is the filter unit in bytes: 1, 2, 3, 4, 6 or 8.
 *   delivery    row r, without its filter byte, at dst_base + dst_off[i] + r * dst_stride[i] (dst_stride[i] >= row_bytes[i]).  The
 *               bytes between row_bytes and the stride and everything outside the extents are untouched.  The dst extents overlap
 *               neither each other nor src.
 *   status[i]   PZG_OK
 *               PZG_E_FILTER     row d0 has the filter byte d1 > 4: rows [0, d0) are delivered, nothing of row d0 onward is written
 *               PZG_E_TRUNCATED  src_len[i] < height * (1 + row_bytes): d0 is the number of rows that lie wholly inside src_len;
 *                                they are delivered -- unless one of them has a bad filter byte, which then wins.  The filter
 *                                bytes of the rows that do not lie wholly inside are not looked at.
 *               height or row_bytes of 0: PZG_OK, nothing read or written.
 *   detail      2n words (d0, d1 per image), or NULL.
 * flags: 0 -- every pointer is host memory: the call stages src, the arrays and dst's extents through the context's arenas and
 * returns when dst and status are filled; PZG_DEVICE_PTRS -- every pointer is device memory, the launch goes on the context's
 * stream (pzg_set_stream) in call order, and with PZG_ASYNC as well the call only enqueues: pzg_decompress_many(... PZG_ASYNC),
 * pzg_unfilter_many(... PZG_ASYNC) and pzg_sync chain without a host round trip, and src_len may be the out_len array the decode
 * wrote (that is why it is an argument).  pzg_last_kernel_ms reports the launch.
 * PZG_RC_BAD_ARG: n == 0, any other flag, a null array, a context of several devices; with host pointers also a bpp outside
 * {1, 2, 3, 4, 6, 8} and a stride below row_bytes (of an image that has rows).  Device arrays are not read by the host: there such
 * an image gets PZG_E_FILTER with d0 = 0xffffffff (d1 = its bpp) and nothing of it is read or written.
 * Offsets and strides are 64-bit.  Nothing is read but the aligned dwords that hold bytes of src_off[i] .. + src_len[i].
 */
PZG_API int pzg_unfilter_many(pzg_ctx *ctx,
        const uint8_t *src_base, const uint64_t *src_off, const uint64_t *src_len,
        uint8_t *dst_base, const uint64_t *dst_off, const uint64_t *dst_stride,
        const uint32_t *row_bytes, const uint32_t *height, const uint8_t *bpp,
        int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t flags);         /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * pzg_adam7_many (0.5): EXTENSION -- Adam7 deinterlacing (PNG specification section 8.2), what follows the unfiltering of an
 * interlaced PNG: the seven reduced images of each of n images woven into the image, all n in one launch, the rows of an image
 * spread over several wavefronts.
 *   source i    the seven reduced images, unfiltered and without filter bytes, dense and back to back in pass order at
 *               src_base + src_off[i].  Pass p holds the pixels (x0 + j dx, y0 + k dy) of the image:
 *                   pass  1  2  3  4  5  6  7
 *                   x0    0  4  0  2  0  1  0
 *                   y0    0  0  4  0  2  0  1
 *                   dx    8  8  4  4  2  2  1
 *                   dy    8  8  8  4  4  2  2
 *               as ph = ceil((height[i] - y0) / dy) rows of prb = ceil(pw * pixel_bits[i] / 8) bytes, pw = ceil((width[i] - x0) / dx);
 *               a pass with pw == 0 or ph == 0 takes no bytes.  The extent is a function of (width, height, pixel_bits) alone --
 *               there is no src_len -- and it is where seven pzg_unfilter_many jobs deliver with dst_stride = row_bytes = prb.
 *   pixel_bits  the bits of a pixel: 1, 2, 4, 8, 16, 24, 32, 48 or 64.  Pixels are moved as bits and bytes, nothing is swapped or
 *               expanded.  Below 8 bits they are packed with the leftmost pixel in the high bits, in each pass row and in each
 *               row delivered; the unused low bits of a delivered row's last byte are written as 0.
 *   delivery    row y of the image, ceil(width[i] * pixel_bits[i] / 8) bytes, at dst_base + dst_off[i] + y * dst_stride[i].  The bytes
 *               between that and the stride and everything outside the extents are untouched.  The dst extents overlap neither
 *               each other nor src.
 *   status[i]   PZG_OK; width or height of 0: PZG_OK, nothing read or written.
 *   detail      2n words (d0, d1 per image), or NULL: 0, 0 of a PZG_OK image.
 * flags: as for pzg_unfilter_many.  0 -- every pointer is host memory: the call stages src, the arrays and dst's extents through
 * the context's arenas and returns when dst and status are filled; PZG_DEVICE_PTRS -- every pointer is device memory, the launch
 * goes on the context's stream (pzg_set_stream) in call order, and with PZG_ASYNC as well the call only enqueues:
 * pzg_decompress_many, pzg_unfilter_many (the pass jobs), pzg_adam7_many and pzg_sync chain without a host round trip.
 * pzg_last_kernel_ms reports the launch.
 * PZG_RC_BAD_ARG: n == 0, any other flag, a null array, a context of several devices; with host pointers also, of an image that has
 * pixels, a pixel_bits outside the list, a stride below the row's bytes and a width or height of 2^31 or more.  Device arrays are
 * not read by the host: there such an image gets PZG_E_FILTER with d0 = 0xffffffff (d1 = its pixel_bits) and nothing of it is read
 * or written.
 * Offsets and strides are 64-bit.  Nothing is read but the aligned dwords that hold bytes of the image's source extent.
 */
PZG_API int pzg_adam7_many(pzg_ctx *ctx,
        const uint8_t *src_base, const uint64_t *src_off,
        uint8_t *dst_base, const uint64_t *dst_off, const uint64_t *dst_stride,
        const uint32_t *width, const uint32_t *height, const uint8_t *pixel_bits,
        int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t flags);         /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * pzg_expand_many (0.5): EXTENSION -- pixel expansion, the last stage of a PNG decode: the rows of n images as PNG stores them
 * (packed 1/2/4-bit samples, palette indices, big-endian 16-bit samples) written as rows of 8-bit RGBA or RGB pixels, all n in one
 * launch, the rows of an image spread over several wavefronts.  It follows pzg_unfilter_many or pzg_adam7_many; like them it knows
 * nothing of PNG's chunks: rows of samples in, rows of 8-bit pixels out.
 *   desc[i]     one image (pzg_expand_desc below; its reserved words are 0):
 *     source      row r, ceil(width * channels * bit_depth / 8) bytes, at src_base + src_off + r * src_stride.
 *     delivery    row r, width * 4 (PZG_PIX_RGBA8: R, G, B, A) or width * 3 (PZG_PIX_RGB8: R, G, B) bytes, at
 *                 dst_base + dst_off + r * dst_stride.  The bytes between that and the stride and everything outside the extents are
 *                 untouched.  The dst extents overlap neither each other nor src.
 *     type        color_type 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha), 6 (RGBA) with bit_depth 1, 2, 4, 8, 16 for type 0,
 *                 1, 2, 4, 8 for type 3 and 8, 16 for the others: PNG's 15 image types.
 *     palette     type 3 only: the entries pal_off .. pal_off + pal_len - 1 (pal_len 1 .. 256) of palette_base, an array of dwords
 *                 whose bytes in memory order are R, G, B, A.  The caller has merged PLTE and tRNS: an entry without a tRNS alpha
 *                 has 255.  palette_base may be NULL in a call without a type 3 image.
 *     key         has_key != 0, types 0 and 2 only (ignored for the others): the tRNS colour key, key[0] for gray and key[0..2] =
 *                 R, G, B, at the source depth.  A pixel whose samples all equal the key gets alpha 0, every other pixel 255.  The
 *                 comparison takes the source samples before any depth reduction: all 16 bits of a 16-bit sample.
 *   samples     Below 8 bits pixels are packed with the leftmost in the high bits; the padding bits of a row's last byte are never
 *               interpreted.  Gray below 8 bits is scaled by bit replication (x 255, x 85, x 17); palette indices are not scaled.
 *               A 16-bit sample gives its HIGH BYTE (what libpng's strip_16 and OpenCV do: no rounding).  Gray fans out to
 *               R = G = B.  The alpha of types 4 and 6 is copied, reduced the same way.  Without alpha, a key or a palette alpha,
 *               A = 255.  PZG_PIX_RGB8 drops alpha: nothing is composited, and there is no gamma.
 *   status[i]   PZG_OK; width or height of 0: PZG_OK, nothing read or written.
 *               PZG_E_PALETTE  a pixel of a type 3 image has an index >= pal_len: d0 = row, d1 = x of the first such pixel in
 *                              row-major order, whichever wavefront and lane met it.  What the image's destination extent then
 *                              holds is unspecified; nothing outside it is written.
 *   detail      2n words (d0, d1 per image), or NULL: 0, 0 of a PZG_OK image.
 * flags: as for pzg_adam7_many.  0 -- every pointer is host memory: the call stages the spans of src and palette_base that the
 * images name, desc and dst's extents through the context's arenas and returns when dst and status are filled (the rows of an image
 * that is not PZG_OK are not copied back); PZG_DEVICE_PTRS -- every pointer is device memory, the launch goes on the context's
 * stream (pzg_set_stream) in call order, and with PZG_ASYNC as well the call only enqueues: pzg_decompress_many, pzg_unfilter_many,
 * [pzg_adam7_many,] pzg_expand_many and pzg_sync chain without a host round trip.  pzg_last_kernel_ms reports the launch.
 * PZG_RC_BAD_ARG: n == 0, any other flag, a null array, a context of several devices; with host pointers also, of an image that has
 * pixels, a (color_type, bit_depth) that is no PNG image type, an unknown out_format, a dst_stride below the delivered row, a
 * src_stride below the source row, a pal_len of 0 or above 256 for type 3 (or a null palette_base), and a width or height of 2^31
 * or more.  Device arrays are not read by the host: there such an image gets PZG_E_FILTER with d0 = 0xffffffff and
 * d1 = color_type << 8 | bit_depth, and nothing of it is read or written.
 * Offsets and strides are 64-bit.  Nothing is read but the aligned dwords that hold bytes of the image's source rows, and its palette
 * entries [pal_off, pal_off + pal_len).
 */
#define PZG_PIX_RGBA8 0u
#define PZG_PIX_RGB8  1u

typedef struct pzg_expand_desc {
    uint64_t src_off, src_stride;   /*  0,  8 */
    uint64_t dst_off, dst_stride;   /* 16, 24 */
    uint32_t width, height;         /* 32, 36 */
    uint32_t pal_off;               /* 40: entry index into palette_base */
    uint16_t pal_len;               /* 44: 1 .. 256 */
    uint16_t key[3];                /* 46 */
    uint8_t color_type, bit_depth;  /* 52, 53 */
    uint8_t out_format;             /* 54: PZG_PIX_* */
    uint8_t has_key;                /* 55 */
    uint32_t reserved[2];           /* 56: 0 */
} pzg_expand_desc;
#if defined(__cplusplus)
static_assert(sizeof(pzg_expand_desc) == 64 && offsetof(pzg_expand_desc, width) == 32 && offsetof(pzg_expand_desc, pal_off) == 40 &&
              offsetof(pzg_expand_desc, pal_len) == 44 && offsetof(pzg_expand_desc, key) == 46 && offsetof(pzg_expand_desc, color_type) == 52 &&
              offsetof(pzg_expand_desc, has_key) == 55 && offsetof(pzg_expand_desc, reserved) == 56, "pzg_expand_desc is 64 bytes, laid out as commented");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(pzg_expand_desc) == 64 && offsetof(pzg_expand_desc, pal_len) == 44 && offsetof(pzg_expand_desc, color_type) == 52,
               "pzg_expand_desc is 64 bytes, laid out as commented");
#endif

PZG_API int pzg_expand_many(pzg_ctx *ctx,
        const uint8_t *src_base, uint8_t *dst_base, const uint32_t *palette_base,
        const pzg_expand_desc *desc,         /* n */
        int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t flags);         /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * pzg_unpredict_many (0.5): EXTENSION -- TIFF horizontal differencing undone (TIFF 6.0 section 14, Predictor 2; the PDF FlateDecode
 * Predictor 2 is the same) and strips or tiles clipped to a window, the second half of reading a Deflate-compressed TIFF: all n
 * jobs in one launch, the rows of a job spread over several wavefronts.  One job is one strip or tile as it was decoded; nothing in
 * the call knows of TIFF's tags.
 *   desc[i]     one job (pzg_unpredict_desc below; its reserved words are 0):
 *     source      `rows` stored rows of src_row_bytes bytes, dense, at src_base + src_off, at any alignment.  For a tile
 *                 src_row_bytes is TileWidth x samples x sample_bytes, padding included, and rows is TileLength; for a strip, rows
 *                 is what that strip really has.
 *     window      what is delivered: the rows [win_row, win_row + win_rows) of the job and, of each, the bytes [win_byte,
 *                 win_byte + win_bytes) of the RECONSTRUCTED row.  Clipping a tile at the image's edge is win_row = win_byte = 0
 *                 with the image's remainder as sizes; a region read clips on all four sides.  The recurrence always starts at
 *                 byte 0 of the stored row, whatever the window.
 *     delivery    window row r at dst_base + dst_off + r * dst_stride (dst_stride >= win_bytes).  The bytes between win_bytes and
 *                 the stride and everything outside the extents are untouched.  The dst extents overlap neither each other nor src.
 *     predictor   1: a clipped copy.  2: horizontal differencing -- sample k of a row is stored[k] + actual[k - samples] modulo
 *                 2^(8 x sample_bytes), taken in the file's byte order (big_endian != 0: most significant byte first) and delivered
 *                 in the file's byte order: nothing is swapped in the output.
 *     samples     1 .. 4: the stride of the recurrence in samples -- SamplesPerPixel for chunky data, 1 for a separate plane.
 *                 sample_bytes: 1, 2, 4 or 8.  (Both are held to their lists with predictor 1 as well, where nothing else is made
 *                 of them.)
 *   src_len[i]  the bytes of job i that src holds: a separate array so that it can be the out_len array a preceding
 *               pzg_decompress_many(... PZG_ASYNC) wrote.
 *   status[i]   PZG_OK
 *               PZG_E_TRUNCATED  src_len[i] < rows * src_row_bytes: d0 is the number of stored rows that lie wholly inside
 *                                src_len[i]; those of them that fall in the window are delivered.
 *               rows, src_row_bytes, win_rows or win_bytes of 0: PZG_OK, nothing read or written.
 *   detail      2n words (d0, d1 per job), or NULL: 0, 0 of a PZG_OK job.
 * flags: as for pzg_expand_many.  0 -- every pointer is host memory: the call stages the spans of src that the jobs name, desc,
 * src_len and dst's extents through the context's arenas and returns when dst and status are filled; PZG_DEVICE_PTRS -- every
 * pointer is device memory, the launch goes on the context's stream (pzg_set_stream) in call order, and with PZG_ASYNC as well the
 * call only enqueues: pzg_decompress_many, pzg_unpredict_many and pzg_sync chain without a host round trip.  pzg_last_kernel_ms
 * reports the launch.
 * PZG_RC_BAD_ARG: n == 0, any other flag, a null array, a context of several devices; with host pointers also, of a job that is not
 * empty, a predictor other than 1 and 2, a sample_bytes or samples outside the lists, a src_row_bytes that is no multiple of
 * samples x sample_bytes with predictor 2, a window that reaches outside the stored job and a dst_stride below win_bytes.  Device
 * arrays are not read by the host: there such a job gets PZG_E_FILTER with d0 = 0xffffffff and
 * d1 = predictor << 16 | sample_bytes << 8 | samples, and nothing of it is read or written.
 * Offsets and strides are 64-bit.  Nothing is read but the aligned dwords that hold bytes of
 * src_off .. + min(src_len[i], rows * src_row_bytes).
 */
typedef struct pzg_unpredict_desc {
    uint64_t src_off;                  /*  0 */
    uint64_t dst_off, dst_stride;      /*  8, 16 */
    uint32_t src_row_bytes, rows;      /* 24, 28 */
    uint32_t win_row, win_rows;        /* 32, 36 */
    uint32_t win_byte, win_bytes;      /* 40, 44 */
    uint8_t predictor, sample_bytes;   /* 48, 49 */
    uint8_t samples, big_endian;       /* 50, 51 */
    uint32_t reserved[3];              /* 52: 0 */
} pzg_unpredict_desc;
#if defined(__cplusplus)
static_assert(sizeof(pzg_unpredict_desc) == 64 && offsetof(pzg_unpredict_desc, dst_off) == 8 && offsetof(pzg_unpredict_desc, src_row_bytes) == 24 &&
              offsetof(pzg_unpredict_desc, win_row) == 32 && offsetof(pzg_unpredict_desc, win_byte) == 40 && offsetof(pzg_unpredict_desc, predictor) == 48 &&
              offsetof(pzg_unpredict_desc, big_endian) == 51 && offsetof(pzg_unpredict_desc, reserved) == 52, "pzg_unpredict_desc is 64 bytes, laid out as commented");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(pzg_unpredict_desc) == 64 && offsetof(pzg_unpredict_desc, src_row_bytes) == 24 && offsetof(pzg_unpredict_desc, predictor) == 48,
               "pzg_unpredict_desc is 64 bytes, laid out as commented");
#endif

PZG_API int pzg_unpredict_many(pzg_ctx *ctx,
        const uint8_t *src_base, const uint64_t *src_len,   /* n */
        uint8_t *dst_base,
        const pzg_unpredict_desc *desc,      /* n */
        int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t flags);         /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * pzg_unshuffle_many (0.5): EXTENSION -- the byte-plane transpose ("shuffle") undone, with or without a byte-wise running sum in front
 * of it, and strips or tiles clipped to a window: all n jobs in one launch, the rows of a job spread over several wavefronts.  With
 * the sum it is TIFF's floating-point predictor (Predictor 3, TIFF Technical Note 3; libtiff fpAcc); the transpose alone is the
 * shuffle filter that HDF5, Zarr (numcodecs Shuffle) and Blosc put in front of zlib.  One job is one strip, tile or chunk as it was
 * decoded; nothing in the call knows of TIFF's tags.
 *   desc[i]     one job (pzg_unshuffle_desc below; its reserved bytes and words are 0).  Source, window and delivery are those of
 *               pzg_unpredict_desc, field for field in the first 48 bytes:
 *     source      `rows` stored rows of src_row_bytes = n x elem_bytes bytes, dense, at src_base + src_off, at any alignment.
 *     window      the rows [win_row, win_row + win_rows) of the job and, of each, the bytes [win_byte, win_byte + win_bytes) of the
 *                 RECONSTRUCTED row: it may start or end inside an element.
 *     delivery    window row r at dst_base + dst_off + r * dst_stride (dst_stride >= win_bytes).  The bytes between win_bytes and
 *                 the stride and everything outside the extents are untouched.  The dst extents overlap neither each other nor src.
 *     elem_bytes  B: 2, 4 or 8.  A stored row is B planes of n bytes.
 *     sum_stride  S.  1 .. 4: first t[k] = stored[k] + t[k - S] modulo 256 for k >= S over ALL n x B bytes of the row -- the sum runs
 *                 straight across the planes' boundaries; n is a multiple of S (the stored samples of a pixel, 1 for a separate
 *                 plane).  0: no sum, t = stored: the transpose alone.
 *     reverse     byte j of output element i is t[j * n + i] where reverse is 0 (plane j is byte j: a big-endian TIFF; HDF5 / Zarr
 *                 shuffle) and t[(B - 1 - j) * n + i] where it is 1 (a little-endian TIFF: plane 0 holds the most significant bytes).
 *   src_len[i]  the bytes of job i that src holds: a separate array so that it can be the out_len array a preceding
 *               pzg_decompress_many(... PZG_ASYNC) wrote.
 *   status[i]   PZG_OK
 *               PZG_E_TRUNCATED  src_len[i] < rows * src_row_bytes: d0 is the number of stored rows that lie wholly inside
 *                                src_len[i]; those of them that fall in the window are delivered.
 *               rows, src_row_bytes, win_rows or win_bytes of 0: PZG_OK, nothing read or written.
 *   detail      2n words (d0, d1 per job), or NULL: 0, 0 of a PZG_OK job.
 * flags: as for pzg_unpredict_many, in both forms; pzg_decompress_many, pzg_unpredict_many, pzg_unshuffle_many and pzg_sync chain
 * without a host round trip.  pzg_last_kernel_ms reports the launch.
 * PZG_RC_BAD_ARG: n == 0, any other flag, a null array, a context of several devices; with host pointers also, of a job that is not
 * empty, an elem_bytes outside the list, a sum_stride above 4, a reverse above 1, a src_row_bytes that is no multiple of elem_bytes,
 * an n that is no multiple of sum_stride, a window that reaches outside the stored job and a dst_stride below win_bytes.  Device
 * arrays are not read by the host: there such a job gets PZG_E_FILTER with d0 = 0xffffffff and
 * d1 = elem_bytes << 16 | sum_stride << 8 | reverse, and nothing of it is read or written.
 * Offsets and strides are 64-bit.  Nothing is read but the aligned dwords that hold bytes of
 * src_off .. + min(src_len[i], rows * src_row_bytes): with a sum every byte of the rows delivered, without one only the elements
 * that hold the window's bytes, from each plane.
 */
typedef struct pzg_unshuffle_desc {
    uint64_t src_off;                  /*  0 */
    uint64_t dst_off, dst_stride;      /*  8, 16 */
    uint32_t src_row_bytes, rows;      /* 24, 28 */
    uint32_t win_row, win_rows;        /* 32, 36 */
    uint32_t win_byte, win_bytes;      /* 40, 44 */
    uint8_t elem_bytes, sum_stride;    /* 48, 49 */
    uint8_t reverse, reserved0;        /* 50, 51: 0 */
    uint32_t reserved[3];              /* 52: 0 */
} pzg_unshuffle_desc;
#if defined(__cplusplus)
static_assert(sizeof(pzg_unshuffle_desc) == 64 && offsetof(pzg_unshuffle_desc, dst_off) == 8 && offsetof(pzg_unshuffle_desc, dst_stride) == 16 &&
              offsetof(pzg_unshuffle_desc, src_row_bytes) == 24 && offsetof(pzg_unshuffle_desc, rows) == 28 && offsetof(pzg_unshuffle_desc, win_row) == 32 &&
              offsetof(pzg_unshuffle_desc, win_rows) == 36 && offsetof(pzg_unshuffle_desc, win_byte) == 40 && offsetof(pzg_unshuffle_desc, win_bytes) == 44 &&
              offsetof(pzg_unshuffle_desc, elem_bytes) == 48 && offsetof(pzg_unshuffle_desc, sum_stride) == 49 && offsetof(pzg_unshuffle_desc, reverse) == 50 &&
              offsetof(pzg_unshuffle_desc, reserved0) == 51 && offsetof(pzg_unshuffle_desc, reserved) == 52, "pzg_unshuffle_desc is 64 bytes, laid out as commented");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(pzg_unshuffle_desc) == 64 && offsetof(pzg_unshuffle_desc, src_row_bytes) == 24 && offsetof(pzg_unshuffle_desc, elem_bytes) == 48,
               "pzg_unshuffle_desc is 64 bytes, laid out as commented");
#endif

PZG_API int pzg_unshuffle_many(pzg_ctx *ctx,
        const uint8_t *src_base, const uint64_t *src_len,   /* n */
        uint8_t *dst_base,
        const pzg_unshuffle_desc *desc,      /* n */
        int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t flags);         /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * pzg_unlzw_many (0.5): EXTENSION -- LZW as TIFF (Compression 5, the post-6.0 form) and PDF (LZWDecode) pack it: n streams in one launch,
 * one wavefront a stream.  The arrays mean what they mean in pzg_decompress_many, so out_len can be the src_len array of
 * pzg_unpredict_many / pzg_unshuffle_many enqueued behind this call.
 * Codes and widths:
 *   - codes are packed most significant bit first; Clear is 256, EOI is 257, the first entry is 258;
 *   - the table starts cleared: a stream need not begin with a Clear;
 *   - before a code is read, let f be the next free entry: 258 after a Clear, and every code after the first one following a Clear
 *     adds an entry;
 *   - the code is read at the smallest width w in 9..12 with f <= (1 << w) - 1 - early_change (mode bit 0, PZG_LZW_EARLY_CHANGE:
 *     1 for TIFF and for PDF's default, 0 for PDF's EarlyChange 0);
 *   - entries are made up to 4095; after that the width stays 12, nothing is added, and decoding goes on.
 * Decoding: a literal emits itself; a code c with 258 <= c < f emits its entry (the string of the code that made it plus the first
 * byte of the code behind that one); c == f with a previous code since the Clear emits the previous string plus its own first byte;
 * any other code is PZG_E_LZW, d0 = the code, d1 = the bytes produced so far.
 * Decoding ends with whichever comes first:
 *   - EOI: PZG_OK;
 *   - out_cap[i] bytes delivered: PZG_OK -- a string that crosses the capacity is cut there, out_len[i] = out_cap[i], and what follows
 *     in the stream is not looked at (LZW carries no end-of-data integrity and libtiff stops the same way): this is NOT
 *     PZG_E_OUT_TOO_SMALL.  out_cap[i] == 0: PZG_OK with nothing read;
 *   - the input runs out inside or before a code: PZG_E_TRUNCATED, out_len[i] the bytes of the complete codes (in_len[i] == 0: 0).
 * A failed stream delivers the bytes [0, out_len[i]) it had produced.  Nothing is ever written past out_cap[i]; nothing is read but
 * the aligned dwords that hold bytes of the stream.  detail: 2n words (d0, d1 per stream), or NULL: 0, 0 unless stated.
 * flags: 0 -- host pointers, through the staging of the host-pointer streams with dictionaries (packed, uploaded, launched, copied
 * back) --; PZG_DEVICE_PTRS -- the launch goes on the context's stream in call order --; PZG_DEVICE_PTRS | PZG_ASYNC.
 * pzg_last_kernel_ms reports the launch.
 * PZG_RC_BAD_ARG: n == 0, a null array (in_base, out_base and detail may be null where nothing needs them), any other flag, mode bits
 * other than bit 0, a context of several devices; with host pointers also an extent that wraps and an out_cap[i] of 4 GiB or more:
 * positions are 32-bit (with device pointers such a capacity is taken as 4 GiB - 1).
 * NOT done: codes packed least significant bit first (GIF), a variable minimum code size, the pre-6.0 TIFF bit order.
 */
#define PZG_LZW_EARLY_CHANGE 1u   /* TIFF, and PDF's default; 0: PDF EarlyChange 0 */
PZG_API int pzg_unlzw_many(pzg_ctx *ctx,
        const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len,
        uint8_t *out_base, const uint64_t *out_off, const uint64_t *out_cap,
        uint64_t *out_len, int32_t *status, uint32_t *detail,   /* detail: 2n, or NULL */
        uint32_t n, uint32_t mode, uint32_t flags);             /* 0, PZG_DEVICE_PTRS, PZG_DEVICE_PTRS | PZG_ASYNC */

/*
 * decompressIncremental / ZlibDecoder (Zlib.hs:3-8, Monad.hs:163-197; driver Deflate.hs:30-48), batched: a pzg_decoder
 * is n suspended zlib decoders (gzip or raw ones: pzg_decoder_create_format) living on the device (a one-device context).  pzg_decoder_feed continues the decoders
 * idx[0..m) (idx = NULL: all n, m ignored) -- one launch, one wavefront per decoder -- as far as their input and
 * output room go.  For decoder k = idx[j]:
 *   in_base + in_off[j] .. + in_len[j]   the bytes the last call did not consume (from its in_used on) followed by
 *                                        the new input; final_in[j] != 0 (array may be NULL): no more input will follow;
 *                                        in_base may be NULL when every in_len[j] is 0
 *   out_base + out_off[j] .. + out_cap[j]  room for the bytes this call delivers (out_cap >= 4096); out_len[j] of them
 *   state[j]     PZG_DEC_NEED_INPUT  suspended on input: the reference's NeedMore
 *                PZG_DEC_OUT_FULL    suspended on room: call again with in_base + in_used[j] onward
 *                PZG_OK              the stream has ended: Done (trailing input is left unconsumed)
 *                PZG_E_*             DecompError; detail[2j..] as for pzg_decompress_many
 *   in_used[j]   input bytes the decoder is done with (it remembers a partly consumed byte itself)
 *   chunks[j]    how many 32,768-byte chunks the reference has published up to this point (cumulative): moveWindow
 *                runs after every match and block end and publishes one when 64 KiB are buffered
 *                (OutputWindow.hs:45-54); the host mirror cuts the delivered bytes into exactly those Chunks, and at
 *                PZG_OK publishes the remainder as the last one (finalize, Monad.hs:349-353).
 * Host pointers only.  Nothing is re-decoded: a feed costs what its new input costs.
 * Footprint: a pzg_decoder keeps, grow-only until pzg_decoder_destroy, staging of the largest feed it has seen --
 * m x (in_len + 32) + m x out_cap bytes of page-locked host memory and as much device memory -- plus ~41 KiB of device
 * state per decoder (its registers and tables, an 8 KiB image of its wave's LDS, and the last 32 KiB it produced).  A feed
 * of 512 decoders or more that moves 64 MiB or more is pipelined in ranges (upload, launch, download and the host-side
 * copies of neighbouring ranges overlap).  Where the system will not lock that much the staging falls back to pageable memory (slower copies,
 * same results).
 */
typedef struct pzg_decoder pzg_decoder;
PZG_API int  pzg_decoder_create(pzg_ctx *ctx, uint32_t n, pzg_decoder **out);  /* takes a reference on ctx */
/* (0.5) pzg_decoder_create for another container.  format: 0 (zlib, the same as pzg_decoder_create), PZG_GZIP or PZG_RAW; anything else
 * (PZG_GZIP | PZG_RAW too) is PZG_RC_BAD_ARG.  All n decoders of the object share the format, pzg_decoder_reset keeps it, and
 * pzg_decoder_feed is what it is for zlib decoders: its suspension protocol, its chunks[] rule (the publication rule does not depend on
 * the wrapper), its pipelined path for large feeds.
 * THE RULE that decides every corner: however the input is cut into feeds and the rooms are sized, the concatenation of the delivered
 * bytes, the terminal state and its detail, the last adler[j] and the sum of the in_used[j] of all calls are what pzg_decompress_many
 * gives with the same flag over the whole input as one stream with enough capacity.  (For a decoder that ends with an error met
 * inside the blocks in_used is unspecified, as it is for a failed stream of that call -- the batch kernels have read ahead of the
 * token that fails -- and never more than what the call was given.)  A terminal error is reported once the batch path would have met it, never earlier because a piece ended.
 * PZG_RAW: no header, no trailer.  The first block header is at bit 0 of the first byte fed; the state is PZG_OK when the final block
 *   ends, and in_used counts up to and including the byte that holds its last bit -- what follows is left alone.  adler[j] is the
 *   running Adler-32 of everything delivered so far, reported and never checked.  PZG_E_HDR_*, PZG_E_CHECKSUM and PZG_E_DICT cannot
 *   occur; with final_in set, input that ends before the final block does is PZG_E_TRUNCATED; detail[1] of PZG_E_HUFF_BUILD counts
 *   bits from the first bit ever fed.
 * PZG_GZIP: a series of RFC 1952 members, as the batch gzip path reads them.
 *   A member header is read as a whole: if the input ends inside it and final_in is not set, the decoder suspends at the header's
 *   first byte (PZG_DEC_NEED_INPUT, in_used stops in front of the header; the next call reads it again from its start -- so a
 *   header, FEXTRA, FNAME and FCOMMENT included, must fit one feed); with final_in a short header is PZG_E_TRUNCATED.  Header errors
 *   are PZG_E_GZIP_HEADER with the batch path's detail words.
 *   The 8-byte trailer is read as a whole, under the same rule.  There the member's ISIZE is checked (PZG_E_GZIP_ISIZE) and its
 *   CRC-32 is folded into the CRC-32 the whole output must have.  Behind a trailer: fewer than 2 bytes left and no final_in --
 *   PZG_DEC_NEED_INPUT (a decoder may then still hold the trailer unread); 1f 8b -- the next member follows; anything else, or the
 *   end of the input with final_in -- PZG_OK, the trailing bytes stay unconsumed.
 *   adler[j] is the running CRC-32 of everything delivered so far, carried across the calls: a pass behind the decode kernel, on the
 *   same stream and in front of every download, takes the CRC-32 of each fed decoder's delivery of this call and appends it.  When
 *   a decoder has ended with PZG_OK or PZG_E_GZIP_ISIZE the pass holds the running value against the expected one; a mismatch makes
 *   the state PZG_E_CHECKSUM with detail = {expected, ours} -- the CRC-32 is looked at first, as zlib does -- now and for every
 *   later call on that decoder. */
PZG_API int  pzg_decoder_create_format(pzg_ctx *ctx, uint32_t n, uint32_t format, pzg_decoder **out);
PZG_API void pzg_decoder_destroy(pzg_decoder *dec);  /* legal before or after pzg_shutdown(ctx); NULL is ignored */
PZG_API int  pzg_decoder_reset(pzg_decoder *dec, const uint32_t *idx, uint32_t m);  /* those decoders start a new stream */
/* (0.5) What the last LARGE pzg_decoder_feed call of `dec` (512 decoders or 64 MiB of rooms and more: the pipelined path) spent where, in
 * milliseconds: [0] the whole call; [1] packing the inputs into page-locked staging (the issuing thread); [2] waiting for the ranges'
 * kernels, [3] bringing down what their decoders delivered (a second thread); [4] copying it out into the caller's rooms (a third).
 * The three threads run side by side: the parts do not add up to the call.  -1: no such call yet. */
PZG_API int  pzg_decoder_last_feed_ms(pzg_decoder *dec, double out[5]);
PZG_API int  pzg_decoder_feed(pzg_decoder *dec, const uint32_t *idx, uint32_t m,
                      const uint8_t *in_base, const uint64_t *in_off, const uint64_t *in_len, const uint8_t *final_in,
                      uint8_t *out_base, const uint64_t *out_off, const uint64_t *out_cap,
                      uint64_t *out_len, int32_t *state, uint32_t *detail, uint64_t *in_used,
                      uint32_t *chunks, uint32_t *adler);

/* decompress: the single-stream form (n = 1, host pointers). */
PZG_API int pzg_decompress(pzg_ctx *ctx, const uint8_t *in, uint64_t in_len,
                   uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                   int32_t *status, uint32_t detail[2], uint64_t *in_used);

/* Adler-32 of one buffer (Codec.Compression.Zlib.Adler32, Adler32.hs:17-57) as a device-wide
 * reduction.  `init` is a finalized Adler value (1 for a fresh checksum). */
PZG_API int pzg_adler32(pzg_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t init,
                uint32_t *out, uint32_t flags);

/* The batched form (BASELINE config 2, 262,144 x 64 KiB): out[i] = Adler-32 of base[off[i] .. off[i]+len[i]), one wave per
 * buffer.  Device memory only (PZG_DEVICE_PTRS). */
PZG_API int pzg_adler32_many(pzg_ctx *ctx, const uint8_t *base, const uint64_t *off, const uint64_t *len,
                     uint32_t *out, uint32_t n, uint32_t flags);

/* Exact `show` text of the DecompressionError the reference returns for (status, detail) on
 * this stream (host memory; needed only for PZG_E_HUFF_BUILD, whose message depends on the
 * trie insertion order).  Writes a NUL-terminated string; returns its length. */
PZG_API int pzg_error_message(const uint8_t *in, uint64_t in_len, int32_t status,
                      const uint32_t detail[2], char *buf, size_t buf_len);

/* Kernel time of the last launch on this context in milliseconds (HIP events on the launch
 * stream), or a negative value if none was recorded. */
PZG_API double pzg_last_kernel_ms(pzg_ctx *ctx);

PZG_API const char *pzg_strerror(int rc);
PZG_API const char *pzg_last_error(pzg_ctx *ctx);
PZG_API uint32_t    pzg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PZG_H */
