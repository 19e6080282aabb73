/*
 * lc_lz4.h -- C ABI of the LZ4 block writer: a serialized LogGroup (lc_sls.h's records and tags) as the one LZ4 block flusher_sls sends,
 * made on the MI355X where the records already lie, so that only the block crosses the link.
 *
 *   reference                                                                       this ABI
 *   -----------------------------------------------------------------------------  ------------------------------------
 *   FlusherSLS's compressor, CompressType::LZ4 by default                           lc_lz4_create
 *   (core/plugin/flusher/sls/FlusherSLS.cpp:559)
 *   LZ4Compressor::Compress: LZ4_compress_default over the whole group, one block   lc_lz4_compress_device (lz4_match_kernel, the scans,
 *   (core/common/compression/LZ4Compressor.cpp:25-44), LZ4_compressBound             lz4_size_kernel, lz4_emit_kernel), lc_lz4_bound
 *   processor_parse_regex_native, SLSEventGroupSerializer, the tags, the above      lc_lz4_match_encode_compress_host (one trip)
 *
 * The entry points live in a library of their own, liblc_lz4.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error, the matcher) and liblc_sls.so (the records); this header is include/lz4/lc_lz4.h.  The ABIs of the other libraries and
 * their headers do not change.
 *
 * There is no CPU path: without a HIP device every entry point that would read a byte returns LC_ERR_NO_DEVICE.
 *
 * DEFINED here, different from the reference:
 *   - VALID LZ4, NOT LZ4_compress_default's BYTES.  A block is the LZ4 block format (no frame) and obeys its end rules (the last match
 *     starts at or before n - 12, the block ends with at least 5 literals), so LZ4_decompress_safe with the raw size gives the input back;
 *     the server only ever decodes.  The bytes are a function of the input and the chunk size alone -- the same on every run, and the
 *     same as the host routine of csrc/lz4_vm.hpp, which states the rules -- but they are not the bytes liblz4 writes.
 *   - THE CHUNK RULE.  A segment is cut into chunks of chunk_bytes; a match and its source lie inside one chunk (every offset is below
 *     chunk_bytes, no match crosses a multiple of it); a literal run may span chunks.  One wavefront serves a chunk with a 4096-entry
 *     table that starts empty.  What it costs (measured): the SLS records of the headline lines shrink to 0.836 /
 *     0.809 / 0.799 of their size at 4 / 16 / 64 KiB chunks where liblz4 reaches 0.784; the multiline corpus to 0.311 / 0.234 / 0.210
 *     where liblz4 reaches 0.185.  The default is 4 KiB, for the time a group takes (a chunk is one wavefront's serial walk).
 *   - NO ZSTD.  The reference's other compressor (CompressType::ZSTD) has no entry here.
 * Kept as the reference has it: one block per group, the raw size beside it (x-log-bodyrawsize), a bound of at most LZ4_compressBound.
 */
#ifndef LC_LZ4_H
#define LC_LZ4_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_regex_gpu.h"
#include "../sls/lc_sls.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a segment is shorter than this (LZ4_MAX_INPUT_SIZE) */
#define LC_LZ4_MAX_SEGMENT 0x7E000000u

typedef struct lc_lz4 lc_lz4_t;

/* chunk_bytes: a multiple of 64 from 64 to 65536, or 0 for the default (lc_lz4_chunk_bytes says which).  LC_ERR_ARG with a message in
 * err for anything else.  A handle holds no device memory and may be shared by threads. */
int lc_lz4_create(uint32_t chunk_bytes, lc_lz4_t** out, char* err, size_t errcap);
void lc_lz4_free(lc_lz4_t* ctx);
uint32_t lc_lz4_chunk_bytes(const lc_lz4_t* ctx);

/* what a block of n input bytes takes at the most: n + n / 255 + 16 */
uint64_t lc_lz4_bound(uint64_t n);
/* bytes of d_scratch for n_seg segments of total_in bytes together (about 2.1 x total_in: a chunk's matches wait there for their place) */
size_t lc_lz4_scratch_bytes(const lc_lz4_t* ctx, uint64_t total_in, uint32_t n_seg);

/* n_seg segments of d_in as n_seg LZ4 blocks, on the current HIP device.
 *   d_seg_begin  uint64[n_seg]: byte offsets into d_in -- any alignment, any order, not necessarily adjacent
 *   d_seg_len    uint32[n_seg], each below LC_LZ4_MAX_SEGMENT
 *   d_out_off    uint64[n_seg + 1]: block s is d_out[d_out_off[s] .. d_out_off[s + 1]); the blocks stand back to back; the last entry is
 *                the total.  Complete whatever out_cap is.
 *   d_out        any alignment.  Writes touch d_out[0 .. total) and nothing else; when the total exceeds out_cap NOT ONE byte is stored
 *                (read d_out_off[n_seg], come back with room).  d_out may be NULL with out_cap 0.
 *   d_scratch    lc_lz4_scratch_bytes(ctx, the sum of d_seg_len, n_seg) bytes, 8-byte aligned
 * A segment of length 0 is the one-byte block 00.  n_seg = 0 stores d_out_off[0] = 0 and nothing else.  Reads touch the segments' bytes
 * only.
 * LC_ERR_ARG: d_out_off or d_scratch misaligned (8 bytes), d_seg_begin (8) or d_seg_len (4) misaligned, a scratch too small for n_seg
 * alone, a d_in that lives on another device than the calling thread's current one.  Without a device: LC_ERR_NO_DEVICE.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream), no host round trip.  The lengths live on the device, so two
 * refusals are the device's: a segment at or above LC_LZ4_MAX_SEGMENT, and a scratch too small for the lengths' sum, leave EVERY entry
 * of d_out_off at UINT64_MAX and store nothing else (lc_lz4_compress_host refuses such a segment with LC_ERR_ARG before it starts). */
int lc_lz4_compress_device(lc_lz4_t* ctx, const uint8_t* d_in, const uint64_t* d_seg_begin, const uint32_t* d_seg_len, uint32_t n_seg,
                           uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, void* d_scratch, size_t scratch_bytes, void* stream);

/* One trip on the calling thread's pinned staging, on the device the thread is bound to (lc_runtime_bind_thread): the segments' bytes up,
 * the blocks down.  Synchronous.  *out: the blocks back to back, a view into the thread's pinned block, valid until the thread's next
 * lc_lz4_* call; out_off: uint64[n_seg + 1] as above.
 * THIS IS NOT THE PATH THE LIBRARY EXISTS FOR: every input byte crosses the link to save a part of them on the way back.  It serves
 * callers whose payload is on the host already, and the tests. */
int lc_lz4_compress_host(lc_lz4_t* ctx, const uint8_t* const* segs, const uint32_t* seg_len, uint32_t n_seg, const uint8_t** out, uint64_t* out_off);

/* The counterpart of lc_sls_match_encode_host (lc_sls.h; plan, re, lines, len, n, time, time_ns, enable_ns, rec_off and status are that
 * entry's): lines up, lc_regex_match_device, lc_sls_encode_device, the caller's tag bytes (the output of lc_sls_append_tags) right behind
 * the records, ONE block over records + tags -- and only the block, *raw_len, the status bytes and, when asked for, rec_off come down.
 *   *out, *out_len  the block: a view into the thread's pinned block, valid until the thread's next lc_lz4_* call
 *   *raw_len        the records' and the tags' bytes together: what the agent puts into x-log-bodyrawsize
 *   rec_off         uint64[n + 1], offsets into the raw bytes; may be NULL
 * The records' total is not known before the scan: the device buffers have room for the bound the plan gives for rows that do not
 * overlap; where a batch exceeds it the records, the tags and the block are made once more with room for the total (the match is not). */
int lc_lz4_match_encode_compress_host(lc_lz4_t* ctx, lc_sls_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len,
                                      uint32_t n, const uint32_t* time, const int32_t* time_ns, int enable_ns, const uint8_t* tags,
                                      uint32_t tags_len, const uint8_t** out, size_t* out_len, uint64_t* raw_len, uint64_t* rec_off, uint8_t* status);

/* releases the calling thread's staging and stream of the two host entries (they are also released when the thread ends) */
void lc_lz4_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_LZ4_H */
