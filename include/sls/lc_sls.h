/*
 * lc_sls.h -- C ABI of the SLS encoder: the log events a regex parse leaves behind, as the wire bytes flusher_sls sends
 * (the `Logs` field of sls_logs.proto's LogGroup), written on the MI355X where the capture table already lies.
 *
 *   reference                                                                       this ABI
 *   -----------------------------------------------------------------------------  ------------------------------------
 *   SLSEventGroupSerializer::CalculateLogEventSize / SerializeLogEvent              lc_sls_encode_device
 *   (core/collection_pipeline/serializer/SLSSerializer.cpp:254-268, :377-395)       (sls_size_kernel, the scan, sls_write_kernel)
 *   over LogGroupSerializer (core/protobuf/sls/LogGroupSerializer.cpp:105-143,
 *   GetLogSize :234-248)
 *   processor_parse_regex_native, then the above                                    lc_sls_match_encode_host (one trip),
 *                                                                                   lc_sls_processor_serialize (a whole group)
 *   AddTopic / AddSource / AddMachineUUID / AddLogTag :145-183,                     lc_sls_append_tags (host; no kernel)
 *   SLSSerializer.cpp:239-249
 *
 * The entry points live in a library of their own, liblc_sls.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error, the matcher), beside liblc_kvsplit.so and liblc_csv.so; this header is include/sls/lc_sls.h.  The ABIs of those
 * three libraries and the headers of include/ do not change.
 *
 * The wire format (no escaping anywhere: tags, varint lengths, copies):
 *   content     0x12 varint(S(klen) + S(vlen)) 0x0A varint(klen) key 0x12 varint(vlen) value          S(x) = 1 + varint_size(x) + x
 *   log record  0x0A varint(logSZ) 0x08 varint5(max(time, 2^28)) content... [0x25 fixed32le(ns)]
 *               logSZ = sum of the content sizes + 6 (+ 5 with ns); the ns part only when the caller asked for it AND the event has one
 *   an event that would hold no content writes no record; records stand in event order
 *
 * There is no CPU path for the encode: without a HIP device every entry point that would read a line returns LC_ERR_NO_DEVICE.
 *
 * DEFINED here, different from the reference:
 *   - A RECORD OF 4 GiB IS NOT WRITTEN.  An event whose record would reach 0xFFFFFFF0 bytes counts as "no record" (size 0 in
 *     rec_off).  The reference's own varint writer packs 32-bit sizes and would write a broken length there.
 *   - A ROW OUTSIDE ITS LINE IS CUT.  A capture row that does not lie inside the line (begin >= the line's length, end beyond it,
 *     end < begin) is cut to the line, or is the empty value; lc_regex_match_device never writes such a row.
 * PINNED ON THE MODEL, not on the compiled reference: the tags of lc_sls_append_tags.  The reference's writer as compiled for the
 * tests (oracle/ref_processor) serializes log events only, so the tag bytes are held to the Python model of the tests
 * (tests/helpers/sls_wire.py) and to a protobuf wire decode of the result, not to the reference's bytes.
 * Kept as the reference has them: everything in the table above, bit for bit.
 */
#ifndef LC_SLS_H
#define LC_SLS_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bounds of a plan: items per list, bytes of all keys together */
#define LC_SLS_MAX_ITEMS 256u
#define LC_SLS_MAX_KEY_BYTES 65536u

/* lc_sls_processor_counters, own[] */
enum {
    LC_SLS_CNT_GROUPS_DEVICE = 0, /* groups lc_sls_processor_serialize wrote on the device */
    LC_SLS_CNT_GROUPS_HOST = 1,   /* groups it parsed and wrote on the host */
    LC_SLS_CNT_FAILED_TRIPS = 2,  /* calls whose device trip failed */
    LC_SLS_CNT_BYTES = 3,         /* wire bytes handed out */
    LC_SLS_CNT_COUNT = 4
};

typedef struct lc_sls_plan lc_sls_plan_t;
typedef struct lc_sls_processor lc_sls_processor_t;

/* A plan says what an event becomes: a table of keys and two item lists, one for a line the parser matched (status LC_MATCH) and
 * one for every other line.  An item is the pair (key index, source) = two uint32: source 0 is the whole line, g >= 1 capture
 * group g.  An empty list means "no record" for those lines.  The plan holds, per item, the constant bytes
 * `0x0A varint(klen) key 0x12`.
 * LC_ERR_UNSUPPORTED with a message in err: more than LC_SLS_MAX_ITEMS items in a list, more than LC_SLS_MAX_KEY_BYTES of keys.
 * LC_ERR_ARG: a key index outside the table, NULL where n > 0. */
int lc_sls_plan_create(const char* const* keys, const uint32_t* key_len, uint32_t n_keys, const uint32_t* matched_items, uint32_t n_matched,
                       const uint32_t* unmatched_items, uint32_t n_unmatched, lc_sls_plan_t** out, char* err, size_t errcap);
void lc_sls_plan_free(lc_sls_plan_t* plan);

/* bytes of d_scratch for n events */
size_t lc_sls_scratch_bytes(uint32_t n);

/* The records of n events on what lc_regex_match_device left behind, on the current HIP device (the contract for d_data, d_off,
 * d_len, sep_bytes, d_caps = int32[n][2 * ngroups] and d_status is that entry's, lc_regex_gpu.h; reads may touch the 16-byte unit
 * around a line).  Status LC_MATCH takes the matched list, every other status byte the unmatched list.
 *   d_time       uint32[n], epoch seconds
 *   d_time_ns    int32[n], < 0: the event has no nanosecond part; may be NULL (none has).  Read only with enable_ns != 0.
 *   d_rec_off    uint64[n + 1]: where event i's record begins in d_out; d_rec_off[n] is the total; a record of size 0 repeats the
 *                offset.  Complete whatever out_cap is: it is what a batcher needs to cut at event borders.
 *   d_out        the records back to back.  Writes touch d_out[0 .. total) and nothing else; when the total exceeds out_cap NOT ONE
 *                byte is stored (read d_rec_off[n], come back with room).  d_out may be NULL with out_cap 0.
 *   d_scratch    lc_sls_scratch_bytes(n) bytes, 8-byte aligned
 * Alignment: d_out 16 bytes, d_rec_off and d_scratch 8 bytes, d_time / d_time_ns 4; anything else is refused with LC_ERR_ARG, as
 * are a plan that names a group above ngroups, n >= 2^31 and a d_data that lives on another device than the calling thread's
 * current one.  n = 0 stores d_rec_off[0] = 0 and nothing else.  Without a device: LC_ERR_NO_DEVICE.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream), no host round trip -- except that a plan's first use on a
 * device uploads its tables (one synchronous copy of a few KiB). */
int lc_sls_encode_device(lc_sls_plan_t* plan, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t sep_bytes,
                         uint32_t n, uint32_t ngroups, const int32_t* d_caps, const uint8_t* d_status, const uint32_t* d_time,
                         const int32_t* d_time_ns, int enable_ns, uint8_t* d_out, uint64_t out_cap, uint64_t* d_rec_off, void* d_scratch,
                         size_t scratch_bytes, void* stream);

/* One trip on the calling thread's pinned staging, on the device the thread is bound to (lc_runtime_bind_thread): lines[i][0 ..
 * len[i]) up (pulled by a kernel, no copy engine), lc_regex_match_device with `re`, the encode, the payload down.  Synchronous.
 *   time, time_ns   as above, host arrays; time_ns may be NULL
 *   *out, *out_len  the records: a view into the thread's pinned block, valid until the thread's next lc_sls_* call
 *   rec_off         uint64[n + 1] back to the caller; may be NULL
 *   status          uint8[n] back to the caller: the matcher's status bytes (LC_GAVE_UP among them: the caller's counters need it)
 * No copy engine in the trip: the kernels store the total, the status bytes and the records into the thread's pinned block through its
 * mapping (rec_off, when asked for, is the one copy).  The payload's size is not known before the scan: the block has room for the bound
 * the plan gives for rows that do not overlap; where a batch exceeds it (nested groups, the line beside its groups) the write kernel has
 * stored nothing, the host reads the total, grows the block and queues the write kernel alone once more. */
int lc_sls_match_encode_host(lc_sls_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
                             const uint32_t* time, const int32_t* time_ns, int enable_ns, const uint8_t** out, size_t* out_len,
                             uint64_t* rec_off, uint8_t* status);

/* The group's tags behind the records, on the host: n (key, value) pairs in the order to write.  `__topic__`, `__source__` and
 * `__machine_uuid__` become the LogGroup's fields 3, 4 and 5 (0x1A / 0x22 / 0x2A, varint(len), bytes), every other pair a LogTag
 * (0x32, laid out like a content).  Writes at most out_cap bytes to out; *out_len is the size needed.  LC_ERR_OVERFLOW (nothing
 * written) when that exceeds out_cap. */
int lc_sls_append_tags(const char* const* keys, const uint32_t* key_len, const char* const* values, const uint32_t* value_len, uint32_t n,
                       uint8_t* out, size_t out_cap, size_t* out_len);

/* releases the calling thread's staging and stream of lc_sls_match_encode_host (they are also released when the thread ends) */
void lc_sls_thread_release(void);

/* processor_parse_regex_native + SLSEventGroupSerializer in one call.  config_json: processor_parse_regex_native's own
 * (lc_processor_create, lc_processor.h).  LC_ERR_UNSUPPORTED / LC_ERR_SYNTAX with a message in err as there. */
int lc_sls_processor_create(const char* config_json, lc_sls_processor_t** out, char* err, size_t errcap);
void lc_sls_processor_destroy(lc_sls_processor_t* p);
/* The bytes the reference produces when processor_parse_regex_native runs on the group and SLSEventGroupSerializer serializes the
 * log events that are left; the group itself is left untouched.  *out is a view into the calling thread's block, valid until the
 * thread's next lc_sls_* call.  *fused: 1 when the device wrote the records (every event a log event holding exactly the SourceKey
 * content, not the whole-line mode, distinct keys, fewer than mark_count + 1, no alarm sink, no line left undecided, a plan within its
 * bounds), 0 when the group was parsed by the parser's host code on a copy and written by the host writer.  An LC_ERR_* code when the
 * device trip failed: no *out then, the group is as before the call, LC_SLS_CNT_FAILED_TRIPS grows and the events count under
 * LC_CNT_DEVICE_FAILED_EVENTS, as behind a failed trip of lc_processor_process. */
int lc_sls_processor_serialize(lc_sls_processor_t* p, lc_event_group_t* group, int enable_ns, const uint8_t** out, size_t* out_len, int* fused);
/* The host writer alone: the log events of a group as they are (behind lc_processor_process, say), as SLSEventGroupSerializer writes
 * them.  *out is a view into the calling thread's block, valid until the thread's next lc_sls_* call. */
int lc_sls_serialize_group_host(lc_event_group_t* group, int enable_ns, const uint8_t** out, size_t* out_len);
/* parse[]: the parser's counters in LC_CNT_* order (lc_processor.h; the instance-level entries are 0): after either path they are what
 * lc_processor_process leaves on the same group, LC_CNT_COMPLEXITY_EXCEEDED among them.  own[]: LC_SLS_CNT_* */
int lc_sls_processor_counters(const lc_sls_processor_t* p, uint64_t parse[LC_CNT_COUNT], uint64_t own[LC_SLS_CNT_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* LC_SLS_H */
