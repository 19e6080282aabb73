/*
 * lc_jsonl.h -- C ABI of the JSON-lines encoder: the log events a regex parse leaves behind, one JSON object per line as
 * flusher_file and flusher_kafka send them, written on the MI355X where the capture table already lies.
 *
 *   reference                                                                       this ABI
 *   -----------------------------------------------------------------------------  ------------------------------------
 *   JsonEventGroupSerializer::Serialize, the log branch                             lc_jsonl_encode_device
 *   (core/collection_pipeline/serializer/JsonSerializer.cpp:30-84, :197)            (jsonl_size_kernel, the scan, jsonl_write_kernel)
 *   over rapidjson's Writer::WriteString (default flags)
 *   the group's tags in front of every record (:52-58, SizedMap::mInner,            lc_jsonl_head (host; no kernel)
 *   core/models/SizedContainer.h:57)
 *   processor_parse_regex_native, then the above                                    lc_jsonl_match_encode_host (one trip),
 *                                                                                   lc_jsonl_processor_serialize (a whole group)
 *
 * The entry points live in a library of their own, liblc_jsonl.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error, the matcher), the seventh beside the six; this header is include/jsonl/lc_jsonl.h.  The ABIs of the other libraries
 * and the headers of include/ do not change.
 *
 * The format:
 *   record   {"<tag key>":"<tag value>",...,"__time__":<seconds>,"<key>":"<value>",...}\n
 *            the tags in the order of a std::map<StringView, StringView>: ascending by key, bytes compared as unsigned, a shorter key
 *            before its extensions; the seconds in decimal (no sign, no leading zeros, 0 is 0), the nanosecond part is never written;
 *            the contents in the event's order; with no tags the record begins {"__time__":
 *   string   " -> \"   \ -> \\   0x08 0x09 0x0A 0x0C 0x0D -> \b \t \n \f \r   every other byte below 0x20 -> \u00XX, UPPER-case hex
 *            everything else is copied as it is: /, 0x7F and every byte >= 0x80, valid UTF-8 or not (no validation, no transcoding)
 *   THE NUL RULE: keys, values, tag keys and tag values are each CUT AT THEIR FIRST 0x00 BYTE (the reference hands
 *            .to_string().c_str() to the const Ch* overloads of Key and String, which take strlen)
 *   an event that would hold no content writes no record; records stand in event order
 *
 * There is no CPU path for the encode: without a HIP device every entry point that would read a line returns LC_ERR_NO_DEVICE.
 *
 * DEFINED here, different from the reference:
 *   - A RECORD OF 4 GiB IS NOT WRITTEN.  An event whose record would reach 0xFFFFFFF0 bytes counts as "no record" (size 0 in
 *     rec_off).
 *   - A ROW OUTSIDE ITS LINE IS CUT.  A capture row that does not lie inside the line (begin >= the line's length, end beyond it,
 *     end < begin) is cut to the line, or is the empty value; lc_regex_match_device never writes such a row.
 *   - AN EVENT THAT IS NOT A LOG EVENT IS SKIPPED.  The reference casts every event of a group to the type of the first, which is
 *     undefined for a mixed group; here such events write nothing and the group takes the host path.
 *   - NO BYTES IS NOT AN ERROR.  The reference returns false with an EMPTY message for a group whose result is empty and with
 *     `empty event group` for a group without events; here both are LC_OK with *out_len == 0.
 * PINNED ON THE MODEL, not on the compiled reference: everything.  rapidjson is not part of the test environment, so the reference's
 * serializer is not compiled for the tests; the format above is held to the Python model of the tests (tests/helpers/jsonl_model.py),
 * written from the rules and not from this library's code.  The model's escape has one independent witness, CPython's json.dumps on
 * the latin-1 decoding (hex digits upper-cased), bytewise the same for every string without a NUL; every record is also parsed back
 * with json.loads.  THE NUL RULE and the order of the tags rest on reading the reference's source alone.
 * Kept as the reference has them (by that reading): everything in "The format" above.
 */
#ifndef LC_JSONL_H
#define LC_JSONL_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bounds of a plan: items per list, escaped bytes of all keys together; of a head */
#define LC_JSONL_MAX_ITEMS 256u
#define LC_JSONL_MAX_KEY_BYTES 65536u
#define LC_JSONL_MAX_HEAD_BYTES 65536u

/* lc_jsonl_processor_counters, own[] */
enum {
    LC_JSONL_CNT_GROUPS_DEVICE = 0, /* groups lc_jsonl_processor_serialize wrote on the device */
    LC_JSONL_CNT_GROUPS_HOST = 1,   /* groups it parsed and wrote on the host */
    LC_JSONL_CNT_FAILED_TRIPS = 2,  /* calls whose device trip failed */
    LC_JSONL_CNT_BYTES = 3,         /* bytes handed out */
    LC_JSONL_CNT_COUNT = 4
};

typedef struct lc_jsonl_plan lc_jsonl_plan_t;
typedef struct lc_jsonl_processor lc_jsonl_processor_t;

/* A plan says what an event becomes: a table of keys and two item lists, one for a line the parser matched (status LC_MATCH) and
 * one for every other line.  An item is the pair (key index, source) = two uint32: source 0 is the whole line, g >= 1 capture
 * group g.  An empty list means "no record" for those lines.  The plan holds, per item, the constant bytes `,"<key>":"` with the key
 * escaped and cut at its first NUL.
 * LC_ERR_UNSUPPORTED with a message in err: more than LC_JSONL_MAX_ITEMS items in a list, more than LC_JSONL_MAX_KEY_BYTES of
 * escaped keys.  LC_ERR_ARG: a key index outside the table, NULL where n > 0. */
int lc_jsonl_plan_create(const char* const* keys, const uint32_t* key_len, uint32_t n_keys, const uint32_t* matched_items, uint32_t n_matched,
                         const uint32_t* unmatched_items, uint32_t n_unmatched, lc_jsonl_plan_t** out, char* err, size_t errcap);
void lc_jsonl_plan_free(lc_jsonl_plan_t* plan);

/* The head of every record of a group, on the host: `{`, the n (key, value) pairs as `"k":"v",` in the map's order (above), escaped
 * and cut, then `"__time__":`.  Two equal keys are LC_ERR_ARG (a map holds none); a key that equals another only after the NUL cut
 * is kept, as the reference would write both.  Writes at most out_cap bytes to out; *out_len is the size needed.  LC_ERR_OVERFLOW
 * (nothing written) when that exceeds out_cap.  The encode entries take heads of 12 to LC_JSONL_MAX_HEAD_BYTES bytes. */
int lc_jsonl_head(const char* const* keys, const uint32_t* key_len, const char* const* values, const uint32_t* value_len, uint32_t n, uint8_t* out,
                  size_t out_cap, size_t* out_len);

/* bytes of d_scratch for n events under this plan: the scan's tile sums and, per event and item, two uint32 the size pass leaves for
 * the write pass */
size_t lc_jsonl_scratch_bytes(const lc_jsonl_plan_t* plan, uint32_t n);

/* The records of n events on what lc_regex_match_device left behind, on the current HIP device (the contract for d_data, d_off,
 * d_len, sep_bytes, d_caps = int32[n][2 * ngroups] and d_status is that entry's, lc_regex_gpu.h; reads touch the 16-byte units
 * around a value).  Status LC_MATCH takes the matched list, every other status byte the unmatched list.
 *   d_time       uint32[n], epoch seconds, written as they are
 *   d_head       head_len bytes of device memory, 4-byte aligned: lc_jsonl_head's bytes; 12 <= head_len <= LC_JSONL_MAX_HEAD_BYTES
 *   d_rec_off    uint64[n + 1]: where event i's record begins in d_out; d_rec_off[n] is the total; a record of size 0 repeats the
 *                offset.  Complete whatever out_cap is: it is what a batcher needs to cut at event borders.
 *   d_out        the records back to back.  Writes touch d_out[0 .. total) and nothing else; when the total exceeds out_cap NOT ONE
 *                byte is stored (read d_rec_off[n], come back with room).  d_out may be NULL with out_cap 0.
 *   d_scratch    lc_jsonl_scratch_bytes(plan, n) bytes, 8-byte aligned
 * Alignment: d_out 16 bytes, d_rec_off and d_scratch 8 bytes, d_time and d_head 4; anything else is refused with LC_ERR_ARG, as are
 * a head_len outside its bounds, a plan that names a group above ngroups, n >= 2^31 and a d_data that lives on another device than the
 * calling thread's current one.  n = 0 stores d_rec_off[0] = 0 and nothing else.  Without a device: LC_ERR_NO_DEVICE.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream), no host round trip -- except that a plan's first use on a
 * device uploads its tables (one synchronous copy of a few KiB). */
int lc_jsonl_encode_device(lc_jsonl_plan_t* plan, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t sep_bytes,
                           uint32_t n, uint32_t ngroups, const int32_t* d_caps, const uint8_t* d_status, const uint32_t* d_time,
                           const uint8_t* d_head, uint32_t head_len, uint8_t* d_out, uint64_t out_cap, uint64_t* d_rec_off, void* d_scratch,
                           size_t scratch_bytes, void* stream);

/* One trip on the calling thread's pinned staging, on the device the thread is bound to (lc_runtime_bind_thread): lines[i][0 ..
 * len[i]) and the head up (pulled by a kernel, no copy engine), lc_regex_match_device with `re`, the encode, the payload down.
 * Synchronous.
 *   time            as above, a host array
 *   head, head_len  lc_jsonl_head's bytes, host memory
 *   *out, *out_len  the records: a view into the thread's pinned block, valid until the thread's next lc_jsonl_* call
 *   rec_off         uint64[n + 1] back to the caller; may be NULL
 *   status          uint8[n] back to the caller: the matcher's status bytes (LC_GAVE_UP among them: the caller's counters need it)
 * No copy engine in the trip: the kernels store the total, the status bytes and the records into the thread's pinned block through its
 * mapping (rec_off, when asked for, is the one copy).  The payload's size is not known before the scan: the block has room for the bound
 * the plan gives for rows that do not overlap, with nothing added for escapes; where a batch exceeds it (reactive bytes, nested groups,
 * the line beside its groups) the write kernel has stored nothing, the host reads the total, grows the block and queues the write
 * kernel alone once more. */
int lc_jsonl_match_encode_host(lc_jsonl_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
                               const uint32_t* time, const uint8_t* head, uint32_t head_len, const uint8_t** out, size_t* out_len,
                               uint64_t* rec_off, uint8_t* status);

/* releases the calling thread's staging and stream of lc_jsonl_match_encode_host (they are also released when the thread ends) */
void lc_jsonl_thread_release(void);

/* processor_parse_regex_native + JsonEventGroupSerializer in one call.  config_json: processor_parse_regex_native's own
 * (lc_processor_create, lc_processor.h).  LC_ERR_UNSUPPORTED / LC_ERR_SYNTAX with a message in err as there. */
int lc_jsonl_processor_create(const char* config_json, lc_jsonl_processor_t** out, char* err, size_t errcap);
void lc_jsonl_processor_destroy(lc_jsonl_processor_t* p);
/* The bytes the reference produces when processor_parse_regex_native runs on the group and JsonEventGroupSerializer serializes the
 * log events that are left, the group's tags in front of each; the group itself is left untouched.  *out is a view into the calling
 * thread's block, valid until the thread's next lc_jsonl_* call; a result of no bytes is LC_OK with *out_len == 0.  *fused: 1 when the
 * device wrote the records (every event a log event holding exactly the SourceKey content, not the whole-line mode, distinct keys,
 * fewer than mark_count + 1, no alarm sink, no line left undecided, a plan within its bounds, a head within LC_JSONL_MAX_HEAD_BYTES),
 * 0 when the group was parsed by the parser's host code on a copy and written by the host writer.  An LC_ERR_* code when the
 * device trip failed: no *out then, the group is as before the call, LC_JSONL_CNT_FAILED_TRIPS grows and the events count under
 * LC_CNT_DEVICE_FAILED_EVENTS, as behind a failed trip of lc_processor_process. */
int lc_jsonl_processor_serialize(lc_jsonl_processor_t* p, lc_event_group_t* group, const uint8_t** out, size_t* out_len, int* fused);
/* The host writer alone: the log events of a group as they are (behind lc_processor_process, say), as JsonEventGroupSerializer
 * writes them.  *out is a view into the calling thread's block, valid until the thread's next lc_jsonl_* call. */
int lc_jsonl_serialize_group_host(lc_event_group_t* group, const uint8_t** out, size_t* out_len);
/* parse[]: the parser's counters in LC_CNT_* order (lc_processor.h; the instance-level entries are 0): after either path they are what
 * lc_processor_process leaves on the same group, LC_CNT_COMPLEXITY_EXCEEDED among them.  own[]: LC_JSONL_CNT_* */
int lc_jsonl_processor_counters(const lc_jsonl_processor_t* p, uint64_t parse[LC_CNT_COUNT], uint64_t own[LC_JSONL_CNT_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* LC_JSONL_H */
