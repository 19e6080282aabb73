/*
 * lc_json.h -- C ABI of the JSON parser: the MI355X replacement for processor_parse_json_native (one JSON object per event, every
 * top-level member becomes a content).
 *
 *   reference                                                                   this ABI
 *   --------------------------------------------------------------------------  ------------------------------------
 *   parser.iterate / doc.get_object / the member loop of                        lc_json_walk_device / lc_json_walk_host
 *     ProcessorParseJsonNative::JsonLogLineParserSimdJson
 *     core/plugin/processor/ProcessorParseJsonNative.cpp:252-377
 *     (unescaped_key :319, the value's kind :193-238, the integer test :157-173)
 *   ProcessorParseJsonNative::Init                                              lc_json_processor_create
 *     ProcessorParseJsonNative.cpp:44-84
 *   ProcessorParseJsonNative::Process / ProcessEvent / AddLog                   lc_json_processor_process
 *     ProcessorParseJsonNative.cpp:87-145, :469-477
 *   OptimizedValueToStringBuffer / ProcessNumberValueOptimized (:150-238)       the stitch of lc_json_processor_process
 *   the plugin counters (:78-81)                                                lc_json_processor_counters
 *   AlarmManager::SendAlarmWarning(PARSE_LOG_FAIL_ALARM, ...) (:278-283)        lc_json_processor_set_alarm_sink
 *
 * Which documents are valid and how values are rendered is fixed by tests/golden/README_json.md (strict RFC 8259 over valid UTF-8,
 * the whole document validated, rendering as the simdjson branch does it).
 * There is no CPU path: without a HIP device every entry point that would walk a line returns LC_ERR_NO_DEVICE.
 */
#ifndef LC_JSON_H
#define LC_JSON_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-line status.  LC_JSON_EMPTY is a line of length 0: the reference answers "failed" for it BEFORE it parses, without a counter
 * and without an alarm (:259).  LC_JSON_DEEP is what the first launch says of a line nested deeper than the 64 levels it keeps in
 * registers; both entry points below finish such lines with a second launch, so a caller of theirs never sees it. */
enum { LC_JSON_FAIL = 0, LC_JSON_OK = 1, LC_JSON_EMPTY = 2, LC_JSON_DEEP = 3 };
/* a member's value */
enum { LC_JSON_STRING = 0, LC_JSON_INT = 1, LC_JSON_DOUBLE = 2, LC_JSON_TRUE = 3, LC_JSON_FALSE = 4, LC_JSON_NULL = 5, LC_JSON_OBJECT = 6,
       LC_JSON_ARRAY = 7 };
/* bit 31 of key_begin / val_begin: the text has escapes.  Its unescaped bytes stand in the shadow buffer at the span's own offset, and
 * the span's end is begin + the UNESCAPED length */
#define LC_JSON_ESCAPED 0x80000000u
/* the deepest nesting a valid document may have (the root object is level 1) */
#define LC_JSON_MAX_DEPTH 1024u

/* one top-level member.  Spans are (begin, end) relative to the line's first byte; a string's span lies inside its quotes.
 *   STRING            the text (unescaped in the shadow buffer when LC_JSON_ESCAPED is set)
 *   INT               an integer literal that fits int64 (negative) or uint64: its digits as written; "-0" points at the "0"
 *   DOUBLE            every other number (an integer literal that does not fit among them): the literal as written
 *   TRUE FALSE NULL   the literal
 *   OBJECT ARRAY      the raw text from the opening to the closing bracket */
typedef struct lc_json_member {
    uint32_t key_begin, key_end, val_begin, val_end;
    uint8_t type, reserved[3];
} lc_json_member_t;

/* n lines that live in device memory on the current HIP device: line i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries;
 * the contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  Per line:
 *   d_status[i]   : LC_JSON_OK / LC_JSON_FAIL / LC_JSON_EMPTY
 *   d_nmembers[i] : the TRUE number of top-level members (0 unless OK), also when it exceeds W
 *   d_errpos[i]   : for a failed line the offset of the first byte that cannot continue a valid document (the line's length when it
 *                   ends too early); 0 otherwise
 *   d_records     : lc_json_member_t[n][W], the first min(d_nmembers[i], W) members in document order.  Entries behind them are
 *                   unspecified (a line that fails half way has written the members it had found).
 *   d_shadow      : as many bytes as d_data.  The unescaped bytes of every LC_JSON_ESCAPED span of line i stand at
 *                   d_shadow[d_off[i] + begin ..); every other byte of it is unspecified.
 * A line with more than W members is not finished anywhere else: the caller runs it again with W >= d_nmembers[i].
 * Two launches on `stream` (hipStream_t, NULL = the default stream): json_walk_kernel, then the same walk with a 1024-level nesting
 * stack in device scratch for the lines the first one left as LC_JSON_DEEP (nothing to do for a batch without such lines).
 * Asynchronous, with one exception: the FIRST call on a (device, stream) pair allocates the second launch's scratch (2 MiB, hipMalloc
 * under a process-wide lock), so make that call outside a stream capture.  The block is kept for that stream for the life of the
 * process (a later stream that gets the same handle value reuses it; a runner thread's own stream frees its block at
 * lc_thread_release).  The second launch costs 0.03 ms per call on a batch of 1 Mi lines without deep lines (profiles/json_bench.json).
 * LC_ERR_ARG when d_data lives on another device than the calling thread's current one. */
int lc_json_walk_device(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_nmembers,
                        uint32_t* d_errpos, lc_json_member_t* d_records, uint8_t* d_shadow, void* stream);
/* The same for lines in host memory (line i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous.  shadow: sum(len) bytes, line i's part begins at len[0] + .. + len[i-1];
 * only the bytes of LC_JSON_ESCAPED spans are written, and only those come back from the device: *shadow_bytes_moved (may be NULL)
 * is the number of bytes that did -- 0 for a batch without escapes. */
int lc_json_walk_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* nmembers,
                      uint32_t* errpos, lc_json_member_t* records, uint8_t* shadow, uint64_t* shadow_bytes_moved);

/* ---- the processor.  config_json: the plugin's JSON object -- SourceKey (mandatory) and the keys of CommonParserOptions
 * (KeepingSourceWhenParseFail, KeepingSourceWhenParseSucceed, RenamedSourceKey, CopingRawLog).  Non-zero (and the reference's message
 * in err) wherever the reference's Init returns false. */
typedef struct lc_json_processor lc_json_processor_t;
int lc_json_processor_create(const char* config_json, lc_json_processor_t** out, char* err, size_t errcap);
void lc_json_processor_destroy(lc_json_processor_t* p);
/* the warnings Init raised where the reference's PARAM_WARNING_* macros fire, one per line; malloc'ed, release with lc_free */
char* lc_json_processor_warnings(const lc_json_processor_t* p);
/* One event group, in place: gather -> one device trip (a second one for the lines with more members than the first kept) -> stitch.
 * 0, or an LC_ERR_* code when the device could not be used: the group is then left untouched, the events are counted under
 * LC_CNT_DEVICE_FAILED_EVENTS and the sink hears alarm kind 3. */
int lc_json_processor_process(lc_json_processor_t* p, lc_event_group_t* group);
/* the same on a logtail::PipelineEventGroup* (lc_group_native() of a fixture group) */
int lc_json_processor_process_native(lc_json_processor_t* p, void* native_group);
/* How many members per line the FIRST trip keeps (0, the default: 32, the reference's tempFields.reserve(32), :309).  The events that
 * come out do not depend on it -- only how many lines take the second trip; the tests set it small to drive that path. */
void lc_json_processor_set_first_trip_members(lc_json_processor_t* p, uint32_t members);
/* LC_CNT_* order (lc_processor.h); entries the JSON parser does not have stay 0 */
int lc_json_processor_counters(const lc_json_processor_t* p, uint64_t out[LC_CNT_COUNT]);
/* kind 0: "parse json fail:<line>"; kind 3: the device trip of a group failed (no reference counterpart) */
void lc_json_processor_set_alarm_sink(lc_json_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
