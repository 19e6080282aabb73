/*
 * lc_apsara.h -- C ABI of the Apsara log parser: the MI355X replacement for processor_parse_apsara_native
 * ("[time]\t[LEVEL]\t[thread]\t[file:line]\tkey:value\tkey:value ...").
 *
 *   reference (core/plugin/processor/ProcessorParseApsaraNative.cpp)              this ABI
 *   --------------------------------------------------------------------------  ------------------------------------
 *   ApsaraEasyReadLogTimeParser without its cache (:251-323), FindBaseFields /   lc_apsara_parse_device / lc_apsara_parse_host
 *     ParseApsaraBaseFields (:342-463), the pair walk of ProcessEvent (:202-224)
 *   Init (:37-84)                                                                lc_apsara_processor_create
 *   Process / ProcessEvent / AddLog, the per-group time cache                    lc_apsara_processor_process
 *   the five plugin counters                                                     lc_apsara_processor_counters / _history_failures
 *   PARSE_TIME_FAIL_ALARM / OUTDATED_LOG_ALARM                                   lc_apsara_processor_set_alarm_sink
 *   time(NULL), ilogtail_discard_old_data / ilogtail_discard_interval            lc_apsara_processor_set_clock / _set_discard
 *
 * There is no CPU path for the parse: without a HIP device every entry point that would parse a line returns LC_ERR_NO_DEVICE.
 * Out of scope: the precise-timestamp key (the reference has it commented out) and the fused lc_pipeline_* path.
 */
#ifndef LC_APSARA_H
#define LC_APSARA_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"
#include "lc_timestamp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status byte of a line */
#define LC_APSARA_TIME_OK 0x01u  /* the line starts with '[', the time text matched and a ']' follows somewhere */
#define LC_APSARA_EPOCH 0x02u    /* byte 1 is '1': the "%s" form; secs is the epoch second, no zone applies.  Clear: the form
                                    "%Y-%m-%d %H:%M:%S", secs holds CIVIL seconds (the fields read as UTC) */
#define LC_APSARA_CANON19 0x04u  /* date form: the seconds format consumed exactly 19 bytes (the reference's cache is then unobservable) */

/* the four base fields, as indices into `base`: (begin, end) relative to the line's first byte; begin < 0: absent */
enum { LC_APSARA_LEVEL = 0, LC_APSARA_THREAD = 1, LC_APSARA_FILE = 2, LC_APSARA_LINE = 3 };

/* per-line results, structure of arrays; every array has n entries (pairs: n * W) */
typedef struct lc_apsara_out {
    uint8_t* status;
    int64_t* secs;
    uint32_t* nanos;   /* "%f" behind the seconds (one byte is skipped), or the tail of the epoch digits; 0: none */
    int32_t* base;     /* int32[n][4][2] */
    uint32_t* npairs;  /* the TRUE number of key:value pairs, also when it exceeds W */
    int32_t* pairs;    /* int32[n][W][3]: (key begin, colon, end) of the first min(npairs, W) pairs; entries at and behind
                          npairs are unspecified (the walk starts over at every base field that closes), nothing is written behind W */
} lc_apsara_out_t;

/* n lines that live in device memory on the current HIP device: line i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries; the
 * contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  Every line is parsed on its own: the reference's per-group
 * time cache is the processor's business.  base and pairs of a line without LC_APSARA_TIME_OK are unspecified but deterministic.
 * Alignment: d_out->base is written as 16-byte vectors and must be 16-byte aligned; secs 8-byte, nanos / npairs / pairs 4-byte aligned.
 * A pointer that is not is refused with LC_ERR_ARG.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream).  LC_ERR_ARG when d_data lives on another device than the calling
 * thread's current one. */
int lc_apsara_parse_device(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, const lc_apsara_out_t* d_out, void* stream);
/* The same for lines in host memory (line i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous. */
int lc_apsara_parse_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, const lc_apsara_out_t* out);

/* ---- the processor.  config_json: SourceKey (mandatory), Timezone ("GMT+08:00"; an invalid one is a warning and the offset stays 0)
 * and the keys of CommonParserOptions.  Non-zero (and the reference's message in err) wherever the reference's Init returns false.
 *
 * The reference's per-group cache (the 19 bytes behind '[' of the last date-form line that was parsed in full, and its second) is
 * unobservable while every date-form line's seconds format consumes exactly 19 bytes: such groups are stitched straight from the
 * device results.  From the first matched date-form line without LC_APSARA_CANON19 on, the rest of the group replays the reference's
 * cache walk on the host (lc_apsara_processor_replayed_lines counts those lines).  Two places where the reference reads memory it does
 * not own are DEFINED here: a time text shorter than the cached 19 bytes is no hit (IsPrefixString reads past its end), and a cache
 * taken from a line of fewer than 20 bytes never hits (the cached view runs past the line). */
typedef struct lc_apsara_processor lc_apsara_processor_t;
int lc_apsara_processor_create(const char* config_json, lc_apsara_processor_t** out, char* err, size_t errcap);
/* clock: what time(NULL) answers (NULL: the system's); Init resolves Timezone against it, the discard rule reads it per group */
int lc_apsara_processor_create_with_clock(const char* config_json, lc_clock_t clock, void* clock_user, lc_apsara_processor_t** out, char* err,
                                          size_t errcap);
void lc_apsara_processor_destroy(lc_apsara_processor_t* p);
/* one warning per line; malloc'ed, release with lc_free */
char* lc_apsara_processor_warnings(const lc_apsara_processor_t* p);
/* mLogTimeZoneOffsetSecond */
int32_t lc_apsara_processor_zone_offset(const lc_apsara_processor_t* p);
/* One event group, in place: gather -> one device trip (a second one for the lines with more pairs than the first kept) -> stitch.
 * 0, or an LC_ERR_* code when the device could not be used: the group is then left untouched, the events are counted under
 * LC_CNT_DEVICE_FAILED_EVENTS and the sink hears alarm kind 3. */
int lc_apsara_processor_process(lc_apsara_processor_t* p, lc_event_group_t* group);
int lc_apsara_processor_process_native(lc_apsara_processor_t* p, void* native_group);
void lc_apsara_processor_set_clock(lc_apsara_processor_t* p, lc_clock_t clock, void* user);
/* ilogtail_discard_old_data (default on) and ilogtail_discard_interval (default 43200) */
void lc_apsara_processor_set_discard(lc_apsara_processor_t* p, int discard_old_data, int32_t interval_seconds);
/* A test and tuning knob, not part of what the reference has: how many pairs per line the FIRST trip keeps (0, the default: 16).
 * The events that come out do not depend on it -- only how many lines take the second trip; the tests set it small to drive that
 * path.  Call before the first lc_apsara_processor_process. */
void lc_apsara_processor_set_first_trip_pairs(lc_apsara_processor_t* p, uint32_t pairs);
int lc_apsara_processor_counters(const lc_apsara_processor_t* p, uint64_t out[LC_CNT_COUNT]);
uint64_t lc_apsara_processor_history_failures(const lc_apsara_processor_t* p);
/* out[0]: lines whose time went through the host's replay of the cache walk; out[1]: lines that took the second trip */
void lc_apsara_processor_replayed_lines(const lc_apsara_processor_t* p, uint64_t out[2]);
/* kind 0: "<first 1024 bytes> $ <logTime>"; kind 1: "logTime: <sec>, log:<first 1024 bytes>"; kind 3: the device trip of a group failed */
void lc_apsara_processor_set_alarm_sink(lc_apsara_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
