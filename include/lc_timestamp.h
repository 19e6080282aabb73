/*
 * lc_timestamp.h -- C ABI of the timestamp parser: the MI355X replacement for processor_parse_timestamp_native.
 *
 *   reference                                                                   this ABI
 *   --------------------------------------------------------------------------  ------------------------------------
 *   strptime_ns(buf, fmt, tm, &nanosecond, &nanosecondLength)                    lc_strptime_create (the format, compiled once)
 *     core/common/Strptime.cpp                                                   lc_strptime_parse_spans_device / _captures_device /
 *                                                                                lc_strptime_parse_host (n values per call)
 *   Strptime(): mktime, the three year modes, DeduceYear  core/common/TimeUtil.cpp   the processor (host): lc_timestamp_zone_seconds
 *   ProcessorParseTimestampNative::Init                                          lc_timestamp_processor_create
 *   ProcessorParseTimestampNative::Process / ProcessEvent / ParseLogTime         lc_timestamp_processor_process
 *   the five plugin counters                                                     lc_timestamp_processor_counters
 *   PARSE_TIME_FAIL_ALARM / OUTDATED_LOG_ALARM                                   lc_timestamp_processor_set_alarm_sink
 *   time(NULL)                                                                   lc_timestamp_processor_set_clock
 *
 * There is no CPU path for the parse: without a HIP device every entry point that would parse a value returns LC_ERR_NO_DEVICE.
 * processor_parse_apsara_native is lc_apsara.h.  Out of scope: the reference's commented-out precise-timestamp key, locales other than C, and the
 * fused lc_pipeline_* path (it does not call this processor).
 */
#ifndef LC_TIMESTAMP_H
#define LC_TIMESTAMP_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of a value's status byte */
#define LC_TS_OK 0x01u       /* the format matched */
#define LC_TS_HAS_YEAR 0x02u /* the format delivered a year: secs = civil seconds (the broken-down fields read as UTC, normalised the way
                                mktime normalises).  Clear: secs = month (0..11) << 40 | day of month << 32 | second of the day, and the
                                caller supplies the year */
#define LC_TS_DST 0x04u      /* the value left tm_isdst = 1 behind (%z with EDT / CDT / MDT / PDT): mktime reads it */
#define LC_TS_EPOCH 0x08u    /* the format is "%s": secs is the epoch second, no zone applies */
#define LC_TS_ABSENT 0x80u   /* capture-table entry: the line did not match, or the group did not take part; nothing else is set */
/* A value that FAILS still reports secs (and LC_TS_HAS_YEAR / LC_TS_DST) from the fields it had set when it failed: the reference's
 * Strptime() runs mktime on them and leaves the result in the caller's LogtailTime, where a later cache hit of the same group finds it. */

#define LC_TS_MAX_PROGRAM 64 /* steps a compiled format may have (the kernel's program window) */

typedef struct lc_strptime lc_strptime_t;
/* per-value results, one array each (device pointers for the *_device entries, host pointers for lc_strptime_parse_host) */
typedef struct lc_ts_out {
    uint8_t* status;        /* [n] LC_TS_* bits */
    int64_t* secs;          /* [n] */
    uint32_t* nanos;        /* [n] %f scaled to nanoseconds in the reference's unsigned 32-bit arithmetic (more than nine digits wrap) */
    int32_t* matched;       /* [n] bytes the format consumed; 0 for a failed value */
    int32_t* frac_len;      /* [n] digits %f (or the tail of a "%s" value) consumed; 0: none */
    uint8_t* same_as_prev;  /* [n] 1: value i and value i - 1 both matched and their matched prefixes (matched - frac_len bytes) are equal */
} lc_ts_out_t;

/* Compiles `format` (SourceFormat; strptime_ns's conversions, composite ones expanded).  LC_ERR_UNSUPPORTED, with the reason in err,
 * for a format whose program exceeds LC_TS_MAX_PROGRAM steps.  A format the reference fails on every value compiles, and fails alike. */
int lc_strptime_create(const char* format, lc_strptime_t** out, char* err, size_t errcap);
void lc_strptime_destroy(lc_strptime_t* t);
/* the compiled program's words (csrc/strptime_vm.hpp); returns their number */
uint32_t lc_strptime_program(const lc_strptime_t* t, uint32_t words[LC_TS_MAX_PROGRAM]);

/* n values in device memory on the current HIP device: value i = d_data[d_off[i] + d_spans[2i] .. d_off[i] + d_spans[2i + 1]).  d_off
 * holds at least n line offsets (the parsers' d_off); the contract for d_data is the one of lc_regex_match_device.  A span with a
 * negative begin is reported LC_TS_ABSENT.  Asynchronous on `stream`. */
int lc_strptime_parse_spans_device(lc_strptime_t* t, const uint8_t* d_data, const uint32_t* d_off, const int32_t* d_spans, uint32_t n,
                                   const lc_ts_out_t* d_out, void* stream);
/* The same over a capture table still in device memory -- the d_caps / d_status of lc_regex_match_device (int32[n][2 * ngroups],
 * value = group `group`, present where d_line_status[i] == LC_MATCH) or the d_spans / d_status of lc_delim_split_device (ngroups = W,
 * group = the column, match_value = LC_DELIM_OK; a doubled-quote column is reported LC_TS_ABSENT).  No host round trip in between:
 * queue it on the parser's stream. */
int lc_strptime_parse_captures_device(lc_strptime_t* t, const uint8_t* d_data, const uint32_t* d_off, const int32_t* d_caps,
                                      uint32_t ngroups, uint32_t group, const uint8_t* d_line_status, uint32_t match_value, uint32_t n,
                                      const lc_ts_out_t* d_out, void* stream);
/* n values in host memory (value i = vals[i][0 .. len[i])), through the calling thread's pinned staging, one trip.  Synchronous. */
int lc_strptime_parse_host(lc_strptime_t* t, const uint8_t* const* vals, const uint32_t* len, uint32_t n, const lc_ts_out_t* out);

/* mktime() of civil seconds in the process's local zone (tm_isdst = dst, 0 or 1), through the per-day offset cache the processor uses:
 * a day without a transition costs one lookup, a day with one goes through mktime itself. */
int64_t lc_timestamp_zone_seconds(int64_t civil_seconds, int dst);
/* forget the cache (after the process changed TZ and called tzset) */
void lc_timestamp_zone_reset(void);

/* ---- the processor.  config_json: SourceKey, SourceFormat (mandatory), SourceTimezone ("GMT+08:00"), SourceYear.  Non-zero (and the
 * reference's message in err) wherever the reference's Init returns false; LC_ERR_UNSUPPORTED for a format beyond the program window. */
typedef struct lc_timestamp_processor lc_timestamp_processor_t;
int lc_timestamp_processor_create(const char* config_json, lc_timestamp_processor_t** out, char* err, size_t errcap);
void lc_timestamp_processor_destroy(lc_timestamp_processor_t* p);
char* lc_timestamp_processor_warnings(const lc_timestamp_processor_t* p); /* one per line; lc_free */
/* the offset Init derived from SourceTimezone (mLogTimeZoneOffsetSecond) */
int32_t lc_timestamp_processor_zone_offset(const lc_timestamp_processor_t* p);
int lc_timestamp_processor_process(lc_timestamp_processor_t* p, lc_event_group_t* group);
int lc_timestamp_processor_process_native(lc_timestamp_processor_t* p, void* native_group);
/* "now" for the year deduction and the discard rule: clock(user) in epoch seconds; NULL = time().  Init resolves SourceTimezone
 * against the local offset at "now" too (GetLocalTimeZoneOffsetSecond): lc_timestamp_processor_create reads time() for that,
 * lc_timestamp_processor_create_with_clock the clock it is given, which then stays the processor's clock. */
typedef int64_t (*lc_clock_t)(void* user);
int lc_timestamp_processor_create_with_clock(const char* config_json, lc_clock_t clock, void* clock_user, lc_timestamp_processor_t** out,
                                             char* err, size_t errcap);
void lc_timestamp_processor_set_clock(lc_timestamp_processor_t* p, lc_clock_t clock, void* user);
/* the agent's flags ilogtail_discard_old_data (default 1) and ilogtail_discard_interval (default 43200), and whether the pipeline is a
 * one-time one (default 0) */
void lc_timestamp_processor_set_discard(lc_timestamp_processor_t* p, int discard_old_data, int32_t interval_seconds, int onetime);
/* 1: walk every value on the host instead of only run heads (same results; the tests compare the two) */
void lc_timestamp_processor_set_plain_walk(lc_timestamp_processor_t* p, int on);
/* values the host walked byte-wise / values that took their result from a same_as_prev run, since create */
void lc_timestamp_processor_walk_stats(const lc_timestamp_processor_t* p, uint64_t out[2]);
/* LC_CNT_* order; LC_CNT_DISCARDED_EVENTS counts what the history rule dropped (the reference counts each under history_failure_total too) */
int lc_timestamp_processor_counters(const lc_timestamp_processor_t* p, uint64_t out[LC_CNT_COUNT]);
uint64_t lc_timestamp_processor_history_failures(const lc_timestamp_processor_t* p);
/* kind 0: PARSE_TIME_FAIL_ALARM "<value> <format>"; kind 1: OUTDATED_LOG_ALARM "logTime: <sec>"; kind 3: the device trip failed */
void lc_timestamp_processor_set_alarm_sink(lc_timestamp_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
