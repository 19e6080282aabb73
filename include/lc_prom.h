/*
 * lc_prom.h -- C ABI of the Prometheus text-line parser: the MI355X replacement for processor_prom_parse_metric_native (one exposition
 * line per RawEvent -> one MetricEvent: name, labels, a double, a timestamp).
 *
 *   reference                                                                        this ABI
 *   -------------------------------------------------------------------------------  ------------------------------------
 *   TextParser::ParseLine, HandleStart .. HandleTimestamp, SkipLeadingWhitespace,    lc_prom_parse_device / _host
 *   IsValidNumberChar (core/prometheus/labels/TextParser.cpp:34-39, 69-335)
 *   StringTo<double> (core/common/StringTools.h:322-342)                             on the device where ONE rounded operation gives
 *                                                                                    strtod's answer; else LC_PROM_VALUE_HOST /
 *                                                                                    LC_PROM_TIME_HOST, finished by _host / the processor
 *   ProcessorPromParseMetricNative::Init (ProcessorPromParseMetricNative.cpp:19-25)  lc_prom_processor_create
 *   ScrapeConfig::InitStaticConfig (core/prometheus/schedulers/ScrapeConfig.cpp)
 *   Process / ProcessEvent (:27-66)                                                  lc_prom_processor_process
 *
 * There is no CPU path for the parse: without a HIP device every entry point that would parse a line returns LC_ERR_NO_DEVICE.
 * Out of scope: processor_prom_relabel_metric_native (relabel configs are ACCEPTED and IGNORED by lc_prom_processor_create: the
 * reference compiles them in InitStaticConfig and refuses a bad one; this processor never reads them), "# HELP" / "# TYPE" / exemplars
 * (the scraper filters comment lines; a '#' line fails here as in the reference), the fused lc_pipeline_* path, and numbers that need
 * more than one rounded operation on the device (they are finished on the host).
 *
 * DEFINED here, undefined in the reference:
 *   - a backslash as the line's last byte inside a label value: the reference reads one byte behind its view (:196) and then fails
 *     with "unexpected end of input in label value".  The byte read does not change the result; it is not read here:
 *     LC_PROM_FAIL_LABEL_VALUE_END.
 *   - a timestamp token that converts to NaN ("nan", "-NaN"): the reference casts NaN to int64_t (:308).  Here the line fails with
 *     LC_PROM_FAIL_TIMESTAMP_NAN.
 *   - a timestamp outside [-2^63, 2^63) after the multiplication (:308, the same cast): on x86-64 the cast gives INT64_MIN and the
 *     line fails with "invalid timestamp"; here LC_PROM_FAIL_TIMESTAMP_SMALL, by definition.
 * The reference's "expected ',' or '}' after label value" (:236) cannot fire: HandleCommaOrCloseBrace is entered only on one of the two
 * bytes.  Its status exists for completeness and is never reported.  The empty timestamp token (:287) cannot occur either.
 */
#ifndef LC_PROM_H
#define LC_PROM_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status byte of a line: OK or the HandleError site that ended it (TextParser.cpp line in brackets) */
enum {
    LC_PROM_OK = 0,
    LC_PROM_FAIL_NAME = 1,              /* "expected metric name" [92] */
    LC_PROM_FAIL_NAME_END = 2,          /* "error end of metric name" [116] */
    LC_PROM_FAIL_EQUAL = 3,             /* "expected '=' after label name" [133] */
    LC_PROM_FAIL_LABEL_NAME = 4,        /* "invalid character in label name" [144] */
    LC_PROM_FAIL_QUOTE = 5,             /* "expected '\"' after '='" [154] */
    LC_PROM_FAIL_LABEL_VALUE_END = 6,   /* "unexpected end of input in label value" [203]: no closing quote */
    LC_PROM_FAIL_LABEL_VALUE_NEXT = 7,  /* "unexpected end of input in label value" [219]: neither ',' nor '}' behind the value */
    LC_PROM_FAIL_COMMA_OR_BRACE = 8,    /* "expected ',' or '}' after label value" [236]: unreachable, never reported */
    LC_PROM_FAIL_VALUE_END = 9,         /* "unexpected end of input in sample value" [248] */
    LC_PROM_FAIL_VALUE = 10,            /* "invalid sample value" [256] */
    LC_PROM_FAIL_TIME_END = 11,         /* "unexpected end of input in sample timestamp" [282] */
    LC_PROM_FAIL_TIMESTAMP = 12,        /* "invalid timestamp" [294]: the token is no number */
    LC_PROM_FAIL_TIMESTAMP_OVERFLOW = 13, /* "timestamp overflow" [301] */
    LC_PROM_FAIL_TIMESTAMP_SMALL = 14,  /* "invalid timestamp" [313]: fewer than 10^9 seconds */
    LC_PROM_FAIL_TIMESTAMP_NAN = 15     /* DEFINED here (see above) */
};
/* flag bits of a line */
#define LC_PROM_VALUE_HOST 0x01u /* the value token [value_span) was NOT decided on the device: std::strtod + the reference's checks decide */
#define LC_PROM_TIME_HOST 0x02u  /* the same for the timestamp token [time_span) */
#define LC_PROM_HAS_TIME 0x04u   /* secs / nanos hold the line's own timestamp (else the caller's default applies) */
#define LC_PROM_ANY_ESCAPE 0x08u /* a label value holds a backslash */

/* the escaped bit of a label: the sign bit of its value-begin field (labels[..][2]) */
#define LC_PROM_LABEL_ESCAPED 0x80000000u
#define LC_PROM_DEFAULT_LABELS 16u

/* per-line results, structure of arrays, n entries each; every span is (begin, end) relative to the line's first byte */
typedef struct lc_prom_out {
    uint8_t* status;
    uint8_t* flags;
    int32_t* name;       /* int32[n][2] */
    uint64_t* value;     /* the IEEE double's bits; 0 while LC_PROM_VALUE_HOST is set, and for a failed line */
    int32_t* value_span; /* int32[n][2]: the value token (every line that reached it) */
    int32_t* time_span;  /* int32[n][2]: the timestamp token, (0, 0) without one */
    int64_t* secs;       /* with LC_PROM_HAS_TIME */
    uint32_t* nanos;
    uint32_t* nlabels;   /* the TRUE number of labels the line held up to where it ended, also above W */
    int32_t* labels;     /* int32[n][W][4]: name begin, name end, value begin | LC_PROM_LABEL_ESCAPED, value end -- the RAW span of the value
                            between its quotes.  Only the first min(nlabels, W) entries of a line are written.  Duplicates are reported
                            as they stand; SizedVectorTags::Insert is the stitch's business. */
} lc_prom_out_t;

/* n lines that live in device memory on the current HIP device: line i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries; the
 * contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  prom_parse_kernel, one line per lane.
 * W: labels kept per line (0: none; labels may then be NULL).
 * Alignment: labels is written as 16-byte vectors and must be 16-byte aligned; name, value, value_span, time_span and secs 8-byte;
 * nanos and nlabels 4-byte.  A pointer that is not is refused with LC_ERR_ARG.  n = 0 returns LC_OK and touches nothing.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream).  LC_ERR_ARG when d_data lives on another device than the calling
 * thread's current one.  Tokens flagged LC_PROM_VALUE_HOST / LC_PROM_TIME_HOST are the caller's to finish. */
int lc_prom_parse_device(int honor_timestamps, const uint8_t* d_data, const int32_t* d_off, uint32_t n, const lc_prom_out_t* d_out, uint32_t W,
                         void* stream);
/* The same for lines in host memory (line i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous.  The deferred tokens are finished before it returns (std::strtod, whole
 * token, no ERANGE; the timestamp rules of :300-316): the flags LC_PROM_VALUE_HOST / LC_PROM_TIME_HOST stay set as a record,
 * status / value / secs / nanos / LC_PROM_HAS_TIME are final.  *deferred_tokens (may be NULL): how many tokens that were. */
int lc_prom_parse_host(int honor_timestamps, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const lc_prom_out_t* out, uint32_t W,
                       uint64_t* deferred_tokens);

/* ---- the processor.  config_json: the keys ScrapeConfig::InitStaticConfig reads that bear on this processor: job_name (string,
 * required, non-empty), honor_timestamps (bool, default true).  Refused as in the reference: a config that is no object, job_name
 * missing / no string / empty, and scrape_interval / scrape_timeout (durations: "15s", "1m") or max_scrape_size (sizes: "10MB") that
 * parse to 0.  relabel_configs / metric_relabel_configs and every other key are accepted and ignored. */
typedef struct lc_prom_processor lc_prom_processor_t;
int lc_prom_processor_create(const char* config_json, lc_prom_processor_t** out, char* err, size_t errcap);
void lc_prom_processor_destroy(lc_prom_processor_t* p);
/* one warning per line; malloc'ed, release with lc_free */
char* lc_prom_processor_warnings(const lc_prom_processor_t* p);
void lc_prom_processor_set_config_name(lc_prom_processor_t* p, const char* name);
/* One event group: every RawEvent's content is parsed (one device trip, a second one for the lines with more labels than the first
 * kept); a line that parses becomes a MetricEvent (labels in order, "__name__" set last), a line that fails leaves no event, every
 * event that is no RawEvent is dropped; order is kept.  The default timestamp is the group's PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC
 * metadata (unparsable: 0, and alarm kind 1 "parse scrape timestamp failed").  A failed line raises no alarm (the reference only logs).
 * 0, or an LC_ERR_* code when the device could not be used: the group is then left untouched, the events are counted under
 * LC_CNT_DEVICE_FAILED_EVENTS and the sink hears alarm kind 3. */
int lc_prom_processor_process(lc_prom_processor_t* p, lc_event_group_t* group);
int lc_prom_processor_process_native(lc_prom_processor_t* p, void* native_group);
/* LC_CNT_* order; failed lines are LC_CNT_OUT_FAILED_EVENTS, metric events LC_CNT_OUT_SUCCESSFUL_EVENTS, dropped non-raw events
 * LC_CNT_DISCARDED_EVENTS */
int lc_prom_processor_counters(const lc_prom_processor_t* p, uint64_t out[LC_CNT_COUNT]);
/* value or timestamp tokens the host finished with std::strtod */
uint64_t lc_prom_processor_deferred_tokens(const lc_prom_processor_t* p);
/* lines that took the second trip (more labels than the first trip kept) */
uint64_t lc_prom_processor_mop_up_lines(const lc_prom_processor_t* p);
/* test knob: labels the first trip keeps per line (default LC_PROM_DEFAULT_LABELS; 0 is taken as 1) */
void lc_prom_processor_set_first_trip_labels(lc_prom_processor_t* p, uint32_t W);
void lc_prom_processor_set_alarm_sink(lc_prom_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
