/*
 * lc_delimiter.h -- C ABI of the delimiter parser: the MI355X replacement for processor_parse_delimiter_native
 * (CSV / TSV / '|'-separated lines, quote-aware).
 *
 *   reference                                                                   this ABI
 *   --------------------------------------------------------------------------  ------------------------------------
 *   DelimiterModeFsmParser(quote, separator) + the Separator / Quote / mode      lc_delim_create / lc_delim_destroy
 *     members of ProcessorParseDelimiterNative                                     core/plugin/processor/ProcessorParseDelimiterNative.cpp:45-109,141-172
 *   the trim, DelimiterModeFsmParser::ParseDelimiterLine, SplitString            lc_delim_split_device / lc_delim_split_host
 *     ProcessorParseDelimiterNative.cpp:220-282, :366-409
 *     core/parser/DelimiterModeFsmParser.cpp:49-113,134-154,172-186,201-223,260-294
 *   ProcessorParseDelimiterNative::Init                                          lc_delimiter_processor_create
 *     ProcessorParseDelimiterNative.cpp:30-184
 *   ProcessorParseDelimiterNative::Process / ProcessEvent / AddLog               lc_delimiter_processor_process
 *     ProcessorParseDelimiterNative.cpp:186-364, :411-419
 *   the plugin counters (:178-181)                                               lc_delimiter_processor_counters
 *   AlarmManager::SendAlarmWarning(PARSE_LOG_FAIL_ALARM, ...) (:292-318)         lc_delimiter_processor_set_alarm_sink
 *
 * There is no CPU path: without a HIP device every entry point that would split a line returns LC_ERR_NO_DEVICE.
 */
#ifndef LC_DELIMITER_H
#define LC_DELIMITER_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-line status.  LC_DELIM_BLANK is the failure the reference meets BEFORE it parses (:220-224, :239-242: an empty line, or nothing
 * left behind the trim): it counts the event as failed and passes it on untouched, while every other failure goes through the
 * source-key rules and raises an alarm -- so the two are told apart here. */
enum { LC_DELIM_FAIL = 0, LC_DELIM_OK = 1, LC_DELIM_BLANK = 2 };
/* OverflowedFieldsTreatment (ProcessorParseDelimiterNative.h: EXTEND, KEEP, DISCARD) */
enum { LC_DELIM_EXTEND = 0, LC_DELIM_KEEP = 1, LC_DELIM_DISCARD = 2 };
/* bit 31 of a span's `begin`: the column holds doubled quotes; its value is the span's bytes with every pair of quotes folded into
 * one (DelimiterModeFsmParser::AddFieldWithUnQuote :83-113), not a view of the line */
#define LC_DELIM_DOUBLED 0x80000000u

typedef struct lc_delim lc_delim_t;

/* separator: 1..4 bytes (:56-65).  quote: one byte.  The quote path (:251) runs when sep_len == 1 and quote != separator[0];
 * otherwise SplitString, which reads mode and n_keys: in keep / discard mode its walk stops once n_keys columns exist and the
 * remainder column begins AT the separator (:398-402).  LC_OK, or LC_ERR_ARG. */
int lc_delim_create(const uint8_t* separator, uint32_t sep_len, uint8_t quote, int mode, uint32_t n_keys, lc_delim_t** out);
void lc_delim_destroy(lc_delim_t* d);
/* 1: the quote-aware state machine, 0: SplitString */
int lc_delim_uses_quote(const lc_delim_t* d);

/* n lines that live in device memory on the current HIP device: line i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries;
 * the contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  Per line:
 *   d_status[i] : LC_DELIM_OK / LC_DELIM_BLANK (an empty or all-blank line) / LC_DELIM_FAIL (a quote inside an unquoted field,
 *                 data behind a closing quote, the end of the line inside a quote)
 *   d_ncols[i]  : the TRUE number of columns (0 for a failed line), also when it exceeds W
 *   d_spans     : int32[n][W][2], (begin, end) relative to the line's first byte of the first min(d_ncols[i], W) columns, behind the
 *                 trim of :226-238; bit 31 of begin = LC_DELIM_DOUBLED.  Entries at and behind d_ncols[i] are unspecified
 *                 (a line that fails half way has written the columns it had found).
 * A line with more than W columns is not finished anywhere else: the caller runs it again with W >= d_ncols[i] (the processor does,
 * in one mop-up trip per group).  Asynchronous on `stream` (hipStream_t, NULL = the default stream).
 * LC_ERR_ARG when d_data lives on another device than the calling thread's current one. */
int lc_delim_split_device(lc_delim_t* d, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status,
                          uint32_t* d_ncols, int32_t* d_spans, void* stream);
/* The same for lines in host memory (line i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous. */
int lc_delim_split_host(lc_delim_t* d, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status,
                        uint32_t* ncols, int32_t* spans);

/* ---- the processor.  config_json: the plugin's JSON object -- SourceKey, Separator (mandatory, at most 4 bytes, "\\t" = TAB), Quote
 * (one byte, default '"'; ignored with a warning under a multi-byte separator), Keys, AllowingShortenedFields,
 * OverflowedFieldsTreatment ("extend" | "keep" | "discard"), and the keys of CommonParserOptions (KeepingSourceWhenParseFail,
 * KeepingSourceWhenParseSucceed, RenamedSourceKey, CopingRawLog).  Non-zero (and the reference's message in err) wherever the
 * reference's Init returns false. */
typedef struct lc_delimiter_processor lc_delimiter_processor_t;
int lc_delimiter_processor_create(const char* config_json, lc_delimiter_processor_t** out, char* err, size_t errcap);
void lc_delimiter_processor_destroy(lc_delimiter_processor_t* p);
/* the warnings Init raised where the reference's PARAM_WARNING_* macros fire, one per line; malloc'ed, release with lc_free */
char* lc_delimiter_processor_warnings(const lc_delimiter_processor_t* p);
/* One event group, in place: gather -> one device trip (a second one for the lines with more columns than the first expected) ->
 * stitch.  0, or an LC_ERR_* code when the device could not be used: the group is then left untouched, the events are counted under
 * LC_CNT_DEVICE_FAILED_EVENTS and the sink hears alarm kind 3. */
int lc_delimiter_processor_process(lc_delimiter_processor_t* p, lc_event_group_t* group);
/* the same on a logtail::PipelineEventGroup* (what the plugin slot hands over; lc_group_native() of a fixture group) */
int lc_delimiter_processor_process_native(lc_delimiter_processor_t* p, void* native_group);
/* How many columns per line the FIRST trip keeps (0, the default: the reference's reserve, Keys.size() + 10 in extend mode, + 1
 * otherwise).  The events that come out do not depend on it -- only how many lines take the second trip; the tests set it small to
 * drive that path.  Call before the first lc_delimiter_processor_process. */
void lc_delimiter_processor_set_first_trip_columns(lc_delimiter_processor_t* p, uint32_t columns);
/* LC_CNT_* order (lc_processor.h); entries the delimiter parser does not have stay 0 */
int lc_delimiter_processor_counters(const lc_delimiter_processor_t* p, uint64_t out[LC_CNT_COUNT]);
/* kind 0: "parse delimiter log fail, logs:<line>"; kind 2: "keys count unmatch columns count :<n>, required:<k>, logs:<line>";
 * kind 4: "no column keys defined"; kind 3: the device trip of a group failed (no reference counterpart) */
void lc_delimiter_processor_set_alarm_sink(lc_delimiter_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
