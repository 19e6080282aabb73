/*
 * lc_csv.h -- C ABI of the CSV decoder: the MI355X replacement for the Go plugin processor_csv (one value such as
 * `12,34,"a ""quoted"" field, with a comma"` -> its fields, named by SplitKeys and appended to the log).
 *
 *   reference (plugins/processor/csv/processor_csv.go)                              this ABI
 *   -----------------------------------------------------------------------------  ------------------------------------
 *   r.Read() of encoding/csv (Go 1.23) with Comma = sep, TrimLeadingSpace as        lc_csv_device / lc_csv_host
 *   configured, LazyQuotes = false, Comment = 0: the FIRST record, or an error      (csv_split_kernel, one value per lane)
 *   Init :46-54 ([]rune(SplitSep) must hold exactly one rune)                       lc_csv_create
 *   ProcessLogs / decodeCSV :60-134: SplitKeys, PreserveOthers, ExpandOthers,       lc_csv_process_logs_json
 *   the csv.Writer remainder, KeepSource, the three alarm sites                     (applied on the host to the engine's rows)
 *
 * The entry points live in a library of their own, liblc_csv.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error), beside liblc_kvsplit.so; this header is include/csv/lc_csv.h.  The ABI of liblc_regex_gpu.so, the one of
 * liblc_kvsplit.so and the headers of include/ do not change.
 *
 * This is NOT the delimiter parser of lc_delimiter.h (DelimiterModeFsmParser): the separator is one rune of 1 to 4 bytes, quoted
 * fields may hold line ends (`\r\n` inside becomes `\n`), leading empty lines are skipped, text behind the first record is ignored,
 * TrimLeadingSpace trims Unicode white space, a `"` inside an unquoted field is an error.
 *
 * There is no CPU path for the decode: without a HIP device every entry point that would read a value returns LC_ERR_NO_DEVICE.
 *
 * DEFINED here, different from the reference:
 *   - NO ERROR POSITIONS.  Go's ParseError prints `parse error on line L, column C: <sentence>`.  The alarm of an error value
 *     carries the sentence alone (`bare " in non-quoted-field` / `extraneous or missing " in quoted-field`): the engine reports a
 *     status byte, not a line and a column.
 *   - THE FOLD IS ON THE HOST.  A field's span whose begin has bit 31 set is not a view of the value: it is the text between the
 *     field's quotes, in which `""` stands for `"` and `\r\n` for `\n`.  The processor folds such a field on the host (rare); a
 *     caller of the engine entries does the same (the bit's convention is the one of lc_delimiter.h).
 *   - a value of 2 GiB or more is refused (LC_ERR_ARG); offsets and spans are int32.
 * Kept as the reference has them: only the first record, the empty record `[""]` for a value that holds no record (io.EOF), the
 * skip of empty lines BEFORE any trimming, one `\r` dropped before a `\n` and at the value's end, a separator of `"`, `\r`, `\n`,
 * U+0000 or U+FFFD accepted by Init and failing every value with `csv: invalid field or comment delimiter`.
 */
#ifndef LC_CSV_H
#define LC_CSV_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of one value */
enum {
    LC_CSV_OK = 0,         /* a record: count >= 1 fields */
    LC_CSV_EOF = 1,        /* io.EOF: nothing but empty lines; zero fields (the processor makes the record [""] of it) */
    LC_CSV_BARE_QUOTE = 2, /* bare " in non-quoted-field */
    LC_CSV_QUOTE = 3       /* extraneous or missing " in quoted-field */
};
/* bit 31 of a span's begin: the field's text has to be folded (`""` -> `"`, `\r\n` -> `\n`) */
#define LC_CSV_FOLD 0x80000000u
/* with PreserveOthers the first trip keeps len(SplitKeys) + LC_CSV_PRESERVE_EXTRA fields per value */
#define LC_CSV_PRESERVE_EXTRA 16u

/* alarm kinds of lc_csv_set_alarm_sink; the texts are what the Go's logger.Warning writes (key:value pairs, each closed by a tab) */
enum {
    LC_CSV_ALARM_NO_SOURCE_KEY = 1, /* "cannot find key:<SourceKey>\t"                                        NoKeyError */
    LC_CSV_ALARM_DECODE = 2,        /* "cannot decode log:<sentence>\tlog:<value, cut at 1024 bytes>\t" */
    LC_CSV_ALARM_KEY_COUNT = 3,     /* "decode keys not match, split len:<count>\tlog:<value, cut at 1024 bytes>\t" */
    LC_CSV_ALARM_TRIP_FAILED = 4    /* the device trip failed: every log of the batch is left unchanged */
};
/* lc_csv_counters order */
enum {
    LC_CSV_CNT_VALUES = 0,        /* values read (one per log that holds the source key, SplitKeys not empty) */
    LC_CSV_CNT_FIELDS = 1,        /* contents appended */
    LC_CSV_CNT_DECODE_ERRORS = 2, /* values with an error status (or an invalid delimiter) */
    LC_CSV_CNT_EOF = 3,           /* values with LC_CSV_EOF */
    LC_CSV_CNT_KEY_COUNT = 4,     /* values whose field count is not len(SplitKeys) */
    LC_CSV_CNT_NO_SOURCE_KEY = 5, /* logs without the source key */
    LC_CSV_CNT_MOP_UP = 6,        /* values that took the second trip (more fields needed than the first trip kept) */
    LC_CSV_CNT_FAILED_TRIPS = 7,
    LC_CSV_CNT_COUNT = 8
};

typedef struct lc_csv lc_csv_t;

/* config_json: the Go struct's fields:
 *   {"SourceKey": "", "NoKeyError": false, "SplitKeys": [], "SplitSep": ",", "TrimLeadingSpace": false, "PreserveOthers": false,
 *    "ExpandOthers": false, "ExpandKeyPrefix": "", "KeepSource": false}
 * LC_ERR_UNSUPPORTED with a message in err: no JSON object, or a SplitSep that is not exactly one rune (`invalid separator:
 * <SplitSep>`, the Go's).  A SplitSep of `"`, `\r`, `\n`, U+0000 or U+FFFD is ACCEPTED, as by the plugin's Init; the handle remembers
 * that every Read fails: the processor fails every value without a trip, the engine entries return LC_ERR_UNSUPPORTED. */
int lc_csv_create(const char* config_json, size_t config_len, lc_csv_t** out, char* err, size_t errcap);
void lc_csv_free(lc_csv_t* p);

/* n values that live in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries;
 * the contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  csv_split_kernel, one value per lane.
 * fields: int32[n][W][2] = begin, end of a field, relative to the value's first byte; for a quoted field the text between its quotes,
 *   with LC_CSV_FOLD set in begin where that text has to be folded.
 * count: the TRUE field count, also above W; only the first min(count, W) rows of a value are written.  W = 0 is allowed, fields
 *   may then be NULL.  status: LC_CSV_*; count and rows of an error value are unspecified, LC_CSV_EOF has count 0.
 * Alignment: fields is written as 8-byte vectors and must be 8-byte aligned, count 4-byte; a pointer that is not is refused with
 * LC_ERR_ARG, as is a NULL fields with W > 0 and a d_data that lives on another device than the calling thread's current one.  n = 0
 * returns LC_OK and touches nothing.  Without a device: LC_ERR_NO_DEVICE.  A handle with an invalid delimiter: LC_ERR_UNSUPPORTED.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream).  The engine knows nothing of SplitKeys or the alarms. */
int lc_csv_device(const lc_csv_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_count,
                  int32_t* d_fields, void* stream);
/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous; no alignment demands on the host arrays. */
int lc_csv_host(const lc_csv_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* count,
                int32_t* fields);

/* ProcessLogs: logs as [[["key","value"],...],...] in, the same shape out; *out_json is malloc'ed, release with lc_csv_free_string.
 * One batch is ONE device trip over the source values of all logs, plus one mop-up trip for the values that need more fields than the
 * first trip kept (at W = the largest count needed).  0, or an LC_ERR_* code when the device could not be used: no *out_json then,
 * every log counts as unchanged, LC_CSV_CNT_FAILED_TRIPS grows and the sink hears LC_CSV_ALARM_TRIP_FAILED. */
int lc_csv_process_logs_json(lc_csv_t* p, const char* logs_json, size_t len, char** out_json);
void lc_csv_free_string(char* s);
int lc_csv_counters(const lc_csv_t* p, uint64_t out[LC_CSV_CNT_COUNT]);
/* one call per alarm site of the Go; kinds LC_CSV_ALARM_* */
void lc_csv_set_alarm_sink(lc_csv_t* p, lc_alarm_sink_t sink, void* user);
/* test knob: fields the first trip keeps per value (0: back to the default, len(SplitKeys), + LC_CSV_PRESERVE_EXTRA with PreserveOthers) */
void lc_csv_set_first_trip_fields(lc_csv_t* p, uint32_t W);
/* releases the calling thread's staging and stream of lc_csv_host (they are also released when the thread ends) */
void lc_csv_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_CSV_H */
