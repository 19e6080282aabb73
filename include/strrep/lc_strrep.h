/*
 * lc_strrep.h -- C ABI of the string-replace processor: the MI355X replacement for two of the three methods of the Go plugin
 * processor_string_replace (plugins/processor/stringreplace/processor_string_replace.go): `const` (cut or replace a fixed byte string,
 * e.g. ANSI colour codes) and `unquote` (turn nginx's `\x22` back into `"`).  It is the second processor here that REWRITES a value to
 * another length (after lc_desensitize.h), and the first one built on the size pass / 64-bit scan / write pass skeleton of the encoders.
 *
 *   reference                                                              this ABI
 *   --------------------------------------------------------------------  ---------------------------------------------------
 *   strings.ReplaceAll :112, strconv.Unquote :117-121, per content         lc_strrep_apply_device / lc_strrep_apply_host
 *                                                                          (strrep_size_kernel, the scan, strrep_write_kernel)
 *   Init :61-95                                                            lc_strrep_create
 *   ProcessLogs :101-140, DestKey, the alarm, the metric                   lc_strrep_process_logs_json (on the host, over the flags
 *                                                                          and new bytes of ONE device trip per batch)
 *
 * The entry points live in a library of their own, liblc_strrep.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error); this header is include/strrep/lc_strrep.h.  The ABI of liblc_regex_gpu.so and the headers of include/ do not change.
 * Everything works on BYTES, as the Go does.  There is no CPU path: without a HIP device the apply calls return LC_ERR_NO_DEVICE.
 *
 * CREATE (Init :61-95).  lc_strrep_create fails, each case with its own message:
 *   - SourceKey is empty                                    "no source key error"     (LC_ERR_ARG)
 *   - Method is not "const", "regex" or "unquote"           "no method error"         (LC_ERR_ARG)
 *   - Method is "const" and Match is empty                  "no match error"          (LC_ERR_ARG)
 *   - Method is "regex"                                     LC_ERR_UNSUPPORTED: the method stays with the Go plugin (see below)
 * RegexTimeoutMs is accepted and ignored.
 *
 * CONST is strings.ReplaceAll(value, Match, ReplaceString): leftmost, non-overlapping occurrences; after an occurrence at p the search
 * goes on at p + len(Match).  `aa` in `aaaaa` gives two replacements and one `a`.  A value with no occurrence is UNCHANGED and takes no
 * output bytes.  ReplaceString may be empty.  A value with an occurrence is CHANGED, also when ReplaceString equals Match.
 *
 * UNQUOTE (:117-121) is strconv.Unquote as of Go 1.23, the version the reference's go.mod names.  The INPUT of the unquote:
 *   form A  the value begins AND ends with `"` (the one-byte value `"` does both): the value itself.
 *   form B  every other value: `"` + the value with every `"` replaced by the four bytes `\x22` + `"`.
 * The decode:
 *   - an input shorter than 2 bytes is an error (the value `"` alone).
 *   - from the byte behind the opening quote, unit by unit up to the first unescaped `"`, which must be the LAST byte of the input;
 *     otherwise an error: `"a"b"`, and a value that ends in an odd run of backslashes, in either form.
 *   - a raw `\n` is an error; every other raw byte below 0x80 is itself.
 *   - a byte >= 0x80 that begins a well-formed UTF-8 sequence (Go's utf8 tables: no overlongs, no surrogates, nothing above U+10FFFF)
 *     is copied whole.  Any other byte >= 0x80 becomes EF BF BD and consumes ONE byte: `E4 B8` at the end gives six bytes, THE OUTPUT
 *     CAN BE UP TO THREE TIMES THE INPUT.  Go's fast path (no `\`, no `\n`, valid UTF-8) gives the same as this loop: one rule.
 *   - escapes: \a \b \f \n \r \t \v \\ \" give their byte; \' is an error; \xHH gives the RAW byte, also >= 0x80 (not re-encoded);
 *     three octal digits \ooo give the raw byte, above 255 is an error, fewer than three digits is an error; \uHHHH and \UHHHHHHHH give
 *     the code point's UTF-8, a surrogate or a value above 0x10FFFF is an error; hex digits in either case; digits cut short by the end
 *     of the input are an error; any other byte behind `\` is an error.
 *   - form B's replacement happens BEFORE the decode: the value `a\"b` becomes `a\\x22b` and decodes to the bytes `a\x22b` with
 *     a literal backslash.  The device gives exactly that without a second copy in memory: in form B a `"` IS the unit stream
 *     `\`, `x`, `2`, `2`.
 *   - on an error the value is UNCHANGED and flagged LC_STRREP_ERROR.
 *   - `""` gives a CHANGED value of zero bytes: the flag says what happened, not the offsets.
 *
 * DEFINED here, undefined or different in the reference:
 *   - Method "regex" is refused at create (LC_ERR_UNSUPPORTED, "... stays with the Go plugin ..."): regexp2's Replace works on runes,
 *     has its own replacement language and a wall-clock timeout, none of which this project can pin.
 *   - Match of at most LC_STRREP_MAX_MATCH (32) bytes, ReplaceString of at most LC_STRREP_MAX_REPLACE (256) bytes; lc_strrep_create
 *     refuses longer ones with a message.  (The reference has no bound.)
 *   - a batch of 2 GiB or more is refused (LC_ERR_ARG); offsets are 32-bit.
 *   - unquote, form B: a value is CHANGED exactly when the decode went through without an error and met a backslash escape or a byte
 *     that became EF BF BD -- which is when the result differs from the value.  A form B value with neither decodes to itself (a `"`
 *     goes to `\x22` and back) and is UNCHANGED.  Every form A value without an error is CHANGED.  (The Go assigns the result either
 *     way; nobody can see the difference.)
 *   - the alarm text is the reference's logger call (:126-127) joined as its logger joins key/value pairs ("k:v\t" each, the join
 *     lc_anchor.h documents), READ OFF THE SOURCE, not off a run:
 *       "error:invalid syntax\tmethod:unquote\tsource_key:<SourceKey>\tcontent:<value>\t"
 */
#ifndef LC_STRREP_H
#define LC_STRREP_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_STRREP_MAX_MATCH 32u
#define LC_STRREP_MAX_REPLACE 256u

/* per-value flags */
enum {
    LC_STRREP_CHANGED = 1, /* the value has a new value, d_out[out_off[i] .. out_off[i+1]); that range may be empty */
    LC_STRREP_ERROR = 2    /* the unquote failed: the value is unchanged */
};
/* alarm kinds of lc_strrep_set_alarm_sink */
enum {
    LC_STRREP_ALARM_UNQUOTE = 1,    /* "error:invalid syntax\tmethod:unquote\tsource_key:<key>\tcontent:<value>\t" */
    LC_STRREP_ALARM_TRIP_FAILED = 2 /* the device trip failed: every log of the batch is left unchanged */
};
/* lc_strrep_counters order */
enum {
    LC_STRREP_CNT_VALUES = 0,         /* contents visited (their key is SourceKey) */
    LC_STRREP_CNT_CHANGED = 1,        /* of them: LC_STRREP_CHANGED */
    LC_STRREP_CNT_UNQUOTE_ERRORS = 2, /* of them: LC_STRREP_ERROR */
    LC_STRREP_CNT_FAILED_TRIPS = 3,
    LC_STRREP_CNT_REPLACE_COUNT = 4,  /* the reference's metric: the sum of replaceCount (:135-138), one per visited content */
    LC_STRREP_CNT_COUNT = 5
};

typedef struct lc_strrep lc_strrep_t;

/* config_json: the Go struct's fields: {"SourceKey": "content", "Method": "const" | "unquote", "Match": "", "ReplaceString": "",
 * "DestKey": "", "RegexTimeoutMs": 0}.  LC_OK, or the code named above with the message in err. */
int lc_strrep_create(const char* config_json, size_t config_len, lc_strrep_t** out, char* err, size_t errcap);
void lc_strrep_free(lc_strrep_t* p);

/* n values in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i + 1]) (uint32 d_off[n + 1], ascending; the
 * contract for d_data is lc_regex_match_device's: the whole 16-byte units a value touches are readable).
 *   d_flags   uint8[n]       LC_STRREP_* per value
 *   d_out_off uint64[n + 1]  where value i's new bytes lie in d_out (8-byte aligned); a value without LC_STRREP_CHANGED takes none
 *   d_out     out_cap bytes; *needed = out_off[n]
 * Output that does not fit out_cap returns LC_ERR_OVERFLOW BEFORE anything is written to d_out; d_flags, d_out_off and *needed are
 * valid, and the call may be repeated with room for *needed.  n == 0 returns LC_OK and touches nothing.  A batch of 2 GiB or more, a
 * NULL array and a d_data on another device than the calling thread's current one return LC_ERR_ARG; without a device:
 * LC_ERR_NO_DEVICE.  Runs on `stream` (hipStream_t, NULL = the default stream) and waits for it: the calling thread's scratch (one
 * 16-byte record per 64 input bytes) is free again when the call returns. */
int lc_strrep_apply_device(const lc_strrep_t* p, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint8_t* d_flags, uint64_t* d_out_off,
                           uint8_t* d_out, uint64_t out_cap, uint64_t* needed, void* stream);
/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to.  flags: uint8[n]; out_off: uint64[n + 1]; *out: the new bytes of the changed values, malloc'ed (release with
 * lc_strrep_free_string; NULL when there are none).  On any failure nothing is handed out.  The values travel in trips of at most 32 MiB,
 * fewer where ReplaceString is longer than Match, so that one trip's new bytes stay below 256 MiB; a single value whose new bytes need
 * more than the device or the pinned staging gives fails the call (LC_ERR_HIP).  No memory for *out: LC_ERR_OVERFLOW. */
int lc_strrep_apply_host(const lc_strrep_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint64_t* out_off,
                         uint8_t** out);

/* ProcessLogs :101-140: logs as [[["key","value"],...],...] in, the same shape out; *out_json is malloc'ed, release with
 * lc_strrep_free_string.  EVERY content whose key is SourceKey is rewritten (a log may hold several).  With DestKey the new value is
 * appended as a new content and the source stays; contents appended during the walk are not visited, also when DestKey == SourceKey.
 * Without DestKey the content is replaced in place.  A log without the key is left alone, with no alarm.  On an unquote error the
 * value stays -- with DestKey the ORIGINAL value is still appended (:128-131) -- and the sink hears LC_STRREP_ALARM_UNQUOTE.
 * One batch is ONE device trip over all source values.  A failed trip leaves every log unchanged, returns the error code (no
 * *out_json), counts under LC_STRREP_CNT_FAILED_TRIPS and alarms LC_STRREP_ALARM_TRIP_FAILED. */
int lc_strrep_process_logs_json(lc_strrep_t* p, const char* logs_json, size_t len, char** out_json);
/* releases what lc_strrep_process_logs_json and lc_strrep_apply_host hand out */
void lc_strrep_free_string(void* s);
/* A handle serves ONE thread at a time: the counters and the sink are plain members (a runner thread owns its processor, as in the
 * Go).  The apply entries read the handle only and may run on several threads at once, each with its own scratch. */
int lc_strrep_counters(const lc_strrep_t* p, uint64_t out[LC_STRREP_CNT_COUNT]);
void lc_strrep_set_alarm_sink(lc_strrep_t* p, lc_alarm_sink_t sink, void* user);
/* releases the calling thread's scratch, staging and stream (they are also released when the thread ends).  lc_thread_release of
 * lc_regex_gpu.h does not know them: this library stands beside liblc_regex_gpu.so */
void lc_strrep_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_STRREP_H */
