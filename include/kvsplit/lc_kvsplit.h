/*
 * lc_kvsplit.h -- C ABI of the key-value splitter: the MI355X replacement for the Go plugin processor_split_key_value (one value such as
 * `class:main\tuserid:123456\tmessage:"wrong user"` or `a=1 b="x y"` -> its key/value pairs, appended to the log).
 *
 *   reference (plugins/processor/split/keyvalue/key_value_splitter.go)                this ABI
 *   -------------------------------------------------------------------------------  ------------------------------------
 *   splitKeyValue :99-143 (the loop, the two running indices), concatQuotePair       lc_kvsplit_device / lc_kvsplit_host
 *   :145-158, getNearestQuote :160-182, getValue :184-192                            (kv_split_kernel, one value per lane)
 *   Init :53-69, newKeyValueSplitter :194-206                                         lc_kvsplit_create
 *   ProcessLogs / processLog :75-97, DiscardWhenSeparatorNotFound, the key            lc_kvsplit_process_logs_json
 *   prefixes and the three ErrIf* alarms of splitKeyValue                             (applied on the host to the engine's rows)
 *
 * The entry points live in a library of their own, liblc_kvsplit.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error); this header is include/kvsplit/lc_kvsplit.h.  The ABI of liblc_regex_gpu.so and the headers of include/ do not change.
 *
 * Everything works on BYTES, as the Go does (string indexing, no runes).  There is no CPU path for the split: without a HIP device
 * every entry point that would split a value returns LC_ERR_NO_DEVICE.
 *
 * DEFINED here, undefined or different in the reference:
 *   - LC_KV_REF_PANIC.  With a Quote of two or more bytes getNearestQuote (:177) can return a position behind the end of the content,
 *     and `content[:dIdx]` (:154) then panics with "slice bounds out of range".  The engine reports exactly those values with this
 *     status; their npairs and pairs are unspecified.  The processor leaves such a log UNCHANGED (source kept, nothing appended),
 *     counts it and raises alarm kind LC_KV_ALARM_REF_PANIC.  (Go would have removed the source and appended the pairs before the
 *     panicking one, and then taken the plugin down.)  A Quote of zero or one byte never panics.
 *   - Delimiter, Separator and Quote are at most LC_KV_MAX_NEEDLE (32) bytes each; lc_kvsplit_create refuses longer ones with a
 *     message.  (The reference has no bound; its own tests use up to 15 bytes.)
 *   - a value of 2 GiB or more is refused (LC_ERR_ARG); offsets are int32.
 * Kept as the reference has them: `Index(pair, Separator+Quote) > 0` (an occurrence at offset 0 does not count), the ` \Q` rule of a
 * one-byte quote, "one byte behind where the search began" without a closing quote, the len(Delimiter) bytes skipped behind an
 * extended pair whatever they are, the len(Separator+Quote) arithmetic of a longer quote (right only for a one-byte separator), the
 * empty pair behind a value that ends with the delimiter, no de-duplication of keys.
 */
#ifndef LC_KVSPLIT_H
#define LC_KVSPLIT_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LC_KV_OK = 0, LC_KV_REF_PANIC = 1 };
#define LC_KV_MAX_NEEDLE 32u
#define LC_KV_DEFAULT_PAIRS 16u
/* key begin of a pair without a separator / with an empty key */
#define LC_KV_NO_SEPARATOR (-1)
#define LC_KV_EMPTY_KEY (-2)

/* alarm kinds of lc_kvsplit_set_alarm_sink; the texts are the Go's (:95, :115, :131) */
enum {
    LC_KV_ALARM_NO_SOURCE_KEY = 1, /* "can not find key: <SourceKey>"                       ErrIfSourceKeyNotFound */
    LC_KV_ALARM_NO_SEPARATOR = 2,  /* "can not find separator in <pair>"                    ErrIfSeparatorNotFound */
    LC_KV_ALARM_EMPTY_KEY = 3,     /* "the key of pair with value (<value>) is empty"       ErrIfKeyIsEmpty */
    LC_KV_ALARM_REF_PANIC = 4,     /* DEFINED here: the value is one the reference panics on */
    LC_KV_ALARM_TRIP_FAILED = 5    /* the device trip failed: every log of the batch is left unchanged */
};
/* lc_kvsplit_counters order */
enum {
    LC_KV_CNT_VALUES = 0,        /* values split (one per log that holds the source key) */
    LC_KV_CNT_PAIRS = 1,         /* pairs appended */
    LC_KV_CNT_NO_SEPARATOR = 2,  /* pairs without a separator (appended or discarded) */
    LC_KV_CNT_EMPTY_KEYS = 3,    /* pairs whose key was empty */
    LC_KV_CNT_NO_SOURCE_KEY = 4, /* logs without the source key */
    LC_KV_CNT_REF_PANIC = 5,     /* values with LC_KV_REF_PANIC */
    LC_KV_CNT_MOP_UP = 6,        /* values that took the second trip (more pairs than the first trip kept) */
    LC_KV_CNT_FAILED_TRIPS = 7,
    LC_KV_CNT_COUNT = 8
};

typedef struct lc_kvsplit lc_kvsplit_t;

/* config_json: the Go struct's fields with newKeyValueSplitter's defaults and Init's replacements of empty strings:
 *   {"SourceKey": "", "Delimiter": "\t", "Separator": ":", "KeepSource": true, "EmptyKeyPrefix": "empty_key_",
 *    "NoSeparatorKeyPrefix": "no_separator_key_", "Quote": "", "DiscardWhenSeparatorNotFound": false,
 *    "ErrIfSourceKeyNotFound": true, "ErrIfSeparatorNotFound": true, "ErrIfKeyIsEmpty": true}
 * LC_ERR_UNSUPPORTED with a message in err: no JSON object, or a Delimiter / Separator / Quote above LC_KV_MAX_NEEDLE bytes. */
int lc_kvsplit_create(const char* config_json, size_t config_len, lc_kvsplit_t** out, char* err, size_t errcap);
void lc_kvsplit_free(lc_kvsplit_t* p);

/* n values that live in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries;
 * the contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  kv_split_kernel, one value per lane.
 * pairs: int32[n][W][4] = key begin, key end, value begin, value end, relative to the value's first byte; the value span is what
 *   getValue returns (quotes already stripped).  key begin = LC_KV_NO_SEPARATOR: no separator, key end = its running index (the
 *   reference's noSeparatorKeyIndex when nothing is discarded); key begin = LC_KV_EMPTY_KEY: empty key, key end = emptyKeyIndex.
 * npairs: the TRUE count, also above W; only the first min(npairs, W) rows of a value are written.  W = 0 is allowed, pairs may then
 *   be NULL.  status: LC_KV_OK or LC_KV_REF_PANIC (npairs and pairs of such a value are unspecified).
 * Alignment: pairs is written as 16-byte vectors and must be 16-byte aligned, npairs 4-byte; a pointer that is not is refused with
 * LC_ERR_ARG, as is a NULL pairs with W > 0 and a d_data that lives on another device than the calling thread's current one.  n = 0
 * returns LC_OK and touches nothing.  Without a device: LC_ERR_NO_DEVICE.  Asynchronous on `stream` (hipStream_t, NULL = the default
 * stream).  The engine knows nothing of DiscardWhenSeparatorNotFound, the prefixes or the alarms. */
int lc_kvsplit_device(const lc_kvsplit_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_npairs,
                      int32_t* d_pairs, void* stream);
/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous; no alignment demands on the host arrays. */
int lc_kvsplit_host(const lc_kvsplit_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* npairs,
                    int32_t* pairs);

/* ProcessLogs: logs as [[["key","value"],...],...] in, the same shape out; *out_json is malloc'ed, release with lc_kvsplit_free_string.
 * One batch is ONE device trip over the source values of all logs, plus one mop-up trip for the values with more pairs than the first
 * trip kept (at W = the largest count seen).  0, or an LC_ERR_* code when the device could not be used: no *out_json then, every log
 * counts as unchanged, LC_KV_CNT_FAILED_TRIPS grows and the sink hears LC_KV_ALARM_TRIP_FAILED. */
int lc_kvsplit_process_logs_json(lc_kvsplit_t* p, const char* logs_json, size_t len, char** out_json);
void lc_kvsplit_free_string(char* s);
int lc_kvsplit_counters(const lc_kvsplit_t* p, uint64_t out[LC_KV_CNT_COUNT]);
/* one call per alarm site the three ErrIf* switches guard, text as in the Go; kinds LC_KV_ALARM_* */
void lc_kvsplit_set_alarm_sink(lc_kvsplit_t* p, lc_alarm_sink_t sink, void* user);
/* test knob: pairs the first trip keeps per value (default LC_KV_DEFAULT_PAIRS; 0 is taken as 1) */
void lc_kvsplit_set_first_trip_pairs(lc_kvsplit_t* p, uint32_t W);
/* releases the calling thread's staging and stream of lc_kvsplit_host (they are also released when the thread ends).  lc_thread_release of
 * lc_regex_gpu.h does not know them: this library stands beside liblc_regex_gpu.so */
void lc_kvsplit_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_KVSPLIT_H */
