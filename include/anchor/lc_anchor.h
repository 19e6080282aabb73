/*
 * lc_anchor.h -- C ABI of the anchor processor: the MI355X replacement for the Go plugin processor_anchor (for every configured anchor
 * the bytes between the first `Start` of the source value and the first `Stop` behind it, appended to the log under `FieldName`:
 * `time:2017.09.12 20:55:36\tlevel:info` with Start "time:" / Stop "\t" -> time = 2017.09.12 20:55:36).
 *
 *   reference (plugins/processor/anchor/anchor.go)                                    this ABI
 *   -------------------------------------------------------------------------------  ------------------------------------
 *   ProcessAnchor :172-199, the two strings.Index per anchor and the string field     lc_anchor_locate_device / lc_anchor_locate_host
 *                                                                                     (anchor_locate_kernel, one value per lane)
 *   Init :74-99                                                                       lc_anchor_create
 *   ProcessLogs / ProcessLog :105-129, KeepSource, the three alarms, the              lc_anchor_process_logs_json
 *   pairs-per-log metric                                                              (applied on the host to the engine's rows)
 *
 * The entry points live in a library of their own, liblc_anchor.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error); this header is include/anchor/lc_anchor.h.  The ABI of liblc_regex_gpu.so and the headers of include/ do not change.
 *
 * Everything works on BYTES, as the Go does (string indexing, no runes).  There is no CPU path for the search: without a HIP device
 * every entry point that would locate an anchor returns LC_ERR_NO_DEVICE.
 *
 * Per anchor, in configuration order, on the same value `val` (anchors never influence each other):
 *   s = Index(val, Start); s < 0: nothing ("no start").  b = s + len(Start).  t = Index(val[b:], Stop); t < 0: nothing ("no stop").
 *   e = len(val) when Stop == "", b + t otherwise.  The field is val[b:e].
 * So Start == "" gives b = 0; a Stop that begins before b does not count (also one that overlaps the tail of Start); a needle whose
 * last bytes would lie behind the value's end is no occurrence.
 *
 * DEFINED here, undefined or different in the reference:
 *   - FieldType "json".  The reference expands such an anchor's field with github.com/buger/jsonparser, whose leniency this project
 *     cannot pin (neither its source nor a Go toolchain was at hand).  lc_anchor_create refuses a configuration that holds one, with
 *     LC_ERR_UNSUPPORTED and a message that names the anchor.  "string", an absent type and every other type are the string type, as
 *     Init :91-92 has it; ExpondJSON, IgnoreJSONError, ExpondConnecter and MaxExpondDepth (the reference's spellings) are accepted
 *     and mean nothing for a string anchor.
 *   - at most LC_ANCHOR_MAX_ANCHORS (16) anchors, Start and Stop of at most LC_ANCHOR_MAX_NEEDLE (32) bytes each; lc_anchor_create
 *     refuses more or longer ones with a message.  (The reference has no bound.)
 *   - a value of 2 GiB or more is refused (LC_ERR_ARG); offsets are int32.
 *   - the alarm texts are the reference's key/value pairs joined as its logger joins them ("k:v\t" each):
 *       "anchor cannot find key:<SourceKey>\t", "anchor no start:<Start>\tcontent:<value cut to 1024 bytes>\t",
 *       "anchor no stop:<Stop>\tcontent:<value cut to 1024 bytes>\t"  (CutString: the whole value below 1024 bytes, else its first 1024).
 */
#ifndef LC_ANCHOR_H
#define LC_ANCHOR_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_ANCHOR_MAX_ANCHORS 16u
#define LC_ANCHOR_MAX_NEEDLE 32u
/* the begin of an entry without a field (its end is -1) */
#define LC_ANCHOR_NO_START (-1)
#define LC_ANCHOR_NO_STOP (-2)

/* alarm kinds of lc_anchor_set_alarm_sink */
enum {
    LC_ANCHOR_ALARM_NO_KEY = 1,     /* "anchor cannot find key:<SourceKey>\t"                 NoKeyError */
    LC_ANCHOR_ALARM_NO_START = 2,   /* "anchor no start:<Start>\tcontent:<cut value>\t"       NoAnchorError */
    LC_ANCHOR_ALARM_NO_STOP = 3,    /* "anchor no stop:<Stop>\tcontent:<cut value>\t"         NoAnchorError */
    LC_ANCHOR_ALARM_TRIP_FAILED = 4 /* the device trip failed: every log of the batch is left unchanged */
};
/* lc_anchor_counters order */
enum {
    LC_ANCHOR_CNT_VALUES = 0,        /* values located (one per log that holds the source key) */
    LC_ANCHOR_CNT_FIELDS = 1,        /* fields appended */
    LC_ANCHOR_CNT_NO_START = 2,      /* anchors whose Start was not found */
    LC_ANCHOR_CNT_NO_STOP = 3,       /* anchors whose Stop was not found behind Start */
    LC_ANCHOR_CNT_NO_SOURCE_KEY = 4, /* logs without the source key */
    LC_ANCHOR_CNT_FAILED_TRIPS = 5,
    LC_ANCHOR_CNT_PAIRS_PER_LOG = 6, /* the reference's metric: the sum of len(Contents) - beginLen + 1 over the logs (:128), as the Go
                                        computes it (a removed source counts -1) */
    LC_ANCHOR_CNT_COUNT = 7
};

typedef struct lc_anchor lc_anchor_t;

/* config_json: the Go struct's fields; nothing has a default, every switch is false when absent:
 *   {"Anchors": [{"Start": "time:", "Stop": "\t", "FieldName": "time", "FieldType": "string", "ExpondJSON": false,
 *                 "IgnoreJSONError": false, "ExpondConnecter": "", "MaxExpondDepth": 0}, ...],
 *    "NoKeyError": false, "NoAnchorError": false, "SourceKey": "", "KeepSource": false}
 * LC_ERR_UNSUPPORTED with a message in err: no JSON object, an anchor of FieldType "json", more than LC_ANCHOR_MAX_ANCHORS anchors,
 * a Start / Stop above LC_ANCHOR_MAX_NEEDLE bytes. */
int lc_anchor_create(const char* config_json, size_t config_len, lc_anchor_t** out, char* err, size_t errcap);
void lc_anchor_free(lc_anchor_t* p);
/* S: entries per row of the span arrays = the anchor count rounded up to an even number (a row is whole 16-byte vectors) */
uint32_t lc_anchor_stride(const lc_anchor_t* p);

/* n values that live in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries;
 * the contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  anchor_locate_kernel, one value per lane.
 * d_spans: int32[n][S][2], S = lc_anchor_stride(p).  Entry a of a row is (b, e) relative to the value's first byte,
 *   (LC_ANCHOR_NO_START, -1) or (LC_ANCHOR_NO_STOP, -1); the pad entry of an odd anchor count is written (-1, -1).
 * Alignment: a row is whole 16-byte units and d_spans must be 16-byte aligned; a pointer that is not is refused with LC_ERR_ARG, as
 * is a NULL d_spans and a d_data that lives on another device than the calling thread's current one.  n = 0 returns LC_OK and touches
 * nothing.  Without a device: LC_ERR_NO_DEVICE.  Asynchronous on `stream` (hipStream_t, NULL = the default stream).  The engine knows
 * nothing of SourceKey, KeepSource, field names or the alarms. */
int lc_anchor_locate_device(const lc_anchor_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, int32_t* d_spans, void* stream);
/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous; no alignment demands on the host arrays. */
int lc_anchor_locate_host(const lc_anchor_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, int32_t* spans);

/* ProcessLogs: logs as [[["key","value"],...],...] in, the same shape out; *out_json is malloc'ed, release with lc_anchor_free_string.
 * One batch is ONE device trip over the source values of all logs that have the key (the row width is fixed: no second trip).  0, or
 * an LC_ERR_* code when the device could not be used: no *out_json then, every log counts as unchanged, LC_ANCHOR_CNT_FAILED_TRIPS
 * grows and the sink hears LC_ANCHOR_ALARM_TRIP_FAILED. */
int lc_anchor_process_logs_json(lc_anchor_t* p, const char* logs_json, size_t len, char** out_json);
void lc_anchor_free_string(char* s);
int lc_anchor_counters(const lc_anchor_t* p, uint64_t out[LC_ANCHOR_CNT_COUNT]);
/* one call per alarm site NoKeyError / NoAnchorError guard, text as above; kinds LC_ANCHOR_ALARM_* */
void lc_anchor_set_alarm_sink(lc_anchor_t* p, lc_alarm_sink_t sink, void* user);
/* releases the calling thread's staging and stream of lc_anchor_locate_host (they are also released when the thread ends).
 * lc_thread_release of lc_regex_gpu.h does not know them: this library stands beside liblc_regex_gpu.so */
void lc_anchor_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_ANCHOR_H */
