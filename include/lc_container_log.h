/*
 * lc_container_log.h -- C ABI of the container stdout parser: the MI355X replacement for processor_parse_container_log_native
 * (containerd text "<time> <stdout|stderr> [P|F ]<content>" and Docker json-file {"log":"..","stream":"..","time":".."}).
 *
 *   reference (core/plugin/processor/inner/ProcessorParseContainerLogNative.cpp)   this ABI
 *   ---------------------------------------------------------------------------  ------------------------------------
 *   ParseContainerdTextLogLine up to ResetContainerdTextLog (:176-257)            lc_container_log_parse_device / _host, format 1
 *   ParseDockerLog / parseLogType / parseValue (:259-462)                         lc_container_log_parse_device / _host, format 2
 *   Init (:45-118)                                                                lc_container_log_processor_create
 *   Process / ProcessEvent / ParseDockerJsonLogLine / ResetContainerdTextLog      lc_container_log_processor_process
 *   out_failed, parse_stdout_total, parse_stderr_total                            lc_container_log_processor_counters / _stream_counts
 *   PARSE_LOG_FAIL_ALARM (:160-172)                                               lc_container_log_processor_set_alarm_sink
 *
 * There is no CPU path for the parse: without a HIP device every entry point that would parse a line returns LC_ERR_NO_DEVICE.
 * Out of scope: the fused lc_pipeline_* path.
 *
 * DEFINED here, undefined in the reference:
 *   - containerd: when the second blank is the line's last byte the reference reads one byte behind its view (:227).  The result does
 *     not depend on that byte (the third-blank search finds nothing either way); it is not read here: empty content, not partial.
 *   - Docker: a "\u" whose four bytes make std::stoul throw (no digit: "G123", four blanks) or std::wstring_convert::to_bytes throw (a
 *     negative number other than zero: "-001") takes the reference's agent down.  Here the line fails with LC_CLOG_FAIL_JSON.
 * The reference's last check (:504, the line shorter than the sum of its three fields) cannot fire: the three spans are disjoint pieces
 * of the line.  It has no status.
 */
#ifndef LC_CONTAINER_LOG_H
#define LC_CONTAINER_LOG_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the group's LOG_FORMAT metadata */
#define LC_CLOG_CONTAINERD 1
#define LC_CLOG_DOCKER 2

/* status byte of a line: OK or the reason of failure */
enum {
    LC_CLOG_OK = 0,
    LC_CLOG_FAIL_TIME = 1,    /* containerd: no blank in the line ("time field cannot be found") */
    LC_CLOG_FAIL_SOURCE = 2,  /* containerd: no second blank ("source field cannot be found") */
    LC_CLOG_FAIL_STREAM = 3,  /* containerd: the source is neither stdout nor stderr ("source field not valid");
                                 Docker: the stream value is ("source field cannot be found", the empty value included) */
    LC_CLOG_FAIL_JSON = 4     /* Docker: ParseDockerLog answers false ("not a valid json obejct"), or a "\u" that throws */
};
/* flag bits of a line */
#define LC_CLOG_STDERR 0x01u   /* the source is stderr (OK lines) */
#define LC_CLOG_PARTIAL 0x02u  /* containerd: tag P */
#define LC_CLOG_ESCAPED 0x04u  /* Docker: a "log" value held a backslash and was rewritten */
#define LC_CLOG_REPLAY 0x08u   /* Docker: the reference's in-place rewrite of the source is more than the winning value's: two "log"
                                  values were rewritten, a rewritten one lost against a later one, or the line failed behind a rewrite.
                                  The host routine over the source in place reproduces it (the processor does that). */

enum { LC_CLOG_SPAN_TIME = 0, LC_CLOG_SPAN_SOURCE = 1, LC_CLOG_SPAN_CONTENT = 2 };

/* per-line results, structure of arrays, n entries each */
typedef struct lc_clog_out {
    uint8_t* status;
    uint8_t* flags;
    int32_t* spans;          /* int32[n][3][2]: (begin, end) of time, source and content relative to the line's first byte.  The content's
                                end is its UNESCAPED end.  containerd gives the source span for LC_CLOG_FAIL_STREAM too (the alarm quotes
                                it); every other span of a failed line is (0, 0).  Docker: a key the line lacks is (0, 0). */
    int32_t* rewrite_begin;  /* Docker, LC_CLOG_ESCAPED without LC_CLOG_REPLAY: the first backslash of the winning "log" value; else 0 */
} lc_clog_out_t;

/* n lines that live in device memory on the current HIP device: line i = d_data[d_off[i] .. d_off[i+1]) (d_off has n + 1 entries; the
 * contract for d_data is the one of lc_regex_match_device, lc_regex_gpu.h).  format: LC_CLOG_CONTAINERD (clog_containerd_kernel;
 * d_shadow is not touched and may be NULL) or LC_CLOG_DOCKER (clog_docker_kernel).
 * d_shadow: as many bytes as d_data.  The unescaped text of a rewritten "log" value of line i stands at d_shadow[d_off[i] + p) for p
 * from the value's first backslash to its unescaped end; the bytes in front of the first backslash are the source's own; every other
 * byte of d_shadow is left as it was.
 * Alignment: spans is written as 8-byte vectors and must be 8-byte aligned, rewrite_begin 4-byte.  A pointer that is not is refused
 * with LC_ERR_ARG, as is another format.
 * Asynchronous on `stream` (hipStream_t, NULL = the default stream).  LC_ERR_ARG when d_data lives on another device than the calling
 * thread's current one. */
int lc_container_log_parse_device(int format, const uint8_t* d_data, const int32_t* d_off, uint32_t n, const lc_clog_out_t* d_out,
                                  uint8_t* d_shadow, void* stream);
/* The same for lines in host memory (line i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to (lc_runtime_bind_thread).  Synchronous.  shadow (Docker; may be NULL for containerd): sum(len) bytes, line i's part
 * begins at len[0] + .. + len[i-1]; only [rewrite_begin, content end) of lines with LC_CLOG_ESCAPED and without LC_CLOG_REPLAY is
 * written, and only those bytes come back from the device: *shadow_bytes_moved (may be NULL) is their number, 0 for a batch without
 * escapes. */
int lc_container_log_parse_host(int format, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const lc_clog_out_t* out,
                                uint8_t* shadow, uint64_t* shadow_bytes_moved);

/* ---- the processor.  config_json: SourceKey (default "content"), IgnoringStdout, IgnoringStderr, IgnoreParseWarning,
 * KeepingSourceWhenParseFail (default true).  A wrongly typed value is a warning and the default stays, as in the reference; Init
 * never refuses a config that is a JSON object. */
typedef struct lc_container_log_processor lc_container_log_processor_t;
int lc_container_log_processor_create(const char* config_json, lc_container_log_processor_t** out, char* err, size_t errcap);
void lc_container_log_processor_destroy(lc_container_log_processor_t* p);
/* one warning per line; malloc'ed, release with lc_free */
char* lc_container_log_processor_warnings(const lc_container_log_processor_t* p);
/* what the alarm text names as "config:" (CollectionPipelineContext::GetConfigName; default empty) */
void lc_container_log_processor_set_config_name(lc_container_log_processor_t* p, const char* name);
/* One event group, in place: gather -> one device trip -> stitch.  The format is the group's LOG_FORMAT metadata ("1" / "2"); a group
 * with another or none, and an empty group, make no trip and stay as they are.  0, or an LC_ERR_* code when the device could not be
 * used: the group is then left untouched, the events are counted under LC_CNT_DEVICE_FAILED_EVENTS and the sink hears alarm kind 3. */
int lc_container_log_processor_process(lc_container_log_processor_t* p, lc_event_group_t* group);
int lc_container_log_processor_process_native(lc_container_log_processor_t* p, void* native_group);
/* LC_CNT_* order; out_failed is LC_CNT_OUT_FAILED_EVENTS */
int lc_container_log_processor_counters(const lc_container_log_processor_t* p, uint64_t out[LC_CNT_COUNT]);
/* out[0]: parse_stdout_total, out[1]: parse_stderr_total (ignored streams are counted) */
void lc_container_log_processor_stream_counts(const lc_container_log_processor_t* p, uint64_t out[2]);
/* Docker lines with LC_CLOG_REPLAY that the host routine finished in place */
uint64_t lc_container_log_processor_replayed_lines(const lc_container_log_processor_t* p);
/* kind 0: "failed to parse log line, error: <msg>\tcontainer runtime: <1|2>\tprocessor: processor_parse_container_log_native\tconfig:
 * <name>" (silent under IgnoreParseWarning); kind 3: the device trip of a group failed */
void lc_container_log_processor_set_alarm_sink(lc_container_log_processor_t* p, lc_alarm_sink_t sink, void* user);

#ifdef __cplusplus
}
#endif
#endif
