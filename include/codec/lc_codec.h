/*
 * lc_codec.h -- C ABI of the field codecs: the MI355X replacement for three Go plugins that rewrite ONE field of a log to a value of
 * another length: processor_base64_encoding (plugins/processor/base64/encoding/processor_base64_encoding.go), processor_base64_decoding
 * (plugins/processor/base64/decoding/processor_base64_decoding.go) and processor_md5 (plugins/processor/md5/processor_md5.go).  Their
 * ProcessLogs shells are the same 25 lines; one handle serves one of them, chosen by the config key "Op".
 *
 *   reference                                                              this ABI
 *   --------------------------------------------------------------------  ---------------------------------------------------
 *   base64.StdEncoding.EncodeToString / DecodeString, md5.Sum + "%x"       lc_codec_apply_device / lc_codec_apply_host
 *   per content                                                            (codec_len_kernel, the scan, b64_encode_kernel;
 *                                                                           b64_decode_size_kernel, the scan, b64_decode_write_kernel;
 *                                                                           codec_len_kernel, md5_field_kernel)
 *   Init (refuses nothing)                                                 lc_codec_create
 *   ProcessLogs, NewKey / MD5Key, the alarms                               lc_codec_process_logs_json (on the host, over the flags and
 *                                                                          new bytes of ONE device trip per batch)
 *
 * The entry points live in a library of their own, liblc_codec.so, linked against liblc_regex_gpu.so (runtime, thread binding,
 * lc_last_error); this header is include/codec/lc_codec.h.  The ABI of liblc_regex_gpu.so and the headers of include/ do not change.
 * Everything works on BYTES.  There is no CPU path: without a HIP device the apply calls return LC_ERR_NO_DEVICE.
 *
 * ENCODE is base64.StdEncoding.EncodeToString: the alphabet A-Z a-z 0-9 + /, `=` padding, 4 * ceil(len / 3) output bytes; the empty
 * value gives the empty value.  Every value has output (LC_CODEC_OUT); there are no errors.
 *
 * MD5 is fmt.Sprintf("%x", md5.Sum(value)): 32 lower-case hex digits, always; the empty value gives d41d8cd98f00b204e9800998ecf8427e.
 *
 * DECODE is base64.StdEncoding.DecodeString (padded, non-strict).
 *
 * DEFINED here: neither Go's sources nor a Go toolchain were at hand.  The decode rules below restate encoding/base64's decodeQuantum
 * and ARE the definition; the accepted values and their bytes are held against CPython's base64 / binascii, the error OFFSETS rest on
 * this restatement alone (tests/golden/README_codec.md).  Encode and MD5 are held against CPython's base64 and hashlib bit for bit.
 *   len = the value's length, k(p) = the number of alphabet bytes in front of raw position p.
 *   - `\r` and `\n` are skipped wherever they stand: inside a quantum, between the two `=`, behind the padding.
 *   - p = the first byte that is neither an alphabet byte nor `\r` / `\n`.  If there is none: with k = k(len), k % 4 == 0 is OK and the
 *     output is 3k / 4 bytes; otherwise an error at offset len - (k % 4) (counted in alphabet bytes only, also when CR/LF stand between).
 *   - the byte at p is not `=`: an error at p.
 *   - the byte at p is `=`, j = k(p) % 4:
 *       j of 0 or 1: an error at p.
 *       j == 2: skip CR/LF behind p.  At the end of the value: an error at len.  The next byte, at q, is not `=`: an error at q - 1
 *               (Go's quirk, kept).  Otherwise go on behind q.
 *       j of 2 or 3: skip CR/LF.  A byte is left, at t: an error at t (trailing garbage).
 *       Otherwise OK, and the output is 3 * (k(p) / 4) + (j - 1) bytes.
 *   - non-strict: the unused low bits of the last quantum are not checked: `QR==` decodes to `A`, as `QQ==` does.
 *   - on an error the value has NO output (the processor discards Go's partial result) and carries the error offset; the error text is
 *     "illegal base64 data at input byte <offset>".
 * Also defined here:
 *   - the selector key "Op": "base64_encode" | "base64_decode" | "md5"; a missing or unknown Op is LC_ERR_ARG with a message.  The
 *     reference's Init refuses nothing, so nothing else is refused: an empty SourceKey matches contents whose key is empty.
 *   - a batch of 2 GiB or more is refused (LC_ERR_ARG); offsets are 32-bit.
 *   - the alarm texts are the reference's logger calls joined as its logger joins key/value pairs ("k:v\t" each, the join lc_anchor.h
 *     documents), READ OFF THE SOURCE, not off a run:
 *       "cannot find key:<SourceKey>\t"                                                 BASE64_E_FIND_ALARM, BASE64_D_FIND_ALARM, MD5_FIND_ALARM
 *       "decode base64 error:illegal base64 data at input byte <N>\t"                   BASE64_D_ALARM
 *     (the alarm type names of pkg/selfmonitor/alarm_type.go; this ABI hands the sink a kind, LC_CODEC_ALARM_*).
 *   - BINARY VALUES: decoded bytes may be any bytes.  The [[["key","value"],...],...] form of lc_codec_process_logs_json goes through the
 *     JSON writer every processor here uses, which is made for UTF-8 text: a decoded value that is not well-formed UTF-8 (a NUL and
 *     multi-byte characters are fine) has no pinned JSON form.  Arbitrary bytes travel through the apply entries.
 */
#ifndef LC_CODEC_H
#define LC_CODEC_H

#include <stddef.h>
#include <stdint.h>

#include "../lc_processor.h"
#include "../lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-value flags */
enum {
    LC_CODEC_OUT = 1,  /* the value has output: out_len[i] bytes at d_out[out_off[i]] (possibly none: the empty value) */
    LC_CODEC_ERROR = 2 /* the decode failed at err_off[i]: no output */
};
/* alarm kinds of lc_codec_set_alarm_sink */
enum {
    LC_CODEC_ALARM_DECODE = 1,     /* "decode base64 error:illegal base64 data at input byte <N>\t" (with DecodeError) */
    LC_CODEC_ALARM_NO_KEY = 2,     /* "cannot find key:<SourceKey>\t" (with NoKeyError) */
    LC_CODEC_ALARM_TRIP_FAILED = 3 /* the device trip failed: every log of the batch is left unchanged */
};
/* lc_codec_counters order */
enum {
    LC_CODEC_CNT_VALUES = 0,        /* contents visited (the first of each log whose key is SourceKey) */
    LC_CODEC_CNT_OUT = 1,           /* of them: LC_CODEC_OUT */
    LC_CODEC_CNT_DECODE_ERRORS = 2, /* of them: LC_CODEC_ERROR */
    LC_CODEC_CNT_NO_KEY = 3,        /* logs without the key */
    LC_CODEC_CNT_FAILED_TRIPS = 4,
    LC_CODEC_CNT_COUNT = 5
};

typedef struct lc_codec lc_codec_t;

/* config_json: the Go struct's fields and the selector: {"Op": "base64_encode" | "base64_decode" | "md5", "SourceKey": "", "NewKey": ""
 * (encode, decode), "MD5Key": "" (md5), "NoKeyError": false, "DecodeError": false (decode)}.  LC_OK, or LC_ERR_ARG with the message in
 * err. */
int lc_codec_create(const char* config_json, size_t config_len, lc_codec_t** out, char* err, size_t errcap);
void lc_codec_free(lc_codec_t* p);

/* n values in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i + 1]) (uint32 d_off[n + 1], ascending; the
 * contract for d_data is lc_regex_match_device's: the whole 16-byte units a value touches are readable).
 *   d_flags   uint8[n]       LC_CODEC_* per value
 *   d_err_off uint32[n]      written for decode errors only; may be NULL
 *   d_out_off uint64[n + 1]  where value i's output begins in d_out: every entry is a multiple of 16, ascending; out_off[n] is the total
 *   d_out_len uint32[n]      value i's true output length (0 without LC_CODEC_OUT); out_off[i] + out_len[i] <= out_off[i + 1]
 *   d_out     out_cap bytes, 16-byte aligned; *needed = out_off[n].  The bytes between a value's end and the next value's begin are
 *             not written.
 * Output that does not fit out_cap returns LC_ERR_OVERFLOW BEFORE anything is written to d_out; d_flags, d_err_off, d_out_off,
 * d_out_len and *needed are valid, and the call may be repeated with room for *needed.  n == 0 returns LC_OK and touches nothing.  A
 * batch of 2 GiB or more, a NULL array (but d_err_off), a d_out that is not 16-byte aligned and a d_data on another device than the
 * calling thread's current one return LC_ERR_ARG; without a device: LC_ERR_NO_DEVICE.  Runs on `stream` (hipStream_t, NULL = the
 * default stream) and waits for it. */
int lc_codec_apply_device(const lc_codec_t* p, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint8_t* d_flags, uint32_t* d_err_off,
                          uint64_t* d_out_off, uint32_t* d_out_len, uint8_t* d_out, uint64_t out_cap, uint64_t* needed, void* stream);
/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's pinned staging, on the device the
 * thread is bound to.  flags: uint8[n]; err_off: uint32[n] or NULL; out_off: uint64[n + 1] (multiples of 16); out_len: uint32[n]; *out:
 * the output bytes, malloc'ed (release with lc_codec_free_string; NULL when there are none).  On any failure nothing is handed out.
 * The values travel in trips of at most 32 MiB and 2^18 values, so that one trip's output stays below 256 MiB.  No memory for *out:
 * LC_ERR_OVERFLOW. */
int lc_codec_apply_host(const lc_codec_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint32_t* err_off,
                        uint64_t* out_off, uint32_t* out_len, uint8_t** out);
/* FOR TESTS: sets the payload bytes of one trip of lc_codec_apply_host, process-wide (0: back to 32 MiB; a value longer than the trip
 * still travels, alone) and returns the number of trips lc_codec_apply_host has made in this process since the last call. */
uint64_t lc_codec_set_trip_bytes(size_t bytes);

/* ProcessLogs: logs as [[["key","value"],...],...] in, the same shape out; *out_json is malloc'ed, release with lc_codec_free_string.
 * In each log only the FIRST content whose key is SourceKey is visited (the Go breaks out of its loop).
 *   encode  a non-empty NewKey appends (NewKey, encoded); an empty NewKey replaces the value in place.
 *   decode  success appends (NewKey, decoded), also when NewKey is empty (the Go has no in-place form here); a failure appends nothing
 *           and, with DecodeError, alarms LC_CODEC_ALARM_DECODE.
 *   md5     appends (MD5Key, digest).
 * A log without the key alarms LC_CODEC_ALARM_NO_KEY, only with NoKeyError.  One batch is ONE device trip over all source values.  A
 * failed trip leaves every log unchanged, returns the error code (no *out_json), counts under LC_CODEC_CNT_FAILED_TRIPS and alarms
 * LC_CODEC_ALARM_TRIP_FAILED. */
int lc_codec_process_logs_json(lc_codec_t* p, const char* logs_json, size_t len, char** out_json);
/* releases what lc_codec_process_logs_json and lc_codec_apply_host hand out */
void lc_codec_free_string(void* s);
/* A handle serves ONE thread at a time: the counters and the sink are plain members.  The apply entries read the handle only and may
 * run on several threads at once, each with its own scratch. */
int lc_codec_counters(const lc_codec_t* p, uint64_t out[LC_CODEC_CNT_COUNT]);
void lc_codec_set_alarm_sink(lc_codec_t* p, lc_alarm_sink_t sink, void* user);
/* releases the calling thread's scratch, staging and stream (they are also released when the thread ends) */
void lc_codec_thread_release(void);

#ifdef __cplusplus
}
#endif
#endif /* LC_CODEC_H */
