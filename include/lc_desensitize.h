/*
 * lc_desensitize.h -- C ABI of processor_desensitize_gpu, the MI355X drop-in for LoongCollector's processor_desensitize_native
 * (core/plugin/processor/ProcessorDesensitizeNative.{h,cpp}): mask secrets in one field of every event.  Two levels: the engine
 * (desens_collect_kernel, desens_size_kernel, desens_write_kernel behind the match kernels of lc_regex_gpu.h) and the processor over
 * event groups.  It is the first processor here that REWRITES a value to another length: results are new bytes, not spans.
 *
 * The pattern is "(" + ContentPatternBeforeReplacedString + ")" + ReplacedContentPattern.  The reference compiles it with RE2
 * (2018-09-01, default options): leftmost-first, '.' does not match '\n', '^' / '$' only at the ends of the text, \s = [\t\n\f\r ],
 * no back-references or look-arounds.  Here: LC_SYNTAX_SEARCH | LC_SYNTAX_NO_DOTALL | LC_SYNTAX_NO_MULTILINE | LC_SYNTAX_REGEXP2,
 * LC_ENGINE_AUTO; engine group 1 is the whole match, group 2 the `before` group, the user's own groups follow.  A pattern the compiler
 * refuses (\p{..}, back-references, look-arounds: the backtracking engine does not run this dialect) fails the create call loudly.
 * The engine matches BYTES; RE2 in UTF-8 mode consumes whole characters in '.' and negated classes, so a rule like [^a]b can differ on
 * non-ASCII text.
 *
 * THE TWO DISCIPLINES (CastOneSensitiveWord :198-249).  They differ, and both are the reference's:
 *
 *   const  (RE2::Replace / RE2::GlobalReplace, rewrite = "\1" + ReplacingString).  Searches are RESUMED INSIDE THE WHOLE VALUE: '^', \b
 *          and '$' see the bytes in front of the resume point (lc_regex_match_device_from's d_from).
 *              p = 0; lastend = none; count = 0
 *              while p <= n:
 *                  m = search(value, from = p)          -- whole match [mb, me); none: stop
 *                  out += value[p:mb]
 *                  if mb == me and mb == lastend:       -- an empty match right behind the last one
 *                      out += value[p] (if p < n); p += 1; continue        -- ONE BYTE (2018-09-01; later releases step a rune)
 *                  out += rewrite(m); p = me; lastend = me; count += 1
 *                  if not ReplacingAll: stop
 *              count == 0: the value is unchanged; else out += value[p:]
 *          The rewrite string is parsed once, at create: \0..\9 name RE2's groups (RE2 group k = engine group k + 1), "\\" is a backslash.
 *          A group that did not take part gives "", and so does a number above the pattern's group count (that release's rule).
 *
 *   md5    (a RE2::FindAndConsume loop).  Every further search is a FRESH SEARCH OF THE REMAINING SUFFIX: '^' matches at the new
 *          start, \b does not see the byte in front.  With s = 0, repeat: find [mb, me) with the `before` group ending at g (offsets in
 *          the whole value); none: stop (unchanged if this was the first search); me == s -- an empty match at the point of
 *          consumption -- : THE WHOLE VALUE STAYS UNCHANGED, earlier replacements included; else out += value[s:g] + MD5(value[g:me])
 *          as 32 UPPER-case hex digits (HashUtil.cpp:319-333), s = me; stop if me >= n or ReplacingAll is off.  Then out += value[s:].
 *          An empty match that is not at s is legal and appends the MD5 of the empty string.
 *
 *   before = "^a", content = "b", value "abab", ReplacingAll: one replacement under const, two under md5.
 *
 * defined_only.  A backslash in the rewrite string in front of anything but 0-9 and '\' (or as its last byte) is an error path in RE2,
 * and what it produces differs between Replace and GlobalReplace.  Here such a handle is a PASS-THROUGH with a create warning: values
 * unchanged, counters as usual.  Named "rewrite_bad_escape" in tests/golden/desensitize_unittest_vectors.json's defined_only.
 *
 * LC_GAVE_UP.  RE2 is linear and never gives up; the device engines can (lc_regex_gpu.h).  Such a value stays UNCHANGED, is flagged
 * LC_DESENS_GAVE_UP, counted under LC_CNT_COMPLEXITY_EXCEEDED and alarmed with its event index -- never silently.
 *
 * There is no CPU path and no host regex engine: without a HIP device the apply calls return LC_ERR_NO_DEVICE.
 */
#ifndef LC_DESENSITIZE_H
#define LC_DESENSITIZE_H

#include <stddef.h>
#include <stdint.h>

#include "lc_processor.h"
#include "lc_regex_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LC_DESENS_CONST = 0, LC_DESENS_MD5 = 1 };
/* per-value flags */
enum {
    LC_DESENS_CHANGED = 1, /* the value has output bytes; without it the value took none and its view stays where it is */
    LC_DESENS_GAVE_UP = 2  /* a search of the value ended LC_GAVE_UP: unchanged */
};

typedef struct lc_desens lc_desens_t;

typedef struct lc_desens_stats {
    uint32_t rounds;         /* search rounds = match launches of the call; exactly 1 with ReplacingAll off.  lc_launched_kernels folds
                                repeated names, so a call that takes a second match launch also notes "desens_search_again" there */
    uint32_t pass_through;   /* 1: the handle is a pass-through (defined_only above), nothing was launched */
    uint64_t searches;       /* values searched, summed over the rounds */
} lc_desens_stats_t;

/* method: LC_DESENS_CONST / LC_DESENS_MD5.  replacing: ReplacingString (const; ignored for md5; the "\1" in front is added here).
 * LC_ERR_SYNTAX / LC_ERR_UNSUPPORTED with the compiler's message in err for a pattern it refuses.  *warning (may be NULL) is set to 1
 * for a pass-through handle. */
int lc_desens_create(int method, const char* before, size_t before_len, const char* content, size_t content_len, const char* replacing,
                     size_t replacing_len, int replacing_all, lc_desens_t** out, int* warning, char* err, size_t errcap);
void lc_desens_free(lc_desens_t* h);
/* the compiled search handle (lc_regex_info tells the engine); owned by h */
lc_regex_t* lc_desens_regex(const lc_desens_t* h);

/* n values in device memory on the current HIP device: value i = d_data[d_off[i] .. d_off[i] + d_len[i]) (d_len NULL: d_off has n + 1
 * entries and the values lie back to back; the contract for d_data is lc_regex_match_device's).
 *   d_flags   uint8[n]      LC_DESENS_* per value
 *   d_out_off uint64[n + 1] where value i's new bytes begin in d_out; an unchanged value takes none (out_off[i + 1] == out_off[i])
 *   d_out     out_cap bytes; *needed = out_off[n].
 * A call whose output does not fit out_cap, or would pass 2^32 - 1 bytes, returns LC_ERR_OVERFLOW BEFORE anything is written to d_out;
 * d_flags, d_out_off and *needed are valid, and the call may be repeated with room for *needed (below 2^32).
 * Runs on `stream` and waits for it: once per search round (four bytes: how many values are still active) and once for the total. */
int lc_desens_apply_device(lc_desens_t* h, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, uint8_t* d_flags,
                           uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, uint64_t* needed, lc_desens_stats_t* stats, void* stream);

/* The same for values in host memory (value i = lines[i][0 .. len[i])), through the calling thread's trip buffers, on the device the
 * thread is bound to.  flags: uint8[n]; out_off: uint64[n + 1]; *out: the new bytes of the changed values, malloc'ed (release with
 * lc_free; NULL when nothing changed).  On any failure nothing is handed out. */
int lc_desens_apply_host(lc_desens_t* h, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint64_t* out_off,
                         uint8_t** out, lc_desens_stats_t* stats);

/* ---- the processor.  config_json: SourceKey, Method ("const" | "md5"), ContentPatternBeforeReplacedString, ReplacedContentPattern
 * (mandatory, non-empty strings), ReplacingString (mandatory for const), ReplacingAll (optional bool, default false; a wrong type is a
 * warning and the default stays).  The create call fails where the reference's Init does, with the readers' messages
 * ("mandatory param X is missing", "param X is not of type string", "mandatory string param X is empty", "string param Method is not
 * valid", "param ContentPatternBeforeReplacedString or ReplacedContentPattern is not a valid regex: ...").
 *
 * Per event (ProcessEvent :159-196): no log event, or no SourceKey: out_failed; an EMPTY SourceKey value: out_key_not_found, left alone;
 * every other event: out_successful, whether or not anything matched.  No event is ever removed.
 * The new bytes of a group are copied ONCE into the group's SourceBuffer and each CHANGED event gets SetContentNoCopy(SourceKey, view);
 * the reference copies every value, changed or not, which no reader of the group can observe.
 *
 * FAILURE POLICY.  Passing a secret on unmasked is worse than passing a line on unparsed.  A failed trip leaves the group UNTOUCHED,
 * raises alarm kind 3 (without a sink: a line on stderr), counts the events under LC_CNT_DEVICE_FAILED_EVENTS and RETURNS THE ERROR: the
 * caller must not forward a group whose call returned non-zero. */
typedef struct lc_desensitize lc_desensitize_t;
int lc_desensitize_create(const char* config_json, lc_desensitize_t** out, char* err, size_t errcap);
void lc_desensitize_destroy(lc_desensitize_t* p);
/* one warning per line; malloc'ed, release with lc_free */
char* lc_desensitize_warnings(const lc_desensitize_t* p);
int lc_desensitize_process(lc_desensitize_t* p, lc_event_group_t* group);
int lc_desensitize_process_native(lc_desensitize_t* p, void* native_group);
/* LC_CNT_* order; LC_CNT_COMPLEXITY_EXCEEDED: values left unchanged because a search gave up */
int lc_desensitize_counters(const lc_desensitize_t* p, uint64_t out[LC_CNT_COUNT]);
/* kind 1: "desensitize: the search gave up on event <index>; the value is left unchanged"; kind 3: the device trip of a group failed */
void lc_desensitize_set_alarm_sink(lc_desensitize_t* p, lc_alarm_sink_t sink, void* user);
/* the engine handle behind the processor (tests, tools); owned by p */
lc_desens_t* lc_desensitize_engine(const lc_desensitize_t* p);
/* match launches of the processor's calls so far */
uint64_t lc_desensitize_rounds(const lc_desensitize_t* p);

#ifdef __cplusplus
}
#endif
#endif
