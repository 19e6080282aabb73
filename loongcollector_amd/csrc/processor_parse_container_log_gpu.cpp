// processor_parse_container_log_gpu.cpp -- see processor_parse_container_log_gpu.hpp.
#include "processor_parse_container_log_gpu.hpp"

#include <cstring>

#include "clog_vm.hpp"

namespace logtail {

const std::string ProcessorParseContainerLogGpu::sName = "processor_parse_container_log_gpu";

namespace {
// ProcessorParseContainerLogNative.cpp:29-43
const std::string kNativeName = "processor_parse_container_log_native";  // the alarm text names the reference's plugin
const std::string kContainerdText = "1", kDockerJsonFile = "2";
const std::string kTimeKey = "_time_", kSourceKey = "_source_", kLogKey = "content";
const std::string kPartLogFlag = "P";  // ProcessorMergeMultilineLogNative::PartLogFlag

// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> kind, status, flags, shadow;
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen;
    std::vector<size_t> lineAt;
    std::vector<int32_t> spans, rewriteBegin;
};

inline StringView spanOf(const char* line, const int32_t* span) { return StringView(line + span[0], size_t(span[1] - span[0])); }
inline std::string first1KB(StringView line) { return std::string(line.data(), line.size() > 1024 ? 1024 : line.size()); }
}  // namespace

// ProcessorParseContainerLogNative::Init :45-118
bool ProcessorParseContainerLogGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    mSourceKey = "content";  // DEFAULT_CONTENT_KEY
    std::string err;
    if (!optionalString(config, "SourceKey", mSourceKey, err)) mInitWarnings.push_back(err);
    if (!optionalBool(config, "IgnoringStdout", mIgnoringStdout, err)) mInitWarnings.push_back(err);
    if (!optionalBool(config, "IgnoringStderr", mIgnoringStderr, err)) mInitWarnings.push_back(err);
    if (!optionalBool(config, "IgnoreParseWarning", mIgnoreParseWarning, err)) mInitWarnings.push_back(err);
    if (!optionalBool(config, "KeepingSourceWhenParseFail", mKeepingSourceWhenParseFail, err)) mInitWarnings.push_back(err);
    return true;
}

// Process :120-136 + ProcessEvent :138-174, restructured as gather -> device trip -> stitch
int ProcessorParseContainerLogGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    const StringView containerType = logGroup.GetMetadata(EventGroupMetaKey::LOG_FORMAT);
    const bool containerd = containerType == StringView(kContainerdText);
    if (!containerd && !(containerType == StringView(kDockerJsonFile))) return LC_OK;  // :151-155: neither branch is taken
    EventsContainer& events = logGroup.MutableEvents();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    (void)gatherSourceValues(events, mSourceKey, S.kind, S.linePtr, S.lineLen);  // :141-147: such events stay untouched, uncounted
    const uint32_t nLines = uint32_t(S.linePtr.size());
    if (!nLines) return LC_OK;
    S.status.resize(nLines);
    S.flags.resize(nLines);
    S.spans.resize(size_t(nLines) * 6);
    S.rewriteBegin.resize(nLines);
    if (!containerd) S.shadow.resize(prefixSums(S.lineLen, S.lineAt) + 1);
    const lc_clog_out_t out{S.status.data(), S.flags.data(), S.spans.data(), S.rewriteBegin.data()};
    const int rc = lc_container_log_parse_host(containerd ? LC_CLOG_CONTAINERD : LC_CLOG_DOCKER, S.linePtr.data(), S.lineLen.data(), nLines, &out,
                                               containerd ? nullptr : S.shadow.data(), nullptr);
    if (rc != LC_OK) return ReportFailedTrip(sName, "container log parse", "unparsed", rc, nLines);
    Tally tally;
    uint64_t nStdout = 0, nStderr = 0, replayed = 0;
    bool anyPartial = false;
    size_t line = 0;
    // errorMsg of a line that failed: counted, and said to the sink unless IgnoreParseWarning (:156-172)
    const auto failed = [&](const std::string& errorMsg) {
        ++tally.outFailed;
        if (!mIgnoreParseWarning)
            RaiseAlarm(0, "failed to parse log line, error: " + errorMsg + "\tcontainer runtime: " + containerType.to_string() + "\tprocessor: " +
                              kNativeName + "\tconfig: " + mConfigName);
        return mKeepingSourceWhenParseFail;
    };
    compactEvents(events, [&](size_t i) {
        if (S.kind[i] != kToParse) return true;
        const uint32_t li = uint32_t(line++);
        LogEvent& ev = events[i].Cast<LogEvent>();
        char* data = const_cast<char*>(reinterpret_cast<const char*>(S.linePtr[li]));
        const StringView raw(data, S.lineLen[li]);
        uint8_t status = S.status[li], flags = S.flags[li];
        const int32_t* span = &S.spans[size_t(li) * 6];
        ClogLine again;
        if (!containerd) {
            // the reference's in-place rewrite of the source value (:470-472)
            if (flags & LC_CLOG_REPLAY) {
                clogParseDockerHost(S.linePtr[li], S.lineLen[li], reinterpret_cast<uint8_t*>(data), again);
                status = again.status;
                flags = again.flags;
                span = &again.span[0].begin;
                ++replayed;
            } else if (flags & LC_CLOG_ESCAPED) {
                const int32_t from = S.rewriteBegin[li], to = span[2 * LC_CLOG_SPAN_CONTENT + 1];
                if (to > from) std::memcpy(data + from, S.shadow.data() + S.lineAt[li] + from, size_t(to - from));
            }
        }
        switch (status) {
            case LC_CLOG_FAIL_TIME:  // :184-190
                return failed("time field cannot be found in log line.\tfirst 1KB log:" + first1KB(raw));
            case LC_CLOG_FAIL_SOURCE:  // :196-202
                return failed("source field cannot be found in log line.\tfirst 1KB log:" + first1KB(raw));
            case LC_CLOG_FAIL_JSON:  // :476-482
                return failed("docker stdout json log line is not a valid json obejct.\tfirst 1KB log:" + first1KB(raw));
            case LC_CLOG_FAIL_STREAM: {
                const std::string source = spanOf(data, span + 2 * LC_CLOG_SPAN_SOURCE).to_string();
                if (containerd) return failed("source field not valid\tsource:" + source + "\tfirst 1KB log:" + first1KB(raw));  // :205-212
                return failed("source field cannot be found in log line.sourceValue:\t" + source + "\tfirst 1KB log:" + first1KB(raw));  // :484-490
            }
            default:
                break;
        }
        // :214-224, :492-502: an ignored stream is counted and erased
        const bool isStderr = (flags & LC_CLOG_STDERR) != 0;
        ++(isStderr ? nStderr : nStdout);
        if (isStderr ? mIgnoringStderr : mIgnoringStdout) return false;
        const StringView timeValue = spanOf(data, span + 2 * LC_CLOG_SPAN_TIME), sourceValue = spanOf(data, span + 2 * LC_CLOG_SPAN_SOURCE);
        StringView content = spanOf(data, span + 2 * LC_CLOG_SPAN_CONTENT);
        if (containerd) {  // ResetContainerdTextLog :527-535
            ev.SetContentNoCopy(StringView(kTimeKey), timeValue);
            ev.SetContentNoCopy(StringView(kSourceKey), sourceValue);
            if (flags & LC_CLOG_PARTIAL) {
                ev.SetContentNoCopy(StringView(kPartLogFlag), StringView());
                anyPartial = true;
            }
            ev.SetContentNoCopy(StringView(kLogKey), content);
        } else {  // :512-522
            ev.SetContent(StringView(kTimeKey), timeValue);
            ev.SetContent(StringView(kSourceKey), sourceValue);
            if (!content.empty() && content.back() == '\n') content = StringView(content.data(), content.size() - 1);
            ev.SetContentNoCopy(StringView(kLogKey), content);
        }
        return true;
    });
    // :252-254: ProcessorMergeMultilineLogNative merges the part logs when it finds this
    if (anyPartial) logGroup.SetMetadata(EventGroupMetaKey::HAS_PART_LOG, kPartLogFlag);
    AddTally(tally);
    if (nStdout) mParseStdoutTotal += nStdout;
    if (nStderr) mParseStderrTotal += nStderr;
    if (replayed) mReplayedLines += replayed;
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_container_log.h)
using logtail::ProcessorParseContainerLogGpu;

struct lc_container_log_processor : logtail::ProcessorHandle<ProcessorParseContainerLogGpu> {};

extern "C" int lc_container_log_processor_create(const char* config_json, lc_container_log_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_container_log_processor_destroy(lc_container_log_processor_t* p) { delete p; }
extern "C" char* lc_container_log_processor_warnings(const lc_container_log_processor_t* p) { return logtail::warningsText(p); }
extern "C" void lc_container_log_processor_set_config_name(lc_container_log_processor_t* p, const char* name) {
    if (p) p->impl.mConfigName = name ? name : "";
}
extern "C" int lc_container_log_processor_process_native(lc_container_log_processor_t* p, void* native_group) {
    return logtail::processNative(p, native_group);
}
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_container_log_processor_process(lc_container_log_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" int lc_container_log_processor_counters(const lc_container_log_processor_t* p, uint64_t out[LC_CNT_COUNT]) {
    return logtail::fillCounters(p, out, true);
}
extern "C" void lc_container_log_processor_stream_counts(const lc_container_log_processor_t* p, uint64_t out[2]) {
    if (!p || !out) return;
    out[0] = p->impl.mParseStdoutTotal;
    out[1] = p->impl.mParseStderrTotal;
}
extern "C" uint64_t lc_container_log_processor_replayed_lines(const lc_container_log_processor_t* p) {
    return p ? uint64_t(p->impl.mReplayedLines) : 0;
}
extern "C" void lc_container_log_processor_set_alarm_sink(lc_container_log_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_parse_container_log_gpu)
extern "C" int lcContainerLogSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_container_log_processor_create, ProcessorParseContainerLogGpu::sName, config_text, state);
}
extern "C" void lcContainerLogSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_container_log_processor_t*>(state), native_group);
}
extern "C" void lcContainerLogSlotFinalize(void* state) { delete static_cast<lc_container_log_processor_t*>(state); }
