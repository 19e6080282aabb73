// processor_parse_container_log_gpu.hpp -- MI355X drop-in for LoongCollector's processor_parse_container_log_native.
//
// Mirrors core/plugin/processor/inner/ProcessorParseContainerLogNative.{h,cpp}.  What differs is where a line is read: the source
// values of a whole group make ONE device trip (lc_container_log_parse_host: clog_containerd_kernel or clog_docker_kernel, by the
// group's LOG_FORMAT metadata) that returns, per line, a status, the stream / partial / escaped flags and the spans of time, source and
// content.  The host then stitches the event with the calls the reference makes, in its order.
//
// Docker: the reference unescapes a "log" value IN PLACE in the source value, which is visible when SourceKey is not "content" and in
// the alarm text.  The device writes the unescaped text into a shadow buffer; the stitch copies [rewrite_begin, content end) back into
// the source at its offset.  Lines flagged LC_CLOG_REPLAY (more than the winning value was rewritten, or the line failed behind a
// rewrite) are finished by clogParseDocker of clog_vm.hpp on the host, in place: the source then holds what the reference leaves.
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_container_log.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, ParseProcessorBase

namespace logtail {

class ProcessorParseContainerLogGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_parse_container_log_gpu"

    // wrongly typed values are warnings (mInitWarnings) and the defaults stay (:45-118); false only for a config that is no object
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    bool mIgnoringStdout = false;
    bool mIgnoringStderr = false;
    bool mIgnoreParseWarning = false;
    bool mKeepingSourceWhenParseFail = true;
    std::string mConfigName;  // the alarm text's "config:"

    std::atomic<uint64_t> mParseStdoutTotal{0}, mParseStderrTotal{0}, mReplayedLines{0};
};

}  // namespace logtail
