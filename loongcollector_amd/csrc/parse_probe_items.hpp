// parse_probe_items.hpp -- what an event of processor_parse_regex_native becomes, READ OFF ProcessorParseRegexGpu itself, for the
// serializers that write it on the device (processor_sls_gpu.cpp, processor_jsonl_gpu.cpp): one probe event with recognisable spans
// goes through StitchMatched + FinishEvent, one through FinishEvent alone for a failed line (as ProcessorPipelineGpu::ProcessFused does
// for its failed tally), and the contents that are left, in their order, are the two item lists of a plan (key index, source).
// KeepingSourceWhenParseFail / Succeed, RenamedSourceKey, the legacy raw-log copy and the slot order (DelContent leaves a hole,
// SetContentNoCopy appends, LogEvent.cpp:83-106) cannot drift from the parser's code.
#pragma once

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parse_processor_shell.hpp"

namespace logtail {

struct ParseProbe {
    // whether the parser's configuration has a device path at all: not the whole-line mode, distinct keys, fewer than mark_count + 1
    static bool serves(const ProcessorParseRegexGpu& parse) {
        return !(parse.mIsWholeLineMode || !parse.mKeysDistinct || size_t(parse.mMarkCount) + 1 <= parse.mKeys.size());
    }
    static inline bool itemLists(ProcessorParseRegexGpu& parse, std::vector<std::string>& keys, std::vector<uint32_t> items[2],
                                 ProcessorParseRegexGpu::Tally& failedTally);
};

// keys: one entry per item, in the lists' order; items[0] the matched list, items[1] the unmatched one, as (key index, source) pairs;
// failedTally: what FinishEvent books for ONE line the parser did not match.  false: a value that is neither the line nor a group.
inline bool ParseProbe::itemLists(ProcessorParseRegexGpu& parse, std::vector<std::string>& keys, std::vector<uint32_t> items[2],
                                  ProcessorParseRegexGpu::Tally& failedTally) {
    using Tally = ProcessorParseRegexGpu::Tally;
    // ---- the probes: a line of L bytes in which group g is the one byte at 2g + 1
    const uint32_t G = uint32_t(parse.mMarkCount), L = 2 * G + 4;
    PipelineEventGroup probeGroup(std::make_shared<SourceBuffer>());
    const StringBuffer lineBuf = probeGroup.GetSourceBuffer()->AllocateStringBuffer(L);
    std::memset(lineBuf.data, 'x', L);
    const StringView raw(lineBuf.data, L);
    std::vector<int32_t> caps(2 * size_t(G));
    for (uint32_t g = 0; g < G; ++g) {
        caps[2 * g] = int32_t(2 * g + 1);
        caps[2 * g + 1] = int32_t(2 * g + 2);
    }
    bool readable = true;
    const auto readBack = [&](const LogEvent& ev, std::vector<uint32_t>& list) {
        for (const auto& kv : ev) {
            const size_t at = size_t(reinterpret_cast<uintptr_t>(kv.second.data()) - reinterpret_cast<uintptr_t>(raw.data()));
            uint32_t source = 0;
            if (kv.second.size() == 1 && at >= 1 && at < L && (at & 1u) && (at - 1) / 2 < G) source = uint32_t((at - 1) / 2) + 1;
            else if (!(at == 0 && kv.second.size() == L)) readable = false;  // a value that is neither the line nor a group
            list.push_back(uint32_t(keys.size()));
            list.push_back(source);
            keys.push_back(kv.first.to_string());
        }
    };
    const GroupMetadata& metadata = probeGroup.GetAllMetadata();
    {
        LogEvent* ev = probeGroup.AddLogEvent();
        ev->SetContentNoCopy(StringView(parse.mSourceKey), raw);
        parse.StitchMatched(*ev, raw, caps.data());
        Tally tally;
        if (parse.FinishEvent(*ev, raw, true, metadata, tally)) readBack(*ev, items[0]);
    }
    {
        LogEvent* ev = probeGroup.AddLogEvent();
        ev->SetContentNoCopy(StringView(parse.mSourceKey), raw);
        failedTally = Tally();
        failedTally.outFailed = 1;
        if (parse.FinishEvent(*ev, raw, false, metadata, failedTally)) readBack(*ev, items[1]);
    }
    return readable;
}

}  // namespace logtail
