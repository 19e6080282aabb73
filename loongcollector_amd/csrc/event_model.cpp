// event_model.cpp -- JSON fixture I/O for the stand-in event model (the format the reference's unit tests use:
// PipelineEventGroup::FromJsonString / ToJsonString, core/models/LogEvent.cpp:169-209).
#include "event_model.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "json_min.hpp"

namespace logtail {

namespace {
const std::pair<const char*, EventGroupMetaKey> kMetaNames[] = {
    {"log.file.path", EventGroupMetaKey::LOG_FILE_PATH},
    {"log.file.path_resolved", EventGroupMetaKey::LOG_FILE_PATH_RESOLVED},
    {"log.file.inode", EventGroupMetaKey::LOG_FILE_INODE},
    {"log.file.offset", EventGroupMetaKey::LOG_FILE_OFFSET_KEY},
    {"has.part.log", EventGroupMetaKey::HAS_PART_LOG},
    {"source.id", EventGroupMetaKey::SOURCE_ID},
    {"container.type", EventGroupMetaKey::LOG_FORMAT},
};
// EventGroupMetaKeyToString (core/models/PipelineEventGroup.cpp:367-383) has no name for the scrape timestamp: it is SHOWN as "unknown".
// extension: the fixture loader reads it under a name of its own (the reference's FromJson cannot set it at all)
const char* const kScrapeTimestampShown = "unknown";
const char* const kScrapeTimestampName = "prometheus.scrape.timestamp.millisec";
// EventGroupMetaValueToString (core/models/PipelineEventGroup.cpp:363-392): the two container log formats are shown by name.  (The
// reference renames the value of EVERY key; here only LOG_FORMAT's, so that no other key's output changes.)
const std::pair<const char*, const char*> kFormatNames[] = {{"1", "containerd_text"}, {"2", "docker_json-file"}};
std::string metaValueToString(EventGroupMetaKey key, const std::string& value) {
    if (key == EventGroupMetaKey::LOG_FORMAT)
        for (const auto& f : kFormatNames)
            if (value == f.first) return f.second;
    return value;
}
// extension: the reference's FromJson cannot set LOG_FORMAT at all; here the shown name reads back as the value it stands for
std::string metaValueFromString(EventGroupMetaKey key, const std::string& shown) {
    if (key == EventGroupMetaKey::LOG_FORMAT)
        for (const auto& f : kFormatNames)
            if (shown == f.second) return f.first;
    return shown;
}
}

bool PipelineEventGroup::SetMetadataByName(const std::string& name, const std::string& value) {
    for (const auto& known : kMetaNames) {
        if (name == known.first) {
            SetMetadata(known.second, metaValueFromString(known.second, value));
            return true;
        }
    }
    if (name == kScrapeTimestampName) {
        SetMetadata(EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC, value);
        return true;
    }
    return false;
}

bool PipelineEventGroup::FromJsonString(const std::string& json, std::string* error) {
    lcjson::Value root;
    try {
        root = lcjson::parse(json);
    } catch (const std::exception& e) {
        if (error) *error = e.what();
        return false;
    }
    if (const lcjson::Value* md = root.find("metadata")) {
        for (const auto& kv : md->obj) (void)SetMetadataByName(kv.first, kv.second.str);
    }
    if (const lcjson::Value* tags = root.find("tags"))
        for (const auto& kv : tags->obj) SetTag(kv.first, kv.second.str);
    const lcjson::Value* events = root.find("events");
    if (!events) return true;
    for (const lcjson::Value& ev : events->arr) {
        const lcjson::Value* type = ev.find("type");
        const int t = type ? int(type->inum) : 1;
        PipelineEvent* base = nullptr;
        if (t == int(PipelineEvent::Type::LOG)) {
            LogEvent* le = AddLogEvent();
            base = le;
            if (const lcjson::Value* contents = ev.find("contents")) {
                if (contents->isObject()) {
                    // jsoncpp iterates object members in key order; the reference fixture loader inherits that
                    std::vector<const std::pair<std::string, lcjson::Value>*> members;
                    for (const auto& kv : contents->obj) members.push_back(&kv);
                    std::stable_sort(members.begin(), members.end(),
                                     [](const auto* a, const auto* b) { return a->first < b->first; });
                    for (const auto* kv : members) le->SetContent(kv->first, kv->second.str);
                } else {  // extension: [[key, value], ...] keeps the given order
                    for (const auto& pair : contents->arr)
                        if (pair.arr.size() == 2) le->SetContent(pair.arr[0].str, pair.arr[1].str);
                }
            }
            const lcjson::Value* fo = ev.find("fileOffset");
            const lcjson::Value* rs = ev.find("rawSize");
            if (fo && rs) le->SetPosition(uint64_t(fo->inum), uint64_t(rs->inum));
        } else {
            RawEvent* re = AddRawEvent();
            base = re;
            if (const lcjson::Value* c = ev.find("content")) {
                StringBuffer b = mSourceBuffer->CopyString(c->str);
                re->SetContentNoCopy(StringView(b.data, b.size));
            }
        }
        const lcjson::Value* ts = ev.find("timestamp");
        const lcjson::Value* ns = ev.find("timestampNanosecond");
        if (ts && ns) base->SetTimestamp(time_t(ts->inum), uint32_t(ns->inum));
        else if (ts) base->SetTimestamp(time_t(ts->inum));
    }
    return true;
}

std::string PipelineEventGroup::ToJsonString() const {
    lcjson::Value root = lcjson::Value::makeObject();
    if (!mMetadata.empty()) {
        lcjson::Value md = lcjson::Value::makeObject();
        for (const auto& kv : mMetadata) {
            if (kv.first == EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC) md.set(kScrapeTimestampShown, lcjson::Value::makeString(kv.second.to_string()));
            for (const auto& name : kMetaNames)
                if (kv.first == name.second) md.set(name.first, lcjson::Value::makeString(metaValueToString(kv.first, kv.second.to_string())));
        }
        root.set("metadata", std::move(md));
    }
    if (!mTags.empty()) {
        lcjson::Value tags = lcjson::Value::makeObject();
        for (const auto& kv : mTags) tags.set(kv.first.to_string(), lcjson::Value::makeString(kv.second.to_string()));
        root.set("tags", std::move(tags));
    }
    if (!mEvents.empty()) {
        lcjson::Value events = lcjson::Value::makeArray();
        for (const auto& e : mEvents) {
            lcjson::Value ev = lcjson::Value::makeObject();
            if (e.Is<LogEvent>()) {
                const LogEvent& le = e.Cast<LogEvent>();
                if (!le.Empty()) {
                    lcjson::Value contents = lcjson::Value::makeObject();  // live contents, in list order
                    for (auto it = le.cbegin(); it != le.cend(); ++it)
                        contents.obj.emplace_back(it->first.to_string(), lcjson::Value::makeString(it->second.to_string()));
                    ev.set("contents", std::move(contents));
                }
                if (le.GetPosition().second) {  // (LogEvent::ToJson prints the position with enableEventMeta; here: whenever one is set)
                    ev.set("fileOffset", lcjson::Value::makeInt(int64_t(le.GetPosition().first)));
                    ev.set("rawSize", lcjson::Value::makeInt(int64_t(le.GetPosition().second)));
                }
            } else if (e.Is<MetricEvent>()) {  // MetricEvent::ToJson (MetricEvent.cpp:125-150); the value also as its bit pattern
                const MetricEvent& me = e.Cast<MetricEvent>();
                ev.set("name", lcjson::Value::makeString(me.GetName().to_string()));
                if (const UntypedSingleValue* v = me.GetValue<UntypedSingleValue>()) {
                    uint64_t bits = 0;
                    std::memcpy(&bits, &v->mValue, 8);
                    char hex[17];
                    std::snprintf(hex, sizeof hex, "%016llx", static_cast<unsigned long long>(bits));
                    ev.set("valueBits", lcjson::Value::makeString(hex));
                }
                lcjson::Value tags = lcjson::Value::makeArray();  // extension: [[key, value], ...] keeps the order
                for (auto it = me.TagsBegin(); it != me.TagsEnd(); ++it) {
                    lcjson::Value pair = lcjson::Value::makeArray();
                    pair.arr.push_back(lcjson::Value::makeString(it->first.to_string()));
                    pair.arr.push_back(lcjson::Value::makeString(it->second.to_string()));
                    tags.arr.push_back(std::move(pair));
                }
                ev.set("tags", std::move(tags));
            } else {
                ev.set("content", lcjson::Value::makeString(e.Cast<RawEvent>().GetContent().to_string()));
            }
            ev.set("timestamp", lcjson::Value::makeInt(int64_t(e->GetTimestamp())));
            if (e->GetTimestampNanosecond())
                ev.set("timestampNanosecond", lcjson::Value::makeInt(int64_t(*e->GetTimestampNanosecond())));
            ev.set("type", lcjson::Value::makeInt(int64_t(e->GetType())));
            events.arr.push_back(std::move(ev));
        }
        root.set("events", std::move(events));
    }
    return lcjson::dump(root);
}

}  // namespace logtail
