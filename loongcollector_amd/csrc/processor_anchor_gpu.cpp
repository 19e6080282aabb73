// processor_anchor_gpu.cpp -- the Go plugin processor_anchor over the device locator (include/anchor/lc_anchor.h): Init, the gather of the
// source values, the one engine trip, the stitch of the rows into the logs, counters, alarms, the JSON form.
#include "processor_anchor_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "json_min.hpp"

namespace lcanchor {

void ProcessorAnchorGpu::Init() {
    if (Anchors.size() > LC_ANCHOR_MAX_ANCHORS)
        throw std::runtime_error(std::to_string(Anchors.size()) + " anchors: the device locator takes at most " + std::to_string(LC_ANCHOR_MAX_ANCHORS));
    cfg = AnchorConfig{};
    for (size_t a = 0; a < Anchors.size(); ++a) {
        const Anchor& an = Anchors[a];
        const std::string name = "anchor " + std::to_string(a) + " (FieldName \"" + an.FieldName + "\")";
        if (an.FieldType == "json")  // :80; every other type is the string type (:78, :91-92)
            throw std::runtime_error(name + " has FieldType \"json\": json anchors are not supported by the device locator");
        const auto tooLong = [&](const char* field, const std::string& s) {
            if (s.size() > LC_ANCHOR_MAX_NEEDLE)
                throw std::runtime_error(name + ": " + field + " is " + std::to_string(s.size()) + " bytes long: the device locator takes at most " +
                                         std::to_string(LC_ANCHOR_MAX_NEEDLE));
        };
        tooLong("Start", an.Start);
        tooLong("Stop", an.Stop);
        const auto bytes = [](const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); };
        if (!anchorAdd(&cfg, bytes(an.Start), an.Start.size(), bytes(an.Stop), an.Stop.size()))
            throw std::runtime_error(name + " does not fit the device locator");
    }
}

// util.CutString(val, 1024)
static std::string cutString(const std::string& val) { return val.size() < 1024 ? val : val.substr(0, 1024); }

int ProcessorAnchorGpu::ProcessLogs(const lc_anchor_t* self, std::vector<Log>& logs) {
    constexpr uint32_t kNoRef = 0xFFFFFFFFu;
    std::vector<uint32_t> refOfLog(logs.size(), kNoRef), contentOfRef;
    std::vector<const uint8_t*> lines;
    std::vector<uint32_t> len;
    for (uint32_t l = 0; l < logs.size(); ++l)
        for (uint32_t c = 0; c < logs[l].Contents.size(); ++c) {
            const LogContent& cont = logs[l].Contents[c];
            if (!SourceKey.empty() && SourceKey != cont.Key) continue;  // :116
            refOfLog[l] = uint32_t(lines.size());
            contentOfRef.push_back(c);
            lines.push_back(reinterpret_cast<const uint8_t*>(cont.Value.data()));
            len.push_back(uint32_t(cont.Value.size()));
            break;  // :122 only the first one
        }
    const uint32_t n = uint32_t(lines.size());
    const uint32_t S = anchorStride(cfg);
    // ---- the trip: every source value, S entries each (the row width is fixed: there is no second trip)
    std::vector<int32_t> rows(size_t(n) * S * 2);
    int rc = LC_OK;
    if (n && S) rc = lc_anchor_locate_host(self, lines.data(), len.data(), n, rows.data());
    if (rc != LC_OK) {
        ++counters[LC_ANCHOR_CNT_FAILED_TRIPS];
        alarm(LC_ANCHOR_ALARM_TRIP_FAILED,
              std::string("anchor: the device trip failed (") + lc_last_error() + "): " + std::to_string(logs.size()) + " logs left unchanged");
        return rc;
    }
    counters[LC_ANCHOR_CNT_VALUES] += n;
    // ---- the stitch, log by log as the Go walks them
    for (uint32_t l = 0; l < logs.size(); ++l) {
        Log& log = logs[l];
        const size_t beginLen = log.Contents.size();  // :113
        const uint32_t r = refOfLog[l];
        if (r == kNoRef) {  // :125-127
            ++counters[LC_ANCHOR_CNT_NO_SOURCE_KEY];
            if (NoKeyError) alarm(LC_ANCHOR_ALARM_NO_KEY, "anchor cannot find key:" + SourceKey + "\t");
        } else {
            const std::string value = log.Contents[contentOfRef[r]].Value;  // (a copy: the contents move below)
            if (!KeepSource) log.Contents.erase(log.Contents.begin() + contentOfRef[r]);  // :118-120
            const int32_t* row = rows.data() + size_t(r) * S * 2;
            for (size_t a = 0; a < Anchors.size(); ++a, row += 2) {  // :173
                if (row[0] == LC_ANCHOR_NO_START) {  // :176-181
                    ++counters[LC_ANCHOR_CNT_NO_START];
                    if (NoAnchorError) alarm(LC_ANCHOR_ALARM_NO_START, "anchor no start:" + Anchors[a].Start + "\tcontent:" + cutString(value) + "\t");
                } else if (row[0] == LC_ANCHOR_NO_STOP) {  // :184-188
                    ++counters[LC_ANCHOR_CNT_NO_STOP];
                    if (NoAnchorError) alarm(LC_ANCHOR_ALARM_NO_STOP, "anchor no stop:" + Anchors[a].Stop + "\tcontent:" + cutString(value) + "\t");
                } else {  // :199
                    log.Contents.push_back({Anchors[a].FieldName, value.substr(uint32_t(row[0]), uint32_t(row[1] - row[0]))});
                    ++counters[LC_ANCHOR_CNT_FIELDS];
                }
            }
        }
        counters[LC_ANCHOR_CNT_PAIRS_PER_LOG] += uint64_t(int64_t(log.Contents.size()) - int64_t(beginLen) + 1);  // :128
    }
    return LC_OK;
}

}  // namespace lcanchor

extern "C" int lc_anchor_create(const char* config_json, size_t config_len, lc_anchor_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto set = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    auto h = std::make_unique<lc_anchor>();
    try {
        const lcjson::Value cfg = lcjson::parse(std::string(config_json, config_len));
        if (!cfg.isObject()) throw std::runtime_error("config must be a JSON object");
        auto text = [](const lcjson::Value& o, const char* key, std::string& dst) {
            if (const lcjson::Value* v = o.find(key))
                if (v->isString()) dst = v->str;
        };
        auto boolean = [](const lcjson::Value& o, const char* key, bool& dst) {
            if (const lcjson::Value* v = o.find(key))
                if (v->isBool()) dst = v->b;
        };
        text(cfg, "SourceKey", h->p.SourceKey);
        boolean(cfg, "NoKeyError", h->p.NoKeyError);
        boolean(cfg, "NoAnchorError", h->p.NoAnchorError);
        boolean(cfg, "KeepSource", h->p.KeepSource);
        if (const lcjson::Value* list = cfg.find("Anchors")) {
            if (!list->isArray()) throw std::runtime_error("Anchors must be a JSON array");
            for (const auto& o : list->arr) {
                if (!o.isObject()) throw std::runtime_error("an anchor must be a JSON object");
                lcanchor::Anchor an;
                text(o, "Start", an.Start);
                text(o, "Stop", an.Stop);
                text(o, "FieldName", an.FieldName);
                text(o, "FieldType", an.FieldType);
                boolean(o, "ExpondJSON", an.ExpondJSON);
                boolean(o, "IgnoreJSONError", an.IgnoreJSONError);
                text(o, "ExpondConnecter", an.ExpondConnecter);
                if (const lcjson::Value* v = o.find("MaxExpondDepth"))
                    if (v->isNumber()) an.MaxExpondDepth = v->isInt ? v->inum : int64_t(v->num);
                h->p.Anchors.push_back(std::move(an));
            }
        }
        h->p.Init();
    } catch (const std::exception& e) {
        set(e.what());
        return LC_ERR_UNSUPPORTED;
    }
    set("");
    *out = h.release();
    return LC_OK;
}
extern "C" void lc_anchor_free(lc_anchor_t* p) { delete p; }
extern "C" uint32_t lc_anchor_stride(const lc_anchor_t* p) { return p ? anchorStride(p->p.cfg) : 0u; }

extern "C" int lc_anchor_process_logs_json(lc_anchor_t* h, const char* logs_json, size_t len, char** out_json) {
    if (!h || !logs_json || !out_json) return LC_ERR_ARG;
    *out_json = nullptr;
    try {
        const lcjson::Value in = lcjson::parse(std::string(logs_json, len));
        if (!in.isArray()) return LC_ERR_ARG;
        std::vector<lcanchor::Log> logs;
        for (const auto& l : in.arr) {
            if (!l.isArray()) return LC_ERR_ARG;
            lcanchor::Log log;
            for (const auto& c : l.arr) {
                if (!c.isArray() || c.arr.size() != 2 || !c.arr[0].isString() || !c.arr[1].isString()) return LC_ERR_ARG;
                log.Contents.push_back({c.arr[0].str, c.arr[1].str});
            }
            logs.push_back(std::move(log));
        }
        const int rc = h->p.ProcessLogs(h, logs);
        if (rc != LC_OK) return rc;
        lcjson::Value out = lcjson::Value::makeArray();
        for (const auto& log : logs) {
            lcjson::Value l = lcjson::Value::makeArray();
            for (const auto& c : log.Contents) {
                lcjson::Value pair = lcjson::Value::makeArray();
                pair.arr.push_back(lcjson::Value::makeString(c.Key));
                pair.arr.push_back(lcjson::Value::makeString(c.Value));
                l.arr.push_back(std::move(pair));
            }
            out.arr.push_back(std::move(l));
        }
        const std::string text = lcjson::dump(out);
        *out_json = static_cast<char*>(std::malloc(text.size() + 1));
        if (!*out_json) return LC_ERR_ARG;
        std::memcpy(*out_json, text.c_str(), text.size() + 1);
        return LC_OK;
    } catch (const std::exception&) {
        return LC_ERR_ARG;
    }
}
extern "C" void lc_anchor_free_string(char* s) { std::free(s); }

extern "C" int lc_anchor_counters(const lc_anchor_t* p, uint64_t out[LC_ANCHOR_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
    std::memcpy(out, p->p.counters, sizeof p->p.counters);
    return LC_OK;
}
extern "C" void lc_anchor_set_alarm_sink(lc_anchor_t* p, lc_alarm_sink_t sink, void* user) {
    if (!p) return;
    p->p.sink = sink;
    p->p.sinkUser = user;
}
