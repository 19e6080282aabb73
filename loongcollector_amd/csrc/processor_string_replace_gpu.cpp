// processor_string_replace_gpu.cpp -- the Go plugin processor_string_replace (const, unquote) over the device rewrite
// (include/strrep/lc_strrep.h): Init, the gather of the source values, the one engine trip, the stitch of the new values into the logs,
// counters, alarms, the JSON form.
#include "processor_string_replace_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "json_min.hpp"

namespace lcstrrep {

int ProcessorStringReplaceGpu::Init(std::string* why) {
    if (SourceKey.empty()) {  // :63-65
        *why = "no source key error";
        return LC_ERR_ARG;
    }
    cfg = StrrepConfig{};
    if (Method == "const") {  // :72-75
        if (Match.empty()) {
            *why = "no match error";
            return LC_ERR_ARG;
        }
        if (Match.size() > LC_STRREP_MAX_MATCH) {
            *why = "Match is " + std::to_string(Match.size()) + " bytes long: the device rewrite takes at most " + std::to_string(LC_STRREP_MAX_MATCH);
            return LC_ERR_UNSUPPORTED;
        }
        if (ReplaceString.size() > LC_STRREP_MAX_REPLACE) {
            *why = "ReplaceString is " + std::to_string(ReplaceString.size()) + " bytes long: the device rewrite takes at most " +
                   std::to_string(LC_STRREP_MAX_REPLACE);
            return LC_ERR_UNSUPPORTED;
        }
        cfg.method = kStrrepConst;
        cfg.matchLen = uint32_t(Match.size());
        cfg.replLen = uint32_t(ReplaceString.size());
        std::memcpy(cfg.match, Match.data(), Match.size());
        if (!ReplaceString.empty()) std::memcpy(cfg.repl, ReplaceString.data(), ReplaceString.size());
        return LC_OK;
    }
    if (Method == "regex") {  // :76-86
        *why = "Method \"regex\" stays with the Go plugin: regexp2's rune-wise Replace, its replacement language and its timeout are not served by the device rewrite";
        return LC_ERR_UNSUPPORTED;
    }
    if (Method == "unquote") {
        cfg.method = kStrrepUnquote;
        return LC_OK;
    }
    *why = "no method error";  // :88-89
    return LC_ERR_ARG;
}

int ProcessorStringReplaceGpu::ProcessLogs(const lc_strrep_t* self, std::vector<Log>& logs) {
    // ---- the gather: every content whose key is SourceKey, in the order the Go visits them
    std::vector<const uint8_t*> lines;
    std::vector<uint32_t> len;
    for (const Log& log : logs)
        for (const LogContent& cont : log.Contents)
            if (cont.Key == SourceKey) {  // :105
                lines.push_back(reinterpret_cast<const uint8_t*>(cont.Value.data()));
                len.push_back(uint32_t(cont.Value.size()));
            }
    const uint32_t n = uint32_t(lines.size());
    // ---- the trip
    std::vector<uint8_t> flags(n);
    std::vector<uint64_t> outOff(size_t(n) + 1, 0);
    uint8_t* bytes = nullptr;
    int rc = LC_OK;
    if (n) rc = lc_strrep_apply_host(self, lines.data(), len.data(), n, flags.data(), outOff.data(), &bytes);
    if (rc != LC_OK) {
        ++counters[LC_STRREP_CNT_FAILED_TRIPS];
        alarm(LC_STRREP_ALARM_TRIP_FAILED,
              std::string("string_replace: the device trip failed (") + lc_last_error() + "): " + std::to_string(logs.size()) + " logs left unchanged");
        return rc;
    }
    // ---- the stitch, log by log as the Go walks them
    uint32_t r = 0;
    for (Log& log : logs) {
        const size_t visited = log.Contents.size();  // (range evaluates the slice once: what is appended below is not visited)
        for (size_t c = 0; c < visited; ++c) {
            if (log.Contents[c].Key != SourceKey) continue;
            const uint8_t f = flags[r];
            std::string value = log.Contents[c].Value;  // (a copy: the contents may move below)
            if (f & LC_STRREP_ERROR) {  // :125-129
                ++counters[LC_STRREP_CNT_UNQUOTE_ERRORS];
                alarm(LC_STRREP_ALARM_UNQUOTE, "error:invalid syntax\tmethod:" + Method + "\tsource_key:" + SourceKey + "\tcontent:" + value + "\t");
            }
            if (f & LC_STRREP_CHANGED) {
                ++counters[LC_STRREP_CNT_CHANGED];
                value.assign(reinterpret_cast<const char*>(bytes) + outOff[r], size_t(outOff[r + 1] - outOff[r]));
            }
            if (!DestKey.empty()) log.Contents.push_back({DestKey, std::move(value)});  // :130-131
            else log.Contents[c].Value = std::move(value);                                // :133
            ++counters[LC_STRREP_CNT_VALUES];
            ++counters[LC_STRREP_CNT_REPLACE_COUNT];  // :135
            ++r;
        }
    }
    std::free(bytes);
    return LC_OK;
}

}  // namespace lcstrrep

extern "C" int lc_strrep_create(const char* config_json, size_t config_len, lc_strrep_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto set = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    auto h = std::make_unique<lc_strrep>();
    try {
        const lcjson::Value cfg = lcjson::parse(std::string(config_json, config_len));
        if (!cfg.isObject()) throw std::runtime_error("config must be a JSON object");
        auto text = [&](const char* key, std::string& dst) {
            if (const lcjson::Value* v = cfg.find(key))
                if (v->isString()) dst = v->str;
        };
        text("SourceKey", h->p.SourceKey);
        text("Method", h->p.Method);
        text("Match", h->p.Match);
        text("ReplaceString", h->p.ReplaceString);
        text("DestKey", h->p.DestKey);
        if (const lcjson::Value* v = cfg.find("RegexTimeoutMs"))
            if (v->isNumber()) h->p.RegexTimeoutMs = v->isInt ? v->inum : int64_t(v->num);
    } catch (const std::exception& e) {
        set(e.what());
        return LC_ERR_ARG;
    }
    std::string why;
    const int rc = h->p.Init(&why);
    set(why);
    if (rc != LC_OK) return rc;
    *out = h.release();
    return LC_OK;
}
extern "C" void lc_strrep_free(lc_strrep_t* p) { delete p; }

extern "C" int lc_strrep_process_logs_json(lc_strrep_t* h, const char* logs_json, size_t len, char** out_json) {
    if (!h || !logs_json || !out_json) return LC_ERR_ARG;
    *out_json = nullptr;
    try {
        const lcjson::Value in = lcjson::parse(std::string(logs_json, len));
        if (!in.isArray()) return LC_ERR_ARG;
        std::vector<lcstrrep::Log> logs;
        for (const auto& l : in.arr) {
            if (!l.isArray()) return LC_ERR_ARG;
            lcstrrep::Log log;
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
        if (!*out_json) return LC_ERR_OVERFLOW;  // (out of memory: there is no code of its own)
        std::memcpy(*out_json, text.c_str(), text.size() + 1);
        return LC_OK;
    } catch (const std::exception&) {
        return LC_ERR_ARG;
    }
}
extern "C" void lc_strrep_free_string(void* s) { std::free(s); }

extern "C" int lc_strrep_counters(const lc_strrep_t* p, uint64_t out[LC_STRREP_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
    std::memcpy(out, p->p.counters, sizeof p->p.counters);
    return LC_OK;
}
extern "C" void lc_strrep_set_alarm_sink(lc_strrep_t* p, lc_alarm_sink_t sink, void* user) {
    if (!p) return;
    p->p.sink = sink;
    p->p.sinkUser = user;
}
