// processor_codec_gpu.cpp -- the Go plugins processor_base64_encoding, processor_base64_decoding and processor_md5 over the device codecs
// (include/codec/lc_codec.h): the selector, the gather of the source values, the one engine trip, the stitch of the new values into the
// logs, counters, alarms, the JSON form.
#include "processor_codec_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "json_min.hpp"

namespace lccodec {

int ProcessorCodecGpu::Init(std::string* why) {
    cfg = CodecConfig{};
    if (Op == "base64_encode") cfg.op = kCodecEncode;
    else if (Op == "base64_decode") cfg.op = kCodecDecode;
    else if (Op == "md5") cfg.op = kCodecMd5;
    else {
        *why = Op.empty() ? "no Op: one of \"base64_encode\", \"base64_decode\", \"md5\"" : "unknown Op \"" + Op + "\": one of \"base64_encode\", \"base64_decode\", \"md5\"";
        return LC_ERR_ARG;
    }
    return LC_OK;
}

int ProcessorCodecGpu::ProcessLogs(const lc_codec_t* self, std::vector<Log>& logs) {
    // ---- the gather: the FIRST content of each log whose key is SourceKey (the Go breaks)
    constexpr size_t kNoKey = ~size_t(0);
    std::vector<size_t> where(logs.size(), kNoKey);
    std::vector<const uint8_t*> lines;
    std::vector<uint32_t> len;
    for (size_t l = 0; l < logs.size(); ++l)
        for (size_t c = 0; c < logs[l].Contents.size(); ++c)
            if (logs[l].Contents[c].Key == SourceKey) {
                where[l] = c;
                lines.push_back(reinterpret_cast<const uint8_t*>(logs[l].Contents[c].Value.data()));
                len.push_back(uint32_t(logs[l].Contents[c].Value.size()));
                break;
            }
    const uint32_t n = uint32_t(lines.size());
    // ---- the trip
    std::vector<uint8_t> flags(n);
    std::vector<uint32_t> errOff(n, 0), outLen(n, 0);
    std::vector<uint64_t> outOff(size_t(n) + 1, 0);
    uint8_t* bytes = nullptr;
    int rc = LC_OK;
    if (n) rc = lc_codec_apply_host(self, lines.data(), len.data(), n, flags.data(), errOff.data(), outOff.data(), outLen.data(), &bytes);
    if (rc != LC_OK) {
        ++counters[LC_CODEC_CNT_FAILED_TRIPS];
        alarm(LC_CODEC_ALARM_TRIP_FAILED, Op + ": the device trip failed (" + lc_last_error() + "): " + std::to_string(logs.size()) + " logs left unchanged");
        return rc;
    }
    // ---- the stitch, log by log as the Go walks them
    const std::string& newKey = cfg.op == kCodecMd5 ? MD5Key : NewKey;
    uint32_t r = 0;
    for (size_t l = 0; l < logs.size(); ++l) {
        Log& log = logs[l];
        if (where[l] == kNoKey) {
            ++counters[LC_CODEC_CNT_NO_KEY];
            if (NoKeyError) alarm(LC_CODEC_ALARM_NO_KEY, "cannot find key:" + SourceKey + "\t");
            continue;
        }
        ++counters[LC_CODEC_CNT_VALUES];
        if (flags[r] & LC_CODEC_OUT) {
            ++counters[LC_CODEC_CNT_OUT];
            std::string value(reinterpret_cast<const char*>(bytes) + outOff[r], size_t(outLen[r]));
            if (cfg.op == kCodecEncode && newKey.empty()) log.Contents[where[l]].Value = std::move(value);
            else log.Contents.push_back({newKey, std::move(value)});
        } else {
            ++counters[LC_CODEC_CNT_DECODE_ERRORS];
            if (DecodeError) alarm(LC_CODEC_ALARM_DECODE, "decode base64 error:illegal base64 data at input byte " + std::to_string(errOff[r]) + "\t");
        }
        ++r;
    }
    std::free(bytes);
    return LC_OK;
}

}  // namespace lccodec

extern "C" int lc_codec_create(const char* config_json, size_t config_len, lc_codec_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto set = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    auto h = std::make_unique<lc_codec>();
    try {
        const lcjson::Value cfg = lcjson::parse(std::string(config_json, config_len));
        if (!cfg.isObject()) throw std::runtime_error("config must be a JSON object");
        auto text = [&](const char* key, std::string& dst) {
            if (const lcjson::Value* v = cfg.find(key))
                if (v->isString()) dst = v->str;
        };
        auto flag = [&](const char* key, bool& dst) {
            if (const lcjson::Value* v = cfg.find(key))
                if (v->isBool()) dst = v->b;
        };
        text("Op", h->p.Op);
        text("SourceKey", h->p.SourceKey);
        text("NewKey", h->p.NewKey);
        text("MD5Key", h->p.MD5Key);
        flag("NoKeyError", h->p.NoKeyError);
        flag("DecodeError", h->p.DecodeError);
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
extern "C" void lc_codec_free(lc_codec_t* p) { delete p; }

extern "C" int lc_codec_process_logs_json(lc_codec_t* h, const char* logs_json, size_t len, char** out_json) {
    if (!h || !logs_json || !out_json) return LC_ERR_ARG;
    *out_json = nullptr;
    try {
        const lcjson::Value in = lcjson::parse(std::string(logs_json, len));
        if (!in.isArray()) return LC_ERR_ARG;
        std::vector<lccodec::Log> logs;
        for (const auto& l : in.arr) {
            if (!l.isArray()) return LC_ERR_ARG;
            lccodec::Log log;
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
extern "C" void lc_codec_free_string(void* s) { std::free(s); }

extern "C" int lc_codec_counters(const lc_codec_t* p, uint64_t out[LC_CODEC_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
    std::memcpy(out, p->p.counters, sizeof p->p.counters);
    return LC_OK;
}
extern "C" void lc_codec_set_alarm_sink(lc_codec_t* p, lc_alarm_sink_t sink, void* user) {
    if (!p) return;
    p->p.sink = sink;
    p->p.sinkUser = user;
}
