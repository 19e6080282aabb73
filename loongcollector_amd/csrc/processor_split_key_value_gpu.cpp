// processor_split_key_value_gpu.cpp -- the Go plugin processor_split_key_value over the device splitter (include/kvsplit/lc_kvsplit.h): Init,
// the gather of the source values, the two engine trips, the stitch of the rows into the logs, counters, alarms, the JSON form.
#include "processor_split_key_value_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "json_min.hpp"

namespace lckv {

void ProcessorSplitKeyValueGpu::Init() {
    if (Delimiter.empty()) Delimiter = "\t";                                // :56-58
    if (Separator.empty()) Separator = ":";                                 // :59-61
    if (EmptyKeyPrefix.empty()) EmptyKeyPrefix = "empty_key_";              // :62-64
    if (NoSeparatorKeyPrefix.empty()) NoSeparatorKeyPrefix = "no_separator_key_";  // :65-67
    const auto tooLong = [](const char* name, const std::string& s) {
        if (s.size() > LC_KV_MAX_NEEDLE)
            throw std::runtime_error(std::string(name) + " is " + std::to_string(s.size()) + " bytes long: the device splitter takes at most " +
                                     std::to_string(LC_KV_MAX_NEEDLE));
    };
    tooLong("Delimiter", Delimiter);
    tooLong("Separator", Separator);
    tooLong("Quote", Quote);
    const auto bytes = [](const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); };
    if (!kvMakeConfig(bytes(Delimiter), Delimiter.size(), bytes(Separator), Separator.size(), bytes(Quote), Quote.size(), &cfg))
        throw std::runtime_error("the needles do not fit the device splitter");
}

int ProcessorSplitKeyValueGpu::ProcessLogs(const lc_kvsplit_t* self, std::vector<Log>& logs) {
    constexpr uint32_t kNoRef = 0xFFFFFFFFu;
    std::vector<uint32_t> refOfLog(logs.size(), kNoRef), contentOfRef;
    std::vector<const uint8_t*> lines;
    std::vector<uint32_t> len;
    for (uint32_t l = 0; l < logs.size(); ++l)
        for (uint32_t c = 0; c < logs[l].Contents.size(); ++c) {
            const LogContent& cont = logs[l].Contents[c];
            if (!SourceKey.empty() && SourceKey != cont.Key) continue;  // :85
            refOfLog[l] = uint32_t(lines.size());
            contentOfRef.push_back(c);
            lines.push_back(reinterpret_cast<const uint8_t*>(cont.Value.data()));
            len.push_back(uint32_t(cont.Value.size()));
            break;  // :91 only the first one
        }
    const uint32_t n = uint32_t(lines.size());
    // ---- the trips: every source value at W pairs, then the values that hold more at the largest count seen
    uint32_t W = firstTripPairs ? firstTripPairs : 1u;
    std::vector<uint8_t> status(n);
    std::vector<uint32_t> npairs(n);
    std::vector<int32_t> rows(size_t(n) * W * 4);
    std::vector<uint32_t> wide;  // refs of the second trip
    std::vector<int32_t> wideRows;
    uint32_t W2 = 0;
    int rc = LC_OK;
    if (n) rc = lc_kvsplit_host(self, lines.data(), len.data(), n, W, status.data(), npairs.data(), rows.data());
    if (rc == LC_OK) {
        for (uint32_t r = 0; r < n; ++r)
            if (status[r] == LC_KV_OK && npairs[r] > W) {
                wide.push_back(r);
                if (npairs[r] > W2) W2 = npairs[r];
            }
        if (!wide.empty()) {
            std::vector<const uint8_t*> wLines;
            std::vector<uint32_t> wLen, wCount(wide.size());
            std::vector<uint8_t> wStatus(wide.size());
            for (uint32_t r : wide) wLines.push_back(lines[r]), wLen.push_back(len[r]);
            wideRows.resize(wide.size() * size_t(W2) * 4);
            rc = lc_kvsplit_host(self, wLines.data(), wLen.data(), uint32_t(wide.size()), W2, wStatus.data(), wCount.data(), wideRows.data());
        }
    }
    if (rc != LC_OK) {
        ++counters[LC_KV_CNT_FAILED_TRIPS];
        alarm(LC_KV_ALARM_TRIP_FAILED, std::string("key-value split: the device trip failed (") + lc_last_error() + "): " + std::to_string(logs.size()) +
                                           " logs left unchanged");
        return rc;
    }
    counters[LC_KV_CNT_VALUES] += n;
    counters[LC_KV_CNT_MOP_UP] += wide.size();
    // ---- the stitch, log by log as the Go walks them
    size_t nextWide = 0;
    for (uint32_t l = 0; l < logs.size(); ++l) {
        Log& log = logs[l];
        const uint32_t r = refOfLog[l];
        if (r == kNoRef) {  // :94-96
            ++counters[LC_KV_CNT_NO_SOURCE_KEY];
            if (ErrIfSourceKeyNotFound) alarm(LC_KV_ALARM_NO_SOURCE_KEY, "can not find key: " + SourceKey);
            continue;
        }
        if (status[r] != LC_KV_OK) {  // DEFINED here: the log stays as it is
            ++counters[LC_KV_CNT_REF_PANIC];
            alarm(LC_KV_ALARM_REF_PANIC, "the reference indexes out of range on this value (a Quote of two or more bytes): log left unchanged");
            continue;
        }
        const int32_t* row = rows.data() + size_t(r) * W * 4;
        if (nextWide < wide.size() && wide[nextWide] == r) row = wideRows.data() + (nextWide++) * size_t(W2) * 4;
        const std::string value = log.Contents[contentOfRef[r]].Value;  // (a copy: the contents move below)
        if (!KeepSource) log.Contents.erase(log.Contents.begin() + contentOfRef[r]);  // :87-89
        uint32_t b = 0;  // the pair's first byte: where the one before ended, plus the delimiter
        for (uint32_t k = 0; k < npairs[r]; ++k, row += 4) {
            const int32_t kb = row[0], ke = row[1];
            const uint32_t vb = uint32_t(row[2]), ve = uint32_t(row[3]);
            // getValue took the quotes off if and only if the value span begins behind the raw value's first byte
            const uint32_t rawBegin = kb == LC_KV_NO_SEPARATOR ? b : kb == LC_KV_EMPTY_KEY ? b + cfg.sepLen : uint32_t(ke) + cfg.sepLen;
            const uint32_t e = vb != rawBegin ? ve + cfg.quoteLen : ve;
            std::string val = value.substr(vb, ve - vb);
            if (kb == LC_KV_NO_SEPARATOR) {  // :113-123
                ++counters[LC_KV_CNT_NO_SEPARATOR];
                if (ErrIfSeparatorNotFound) alarm(LC_KV_ALARM_NO_SEPARATOR, "can not find separator in " + value.substr(b, e - b));
                if (!DiscardWhenSeparatorNotFound) {
                    log.Contents.push_back({NoSeparatorKeyPrefix + std::to_string(ke), std::move(val)});
                    ++counters[LC_KV_CNT_PAIRS];
                }
            } else if (kb == LC_KV_EMPTY_KEY) {  // :127-133
                ++counters[LC_KV_CNT_EMPTY_KEYS];
                if (ErrIfKeyIsEmpty) alarm(LC_KV_ALARM_EMPTY_KEY, "the key of pair with value (" + val + ") is empty");
                log.Contents.push_back({EmptyKeyPrefix + std::to_string(ke), std::move(val)});
                ++counters[LC_KV_CNT_PAIRS];
            } else {
                log.Contents.push_back({value.substr(uint32_t(kb), uint32_t(ke - kb)), std::move(val)});
                ++counters[LC_KV_CNT_PAIRS];
            }
            b = e + cfg.delimLen;
        }
    }
    return LC_OK;
}

}  // namespace lckv

extern "C" int lc_kvsplit_create(const char* config_json, size_t config_len, lc_kvsplit_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto set = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    auto h = std::make_unique<lc_kvsplit>();
    try {
        const lcjson::Value cfg = lcjson::parse(std::string(config_json, config_len));
        if (!cfg.isObject()) throw std::runtime_error("config must be a JSON object");
        auto text = [&](const char* key, std::string& dst) {
            if (const lcjson::Value* v = cfg.find(key))
                if (v->isString()) dst = v->str;
        };
        auto boolean = [&](const char* key, bool& dst) {
            if (const lcjson::Value* v = cfg.find(key))
                if (v->isBool()) dst = v->b;
        };
        text("SourceKey", h->p.SourceKey);
        text("Delimiter", h->p.Delimiter);
        text("Separator", h->p.Separator);
        text("EmptyKeyPrefix", h->p.EmptyKeyPrefix);
        text("NoSeparatorKeyPrefix", h->p.NoSeparatorKeyPrefix);
        text("Quote", h->p.Quote);
        boolean("KeepSource", h->p.KeepSource);
        boolean("DiscardWhenSeparatorNotFound", h->p.DiscardWhenSeparatorNotFound);
        boolean("ErrIfSourceKeyNotFound", h->p.ErrIfSourceKeyNotFound);
        boolean("ErrIfSeparatorNotFound", h->p.ErrIfSeparatorNotFound);
        boolean("ErrIfKeyIsEmpty", h->p.ErrIfKeyIsEmpty);
        h->p.Init();
    } catch (const std::exception& e) {
        set(e.what());
        return LC_ERR_UNSUPPORTED;
    }
    set("");
    *out = h.release();
    return LC_OK;
}
extern "C" void lc_kvsplit_free(lc_kvsplit_t* p) { delete p; }

extern "C" int lc_kvsplit_process_logs_json(lc_kvsplit_t* h, const char* logs_json, size_t len, char** out_json) {
    if (!h || !logs_json || !out_json) return LC_ERR_ARG;
    *out_json = nullptr;
    try {
        const lcjson::Value in = lcjson::parse(std::string(logs_json, len));
        if (!in.isArray()) return LC_ERR_ARG;
        std::vector<lckv::Log> logs;
        for (const auto& l : in.arr) {
            if (!l.isArray()) return LC_ERR_ARG;
            lckv::Log log;
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
extern "C" void lc_kvsplit_free_string(char* s) { std::free(s); }

extern "C" int lc_kvsplit_counters(const lc_kvsplit_t* p, uint64_t out[LC_KV_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
    std::memcpy(out, p->p.counters, sizeof p->p.counters);
    return LC_OK;
}
extern "C" void lc_kvsplit_set_alarm_sink(lc_kvsplit_t* p, lc_alarm_sink_t sink, void* user) {
    if (!p) return;
    p->p.sink = sink;
    p->p.sinkUser = user;
}
extern "C" void lc_kvsplit_set_first_trip_pairs(lc_kvsplit_t* p, uint32_t W) {
    if (p) p->p.firstTripPairs = W ? W : 1u;
}
