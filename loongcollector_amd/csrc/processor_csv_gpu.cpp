// processor_csv_gpu.cpp -- the Go plugin processor_csv over the device decoder (include/csv/lc_csv.h): Init, the gather of the source
// values, the two engine trips, the fold and the stitch of the rows into the logs, the csv.Writer remainder, counters, alarms, the JSON form.
#include "processor_csv_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "json_min.hpp"

namespace lccsv {

namespace {

struct BytesSource {
    const uint8_t* p;
    uint32_t byteAt(uint32_t i) const { return p[i]; }
};

// utf8.DecodeRuneInString: the rune at s[at] and its width; malformed input is U+FFFD of width 1
uint32_t decodeRune(const std::string& s, size_t at, size_t* width) {
    const auto b = [&](size_t i) { return uint32_t(uint8_t(s[i])); };
    const size_t left = s.size() - at;
    const uint32_t c = b(at);
    *width = 1;
    if (c < 0x80u) return c;
    const auto cont = [&](size_t i) { return (b(i) & 0xC0u) == 0x80u; };
    if (c >= 0xC2u && c <= 0xDFu && left >= 2 && cont(at + 1)) {
        *width = 2;
        return ((c & 0x1Fu) << 6) | (b(at + 1) & 0x3Fu);
    }
    if (c >= 0xE0u && c <= 0xEFu && left >= 3 && cont(at + 1) && cont(at + 2)) {
        const uint32_t r = ((c & 0x0Fu) << 12) | ((b(at + 1) & 0x3Fu) << 6) | (b(at + 2) & 0x3Fu);
        if (r >= 0x800u && (r < 0xD800u || r > 0xDFFFu)) {
            *width = 3;
            return r;
        }
    }
    if (c >= 0xF0u && c <= 0xF4u && left >= 4 && cont(at + 1) && cont(at + 2) && cont(at + 3)) {
        const uint32_t r = ((c & 0x07u) << 18) | ((b(at + 1) & 0x3Fu) << 12) | ((b(at + 2) & 0x3Fu) << 6) | (b(at + 3) & 0x3Fu);
        if (r >= 0x10000u && r <= 0x10FFFFu) {
            *width = 4;
            return r;
        }
    }
    return 0xFFFDu;
}

bool beginsWithSpaceRune(const std::string& s) {
    const BytesSource src{reinterpret_cast<const uint8_t*>(s.data())};
    return !s.empty() && csvSpaceRune(src, 0, uint32_t(s.size()), 0, uint8_t(s[0])) != 0;
}

std::string cutString(const std::string& s) { return s.size() < 1024 ? s : s.substr(0, 1024); }  // util.CutString(value, 1024)

const char* kInvalidDelim = "csv: invalid field or comment delimiter";
const char* sentenceOf(uint8_t status) { return status == LC_CSV_BARE_QUOTE ? "bare \" in non-quoted-field" : "extraneous or missing \" in quoted-field"; }

}  // namespace

std::string writeRecord(const std::vector<std::string>& fields, const std::string& sep) {
    std::string out;
    for (size_t n = 0; n < fields.size(); ++n) {
        const std::string& f = fields[n];
        if (n) out += sep;
        const bool quote = !f.empty() && (f == "\\." || f.find(sep) != std::string::npos || f.find_first_of("\"\r\n") != std::string::npos || beginsWithSpaceRune(f));
        if (!quote) {
            out += f;
            continue;
        }
        out += '"';
        for (char c : f) {
            if (c == '"') out += '"';
            out += c;
        }
        out += '"';
    }
    return out;
}

void ProcessorCsvGpu::Init() {
    size_t runes = 0, width = 0;
    uint32_t rune = 0;
    for (size_t at = 0; at < SplitSep.size(); at += width, ++runes) rune = decodeRune(SplitSep, at, &width);  // []rune(p.SplitSep)
    if (runes != 1) throw std::runtime_error("invalid separator: " + SplitSep);                               // :48-50
    cfg = CsvConfig{};
    cfg.trim = TrimLeadingSpace ? 1u : 0u;
    cfg.invalidDelim = (rune == 0 || rune == '"' || rune == '\r' || rune == '\n' || rune == 0xFFFDu) ? 1u : 0u;  // validDelim of encoding/csv
    if (!cfg.invalidDelim) {
        cfg.sepLen = uint32_t(SplitSep.size());
        cfg.sepWord = 0;
        for (size_t j = 0; j < SplitSep.size(); ++j) cfg.sepWord |= uint32_t(uint8_t(SplitSep[j])) << (8 * j);
    }
}

int ProcessorCsvGpu::ProcessLogs(const lc_csv_t* self, std::vector<Log>& logs) {
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
    const uint32_t n = uint32_t(lines.size()), nkeys = uint32_t(SplitKeys.size());
    const bool read = nkeys != 0 && !cfg.invalidDelim;  // what reaches the device
    // ---- the trips: every source value at W fields, then the values that need more at the largest count needed
    const uint32_t W = firstTripFields ? firstTripFields : nkeys + (PreserveOthers ? LC_CSV_PRESERVE_EXTRA : 0u);
    const auto needed = [&](uint32_t count) { return PreserveOthers || count < nkeys ? count : nkeys; };
    std::vector<uint8_t> status(n);
    std::vector<uint32_t> count(n);
    std::vector<int32_t> rows(read ? size_t(n) * W * 2 : 0);
    std::vector<uint32_t> wide;  // refs of the second trip
    std::vector<int32_t> wideRows;
    uint32_t W2 = 0;
    int rc = LC_OK;
    if (read && n) rc = lc_csv_host(self, lines.data(), len.data(), n, W, status.data(), count.data(), rows.data());
    if (read && rc == LC_OK) {
        for (uint32_t r = 0; r < n; ++r)
            if (status[r] == LC_CSV_OK && needed(count[r]) > W) {
                wide.push_back(r);
                if (needed(count[r]) > W2) W2 = needed(count[r]);
            }
        if (!wide.empty()) {
            std::vector<const uint8_t*> wLines;
            std::vector<uint32_t> wLen, wCount(wide.size());
            std::vector<uint8_t> wStatus(wide.size());
            for (uint32_t r : wide) wLines.push_back(lines[r]), wLen.push_back(len[r]);
            wideRows.resize(wide.size() * size_t(W2) * 2);
            rc = lc_csv_host(self, wLines.data(), wLen.data(), uint32_t(wide.size()), W2, wStatus.data(), wCount.data(), wideRows.data());
        }
    }
    if (rc != LC_OK) {
        ++counters[LC_CSV_CNT_FAILED_TRIPS];
        alarm(LC_CSV_ALARM_TRIP_FAILED,
              std::string("CSV decode: the device trip failed (") + lc_last_error() + "): " + std::to_string(logs.size()) + " logs left unchanged");
        return rc;
    }
    if (read) {
        counters[LC_CSV_CNT_VALUES] += n;
        counters[LC_CSV_CNT_MOP_UP] += wide.size();
    }
    // ---- the stitch, log by log as the Go walks them
    size_t nextWide = 0;
    for (uint32_t l = 0; l < logs.size(); ++l) {
        Log& log = logs[l];
        const uint32_t r = refOfLog[l];
        if (r == kNoRef) {  // :125-127
            ++counters[LC_CSV_CNT_NO_SOURCE_KEY];
            if (NoKeyError) alarm(LC_CSV_ALARM_NO_SOURCE_KEY, "cannot find key:" + SourceKey + "\t");
            continue;
        }
        const std::string value = log.Contents[contentOfRef[r]].Value;  // (a copy: the contents move below)
        const auto append = [&](std::string key, std::string val) {
            log.Contents.push_back({std::move(key), std::move(val)});
            ++counters[LC_CSV_CNT_FIELDS];
        };
        if (nkeys == 0) {  // :61-66
            if (PreserveOthers) append("_decode_preserve_", value);
            if (!KeepSource) log.Contents.erase(log.Contents.begin() + contentOfRef[r]);
            continue;
        }
        if (cfg.invalidDelim || (status[r] != LC_CSV_OK && status[r] != LC_CSV_EOF)) {  // :74-77: the source stays whatever KeepSource says
            ++counters[LC_CSV_CNT_DECODE_ERRORS];
            alarm(LC_CSV_ALARM_DECODE, std::string("cannot decode log:") + (cfg.invalidDelim ? kInvalidDelim : sentenceOf(status[r])) + "\tlog:" + cutString(value) + "\t");
            continue;
        }
        std::vector<std::string> record;
        uint32_t fieldCount = count[r];
        if (status[r] == LC_CSV_EOF) {  // :81-83
            ++counters[LC_CSV_CNT_EOF];
            record.push_back("");
            fieldCount = 1;
        } else {
            const int32_t* row = rows.data() + size_t(r) * W * 2;
            if (nextWide < wide.size() && wide[nextWide] == r) row = wideRows.data() + (nextWide++) * size_t(W2) * 2;
            for (uint32_t k = 0; k < needed(fieldCount); ++k, row += 2) {
                const uint32_t b = uint32_t(row[0]) & ~LC_CSV_FOLD, e = uint32_t(row[1]);
                if (uint32_t(row[0]) & LC_CSV_FOLD) record.push_back(csvFold<std::string>(reinterpret_cast<const uint8_t*>(value.data()) + b, e - b));
                else record.push_back(value.substr(b, e - b));
            }
        }
        uint32_t k = 0;
        for (; k < nkeys && k < fieldCount; ++k) append(SplitKeys[k], std::move(record[k]));  // :85-88
        if (k < fieldCount && PreserveOthers) {
            if (ExpandOthers) {
                for (; k < fieldCount; ++k) append(ExpandKeyPrefix + std::to_string(k + 1 - nkeys), std::move(record[k]));  // :92-94
            } else {
                append("_decode_preserve_", writeRecord(std::vector<std::string>(record.begin() + k, record.end()), SplitSep));  // :96-102
            }
        }
        if (nkeys != fieldCount) {  // :106-108
            ++counters[LC_CSV_CNT_KEY_COUNT];
            alarm(LC_CSV_ALARM_KEY_COUNT, "decode keys not match, split len:" + std::to_string(fieldCount) + "\tlog:" + cutString(value) + "\t");
        }
        if (!KeepSource) log.Contents.erase(log.Contents.begin() + contentOfRef[r]);  // :119-121
    }
    return LC_OK;
}

}  // namespace lccsv

extern "C" int lc_csv_create(const char* config_json, size_t config_len, lc_csv_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto set = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    auto h = std::make_unique<lc_csv>();
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
        text("SplitSep", h->p.SplitSep);
        text("ExpandKeyPrefix", h->p.ExpandKeyPrefix);
        boolean("NoKeyError", h->p.NoKeyError);
        boolean("TrimLeadingSpace", h->p.TrimLeadingSpace);
        boolean("PreserveOthers", h->p.PreserveOthers);
        boolean("ExpandOthers", h->p.ExpandOthers);
        boolean("KeepSource", h->p.KeepSource);
        if (const lcjson::Value* v = cfg.find("SplitKeys"))
            if (v->isArray())
                for (const auto& k : v->arr)
                    if (k.isString()) h->p.SplitKeys.push_back(k.str);
        h->p.Init();
    } catch (const std::exception& e) {
        set(e.what());
        return LC_ERR_UNSUPPORTED;
    }
    set("");
    *out = h.release();
    return LC_OK;
}
extern "C" void lc_csv_free(lc_csv_t* p) { delete p; }

extern "C" int lc_csv_process_logs_json(lc_csv_t* h, const char* logs_json, size_t len, char** out_json) {
    if (!h || !logs_json || !out_json) return LC_ERR_ARG;
    *out_json = nullptr;
    try {
        const lcjson::Value in = lcjson::parse(std::string(logs_json, len));
        if (!in.isArray()) return LC_ERR_ARG;
        std::vector<lccsv::Log> logs;
        for (const auto& l : in.arr) {
            if (!l.isArray()) return LC_ERR_ARG;
            lccsv::Log log;
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
extern "C" void lc_csv_free_string(char* s) { std::free(s); }

extern "C" int lc_csv_counters(const lc_csv_t* p, uint64_t out[LC_CSV_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
    std::memcpy(out, p->p.counters, sizeof p->p.counters);
    return LC_OK;
}
extern "C" void lc_csv_set_alarm_sink(lc_csv_t* p, lc_alarm_sink_t sink, void* user) {
    if (!p) return;
    p->p.sink = sink;
    p->p.sinkUser = user;
}
extern "C" void lc_csv_set_first_trip_fields(lc_csv_t* p, uint32_t W) {
    if (p) p->p.firstTripFields = W;
}
