// strptime_program.cpp -- see strptime_program.hpp.
#include "strptime_program.hpp"

#include <vector>

namespace {
constexpr unsigned kAltE = 1, kAltO = 2;

bool isSpaceByte(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

// one call of strptime_ns on `fmt`: its own split_year, its own modifier state
void compileInto(const char* fmt, std::vector<uint32_t>& ops) {
    bool splitYear = false;
    const auto num = [&](StrptimeField f, uint32_t llim, uint32_t ulim) { ops.push_back(tsWord(TS_OP_NUM, f, llim, ulim)); };
    const auto fail = [&] { ops.push_back(tsWord(TS_OP_FAIL)); };
    while (unsigned char c = static_cast<unsigned char>(*fmt++)) {
        unsigned alt = 0;
        if (isSpaceByte(c)) {
            ops.push_back(tsWord(TS_OP_SPACE));
            continue;
        }
        if (c != '%') {
            ops.push_back(tsWord(TS_OP_LIT, c));
            continue;
        }
        // LEGAL_ALT(x) BEHIND a conversion's effects: the value fails there when a modifier outside x is set
        const auto legalAfter = [&](unsigned allowed) {
            if (alt & ~allowed) fail();
            return !(alt & ~allowed);
        };
        bool stop = false;
        for (bool again = true; again && !stop;) {
            again = false;
            c = static_cast<unsigned char>(*fmt);
            if (c) ++fmt;
            const char* composite = nullptr;
            switch (c) {
                case '%':
                    ops.push_back(tsWord(TS_OP_LIT, '%'));
                    stop = !legalAfter(0);
                    break;
                case 'E':
                case 'O':
                    if (alt) {
                        fail();
                        stop = true;
                    } else {
                        alt |= c == 'E' ? kAltE : kAltO;
                        again = true;
                    }
                    break;
                case 'c': composite = "%a %b %d %H:%M:%S %Y"; break;
                case 'X': composite = "%H:%M:%S"; break;
                case 'x': composite = "%m/%d/%y"; break;
                case 'D': case 'F': case 'R': case 'r': case 'T':
                    if (alt) {
                        fail();
                        stop = true;
                        break;
                    }
                    composite = c == 'D' ? "%m/%d/%y" : c == 'F' ? "%Y-%m-%d" : c == 'R' ? "%H:%M" : c == 'r' ? "%I:%M:%S %p" : "%H:%M:%S";
                    break;
                case 'A': case 'a':
                    ops.push_back(tsWord(TS_OP_NAME, TS_NAME_DAY));
                    stop = !legalAfter(0);
                    break;
                case 'B': case 'b': case 'h':
                    ops.push_back(tsWord(TS_OP_NAME, TS_NAME_MON));
                    stop = !legalAfter(0);
                    break;
                case 'C':
                    num(splitYear ? TS_F_CENT_SPLIT : TS_F_CENT_FIRST, 0, 99);
                    splitYear = true;
                    stop = !legalAfter(kAltE);
                    break;
                case 'd': case 'e':
                    num(TS_F_MDAY, 1, 31);
                    stop = !legalAfter(kAltO);
                    break;
                case 'f':
                    ops.push_back(tsWord(TS_OP_FRAC));
                    stop = !legalAfter(kAltO);
                    break;
                case 'k': case 'H':
                    if (c == 'k' && alt) {
                        fail();
                        stop = true;
                        break;
                    }
                    num(TS_F_HOUR, 0, 23);
                    stop = !legalAfter(kAltO);
                    break;
                case 'l': case 'I':
                    if (c == 'l' && alt) {
                        fail();
                        stop = true;
                        break;
                    }
                    num(TS_F_HOUR12, 1, 12);
                    stop = !legalAfter(kAltO);
                    break;
                case 'j':  // parsed, range-checked, and of no effect on the second (mktime does not read tm_yday)
                    num(TS_F_IGNORE, 1, 366);
                    stop = !legalAfter(0);
                    break;
                case 'M':
                    num(TS_F_MIN, 0, 59);
                    stop = !legalAfter(kAltO);
                    break;
                case 'm':
                    num(TS_F_MON1, 1, 12);
                    stop = !legalAfter(kAltO);
                    break;
                case 'p':
                    ops.push_back(tsWord(TS_OP_NAME, TS_NAME_AMPM));
                    stop = !legalAfter(0);
                    break;
                case 'S':
                    num(TS_F_SEC, 0, 61);
                    stop = !legalAfter(kAltO);
                    break;
                case 'U': case 'W':
                    num(TS_F_IGNORE, 0, 53);
                    stop = !legalAfter(kAltO);
                    break;
                case 'w':
                    num(TS_F_IGNORE, 0, 6);
                    stop = !legalAfter(kAltO);
                    break;
                case 'u':
                    num(TS_F_IGNORE, 1, 7);
                    stop = !legalAfter(kAltO);
                    break;
                case 'g':
                    num(TS_F_IGNORE, 0, 99);
                    break;
                case 'G':
                    ops.push_back(tsWord(TS_OP_SKIP_G));
                    break;
                case 'V':
                    num(TS_F_IGNORE, 0, 53);
                    break;
                case 'Y':
                    num(TS_F_YEAR4, 0, 9999);
                    stop = !legalAfter(kAltE);
                    break;
                case 'y':
                    num(splitYear ? TS_F_YY_SPLIT : TS_F_YY_FIRST, 0, 99);
                    splitYear = true;
                    break;
                case 'Z':
                    ops.push_back(tsWord(TS_OP_ZNAME));
                    break;
                case 'z':
                    ops.push_back(tsWord(TS_OP_ZOFF));
                    break;
                case 'n': case 't':
                    ops.push_back(tsWord(TS_OP_SPACE));
                    stop = !legalAfter(0);
                    break;
                default:  // unknown conversion, "%s" inside a longer format and the end of the format among them
                    fail();
                    stop = true;
                    break;
            }
            if (composite) {
                ops.push_back(tsWord(TS_OP_RESET_NS));
                compileInto(composite, ops);
                stop = !legalAfter(kAltE);
            }
        }
        if (stop) return;  // every value has failed by here: what follows in the format is never reached
    }
}
}  // namespace

bool strptimeCompile(const std::string& format, StrptimeProgram* out, std::string* error) {
    std::vector<uint32_t> ops;
    // (an embedded NUL ends the format, as it ends the reference's C string)
    const std::string fmt = format.substr(0, format.find('\0'));
    if (fmt == "%s") ops.push_back(tsWord(TS_OP_EPOCH));
    else compileInto(fmt.c_str(), ops);
    if (ops.size() > kStrptimeMaxOps) {
        if (error)
            *error = "SourceFormat compiles to " + std::to_string(ops.size()) + " steps, the device program window holds " +
                     std::to_string(kStrptimeMaxOps);
        return false;
    }
    out->n = uint32_t(ops.size());
    for (uint32_t i = 0; i < kStrptimeMaxOps; ++i) out->words[i] = i < ops.size() ? ops[i] : tsWord(TS_OP_FAIL);
    return true;
}
