// strptime_program.hpp -- the format compiler of processor_parse_timestamp_gpu (host only, HIP-free): SourceFormat -> the linear program
// strptimeRun() of strptime_vm.hpp executes.  It accepts what the reference's strptime_ns (core/common/Strptime.cpp) accepts and fails
// where it fails: a conversion it does not know, or a modifier a conversion does not allow, becomes a FAIL op at the place where the
// reference returns NULL -- behind the effects it has had by then.  Composite conversions (%D %F %R %r %T %c %x %X) are expanded inline;
// whether %y / %C meet a century or a year that came before them is known from the format alone and is resolved here.
// Out of scope: locales other than C (the reference has none either).
#pragma once

#include <string>

#include "strptime_vm.hpp"

// false (and `error`) when the program does not fit the kernel's window of kStrptimeMaxOps ops
bool strptimeCompile(const std::string& format, StrptimeProgram* out, std::string* error);
