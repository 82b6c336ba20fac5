// Status-code plumbing of the libmsfno translation units: the thread's last error message
// and the early-return macros.  No HIP here: tables.cpp builds with a plain host compiler.
#pragma once
#include <string>

#include "../../include/msfno.h"

namespace msfno {

void set_error(const std::string& msg);

#define MSFNO_REQUIRE(cond, code, msg)          \
  do {                                          \
    if (!(cond)) {                              \
      ::msfno::set_error(msg);                  \
      return (code);                            \
    }                                           \
  } while (0)

#define MSFNO_TRY(expr)              \
  do {                               \
    int _rc = (expr);                \
    if (_rc != MSFNO_OK) return _rc; \
  } while (0)

}  // namespace msfno
