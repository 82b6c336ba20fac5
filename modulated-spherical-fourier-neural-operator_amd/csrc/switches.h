// Run-time switches (the MSFNO_* environment variables of DESIGN.md §9b): the one place
// that says how a switch is read, and the only getenv() in csrc/.  Plain C++17, no HIP.
//
// Switches are A/B only: each selects between two kept implementations so that they can
// be measured against each other; the default is the measured winner and nothing but a
// test or a measurement sets one.  A switch that has lost is retired with the code only
// it reaches ("Retired in round ...").
//
// The rules, for a variable that is unset / set to the string v:
//   sw_raw(n)        nullptr / v.  For values that are not flags: MSFNO_MH_TRACE (a file
//                    name; "" counts as unset at the call site), MSFNO_SKIP_GRID (atof).
//   sw_set(n)        false / true, also for v = "" (MSFNO_NO_SYM).
//   sw_char(n)       '\0' / the first character of v ('\0' for v = "").  Call sites
//                    compare it with one digit (MSFNO_X3F_NS '2', MSFNO_MG_PG '1').
//   sw_on(n)         on unless v starts with '0': true / sw_char(n) != '0'.  "", "1",
//                    "10", "x6", "-3" are on; "0", "00" are off.  The default-on switches.
//   sw_is1(n)        on only if v starts with '1': false / sw_char(n) == '1'.  "1", "10"
//                    are on; "", "0", "x6" are off.  The default-off switches.
//   sw_is1_or(n, d)  d / sw_is1(n): a switch that follows another setting (the engine)
//                    unless it is set; set to "" it is off (MSFNO_LEG_X3, _SPEC_X3H,
//                    _SKIP_X3H).
//   sw_eq(n, w)      false / v == w, the whole string ("x6 " is not "x6"):
//                    MSFNO_ENGINE=x6, MSFNO_GEMM=f32.
//   sw_int(n, d)     d / atoi(v): leading blanks, an optional sign and the leading digits,
//                    0 if there are none ("" and "x6" give 0, "4x128" 4, "-3" -3, "10" 10):
//                    MSFNO_X3C_BM64, MSFNO_C2R_WV.
//
// Nothing here caches.  A value is cached for the process by the `static const` at its
// call site.  Exactly these are read on every call instead, because tests flip them
// inside one process: MSFNO_SIDE_STREAM, MSFNO_SKIP_P, MSFNO_SKIP_GRID, MSFNO_MG_EARLY,
// MSFNO_MH_TRACE, and MSFNO_NO_SYM (at every table load).
#pragma once
#include <cstdlib>
#include <cstring>

namespace msfno {

inline const char* sw_raw(const char* name) { return std::getenv(name); }

inline bool sw_set(const char* name) { return sw_raw(name) != nullptr; }

inline char sw_char(const char* name) {
  const char* e = sw_raw(name);
  return e ? e[0] : '\0';
}

inline bool sw_on(const char* name) { return sw_char(name) != '0'; }

inline bool sw_is1(const char* name) { return sw_char(name) == '1'; }

inline bool sw_is1_or(const char* name, bool unset) {
  return sw_set(name) ? sw_is1(name) : unset;
}

inline bool sw_eq(const char* name, const char* word) {
  const char* e = sw_raw(name);
  return e && std::strcmp(e, word) == 0;
}

inline int sw_int(const char* name, int unset) {
  const char* e = sw_raw(name);
  return e ? std::atoi(e) : unset;
}

}  // namespace msfno
