// host_err.h -- the error message of the entry points that take no bcx_solver* (projection, moments, Gram, PSVI, SVI,
// quasi-Newton, Gaussian, linear-regression posterior, Laplace, HMC, NUTS, predictive, pair statistics): one string per host
// thread, set only through bcx_fail and read by bcx_project_last_error().  Host only, and no HIP header (a HIP status takes
// hip_fail / BCX_TRY of launch_host.h; tests/host/host_err_check.cpp compiles this file alone).
#pragma once
#include <string>

inline std::string& bcx_fail_slot() {
  static thread_local std::string text;
  return text;
}
// The calling thread's message becomes "<who>: <what>"; returns `code`, so a failure path is one `return bcx_fail(...)`.
inline int bcx_fail(int code, const char* who, const std::string& what) {
  bcx_fail_slot() = std::string(who) + ": " + what;
  return code;
}
// The calling thread's message ("" before its first failure): valid and unchanged until that thread's next bcx_fail.
inline const char* bcx_fail_text() { return bcx_fail_slot().c_str(); }
