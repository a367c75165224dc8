// errors.h — how libearhip's host code reports a failure: the exception every layer throws, the thread-local error
// string, and the translation into a status code at the C boundary.  The status codes of include/earhip.h and the
// standard library, nothing else: code that needs no device (host_pipeline.h) includes this and not common.h.
#pragma once

#include <exception>
#include <new>
#include <string>

#include "../../include/earhip.h"

namespace earhip {

struct Error {
  int code;
  std::string msg;
};

void set_last_error(const std::string &msg);

// Runs f, translating earhip::Error / std::exception into a status code.
template <typename F>
int guarded(F &&f) {
  try {
    f();
    return EARHIP_OK;
  } catch (const Error &e) {
    set_last_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc &) {
    set_last_error("out of host memory");
    return EARHIP_INTERNAL_ERROR;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return EARHIP_INTERNAL_ERROR;
  }
}

[[noreturn]] inline void fail_invalid(const std::string &m) {
  throw Error{EARHIP_INVALID_ARGUMENT, m};
}
[[noreturn]] inline void fail_internal(const std::string &m) {
  throw Error{EARHIP_INTERNAL_ERROR, "internal error: " + m};
}
inline void require(bool ok, const char *m) {
  if (!ok) fail_invalid(m);
}

}  // namespace earhip
