// The library's last-error string (rdyhip_last_error) and fail(), which sets it and returns the code.  C++17 inline
// definitions: the library and a stand-alone host program that includes host_layout.h share them.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

namespace rdyhip {

inline thread_local std::string g_err;

inline int fail(int code, const char *fmt, ...) {
  char    buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace rdyhip
