// check.h -- what the stand-alone host check programs share.  Each is built from its own file and
// csrc/dcor_plan.cpp alone with a host compiler (no HIP, no device); exit status 0: every check held.
// heap() gives a block of exactly the vector's length, so a planner that reads past its segments,
// masks or eta is caught when the program is built with a sanitizer.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dcor_plan.h"

using namespace dcor;
using namespace dcor::host;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static inline std::string last_error() {
  char buf[512];
  dcor_last_error(buf, sizeof(buf));
  return buf;
}
// The call returns `code`; its message contains `msg` (CHECK_FAILS) or is `msg` (CHECK_FAILS_EXACT).
#define CHECK_MESSAGE(call, code, matches)                                 \
  do {                                                                     \
    CHECK((call) == (code));                                               \
    if (!(matches)) {                                                      \
      std::fprintf(stderr, "%s:%d: message '%s'\n", __FILE__, __LINE__, last_error().c_str()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)
#define CHECK_FAILS(call, code, msg) CHECK_MESSAGE(call, code, last_error().find(msg) != std::string::npos)
#define CHECK_FAILS_EXACT(call, code, msg) CHECK_MESSAGE(call, code, last_error() == (msg))

template <class T>
static inline std::unique_ptr<T[]> heap(const std::vector<T>& v) {   // exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}
