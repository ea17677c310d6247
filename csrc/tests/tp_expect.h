// The failure counter and the EXPECT macro of the host validation programs (*_validation.cpp): a
// failed condition is reported with its location and counted; main() returns non-zero when any failed.
#pragma once
#include <cstdio>

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)
