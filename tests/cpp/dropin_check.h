// What the test_dropin*.cpp programs count their checks with: CHECK, CHECK_THROWS_AS and the summary line the Python tests read.
#pragma once
#include <cstdio>

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    g_checks++;                                                     \
    if (!(cond)) {                                                  \
      g_failed++;                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                               \
  } while (0)
// one check: expr throws a `type`
#define CHECK_THROWS_AS(expr, type) \
  do {                              \
    bool thrown_ = false;           \
    try {                           \
      expr;                         \
    } catch (const type &) {        \
      thrown_ = true;               \
    }                               \
    CHECK(thrown_);                 \
  } while (0)

// prints "N passed, M failed", after "prefix: " if there is one; true when a check failed: main returns it
static inline bool summary(const char *prefix = nullptr) {
  if (prefix) std::printf("%s: ", prefix);
  std::printf("%d passed, %d failed\n", g_checks - g_failed, g_failed);
  return g_failed != 0;
}
