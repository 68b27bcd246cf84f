// What the stand-alone host programs of this directory share (orb*_host_check.hip: each has its own main, is compiled together with one csrc/orb*.hip with the
// host side under AddressSanitizer and UndefinedBehaviorSanitizer, and touches no device).
//
// Why the stubs: the entry points report a refusal through nq_fail and open a profiler scope (NQ_PROF) before they launch.  In the library both hooks of
// csrc/common.h are defined by engine.hip, which would pull the whole engine into these programs; they are defined here for the programs alone.  nq_fail keeps
// the message, so that a program can ask which check refused a call; the profiler scope does nothing (no call below gets as far as a stream).
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../nabladft_amd/csrc/orbstate.h"

thread_local char nq_err_buf[512] = "";
int nq_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(nq_err_buf, sizeof(nq_err_buf), fmt, ap);
  va_end(ap);
  return code;
}
int nq_profile_on = 0;
NqProfScope::NqProfScope(hipStream_t s, const char*) : st(s), slot(-1) {}
NqProfScope::~NqProfScope() {}
void NqProfScope::add_flops(double) {}

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, nq_err_buf); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)
// the call is refused as a bad argument, and by the check whose message holds `word`
#define REFUSED(call, word) EXPECT((call) == NQ_ERR_ARG && strstr(nq_err_buf, word))

// the last statement of main: "<name>: ok" and 0, or the count of failed expectations and 1
static int host_check_report(const char* name) {
  if (failures) {
    fprintf(stderr, "%s: %d failure(s)\n", name, failures);
    return 1;
  }
  printf("%s: ok\n", name);
  return 0;
}
