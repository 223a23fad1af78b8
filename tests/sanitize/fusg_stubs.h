// What a translation unit of csrc/ expects of the rest of the library, for the stand-alone sanitizer programs of this directory:
// declarations and trivial bodies only.  Each program includes this once, next to its own main, and is linked with the one
// translation unit it checks; errors go to stderr, nothing is ever recording and no routing batch is set.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <hip/hip_runtime.h>
#include "../../include/fusg.h"

namespace fusg {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}
bool plan_recording() { return false; }
void plan_append(hipStream_t, std::function<int(hipStream_t)>) {}
int32_t route_batch_now() { return 0; }
struct RouteBatchScope {
    int32_t prev;
    explicit RouteBatchScope(int32_t r);
    ~RouteBatchScope();
};
RouteBatchScope::RouteBatchScope(int32_t) : prev(0) {}
RouteBatchScope::~RouteBatchScope() {}
}  // namespace fusg
