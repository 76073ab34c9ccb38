// What a C entry point of libsplatraster.so needs on the host.  include/splatraster.h is the contract; api.hip holds the
// rasterizer's entries and defines what is declared here, every other op's entries stand below its launchers in its own file.
#pragma once
#include <cstdint>
#include <string>
#include "common.h"

namespace sr {

// the calling thread's message for sr_last_error; returns 1
int fail(const std::string& msg);
// 0, or fail("<what>: <the runtime's message>")
int check_hip(hipError_t e, const char* what);

// any of these pointers (NULL counts as aligned) off a 4-byte boundary
template <typename... P>
bool any_unaligned4(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 3u) != 0; }

#define SR_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

// a job list's pointers (planegen.hip, attention.hip): inside `for (int i_ ...)`, names the job and the condition it misses
#define SR_PLANE_NEED(who, cond) do { if (!(cond)) return sr::fail(std::string("null pointer in ") + who + ", job " + std::to_string(i_) + ": needs " #cond); } while (0)

// k of a neighbour graph: knn.hip builds it, moran.hip reads it, both refuse what lies outside
constexpr int kKnnMinK = 2, kKnnMaxK = 8;

// optional per-stage timing (sr_profile_enable / sr_profile_collect): HIP events on the launch stream around the launches of
// its scope, nothing when profiling is off
struct StageTimer {
    StageTimer(int stage, hipStream_t s);
    ~StageTimer();
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
private:
    int idx = -1; hipStream_t st;
    hipEvent_t end = nullptr;
    unsigned long long serial = 0;
};

}  // namespace sr
