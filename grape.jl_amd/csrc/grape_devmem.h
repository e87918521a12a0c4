// Who owns device memory (host code only, no kernels).
//
// DeviceBufs: every buffer of a handle is requested through one of these, which frees what it handed out -- there is no list
// of pointers to keep in step.  GroupStore: the grow-only storage of a launch group (grape_eval_batch, grape_hvp,
// grape_open_hvp, grape_open_eval_batch) with the one memory-budget rule they share.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

// One hipMalloc per request: no arena, no sub-allocation -- addresses, alignment and the granularity of running out of memory
// are the runtime's.  A request of zero elements is the caller's to round up or to skip.
class DeviceBufs {
    struct Rec { void *ptr; void *slot; void (*clear)(void *slot); };
    std::vector<Rec> dev_, pinned_;
    size_t bytes_ = 0;
    template <typename T>
    static void clear_slot(void *slot) { *static_cast<T **>(slot) = nullptr; }

public:
    DeviceBufs() = default;
    DeviceBufs(const DeviceBufs &) = delete;
    DeviceBufs &operator=(const DeviceBufs &) = delete;
    ~DeviceBufs() { release(); }

    // *p = count elements of device memory, recorded and counted; on failure nothing is recorded and *p is null.  A pointer
    // that merely aliases a recorded one (d_H0p3 = d_H0q3) is never recorded, so it is never freed.
    template <typename T>
    hipError_t alloc(T **p, size_t count) {
        void *q = nullptr;
        *p = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        *p = static_cast<T *>(q);
        dev_.push_back({q, p, &clear_slot<T>});
        bytes_ += count * sizeof(T);
        return hipSuccess;
    }
    // the same for pinned host memory; bytes() does not count it
    template <typename T>
    hipError_t alloc_pinned(T **p, size_t count) {
        void *q = nullptr;
        *p = nullptr;
        const hipError_t e = hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        *p = static_cast<T *>(q);
        pinned_.push_back({q, p, &clear_slot<T>});
        return hipSuccess;
    }
    // frees everything recorded, once, in the order of the requests, and nulls the pointers it filled
    void release() {
        for (const Rec &r : dev_) { (void)hipFree(r.ptr); r.clear(r.slot); }
        for (const Rec &r : pinned_) { (void)hipHostFree(r.ptr); r.clear(r.slot); }
        dev_.clear(); pinned_.clear();
        bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }   // device memory held
};

// The storage of a launch group: `cap` units (pulse sets, directions) of `per` bytes each.  It only grows; a call with more
// units than one group holds runs several groups through the same storage.
struct GroupStore {
    DeviceBufs mem;
    int cap = 0;   // units the storage holds
    int env = 0;   // units per launch group from the environment at create (tests; 0: from the memory budget)

    void release() { mem.release(); cap = 0; }

    // units per launch group for a call that wants `want`: at most 65535 (the unit is a grid dimension of the launches), the
    // override if set; otherwise, when more is wanted than the storage holds, what fits half of the device's free memory --
    // what the storage already holds counts as free -- and budget_cap bytes, at least one
    hipError_t plan(int want, size_t per, double budget_cap, int *units) const {
        int n = std::min(want, 65535);
        if (env > 0) n = std::min(n, env);
        else if (n > cap) {
            size_t free_b = 0, total_b = 0;
            const hipError_t e = hipMemGetInfo(&free_b, &total_b);
            if (e != hipSuccess) return e;
            const double budget = std::min(0.5 * ((double)free_b + (double)mem.bytes()), budget_cap);
            n = (int)std::max<double>(1.0, std::min<double>((double)n, std::floor(budget / (double)per)));
        }
        *units = n;
        return hipSuccess;
    }

    // what a layout callback asks through: one alloc per buffer, nothing more after the first failure
    struct Requests {
        DeviceBufs &mem;
        hipError_t err = hipSuccess;
        template <typename T>
        void operator()(T **p, size_t count) { if (err == hipSuccess) err = mem.alloc(p, count); }
    };
    enum class Grow { fits, grown, sync_failed, alloc_failed };

    // storage for `units`: nothing when they fit; else wait for the stream (work on the old storage may be in flight), release,
    // and run layout(requests).  A failed request releases everything and leaves cap at 0.  *err: the HIP error of a failure.
    template <typename Layout>
    Grow grow(int units, hipStream_t stream, Layout &&layout, hipError_t *err) {
        if (units <= cap) return Grow::fits;
        if ((*err = hipStreamSynchronize(stream)) != hipSuccess) return Grow::sync_failed;
        release();
        Requests get{mem};
        layout(get);
        if ((*err = get.err) != hipSuccess) { release(); return Grow::alloc_failed; }
        cap = units;
        return Grow::grown;
    }

    static std::string oom_message(const char *call, int units, const char *unit_word, size_t per, const char *env_name) {
        return std::string(call) + ": out of device memory for the storage of " + std::to_string(units) + " " + unit_word + " (" +
               std::to_string(per * (size_t)units >> 20) + " MB); " + env_name + "=<n> makes the launch groups smaller";
    }
};
