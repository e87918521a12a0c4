// Stand-alone check of csrc/grape_devmem.h under -fsanitize=address,undefined (tests/test_devmem_host.py builds and runs it).
// The six HIP calls the header makes are defined here over malloc / free, so the program links without the HIP runtime and
// needs no device.  Expected values of the planning rule are worked out by hand from the rule as grape_eval_batch, grape_hvp,
// grape_open_hvp and grape_open_eval_batch state it: min(want, 65535); the override; else, when more is wanted than held,
// max(1, min(want, floor(min(0.5 (free + held), cap) / per))).
#include "grape_devmem.h"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {
size_t g_free = 0;              // what hipMemGetInfo reports
long g_allocs = 0, g_frees = 0, g_meminfo = 0, g_syncs = 0;
long g_fail_at = 0;             // the n-th device allocation from now fails (0: none)
std::set<void *> g_dev, g_pinned;   // live allocations

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)
size_t live() { return g_dev.size() + g_pinned.size(); }
}  // namespace

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) {
    ++g_allocs;
    if (g_fail_at && --g_fail_at == 0) return hipErrorOutOfMemory;
    *ptr = std::malloc(size ? size : 1);
    g_dev.insert(*ptr);
    return hipSuccess;
}
hipError_t hipFree(void *ptr) {
    ++g_frees;
    CHECK(g_dev.erase(ptr) == 1);   // (freed twice, or never allocated)
    std::free(ptr);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) {
    *ptr = std::malloc(size ? size : 1);
    g_pinned.insert(*ptr);
    return hipSuccess;
}
hipError_t hipHostFree(void *ptr) {
    CHECK(g_pinned.erase(ptr) == 1);
    std::free(ptr);
    return hipSuccess;
}
hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b) {
    ++g_meminfo;
    *free_b = g_free; *total_b = 2 * g_free;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
}

namespace {
constexpr size_t MB = 1 << 20, GB = 1 << 30;
constexpr double CAP8 = 8.0 * 1073741824.0;

struct Bufs4 { double *a = nullptr; int *b = nullptr; unsigned long long *c = nullptr; double *d = nullptr; };

// four buffers of a, 2a, a, 4a elements per unit: (8 + 8 + 8 + 32) a bytes
GroupStore::Grow grow4(GroupStore &g, Bufs4 &p, int units, size_t a, hipError_t *e) {
    return g.grow(units, nullptr, [&](GroupStore::Requests &get) {
        const size_t n = (size_t)units;
        get(&p.a, n * a); get(&p.b, n * 2 * a); get(&p.c, n * a); get(&p.d, n * 4 * a);
    }, e);
}

void case_a_release_twice() {
    DeviceBufs m;
    double *x = nullptr; int *y = nullptr; double *pin = nullptr;
    CHECK(m.alloc(&x, 100) == hipSuccess && m.alloc(&y, 7) == hipSuccess && m.alloc_pinned(&pin, 50) == hipSuccess);
    x[99] = 1.0; y[6] = 2; pin[49] = 3.0;
    CHECK(live() == 3 && m.bytes() == 100 * 8 + 7 * 4);   // (pinned memory is not counted)
    m.release();
    CHECK(live() == 0 && m.bytes() == 0 && !x && !y && !pin);
    const long frees = g_frees;
    m.release();
    CHECK(g_frees == frees && live() == 0);
    {   // what is still held when the owner goes is freed with it
        DeviceBufs scoped;
        CHECK(scoped.alloc(&x, 4) == hipSuccess && live() == 1);
    }
    CHECK(live() == 0);
    // a failed request records nothing
    g_fail_at = 1;
    CHECK(m.alloc(&x, 10) == hipErrorOutOfMemory && !x && m.bytes() == 0 && live() == 0);
}

void case_b_alias() {
    DeviceBufs m;
    double *q = nullptr, *p = nullptr;
    CHECK(m.alloc(&q, 16) == hipSuccess);
    p = q;   // (Hermitian operators: the adjoint array IS the plain one -- never requested, never recorded)
    const long frees = g_frees;
    m.release();
    CHECK(g_frees == frees + 1 && live() == 0 && !q && p);
}

void case_c_failure_at_each_position() {
    for (int held = 0; held <= 2; held += 2)        // from empty, and from a storage that holds two units
        for (int pos = 1; pos <= 4; ++pos) {
            GroupStore g;
            Bufs4 p;
            hipError_t e = hipSuccess;
            if (held) CHECK(grow4(g, p, held, 10, &e) == GroupStore::Grow::grown && g.cap == held);
            g_fail_at = pos;
            CHECK(grow4(g, p, 4, 10, &e) == GroupStore::Grow::alloc_failed && e == hipErrorOutOfMemory);
            CHECK(g.cap == 0 && g.mem.bytes() == 0 && live() == 0 && !p.a && !p.b && !p.c && !p.d);
            CHECK(g_fail_at == 0);                  // (nothing was requested behind the failure: the switch fired exactly once)
            CHECK(grow4(g, p, 4, 10, &e) == GroupStore::Grow::grown && e == hipSuccess && g.cap == 4 && live() == 4);
            CHECK(p.a && p.b && p.c && p.d);
            p.d[4 * 4 * 10 - 1] = 1.0;
        }
    CHECK(live() == 0);
}

void case_d_grow_only() {
    GroupStore g;
    Bufs4 p;
    hipError_t e = hipSuccess;
    const long syncs = g_syncs;
    CHECK(grow4(g, p, 4, 10, &e) == GroupStore::Grow::grown && g.cap == 4 && g.mem.bytes() == 4 * 56 * 10 && g_syncs == syncs + 1);
    CHECK(grow4(g, p, 8, 10, &e) == GroupStore::Grow::grown && g.cap == 8 && g.mem.bytes() == 8 * 56 * 10 && live() == 4);
    const double *a = p.a;
    const long allocs = g_allocs, frees = g_frees, syncs2 = g_syncs;
    CHECK(grow4(g, p, 1, 10, &e) == GroupStore::Grow::fits && g.cap == 8 && g.mem.bytes() == 8 * 56 * 10 && p.a == a);
    CHECK(g_allocs == allocs && g_frees == frees && g_syncs == syncs2);
    g.release();
    CHECK(g.cap == 0 && g.mem.bytes() == 0 && live() == 0 && !p.a);
}

void case_e_plan() {
    int n = 0;
    {
        GroupStore g;
        g_free = (size_t)1 << 40;
        CHECK(g.plan(70000, 1024, CAP8, &n) == hipSuccess && n == 65535);            // the grid dimension
        g.env = 2;
        const long mi = g_meminfo;
        CHECK(g.plan(70000, 1024, CAP8, &n) == hipSuccess && n == 2);                // the override ...
        CHECK(g.plan(1, 1024, CAP8, &n) == hipSuccess && n == 1 && g_meminfo == mi); // ... never raises, never asks the device
    }
    {
        GroupStore g;
        g_free = 10 * MB;
        CHECK(g.plan(100, MB, CAP8, &n) == hipSuccess && n == 5);                    // half of what is free
        CHECK(g.plan(3, MB, CAP8, &n) == hipSuccess && n == 3);                      // ... when less is wanted
        double *buf = nullptr;
        hipError_t e = hipSuccess;
        CHECK(g.grow(4, nullptr, [&](GroupStore::Requests &get) { get(&buf, 4 * MB / 8); }, &e) == GroupStore::Grow::grown);
        CHECK(g.mem.bytes() == 4 * MB);
        CHECK(g.plan(100, MB, CAP8, &n) == hipSuccess && n == 7);                    // what is held counts as free: 0.5 (10 + 4)
        const long mi = g_meminfo;
        CHECK(g.plan(4, MB, CAP8, &n) == hipSuccess && n == 4 && g_meminfo == mi);   // wanted <= held: the device is not asked
        CHECK(g.plan(2, MB, CAP8, &n) == hipSuccess && n == 2 && g_meminfo == mi);
        g_free = 0;
        CHECK(g.plan(4, MB, CAP8, &n) == hipSuccess && n == 4);                      // ... whatever is free
    }
    {
        GroupStore g;
        g_free = 100 * GB;
        CHECK(g.plan(100, GB, CAP8, &n) == hipSuccess && n == 8);                    // the cap, 8 GB
        CHECK(g.plan(100, GB, 2 * CAP8, &n) == hipSuccess && n == 16);               // ... 16 GB (grape_eval_batch)
        g_free = GB / 2;
        CHECK(g.plan(100, GB, CAP8, &n) == hipSuccess && n == 1);                    // the floor: one unit is always tried
    }
}

void case_f_zero_count_skipped() {
    GroupStore g;
    double *eps = nullptr, *Sf = nullptr, *pin = nullptr;
    hipError_t e = hipSuccess;
    const size_t counts[2] = {24, 0};
    CHECK(g.grow(3, nullptr, [&](GroupStore::Requests &req) {
        auto get = [&](auto **ptr, size_t count) { if (count) req(ptr, count); };   // (the closed batch storage)
        get(&eps, 3 * counts[0]); get(&Sf, 3 * counts[1]);
    }, &e) == GroupStore::Grow::grown);
    CHECK(eps && !Sf && live() == 1 && g.mem.bytes() == 3 * 24 * 8);
    CHECK(g.mem.alloc_pinned(&pin, 16) == hipSuccess && live() == 2 && g.mem.bytes() == 3 * 24 * 8);
    g.release();
    CHECK(live() == 0 && !eps && !pin);
}

void case_message() {
    CHECK(GroupStore::oom_message("grape_hvp", 3, "directions", 5 * MB / 2, "GRAPE_HVP_DIRS") ==
          "grape_hvp: out of device memory for the storage of 3 directions (7 MB); GRAPE_HVP_DIRS=<n> makes the launch groups smaller");
    CHECK(GroupStore::oom_message("grape_open_eval_batch", 12, "pulse sets", 100 * MB, "GRAPE_OPEN_BATCH_SETS") ==
          "grape_open_eval_batch: out of device memory for the storage of 12 pulse sets (1200 MB); GRAPE_OPEN_BATCH_SETS=<n> makes "
          "the launch groups smaller");
}
}  // namespace

int main() {
    case_a_release_twice();
    case_b_alias();
    case_c_failure_at_each_position();
    case_d_grow_only();
    case_e_plan();
    case_f_zero_count_skipped();
    case_message();
    CHECK(live() == 0);
    std::printf("devmem-driver OK\n");
    return 0;
}
