// The parked-thread type of the host code (lora_sdr_amd/csrc/lorahip_worker.h) on its own: a plain C++ program over that header and
// the standard library, no HIP, no GPU. It exits non-zero with a message on the first case that fails. tests/test_worker_cpu.py
// builds it plainly and runs it; under the sanitizers it is built and run by hand, on a machine's CPU only:
//
//   g++     -std=c++17 -O2 -pthread                                    -I lora_sdr_amd/csrc tests/worker_check.cpp -o worker_check
//   clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread               -I lora_sdr_amd/csrc tests/worker_check.cpp -o worker_check_tsan
//   g++     -std=c++17 -O1 -g -pthread -fsanitize=address,undefined    -I lora_sdr_amd/csrc tests/worker_check.cpp -o worker_check_asan
//
// The fan-out case restates how lorahip_upload.cpp uses the type (its Seg, copyShare and CopyPool::run, without the HIP around them):
// the pool it replaced, one shared mailbox with a generation counter, fails exactly there -- a helper created after the pool had run a
// job could run that job again, on a segment list that was freed since (lorahip_upload.cpp:93).
#include "lorahip_worker.h"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using lorahip::ParkedThread;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "worker_check: %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); \
                                             std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

// the library's last error, restated: one text per thread
static thread_local std::string lastError;

//! what the containers do (lorahip_own.h, runOnThreads): the failing task's text is read on the worker and handed to the caller
template <class ThreadOf, class Fn> static int runWithText(const size_t n, const ThreadOf &threadOf, const Fn &fn)
{
    std::vector<std::string> err(n);
    size_t failed = 0;
    const int rc = lorahip::runOnAll(n, threadOf, [&](const size_t i) { const int r = fn(i); if (r != 0) err[i] = lastError; return r; }, &failed);
    if (rc != 0) lastError = err[failed];
    return rc;
}

static void roundTrips()
{
    ParkedThread t;
    CHECK(t.start(), "start");
    CHECK(t.start(), "a second start is a no-op");
    long sum = 0;
    for (int i = 0; i < 5000; i++)
    {
        auto task = [&sum, i] { sum += i; return i % 7 == 3 ? -i : i; };
        t.post(task);
        const int rc = t.wait();
        CHECK(rc == (i % 7 == 3 ? -i : i), "round trip %d returned %d", i, rc);
    }
    CHECK(sum == 5000L * 4999 / 2, "tasks ran %ld, not once each", sum);
    // the wrapper: codes and texts of the worker's thread reach the caller's
    const auto only = [&t](size_t) { return &t; };
    for (int i = 0; i < 2000; i++)
    {
        lastError = "the caller's own";
        const int rc = runWithText(1, only, [i](size_t) { if (i % 3) return 0; lastError = "task " + std::to_string(i); return -2; });
        CHECK(rc == (i % 3 ? 0 : -2), "wrapped round trip %d returned %d", i, rc);
        CHECK(lastError == (i % 3 ? std::string("the caller's own") : "task " + std::to_string(i)), "wrapped round trip %d: text '%s'", i, lastError.c_str());
    }
}

static void destruction()
{
    for (int i = 0; i < 300; i++)
    {
        { ParkedThread never; }
        { ParkedThread idle; CHECK(idle.start(), "start"); }
        std::atomic<int> ran{0};
        auto task = [&ran] { std::this_thread::sleep_for(std::chrono::microseconds(200)); ran = 1; return 0; };       // (declared first: it outlives the thread)
        {
            ParkedThread t;
            CHECK(t.start(), "start");
            t.post(task);
        }
        CHECK(ran == 1, "the destructor returned before the posted task had run (repetition %d)", i);
    }
}

// ---- the upload's fan-out -------------------------------------------------------------------------------------------------------
struct Seg { char *dst; const char *src; size_t bytes; };

static void copyShare(const std::vector<Seg> &segs, const size_t share, const int k)
{
    const size_t lo = size_t(k) * share, hi = lo + share;
    size_t at = 0;
    for (const Seg &s : segs)
    {
        const size_t a = at > lo ? at : lo, b = (at + s.bytes) < hi ? (at + s.bytes) : hi;
        if (a < b) std::memcpy(s.dst + (a - at), s.src + (a - at), b - a);
        at += s.bytes;
        if (at >= hi) break;
    }
}

struct Pool
{
    struct Helper
    {
        const std::vector<Seg> *segs = nullptr;
        size_t share = 0;
        int k = 0;
        ParkedThread th;
        int operator()() const { copyShare(*segs, share, k); return 0; }
    };
    std::vector<std::unique_ptr<Helper>> helper;
    int emptySlot = 0;                                    // the helper whose start "fails" (0: none)

    void start(const int T)
    {
        if (helper.size() < size_t(T - 1)) helper.resize(size_t(T - 1));
        for (int k = 1; k < T; k++)
        {
            if (helper[size_t(k - 1)] || k == emptySlot) continue;
            auto h = std::make_unique<Helper>();
            if (h->th.start()) helper[size_t(k - 1)] = std::move(h);
        }
    }
    void run(const std::vector<Seg> &s, const size_t total, const int T)
    {
        start(T);
        const size_t sh = (total + size_t(T) - 1) / size_t(T);
        const auto helperOf = [&](const int k) { return size_t(k - 1) < helper.size() ? helper[size_t(k - 1)].get() : nullptr; };
        for (int k = 1; k < T; k++)
            if (Helper *h = helperOf(k)) { h->segs = &s; h->share = sh; h->k = k; h->th.post(*h); }
        copyShare(s, sh, 0);
        for (int k = 1; k < T; k++) if (helperOf(k) == nullptr) copyShare(s, sh, k);
        for (int k = 1; k < T; k++) if (Helper *h = helperOf(k)) (void)h->th.wait();
    }
};

//! one staging fill: a fresh source, a fresh destination and a heap-allocated segment list that dies right after the job
static void fill(Pool &pool, const int T, const unsigned seed)
{
    static const size_t lens[] = {70001, 3, 262144, 99991, 1, 150000, 8191, 40960};
    size_t total = 0;
    for (const size_t n : lens) total += n;
    std::unique_ptr<char[]> src(new char[total]), dst(new char[total]);
    unsigned long long x = seed * 2654435761ull + 1u;
    for (size_t i = 0; i < total; i += sizeof(x))
    {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        std::memcpy(src.get() + i, &x, total - i < sizeof(x) ? total - i : sizeof(x));
    }
    std::memset(dst.get(), 0, total);
    {
        std::unique_ptr<std::vector<Seg>> segs(new std::vector<Seg>());
        size_t at = 0;
        for (const size_t n : lens) { segs->push_back(Seg{dst.get() + at, src.get() + at, n}); at += n; }
        pool.run(*segs, total, T);
    }
    CHECK(std::memcmp(src.get(), dst.get(), total) == 0, "fan-out with T = %d: the copy differs from its source", T);
}

static void fanOut()
{
    for (unsigned rep = 0; rep < 300; rep++)
    {
        Pool pool;
        pool.emptySlot = rep % 3 == 2 ? 4 : 0;            // every third repetition: helper 4 "could not be started", the caller copies share 4
        fill(pool, 2, rep);                               // one helper
        fill(pool, 6, rep + 1000);                        // four more join a pool that has already run a job
        CHECK(pool.helper.size() == 5 && (pool.helper[3] == nullptr) == (pool.emptySlot == 4), "helper slots");
        fill(pool, 3, rep + 2000);                        // T smaller than the helpers that exist: the others are posted nothing
        fill(pool, 6, rep + 3000);
    }
}

static void postAllWaitAll()
{
    const size_t n = 5;
    std::vector<std::unique_ptr<ParkedThread>> th(n);
    for (size_t i = 0; i < n; i++)
        if (i != 2) { th[i] = std::make_unique<ParkedThread>(); CHECK(th[i]->start(), "start"); }          // (slot 2 stays empty: a shard without channels)
    const auto threadOf = [&th](const size_t i) { return th[i].get(); };
    for (int rep = 0; rep < 50; rep++)
    {
        std::atomic<int> finished{0};
        const size_t slow = size_t(rep) % n == 2 ? 4 : size_t(rep) % n;
        lastError = "before";
        const int rc = runWithText(n, threadOf, [&](const size_t i) {
            std::this_thread::sleep_for(std::chrono::microseconds(i == slow ? 3000 : 100 * i));
            finished++;
            if (rep % 2 && (i == 1 || i == 3)) { lastError = "part " + std::to_string(i); return -int(i); }
            return 0; });
        CHECK(finished == 4, "returned with %d of 4 tasks finished (repetition %d)", int(finished), rep);
        if (rep % 2) CHECK(rc == -1 && lastError == "part 1", "first failure: code %d, text '%s'", rc, lastError.c_str());
        else CHECK(rc == 0 && lastError == "before", "no failure: code %d, text '%s'", rc, lastError.c_str());
    }
}

int main()
{
    roundTrips();
    destruction();
    fanOut();
    postAllWaitAll();
    std::printf("worker_check: ok\n");
    return 0;
}
