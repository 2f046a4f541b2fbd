// The one way the host code parks a thread: ParkedThread is one thread and one mailbox. The owner posts a task, the thread runs it,
// the owner waits for its code; between tasks the thread sleeps. Three places use it: the launch thread per device of the batch
// scheduler (lorahip_mixed.cpp), the run thread per (device, SF) part of a mixed level-3 handle (lorahip_rx.cpp) and the helpers that
// fill a pinned staging buffer (lorahip_upload.cpp). A mailbox per thread has no generation to get wrong: a thread can only ever see
// a task that was posted to IT. Host only, standard library only: a plain C++ program can include this (tests/worker_check.cpp).
#pragma once
#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <thread>
#include <vector>

namespace lorahip {

class ParkedThread
{
public:
    ParkedThread() = default;
    ParkedThread(const ParkedThread &) = delete;                // (nor movable: the thread holds `this`; containers hold a std::unique_ptr)
    ParkedThread &operator=(const ParkedThread &) = delete;
    //! an outstanding task is run to its end first; an object that was never started touches no thread
    ~ParkedThread()
    {
        if (!th.joinable()) return;
        { std::lock_guard<std::mutex> g(mu); quit = true; }
        cv.notify_all();
        th.join();
    }
    //! false when the thread could not be created (the object stays "never started"); nothing is thrown
    bool start() noexcept
    {
        if (th.joinable()) return true;
        try { th = std::thread(&ParkedThread::loop, this); }
        catch (...) { return false; }
        return true;
    }
    //! hands `task` (anything callable as int()) to the started thread when none is outstanding. The task is BORROWED: it stays the
    //! caller's and lives until wait() has returned. So a post allocates nothing, copies two pointers and cannot fail.
    template <class F> void post(F &task) noexcept
    {
        { std::lock_guard<std::mutex> g(mu); fn = [](void *t) -> int { return (*static_cast<F *>(t))(); }; arg = &task; }
        cv.notify_all();
    }
    //! blocks until the posted task has run; its code
    int wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return fn == nullptr; });
        return rc;
    }
private:
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;)
        {
            cv.wait(lk, [this] { return fn != nullptr || quit; });
            if (fn == nullptr) return;                          // told to leave, nothing outstanding
            lk.unlock();
            const int r = fn(arg);
            lk.lock();
            rc = r; fn = nullptr;                               // (fn stays set while the task runs: "outstanding" is one state, not two flags)
            cv.notify_all();
        }
    }
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    int (*fn)(void *) = nullptr;                                // non-null: a task is posted or running
    void *arg = nullptr;
    int rc = 0;
    bool quit = false;
};

//! task(i) on threadOf(i) for every i < n at once (nothing where threadOf(i) is null), then all awaited: 0, or the code of the first
//! i whose task returned another one, that i in *failed. May throw std::bad_alloc -- before anything is posted.
template <class ThreadOf, class Task> int runOnAll(const size_t n, const ThreadOf &threadOf, const Task &task, size_t *failed = nullptr)
{
    struct Call { const Task *task; size_t i; int operator()() const { return (*task)(i); } };
    std::vector<Call> calls(n);
    for (size_t i = 0; i < n; i++)
        if (ParkedThread *t = threadOf(i)) { calls[i] = Call{&task, i}; t->post(calls[i]); }
    int rc = 0;
    for (size_t i = 0; i < n; i++)
        if (ParkedThread *t = threadOf(i))
        {
            const int r = t->wait();
            if (r != 0 && rc == 0) { rc = r; if (failed) *failed = i; }
        }
    return rc;
}

} // namespace lorahip
