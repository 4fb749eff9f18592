// host_pool.cpp -- product host code: the worker pool of the host stages (see host_bitstream.h).
// The 1 + 6K streams of a container are coded independently and only concatenated bit-wise afterwards, so they are coded on a
// small thread pool (the reference is single-threaded; the bytes do not depend on it).
#include "host_bitstream.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>

namespace mpc {

int host_thread_count() {
    if (const char* v = std::getenv("MPC_HOST_THREADS")) {
        const int n = std::atoi(v);
        if (n > 0) return n;
    }
    const unsigned hc = std::thread::hardware_concurrency();
    return static_cast<int>(hc == 0 ? 1 : (hc > 16 ? 16 : hc));
}

namespace {
// A small persistent pool: the workers are created on first use and sleep between calls (creating and joining 16
// threads per call cost more than coding a 1080p frame's streams).  One call at a time (callers serialise on
// `submit_`); the calling thread works too.
class WorkerPool {
public:
    void run(int n, int workers, const std::function<void(int)>& body) {
        std::lock_guard<std::mutex> one_at_a_time(submit_);
        ensure(workers - 1);
        {
            std::lock_guard<std::mutex> hold(lock_);
            body_ = &body;
            total_ = n;
            next_.store(0);
            pending_ = std::min<int>(workers - 1, static_cast<int>(threads_.size()));
            active_limit_ = pending_;
            ++generation_;
        }
        wake_.notify_all();
        work(body, n);
        // Whatever a job threw, the generation is drained before `body` (the caller's stack) goes away; the first exception is
        // then rethrown on the calling thread, where the C ABI's `guarded` turns it into a status.
        std::exception_ptr first;
        {
            std::unique_lock<std::mutex> hold(lock_);
            done_.wait(hold, [&] { return pending_ == 0; });
            body_ = nullptr;
            first = error_;
            error_ = nullptr;
        }
        if (first) std::rethrow_exception(first);
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> hold(lock_);
            stop_ = true;
            ++generation_;
        }
        wake_.notify_all();
        for (auto& t : threads_) t.join();
    }

private:
    // this thread's share of the jobs; a job that throws ends the call's remaining jobs (nobody starts another) and is remembered
    void work(const std::function<void(int)>& body, int total) {
        try {
            for (int i = next_.fetch_add(1); i < total; i = next_.fetch_add(1)) body(i);
        } catch (...) {
            next_.store(total);
            std::lock_guard<std::mutex> hold(lock_);
            if (!error_) error_ = std::current_exception();
        }
    }
    void ensure(int count) {
        while (static_cast<int>(threads_.size()) < count) {
            const int id = static_cast<int>(threads_.size());
            threads_.emplace_back([this, id] { loop(id); });
        }
    }
    void loop(int id) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)>* body = nullptr;
            int total = 0;
            {
                std::unique_lock<std::mutex> hold(lock_);
                wake_.wait(hold, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                if (id >= active_limit_) continue;             // this call wants fewer workers
                body = body_;
                total = total_;
            }
            work(*body, total);
            {
                std::lock_guard<std::mutex> hold(lock_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::mutex submit_, lock_;
    std::condition_variable wake_, done_;
    std::vector<std::thread> threads_;
    const std::function<void(int)>* body_ = nullptr;
    std::atomic<int> next_{0};
    int total_ = 0, pending_ = 0, active_limit_ = 0;
    unsigned long long generation_ = 0;
    bool stop_ = false;
    std::exception_ptr error_;
};

void run_on(WorkerPool& pool, int n, int workers, const std::function<void(int)>& body) {
    workers = std::min(std::min(workers, host_thread_count()), n);
    if (workers <= 1) {
        for (int i = 0; i < n; ++i) body(i);
        return;
    }
    pool.run(n, workers, body);
}
}  // namespace

void parallel_jobs(int n, const std::function<void(int)>& body) {
    static WorkerPool pool;
    run_on(pool, n, n, body);
}

void parallel_io_jobs(int n, int workers, const std::function<void(int)>& body) {
    static WorkerPool pool;                                 // a second pool: frame uploads run beside the entropy stage's jobs
    run_on(pool, n, workers, body);
}

}  // namespace mpc
