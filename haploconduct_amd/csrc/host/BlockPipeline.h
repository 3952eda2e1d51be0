// BlockPipeline.h — the ordering and the error handling of the stage's block routes (EdgeCalculator.cpp: score_device_parsed,
// score_device_lines, score_host_parsed), written once.  Blocks are numbered 0, 1, 2, ...; a producer publishes them in order, collectors take
// them, work on them side by side and run a serial half strictly in block order.  The rule the gate keeps: EVERY PUBLISHED BLOCK IS RETIRED
// EXACTLY ONCE, also after an error and also when the producer throws — so a route that waits for the device's block object inside
// collect()'s side-by-side half leaves no block object in flight, whatever happened.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

#include "Types.h"

namespace hc {

constexpr int kBlockErrNoMem = -2;  // HC_ERR_NOMEM of include/hcedge.h (asserted where both are seen): this header stands without the C ABI

// The catch ladder: what fn threw as a FatalError (status 0: nothing).  A std::exception is out of memory, as far as the stage can tell;
// nothing else leaves either: a route's threads are joined whatever was thrown.
template <class Fn>
FatalError error_of(Fn&& fn) {
    try {
        fn();
    } catch (const FatalError& e) {
        return e;
    } catch (const std::exception& e) {
        return FatalError{kBlockErrNoMem, e.what()};
    } catch (...) {
        return FatalError{kBlockErrNoMem, "unknown exception"};
    }
    return FatalError{0, ""};
}

class BlockGate {
public:
    // Producer: wait until fewer than `window` blocks before k are un-retired (the ring slot, the block object of block k - window is free
    // again).  false: an error has been recorded, put nothing more in flight.
    bool wait_room(size_t k, size_t window) {
        std::unique_lock<std::mutex> g(m_mu);
        m_cv.wait(g, [&] { return m_retired + window > k; });
        return !m_error.status;
    }
    void publish(size_t k) {
        {
            std::lock_guard<std::mutex> g(m_mu);
            m_published = k + 1;
        }
        m_cv.notify_all();
    }
    // No more blocks will be published (the producer is done, or gave up).
    void close() {
        {
            std::lock_guard<std::mutex> g(m_mu);
            m_closed = true;
        }
        m_cv.notify_all();
    }
    // Collector: false once the gate is closed and block k was never published.
    bool wait_published(size_t k) {
        std::unique_lock<std::mutex> g(m_mu);
        m_cv.wait(g, [&] { return m_published > k || m_closed; });
        return m_published > k;
    }
    void wait_turn(size_t k) {
        std::unique_lock<std::mutex> g(m_mu);
        m_cv.wait(g, [&] { return m_retired == k; });
    }
    void retire(size_t k) {
        {
            std::lock_guard<std::mutex> g(m_mu);
            m_retired = k + 1;
        }
        m_cv.notify_all();
    }
    // The first error recorded wins.
    void record(const FatalError& e) {
        if (!e.status) return;
        {
            std::lock_guard<std::mutex> g(m_mu);
            if (m_error.status) return;
            m_error = e;
            m_failed.store(true, std::memory_order_release);
        }
        m_cv.notify_all();
    }
    bool failed() const { return m_failed.load(std::memory_order_acquire); }
    template <class Fn>
    bool guarded(Fn&& fn) {
        const FatalError e = error_of(fn);
        record(e);
        return !e.status;
    }
    void rethrow() {
        std::lock_guard<std::mutex> g(m_mu);
        if (m_error.status) throw m_error;
    }
    // Collector c of C, until the gate is closed: every published block k = c, c + C, ... goes through side(k) — beside the other collectors,
    // and also after an error: this is where a route waits for the device's block —, then, at its turn and only while no error is recorded,
    // through serial(k), and is retired.  What side(k) threw is recorded at the block's turn, so the error that comes back is the first one
    // in block order.
    template <class Side, class Serial>
    void collect(size_t c, size_t C, Side&& side, Serial&& serial) {
        for (size_t k = c; wait_published(k); k += C) {
            const FatalError mine = error_of([&] { side(k); });
            wait_turn(k);
            record(mine);
            if (!failed()) guarded([&] { serial(k); });
            retire(k);
        }
    }

private:
    std::mutex m_mu;
    std::condition_variable m_cv;
    size_t m_published = 0, m_retired = 0;
    bool m_closed = false;
    FatalError m_error{0, ""};
    std::atomic<bool> m_failed{false};
};

// A thread that runs the jobs pushed to it in push order.  After the first job that throws, the rest are taken off the queue unrun and the
// error is kept.
class JobThread {
public:
    explicit JobThread(std::function<void()> on_start) {
        m_thread = std::thread([this, on_start] {
            if (on_start) on_start();
            for (;;) {
                std::function<void()> job;
                {
                    std::unique_lock<std::mutex> g(m_mu);
                    m_cv.wait(g, [&] { return !m_jobs.empty() || m_no_more; });
                    if (m_jobs.empty()) return;
                    job = std::move(m_jobs.front());
                    m_jobs.pop_front();
                }
                if (m_error.status) continue;  // drain
                m_error = error_of(job);
                if (m_error.status) m_failed.store(true, std::memory_order_release);
            }
        });
    }
    JobThread(const JobThread&) = delete;
    JobThread& operator=(const JobThread&) = delete;
    ~JobThread() { finish(); }
    void push(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> g(m_mu);
            m_jobs.push_back(std::move(job));
        }
        m_cv.notify_one();
    }
    // Everything queued has run (or was drained) and the thread is joined.
    void finish() {
        {
            std::lock_guard<std::mutex> g(m_mu);
            m_no_more = true;
        }
        m_cv.notify_one();
        if (m_thread.joinable()) m_thread.join();
    }
    bool failed() const { return m_failed.load(std::memory_order_acquire); }  // may be asked while the thread runs
    const FatalError& error() const { return m_error; }                       // after finish()

private:
    std::thread m_thread;
    std::mutex m_mu;
    std::condition_variable m_cv;
    std::deque<std::function<void()>> m_jobs;
    bool m_no_more = false;
    FatalError m_error{0, ""};
    std::atomic<bool> m_failed{false};
};

}  // namespace hc
