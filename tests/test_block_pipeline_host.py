"""host/BlockPipeline.h on the CPU: the ordered gate and the FIFO job thread the stage's three block routes run on.  A small C++ program with
its own main drives them with fake blocks (a number and an in-flight flag) the way the routes do — a producer that waits for room and hands
"submit block k, then publish k" to the job thread, C collectors with a side-by-side half (which waits for the "device") and an in-order half —
and is run under -fsanitize=thread and under -fsanitize=address,undefined.  The flags and lists of the fake blocks are plain memory on purpose:
the gate's own mutex is all that orders them, so ThreadSanitizer checks exactly that.  A missed retire deadlocks (window 1, more than one
block); the subprocess timeout makes that a failure."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <set>
#include <string>
#include <vector>
#include "host/BlockPipeline.h"
using namespace hc;

enum Where { NONE, SIDE, SERIAL, PRODUCER, JOB };
static const char* names[] = {"none", "side", "serial", "producer", "job"};

#define REQUIRE(cond)                                                                                                          \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            printf("K %zu C %zu window %zu failure in %s at %zu: %s\n", K, C, W, names[where], f, #cond);                      \
            return false;                                                                                                      \
        }                                                                                                                      \
    } while (0)

// One route: K blocks, C collectors, at most W blocks un-retired; `where` throws at block f.
static bool run(size_t K, size_t C, size_t W, Where where, size_t f) {
    struct Block {
        int in_flight = 0, submits = 0, waits = 0, serials = 0;
    };
    std::vector<Block> blocks(K);
    std::vector<size_t> serial_order, job_order;
    size_t pushed = 0;
    std::atomic<size_t> threads_ended{0};
    const std::string text = std::string(names[where]) + " " + std::to_string(f) + std::string(300, 'x');
    const FatalError injected{-7, text};
    BlockGate gate;
    std::vector<std::thread> collectors;
    for (size_t c = 0; c < C; c++)
        collectors.emplace_back([&, c] {
            gate.collect(
                c, C,
                [&](size_t k) {  // the wait for the device's block: also after an error
                    blocks[k].waits++;
                    blocks[k].in_flight = 0;
                    if (where == SIDE && k == f) throw injected;
                },
                [&](size_t k) {
                    blocks[k].serials++;
                    serial_order.push_back(k);
                    if (where == SERIAL && k == f) throw injected;
                });
            threads_ended++;
        });
    {
        JobThread submitter([&] { threads_ended++; });  // (counted at its start; finish() below joins it)
        gate.guarded([&] {
            for (size_t k = 0; k < K && gate.wait_room(k, W); k++) {
                if (where == PRODUCER && k == f) throw injected;
                pushed++;
                submitter.push([&, k] {
                    job_order.push_back(k);
                    if (!gate.failed())
                        gate.guarded([&] {
                            if (where == JOB && k == f) throw injected;
                            blocks[k].submits++;
                            blocks[k].in_flight = 1;
                        });
                    gate.publish(k);
                });
            }
        });
        submitter.finish();
        REQUIRE(!submitter.failed() && submitter.error().status == 0);  // (these jobs keep their errors in the gate)
    }
    gate.close();
    for (auto& t : collectors) t.join();
    REQUIRE(threads_ended == C + 1);
    // the job thread ran every job, in push order
    REQUIRE(job_order.size() == pushed);
    for (size_t k = 0; k < pushed; k++) REQUIRE(job_order[k] == k);
    // the drain rule: every published block went through the side-by-side half once and was retired (all of them: the gate has room for
    // block `pushed` with a window of 1), none is in flight
    REQUIRE(gate.wait_room(pushed, 1) == (where == NONE));
    for (size_t k = 0; k < K; k++) {
        REQUIRE(blocks[k].waits == (k < pushed ? 1 : 0));
        REQUIRE(blocks[k].in_flight == 0);
        REQUIRE(blocks[k].submits <= 1 && blocks[k].serials <= 1);
    }
    // the serial halves ran in order, and none after the failure
    for (size_t k = 0; k < serial_order.size(); k++) REQUIRE(serial_order[k] == k);
    bool thrown = false;
    try {
        gate.rethrow();
    } catch (const FatalError& e) {
        thrown = true;
        REQUIRE(e.status == injected.status && e.what == injected.what);
    }
    if (where == NONE) {
        REQUIRE(!thrown && !gate.failed() && pushed == K && serial_order.size() == K);
    } else {
        REQUIRE(thrown && gate.failed());
        if (where == SIDE) REQUIRE(serial_order.size() == f);         // recorded at block f's turn
        if (where == SERIAL) REQUIRE(serial_order.size() == f + 1);   // (f's own half began)
        if (where == PRODUCER) REQUIRE(pushed == f);
        if (where == PRODUCER || where == JOB) REQUIRE(serial_order.size() <= f && blocks[f].submits == 0);
    }
    return true;
}

// The job thread by itself, as the stage's appender uses it: job f throws; the ones before it ran in order, the ones behind it did not run.
static bool run_jobs(size_t K, size_t f) {
    const size_t C = 0, W = 0;
    const Where where = JOB;
    std::vector<size_t> order;
    const FatalError injected{-3, "append " + std::to_string(f) + std::string(300, 'y')};
    JobThread jobs(nullptr);
    for (size_t k = 0; k < K; k++)
        jobs.push([&, k] {
            order.push_back(k);
            if (k == f) throw injected;
        });
    jobs.finish();
    REQUIRE(order.size() == (f < K ? f + 1 : K));
    for (size_t k = 0; k < order.size(); k++) REQUIRE(order[k] == k);
    REQUIRE(jobs.failed() == (f < K));
    if (f < K) REQUIRE(jobs.error().status == injected.status && jobs.error().what == injected.what);
    else REQUIRE(jobs.error().status == 0);
    jobs.finish();  // (a second finish, as the destructor's, is harmless)
    return true;
}

// Two threads record at once: one error, whole, comes back.
static bool record_race() {
    const size_t K = 0, C = 2, W = 0, f = 0;
    const Where where = NONE;
    const FatalError a{-1, std::string(1000, 'a')}, b{-2, std::string(1000, 'b')};
    for (int round = 0; round < 200; round++) {
        BlockGate gate;
        std::atomic<int> ready{0};
        auto racer = [&](const FatalError& e) {
            ready++;
            while (ready.load() < 2) {
            }
            gate.record(e);
        };
        std::thread ta(racer, std::cref(a)), tb(racer, std::cref(b));
        ta.join();
        tb.join();
        bool thrown = false;
        try {
            gate.rethrow();
        } catch (const FatalError& e) {
            thrown = true;
            REQUIRE((e.status == a.status && e.what == a.what) || (e.status == b.status && e.what == b.what));
        }
        REQUIRE(thrown && gate.failed());
        REQUIRE(!gate.guarded([] { throw std::runtime_error("late"); }));  // a later error, here a std::exception, does not replace it
        try {
            gate.rethrow();
        } catch (const FatalError& e) {
            REQUIRE(e.status == a.status || e.status == b.status);
        }
    }
    BlockGate other;  // neither does anything else leave guarded()
    REQUIRE(!other.guarded([] { throw 5; }) && other.failed());
    BlockGate gate;  // a std::exception is reported as out of memory
    REQUIRE(!gate.guarded([] { throw std::runtime_error("no memory"); }));
    try {
        gate.rethrow();
        REQUIRE(false);
    } catch (const FatalError& e) {
        REQUIRE(e.status == kBlockErrNoMem && e.what == "no memory");
    }
    return true;
}

int main() {
    size_t runs = 0;
    for (size_t C : {1, 2, 4}) {
        std::set<size_t> Ks = {0, 1, C - 1, C, C + 1, 37}, Ws = {1, 2, C};
        for (size_t K : Ks)
            for (size_t W : Ws) {
                if (!run(K, C, W, NONE, 0)) return 1;
                runs++;
                if (K == 0) continue;
                for (Where where : {SIDE, SERIAL, PRODUCER, JOB})
                    for (size_t f : std::set<size_t>{0, K / 2, K - 1}) {
                        if (!run(K, C, W, where, f)) return 1;
                        runs++;
                    }
            }
    }
    for (size_t K : {0, 1, 5})
        for (size_t f : std::set<size_t>{0, K / 2, K ? K - 1 : 0, K})
            if (!run_jobs(K, f)) return 2;
    if (!record_race()) return 3;
    printf("ok %zu\n", runs);
    return 0;
}
'''


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_gate_and_job_thread_keep_order_and_drain(tmp_path, sanitizer):
    src = tmp_path / "block_pipeline.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "block_pipeline")
    san = [f"-fsanitize={sanitizer}", "-fno-omit-frame-pointer", "-g", "-O1"]
    if sanitizer != "thread":
        san += ["-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-pthread", "-I", os.path.join(ROOT, "haploconduct_amd", "csrc"), "-o", exe, str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)  # a deadlock is a failure, not a hang
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 300  # every (K, C, window, failure) case ran
