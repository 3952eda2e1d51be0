// EnvKnobs.h — every HC_* environment variable the library reads, in one list, and the one place that reads one (raw()).
// What each knob means is written in DESIGN.md section 9 alone (tests/test_env_knobs.py holds the two lists equal).
// Nothing here keeps a value: every accessor reads the environment when it is called, because the resident process
// gives each job its client's HC_* environment (cli/hc_cli.cpp) and tests switch knobs inside one process.
// Plain C++17, no HIP header: the host sources and the launcher, which links no library, include it as it is.
#pragma once

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// X(NAME, class): the variable is HC_<NAME>.  ship: a route or a diagnostic a user may need; test: makes small
// inputs reach large-input code.
#define HC_ENV_KNOBS(X)        \
    X(BALANCE, test)           \
    X(CLI_TEARDOWN, ship)      \
    X(COLLECTORS, test)        \
    X(COOP_DMA_MIN, test)      \
    X(DEVICE, ship)            \
    X(DEVICE_LIST, test)       \
    X(FASTQ_GRAIN, test)       \
    X(FASTQ_PARALLEL_MIN, test) \
    X(FASTQ_THREADS, test)     \
    X(FETCH_GROUP, test)       \
    X(FETCH_PIECE_BYTES, test) \
    X(FIND_BATCH_HITS, test)   \
    X(FIND_TIMING, ship)       \
    X(FNO, ship)               \
    X(FNO_DEBUG, ship)         \
    X(FNO_TIMING, ship)        \
    X(FNO_WALK, ship)          \
    X(INSERT_MODE, ship)       \
    X(LOCALITY, test)          \
    X(LOCALITY_MIN, test)      \
    X(NUMA, ship)              \
    X(PARSE, ship)             \
    X(PARSE_FALLBACK, ship)    \
    X(QIDX_ORDER, test)        \
    X(REGULAR_STORE, test)     \
    X(RESIDENT_DIR, ship)      \
    X(RESIDENT_IDLE_S, ship)   \
    X(RESOLVE, ship)           \
    X(SFO_BUCKETS, test)       \
    X(SFO_CHUNK, test)         \
    X(SFO_COPY_THREADS, ship)  \
    X(SFO_FILTER, test)        \
    X(SFO_PARSE, ship)         \
    X(SFO_TEXT_GENERAL, test)  \
    X(SFO_TIMING, ship)        \
    X(SFO_VIA_MATCHER, test)   \
    X(SLOT_ALIGN, test)        \
    X(SR_SELF_BAND_LOG2, test) \
    X(STAGE_BLOCK, test)       \
    X(STAGE_TIMING, ship)      \
    X(TEXT_BLOCK, test)        \
    X(TEXT_DEPTH, test)        \
    X(TEXT_SOURCE, ship)       \
    X(WARM, ship)              \
    X(WIDE_DMA, test)

namespace hc {
namespace env __attribute__((visibility("hidden"))) {  // (hidden: these inlines add nothing to what libhcedge.so exports)

enum class Knob {
#define X(NAME, CLASS) NAME,
    HC_ENV_KNOBS(X)
#undef X
};

enum class Class { ship, test };

inline const char* name(Knob k) {
    static const char* const names[] = {
#define X(NAME, CLASS) "HC_" #NAME,
        HC_ENV_KNOBS(X)
#undef X
    };
    return names[(int)k];
}

inline Class class_of(Knob k) {
    static const Class classes[] = {
#define X(NAME, CLASS) Class::CLASS,
        HC_ENV_KNOBS(X)
#undef X
    };
    return classes[(int)k];
}

inline const char* raw(Knob k) { return getenv(name(k)); }
inline bool given(Knob k) { return raw(k) != nullptr; }  // set, even if empty
inline bool is(Knob k, const char* word) {
    const char* v = raw(k);
    return v && strcmp(v, word) == 0;
}
inline int i(Knob k, int dflt) {
    const char* v = raw(k);
    return v ? atoi(v) : dflt;
}
inline uint64_t u64(Knob k, uint64_t dflt) {
    const char* v = raw(k);
    return v ? strtoull(v, nullptr, 10) : dflt;
}

// lap(what) prints "<prefix><what> <seconds since the last lap> s" to stderr when the knob was set at construction.
struct Lap {
    Lap(Knob k, const char* prefix) : on_(given(k)), prefix_(prefix), last_(std::chrono::steady_clock::now()) {}
    void operator()(const char* what) {
        if (!on_) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "%s%s %.3f s\n", prefix_, what, std::chrono::duration<double>(t - last_).count());
        last_ = t;
    }

private:
    const bool on_;
    const char* const prefix_;
    std::chrono::steady_clock::time_point last_;
};

}  // namespace env
}  // namespace hc
