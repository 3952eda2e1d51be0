"""The HC_* environment knobs: the list in host/EnvKnobs.h equals the table of DESIGN.md section 9, nothing under csrc/ reads
the environment past that header, and its accessors parse as libc does on the same string — at every call, with nothing kept."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "haploconduct_amd", "csrc")
HEADER = os.path.join(CSRC, "host", "EnvKnobs.h")


def _sources():
    return sorted(p for ext in ("cpp", "h", "hip") for p in glob.glob(os.path.join(CSRC, "**", "*." + ext), recursive=True))


def _header_knobs():
    return re.findall(r"^\s*X\((\w+),\s*(ship|test)\)", open(HEADER).read(), re.M)


def test_the_table_equals_the_document():
    knobs = _header_knobs()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 9. Environment knobs"):design.index("## 10. ")]
    rows = re.findall(r"^\| `HC_(\w+)` \| (\w+) \|", section, re.M)
    assert len(knobs) == 45 and len({n for n, _ in knobs}) == 45
    assert len(rows) == 45 and len({n for n, _ in rows}) == 45
    assert set(knobs) == set(rows)
    assert {c for _, c in rows} == {"ship", "test"}


def test_nothing_reads_a_knob_past_the_table():
    names = {n for n, _ in _header_knobs()}
    reads = []  # (file, the rest of the line from the call on)
    for p in _sources():
        text = open(p).read()
        assert not re.search(r"static[^;\n]*env::", text), f"{p}: a static initialised from a knob keeps the first job's value"
        for m in re.finditer(r"getenv\s*\(.*", text):
            reads.append((os.path.relpath(p, CSRC), m.group(0)))
    by_file = {}
    for f, line in reads:
        by_file.setdefault(f, []).append(line)
    assert sorted(by_file) == ["cli/hc_edgecalc_main.cpp", "hc_kernels.hip", "host/EnvKnobs.h"], by_file
    assert len(by_file["host/EnvKnobs.h"]) == 1
    kernel = sorted(re.search(r'getenv\s*\(\s*"HC_(\w+)"', line).group(1) for line in by_file["hc_kernels.hip"])
    assert kernel == ["COOP_DMA_MIN", "WIDE_DMA"] and set(kernel) <= names
    assert len(by_file["cli/hc_edgecalc_main.cpp"]) == 2  # XDG_RUNTIME_DIR and the device-visibility variables: the system's, not knobs
    assert not any('"HC_' in line for line in by_file["cli/hc_edgecalc_main.cpp"])


PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "EnvKnobs.h"

namespace env = hc::env;
using env::Knob;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("line %d: %s (value %s)\n", __LINE__, #c, shown);      \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main(int argc, char** argv) {
    const Knob K = Knob::STAGE_BLOCK;
    const char* const N = "HC_STAGE_BLOCK";
    const char* shown = "<unset>";
    if (argc > 1) {  // the lap helper: argv[1] = on | off
        if (!strcmp(argv[1], "on")) setenv("HC_FNO_TIMING", "", 1);
        else unsetenv("HC_FNO_TIMING");
        env::Lap lap(Knob::FNO_TIMING, "[some prefix] walk: ");
        lap("first lap");
        lap("second");
        return 0;
    }
    CHECK(!strcmp(env::name(K), N));
    unsetenv(N);
    CHECK(env::raw(K) == nullptr && !env::given(K) && !env::is(K, "host") && !env::is(K, ""));
    CHECK(env::i(K, -17) == -17 && env::i(K, 5) == 5);
    CHECK(env::u64(K, 18446744073709551615ull) == 18446744073709551615ull && env::u64(K, 3) == 3);
    const char* values[] = {"", "0", "1", "-3", " 7", "12abc", "host", "18446744073709551615"};
    for (const char* v : values) {
        shown = v;
        setenv(N, v, 1);
        const char* libc = getenv(N);
        CHECK(libc != nullptr && env::raw(K) != nullptr && !strcmp(env::raw(K), libc));
        CHECK(env::given(K) == (libc != nullptr));
        CHECK(env::is(K, "host") == (strcmp(libc, "host") == 0));
        CHECK(env::i(K, 99) == atoi(libc));
        CHECK(env::u64(K, 99) == strtoull(libc, nullptr, 10));
    }
    // nothing is kept: a read after setenv / unsetenv sees the change
    shown = "switching";
    setenv(N, "41", 1);
    CHECK(env::given(K) && env::i(K, 0) == 41 && env::u64(K, 0) == 41);
    setenv(N, "host", 1);
    CHECK(env::is(K, "host") && env::i(K, 7) == 0);
    unsetenv(N);
    CHECK(!env::given(K) && env::i(K, 7) == 7 && env::u64(K, 8) == 8 && !env::is(K, "host"));
    setenv(N, "2", 1);
    CHECK(env::given(K) && env::i(K, 7) == 2);
    // every entry has its name and one of the two classes
    CHECK(!strcmp(env::name(Knob::WIDE_DMA), "HC_WIDE_DMA") && !strcmp(env::name(Knob::BALANCE), "HC_BALANCE"));
    CHECK(env::class_of(Knob::STAGE_TIMING) == env::Class::ship && env::class_of(Knob::STAGE_BLOCK) == env::Class::test);
    printf("ok\n");
    return 0;
}
'''


def test_every_parse_is_libcs_parse_and_nothing_is_kept(tmp_path):
    src, exe = str(tmp_path / "knobs.cpp"), str(tmp_path / "knobs")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.dirname(HEADER),
                    "-o", exe, src], check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("HC_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.stdout, r.stderr)
    on = subprocess.run([exe, "on"], env=env, capture_output=True, text=True, timeout=60)
    assert on.returncode == 0 and on.stdout == ""
    assert re.fullmatch(r"\[some prefix\] walk: first lap \d+\.\d{3} s\n\[some prefix\] walk: second \d+\.\d{3} s\n", on.stderr), on.stderr
    off = subprocess.run([exe, "off"], env=env, capture_output=True, text=True, timeout=60)
    assert off.returncode == 0 and off.stdout == "" and off.stderr == ""
