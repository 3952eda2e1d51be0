"""AddressSanitizer + UBSan over the host mirror of the self-overlap merge (csrc/host/SrSelfOverlap.cpp): the mirror, a one-line stub of
set_last_error and a small C++ program with its own main are compiled with g++ -fsanitize=address,undefined into one executable, which
runs every golden case and a set of hostile pairs through the C entry point.  The test writes the calls as a flat text file (the program
reads no JSON); every buffer the program hands over is a heap block of exactly the size the contract names, so a byte read or written
beyond it is caught."""
import json
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "self_overlap.json")

PROGRAM = r'''
// One call per record of the file named on the command line:
//   mismatch min_read_len min_score min_qual min_overlap n_threads cap n_bytes seq_hex qual_hex n_pairs {off1 off2 len1 len2}...
//   expect_pos expect_seq_hex expect_qual_hex         ("-" for the three: nothing is compared, only the sanitizers judge)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include "hcsr.h"
namespace hc { int set_last_error(int s, const std::string&) { return s; } }
static std::unique_ptr<uint8_t[]> unhex(const std::string& h, uint64_t n) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
    for (uint64_t i = 0; i < n; i++) b[i] = (uint8_t)strtoul(h.substr(1 + 2 * i, 2).c_str(), nullptr, 16);
    return b;
}
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string mismatch, min_score, min_qual, seq_hex, qual_hex, e_pos, e_seq, e_qual;
    uint32_t min_read_len, min_overlap, n_threads;
    uint64_t cap, n_bytes, n_pairs, n_calls = 0, n_compared = 0;
    while (in >> mismatch >> min_read_len >> min_score >> min_qual >> min_overlap >> n_threads >> cap >> n_bytes >> seq_hex >> qual_hex >> n_pairs) {
        std::unique_ptr<hc_sr_pair[]> pairs(new hc_sr_pair[n_pairs]);
        for (uint64_t i = 0; i < n_pairs; i++) in >> pairs[i].off1 >> pairs[i].off2 >> pairs[i].len1 >> pairs[i].len2;
        in >> e_pos >> e_seq >> e_qual;
        if (!in || seq_hex.size() != 1 + 2 * n_bytes || qual_hex.size() != 1 + 2 * n_bytes) return 3;
        auto seq = unhex(seq_hex, n_bytes), qual = unhex(qual_hex, n_bytes);
        hc_settings ec;
        memset(&ec, 0, sizeof ec);
        ec.mismatch = strtod(mismatch.c_str(), nullptr);
        ec.min_read_len = min_read_len;
        hc_sr_self_settings st = {strtod(min_score.c_str(), nullptr), strtod(min_qual.c_str(), nullptr), min_overlap, n_threads};
        std::unique_ptr<int32_t[]> pos(new int32_t[n_pairs]);
        std::unique_ptr<double[]> score(new double[n_pairs]);
        std::unique_ptr<uint32_t[]> status(new uint32_t[n_pairs]);
        std::unique_ptr<uint64_t[]> off(new uint64_t[n_pairs + 1]);
        std::unique_ptr<uint8_t[]> ms(new uint8_t[cap]), mq(new uint8_t[cap]);
        uint64_t n_out = 0;
        hc_sr_self_stats stats;
        const int rc = hc_host_sr_merge_self_overlaps(&ec, seq.get(), qual.get(), n_bytes, pairs.get(), n_pairs, &st, pos.get(), score.get(), status.get(),
                                                      off.get(), ms.get(), mq.get(), cap, &n_out, (n_calls & 1) ? &stats : nullptr);
        n_calls++;
        if (e_pos == "-") continue;
        const uint64_t n = (e_seq.size() - 1) / 2;
        auto want_seq = unhex(e_seq, n), want_qual = unhex(e_qual, n);
        if (rc != HC_OK || n_pairs != 1 || pos[0] != atoi(e_pos.c_str()) || off[1] != n || n_out != n || memcmp(ms.get(), want_seq.get(), n) ||
            memcmp(mq.get(), want_qual.get(), n)) {
            fprintf(stderr, "call %llu differs from the golden case\n", (unsigned long long)n_calls);
            return 4;
        }
        n_compared++;
    }
    printf("sanitizer driver finished: %llu calls, %llu compared\n", (unsigned long long)n_calls, (unsigned long long)n_compared);
    return 0;
}
'''


def _hex(b):
    return "x" + bytes(b).hex()  # (the prefix keeps an empty buffer a token)


def _call(mismatch, min_read_len, st, cap, seq, qual, pairs, expect=None):
    cap = min(sum(p[2] + p[3] for p in pairs), 1 << 16) if cap is None else cap
    w = [repr(float(mismatch)), min_read_len, *st[:2], *st[2:], cap, len(seq), _hex(seq), _hex(qual), len(pairs)]
    for p in pairs:
        w += list(p)
    w += ["-", "-", "-"] if expect is None else [expect[0], _hex(expect[1]), _hex(expect[2])]
    return " ".join(str(x) for x in w)


def _calls():
    lines = []
    for c in json.load(open(GOLDEN))["cases"]:
        seq, qual = (c["seq1"] + c["seq2"]).encode(), (c["qual1"] + c["qual2"]).encode()
        lines.append(_call(c["mismatch"], c["min_read_len"], (0.99, c["min_qual"], 15, 1), None, seq, qual,
                           [(0, len(c["seq1"]), len(c["seq1"]), len(c["seq2"]))], (c["overlap_pos"], c["merged_seq"].encode(), c["merged_qual"].encode())))
    n_golden = len(lines)
    # hostile pairs: every field at its limits, arbitrary bytes, several threads; only the sanitizers judge
    rng = random.Random(5)
    for _ in range(300):
        nb = rng.choice([0, 1, 40, 400])
        seq = bytes(rng.choice(b"ACGTN" if rng.random() < 0.9 else bytes(range(256))) for _ in range(nb))
        qual = bytes(rng.choice(b"!5I~" if rng.random() < 0.9 else bytes(range(256))) for _ in range(nb))
        lim = [0, 1, 15, 16, nb, nb + 1, 2**31 - 1, 2**31, 2**32 - 1]
        pairs = [(rng.choice([0, 1, nb // 2, nb, 2**63, 2**64 - 1]), rng.choice([0, 1, nb // 2, nb, 2**63, 2**64 - 1]), rng.choice(lim + [rng.randrange(nb + 1)]),
                  rng.choice(lim + [rng.randrange(nb + 1)])) for _ in range(rng.randrange(0, 40))]
        st = (rng.choice([0.99, 0.0, 1.0, -1.0, float("inf")]), rng.choice([0.99, 0.0, 1.0, 2.0]), rng.choice([15, 0, 1, 2**31, 2**32 - 1]), rng.choice([0, 1, 5, 1000]))
        lines.append(_call(rng.choice([0.0, 0.01, 1.0, 2.0]), rng.choice([0, 20, 2**32 - 1]), st, rng.choice([None, 0, 7]), seq, qual, pairs))
    return lines, n_golden


def test_self_overlap_mirror_under_asan_ubsan(tmp_path):
    lines, n_golden = _calls()
    assert n_golden >= 150
    calls = tmp_path / "calls.txt"
    calls.write_text("\n".join(lines) + "\n")
    src = tmp_path / "srself_asan_main.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "srself_asan")
    # (the runtimes are linked statically: the program then starts whatever else the environment has the loader bring in first)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(["g++", "-std=c++17", *san, "-pthread", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
                        os.path.join(ROOT, "haploconduct_amd", "csrc", "host", "SrSelfOverlap.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(calls)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"), capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and f"{len(lines)} calls, {n_golden} compared" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
