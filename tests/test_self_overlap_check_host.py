"""host/SrSelfCheck.h on the CPU: the tests of a pair that the host's check_pair and the device's sr_self_check_kernel share.  A small C++
program with its own main, compiled with g++ -fsanitize=address,undefined, holds the packed four-symbols-at-once validity test against the
plain one for every (base, quality) byte pair in every byte lane, the byte-range mask against a loop, and the range test at its edges."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include "host/SrSelfCheck.h"
using namespace hc::srself;
int main() {
    // every (base, quality) pair in every lane, the other three lanes holding valid and invalid neighbours in turn
    const uint32_t fill_b[2] = {0x41474354u, 0x78007aFFu}, fill_q[2] = {0x49217e46u, 0x207f80FFu};
    for (int f = 0; f < 2; f++)
        for (int lane = 0; lane < 4; lane++)
            for (uint32_t b = 0; b < 256; b++)
                for (uint32_t q = 0; q < 256; q++) {
                    const uint32_t keep = ~(0xFFu << (8 * lane));
                    const uint32_t wb = (fill_b[f] & keep) | b << (8 * lane), wq = (fill_q[f] & keep) | q << (8 * lane);
                    const uint32_t got = bytes_bad(wb, wq);
                    for (int k = 0; k < 4; k++) {
                        const bool want = symbol_bad((uint8_t)(wb >> (8 * k)), (uint8_t)(wq >> (8 * k)));
                        if ((((got >> (8 * k)) & 0xFFu) == 0x80u) != want || ((got >> (8 * k)) & 0x7Fu)) {
                            printf("bytes_bad differs: base %u quality %u lane %d fill %d byte %d\n", b, q, lane, f, k);
                            return 1;
                        }
                    }
                }
    for (int64_t lo = -40; lo <= 40; lo++)
        for (int64_t hi = -40; hi <= 40; hi++) {
            uint32_t want = 0;
            for (int64_t k = 0; k < 4; k++)
                if (lo <= k && k < hi) want |= 0x80u << (8 * k);
            if (bytes_between(lo, hi) != want) {
                printf("bytes_between(%lld, %lld)\n", (long long)lo, (long long)hi);
                return 2;
            }
        }
    if (bytes_between(INT64_MIN / 2, INT64_MAX / 2) != 0x80808080u || bytes_between(5, INT64_MAX) != 0) return 3;
    // the range test: (off1, off2, len1, len2) against n_bytes = 100
    struct Case { hc_sr_pair P; bool ok; };
    const Case cases[] = {
        {{0, 50, 50, 50}, true},  {{0, 50, 50, 51}, false}, {{100, 0, 1, 1}, false}, {{99, 0, 1, 100}, true}, {{0, 0, 0, 5}, false},
        {{0, 0, 5, 0}, false},    {{1ull << 63, 0, 5, 5}, false}, {{0, ~0ull, 5, 5}, false}, {{0, 101, 5, 0}, false}, {{0, 0, 100, 100}, true},
        {{0, 0, 0x7FFFFFFFu, 1}, false}, {{100, 100, 0, 0}, false}};
    for (const Case& c : cases)
        if (pair_in_range(100, c.P) != c.ok) {
            printf("pair_in_range: off1 %llu off2 %llu len1 %u len2 %u\n", (unsigned long long)c.P.off1, (unsigned long long)c.P.off2, c.P.len1, c.P.len2);
            return 4;
        }
    const hc_sr_pair big = {0, 0, 0x40000000u, 0x3FFFFFFFu}, too_big = {0, 0, 0x40000000u, 0x40000000u};
    if (!pair_in_range(1ull << 31, big) || pair_in_range(1ull << 31, too_big)) return 5;  // len1 + len2 <= INT32_MAX
    if (first_offset(150, 15) != 135 || first_offset(15, 15) != 0 || first_offset(3, 15) != 0 || first_offset(0xFFFFFFFFu, 0) != 0xFFFFFFFFu) return 6;
    printf("ok\n");
    return 0;
}
'''


def test_shared_pair_checks_under_asan_ubsan(tmp_path):
    src = tmp_path / "srself_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "srself_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "haploconduct_amd", "csrc"), "-o", exe, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-500:], r.stderr[-3000:])
