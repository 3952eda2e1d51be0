"""AddressSanitizer + UBSan over the host mirror of the super-read consensus (csrc/host/SrConsensus.cpp): a CPU build with
g++ -fsanitize=address,undefined runs every golden case and a set of hostile layouts through the C entry points, the way
tests/test_sanitizers.py does for the rest of the host code."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build", "asan")

DRIVER = r'''
import ctypes as C, json, os, random, struct
lib = C.CDLL(os.environ["HC_ASAN_SR"])
g = json.load(open(os.environ["HC_SR_GOLDEN"]))
seqs, quals, first, index = [], [], [0], {}
order = [i for i, r in enumerate(g["reads"]) if len(r) == 1] + [i for i, r in enumerate(g["reads"]) if len(r) == 2]
for k, i in enumerate(order):
    index[i] = k
    for s, q in g["reads"][i]:
        seqs.append(s.encode()); quals.append(q.encode())
    first.append(first[-1] + len(g["reads"][i]))
off = [0]
for s in seqs: off.append(off[-1] + len(s))
bases, qual = b"".join(seqs), b"".join(quals)
seq_off = (C.c_uint64 * len(off))(*off); first_a = (C.c_uint32 * len(first))(*first)
n_reads = len(first) - 1
class St(C.Structure):
    _fields_ = [("min_qual", C.c_double), ("mcs", C.c_uint32), ("ec", C.c_uint32), ("sub", C.c_uint32), ("threads", C.c_uint32)]
def run(layouts, members, st, cap=None):
    n, nm = len(layouts), len(members)
    lay = b"".join(struct.pack("<QIi", *l) for l in layouts); mem = b"".join(struct.pack("<IiBBxx", *m) for m in members)
    ret = (C.c_int32 * max(n, 1))(); status = (C.c_uint32 * max(n, 1))(); out_off = (C.c_uint64 * (n + 1))(); nb = C.c_uint64()
    cap = min(sum(max(l[2], 0) for l in layouts), 1 << 16) if cap is None else cap
    s, q = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1))
    rc = lib.hc_host_sr_consensus(bases, qual, seq_off, first_a, C.c_uint32(n_reads), lay, C.c_uint64(n), mem, C.c_uint64(nm), C.byref(st), ret, status, out_off,
                                  s, q, C.c_uint64(cap), C.byref(nb), None)
    return rc, list(ret), list(status), list(out_off), s.raw, q.raw
n_ok = 0
for c in g["cases"]:
    t = c["settings"]
    st = St(t["min_qual"], t["min_clique_size"], t["error_correction"], t["subreads_needed"], 1)
    members = [(index[m["read"]], m["pos"], m["seq"], m["rev"]) for m in c["members"]]
    rc, ret, status, o, s, q = run([(0, len(members), c["total_len"])], members, st)
    assert rc == 0 and ret[0] == c["ret"] and s[:o[1]].decode() == c["cons_seq"] and q[:o[1]].decode() == c["cons_qual"], c["name"]
    n_ok += 1
assert n_ok >= 150
# hostile layouts: every field at its limits, on several threads; only the sanitizers judge
rng = random.Random(5)
edge = [0, 1, 2, 3, 127, 255, 2**31 - 1, 2**32 - 1]
for _ in range(300):
    members = [(rng.choice([rng.randrange(n_reads), n_reads, 2**32 - 1]), rng.choice([0, 0, 5, -1, 2**31 - 1, -2**31, rng.randrange(200)]), rng.choice([0, 0, 1, 2, 3, 255]),
                rng.choice([0, 1, 2, 255])) for _ in range(rng.randrange(0, 12))]
    layouts = [(rng.choice([0, 1, len(members), 2**63, 2**64 - 1, rng.randrange(12)]), rng.choice(edge + [len(members)]),
                rng.choice([0, 1, 90, -1, 2**31 - 1, -2**31, rng.randrange(400)])) for _ in range(rng.randrange(0, 30))]
    st = St(rng.choice([0.99, 0.0, 1.0, 2.0, -1.0]), rng.choice([0, 1, 2, 4, 2**32 - 1]), rng.randrange(2), rng.randrange(2), rng.choice([0, 1, 5, 1000]))
    run(layouts, members, st, cap=rng.choice([None, 0, 7]))
lib.hc_host_sr_table.argtypes = [C.c_double, C.c_uint32, C.c_void_p]
t = C.create_string_buffer(25 * 128 * 128 + 5 * 128)
assert lib.hc_host_sr_table(0.99, 95, t) == 0 and lib.hc_host_sr_table(0.99, 96, t) != 0
col = C.create_string_buffer(2)
lib.hc_host_sr_column.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_double, C.c_void_p]
for nuc, ql in ((b"", b""), (b"ACGTN", b"!~I5#"), (b"xx", b"\x00\xff"), (b"A" * 500, b"~" * 500)):
    lib.hc_host_sr_column(nuc, ql, len(nuc), 0.99, col)
# the edge-merge helper on hostile records
lens = (C.c_uint32 * n_reads)(*[off[first[r] + 1] - off[first[r]] for r in range(n_reads)])
paired = (C.c_uint8 * n_reads)(*[first[r + 1] - first[r] == 2 for r in range(n_reads)])
for _ in range(2000):
    rec = struct.pack("<ddiiiiBBBBIIIQQiiii", 1.0, 0.0, rng.choice([0, 5, -5, 2**31 - 1, -2**31]), 0, 0, 0, rng.randrange(2), rng.randrange(2), 45, 0,
                      rng.choice([rng.randrange(n_reads), 2**32 - 1]), rng.randrange(n_reads), 0, rng.randrange(400), rng.randrange(400), 100, 100, 100, 0)
    lay = C.create_string_buffer(16); mem = C.create_string_buffer(24); bad = C.c_uint64()
    lib.hc_host_sr_edge_layouts(rec, C.c_uint64(1), lens, paired, C.c_uint32(n_reads), lay, mem, C.byref(bad))
print("sanitizer driver finished")
'''


def test_consensus_mirror_under_asan_ubsan(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libhcsr_asan.so")
    stub = os.path.join(BUILD, "stub_sr.cpp")
    open(stub, "w").write('#include <string>\nnamespace hc { int set_last_error(int s, const std::string&) { return s; } }\n')
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-fPIC", "-shared"]
    r = subprocess.run(["g++", "-std=c++17", *san, "-pthread", "-o", so, os.path.join(ROOT, "haploconduct_amd", "csrc", "host", "SrConsensus.cpp"), stub],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    libstdcpp = subprocess.run(["gcc", "-print-file-name=libstdc++.so.6"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=libasan + " " + libstdcpp, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HC_ASAN_SR=so,
               HC_SR_GOLDEN=os.path.join(ROOT, "tests", "golden", "consensus.json"))
    r = subprocess.run([sys.executable, "-c", DRIVER], env=env, capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "sanitizer driver finished" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
