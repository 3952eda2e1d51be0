"""A Python restatement of SRBuilder's FASTQ writers (reference src/SRBuilder.cpp:1386-1556), for the tests of hc_sr_fastq_write_text and its
host mirrors: each function cites the lines it restates.  Also the seeded stores the tests share."""
import numpy as np

from haploconduct_amd.readstore import ReadSet

FILE_NAMES = ("singles.fastq", "paired1.fastq", "paired2.fastq", "removed_tip_sequences.fastq")


def record(rid, seq, qual):
    """outfile << "@" << ID << "\\n" << seq << "\\n" << "+\\n" << phred << "\\n" (:1484-1487; the same four lines at :1434-1437,
    :1438-1441, :1444-1447, :1528-1531, :1532-1535)"""
    return b"@" + str(rid).encode() + b"\n" + seq + b"\n+\n" + qual + b"\n"


def store_files(reads):
    """What the three writers append for a store, read r carrying id r: writeSinglesToFile (:1479-1487) and the else branch of
    writeTrivialsToFile (:1443-1447) go to singles.fastq, writeTrivialsToFile's paired branch (:1433-1441) and writePairsToFile (:1519-1535)
    to paired1 / paired2.fastq.  The store numbers singles, trivials, pairs in that order (:1280, :1370-1371, :1378), the order the writers
    run in (:1280, :1377-1378), so each file is in ascending id."""
    out = [b"", b"", b""]
    for r in range(reads.n_reads):
        q = int(reads.read_first_seq[r])
        if reads.is_paired(r):
            out[1] += record(r, *reads.seq(q))
            out[2] += record(r, *reads.seq(q + 1))
        else:
            out[0] += record(r, *reads.seq(q))
    return out


def tips_file(reads, tip_reads):
    """writeTipsToFile (:1386-1414): new_ID from 0, "@ID_1" / "@ID_2" for a paired read (:1394-1403), "@ID" otherwise (:1405-1410); the reads
    are the stored ones whatever the vertex (tips_vec.push_back(*read), :1302, :1309)."""
    out = b""
    for k, r in enumerate(tip_reads):
        q = int(reads.read_first_seq[r])
        if reads.is_paired(r):
            out += record(f"{k}_1", *reads.seq(q)) + record(f"{k}_2", *reads.seq(q + 1))
        else:
            out += record(k, *reads.seq(q))
    return out


def make_store(rng, lens, kind, with_n=True):
    """A store whose sequences have the lengths `lens` in turn.  kind: "single", "paired" (consecutive lengths are mates; an odd one out is
    dropped) or "mixed" (every third read single-end, in store order).  Bases ACGTN (with_n = False: ACGT, for reads that have to pass
    test_N_rate as trivial super-reads), qualities from bytes 33 ... 126."""
    lens = list(lens)
    seqs, first = [], [0]
    i = 0
    while i < len(lens):
        two = kind == "paired" or (kind == "mixed" and len(first) % 3 != 0)
        if two and i + 1 >= len(lens):
            if kind == "paired":
                break
            two = False
        seqs += lens[i:i + (2 if two else 1)]
        first.append(first[-1] + (2 if two else 1))
        i += 2 if two else 1
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum(seqs)
    total = int(off[-1])
    bases = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5 if with_n else 4, total)]
    quals = rng.integers(33, 127, total).astype(np.uint8)
    n = len(first) - 1
    return ReadSet(bases, quals, off, np.array(first, np.uint32), np.arange(n, dtype=np.uint64))


def store_of_case(case, vecs=("singles", "trivials", "pairs")):
    """The store a case of tests/golden/fastq_text.json describes: its reads of the named vectors, vector after vector — the ids the writers gave."""
    seqs, quals, first = [], [], [0]
    for v in vecs:
        for r in case["reads"]:
            if r["vec"] != v:
                continue
            mates = ("1", "2") if "seq2" in r else ("1",)
            for m in mates:
                seqs.append(r["seq" + m].encode())
                quals.append(r["qual" + m].encode())
            first.append(first[-1] + len(mates))
    off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs])
    return ReadSet(np.frombuffer(b"".join(seqs), np.uint8), np.frombuffer(b"".join(quals), np.uint8), off, np.array(first, np.uint32),
                   np.arange(len(first) - 1, dtype=np.uint64))
