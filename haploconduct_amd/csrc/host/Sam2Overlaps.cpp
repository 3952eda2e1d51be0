// Sam2Overlaps.cpp — SAM ingest: bwa's SAM records and the reference FASTA to SAVAGE's 13-column overlaps file with the semantics of the
// reference's scripts/sam2overlaps.py (cited per function): `savage --ref` (savage.py:690-692) and POLYTE's reference-guided start
// (polyte.py:535).  Three pieces behind include/hcedge_host.h: the reader (the script's reading, :46-101 and :138-266, into the records of
// include/hcedge.h), the mirror (the script's loops as written, :489-554 and :372-480, with its list of active reads) and the writer.
// Kept on purpose because they shape the output:
//   * `@` lines are skipped only until the first other line (:145-147);
//   * a leading S or H moves the position, leading and trailing H lengthen the sequence (:162-180); only its length matters later;
//   * the paired file's state machine (:189-266): an id mismatch drops the older line and keeps the newer;
//   * the loop tests the PREVIOUS record's position against the reference's end (:535);
//   * a read is dropped from the active list by `len - d >= min_overlap_len`, a line by `len <= min_overlap_len` (:393, :396);
//   * the single-record / paired-read branch writes the types s, p (:438); Python 2's round() in the percentage (:333).
// Every place the script dies is a FatalError naming the exception and the place.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../../include/hcedge_host.h"
#include "../hc_sam_items.h"
#include "Types.h"
#include "api_helpers.h"

struct hc_sam {
    std::vector<hc_sam_aln> alns;
    std::vector<hc_sam_rec> recs;
    std::vector<hc_sam_op> ops;
    std::string id_text;
    std::vector<uint64_t> ref_len;
    uint64_t n_singles = 0;
    hc_sam_view view() const {
        return hc_sam_view{alns.data(), recs.data(), ops.data(), id_text.data(), ref_len.data(), alns.size(), recs.size(), n_singles, ops.size(), id_text.size(),
                           ref_len.size()};
    }
};

namespace hc {
namespace {

[[noreturn]] void dies(const char* exception, const std::string& where) { throw FatalError{HC_ERR_FORMAT, std::string(exception) + ": " + where}; }

bool read_file(const char* path, std::string& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    fclose(f);
    return true;
}

inline bool py_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// Python's int(text): blanks around, one sign, decimal digits
bool py_int(const char* p, size_t n, int64_t& v) {
    while (n && py_space(*p)) p++, n--;
    while (n && py_space(p[n - 1])) n--;
    bool neg = false;
    if (n && (*p == '+' || *p == '-')) {
        neg = *p == '-';
        p++, n--;
    }
    if (n == 0 || n > 18) return false;  // (beyond 10^18: not a number of a SAM file)
    int64_t u = 0;
    for (size_t i = 0; i < n; i++) {
        if (p[i] < '0' || p[i] > '9') return false;
        u = u * 10 + (p[i] - '0');
    }
    v = neg ? -u : u;
    return true;
}

// the FASTA (:46-77): lengths in file order, names -> index (a repeated name keeps its last index)
void read_fasta(const std::string& text, std::vector<uint64_t>& ref_len, std::map<std::string, uint32_t>& ref_dict) {
    if (text.empty()) dies("SystemExit", "empty reference fasta (sam2overlaps.py:50-52)");
    std::string ref_id;
    uint64_t seq_len = 0;
    size_t pos = 0;
    while (pos < text.size()) {
        const char* nl = (const char*)memchr(text.data() + pos, '\n', text.size() - pos);
        const size_t end = nl ? (size_t)(nl - text.data()) : text.size();
        const char* line = text.data() + pos;
        const size_t len = end - pos;  // without the newline
        if (len && line[0] == '>') {
            if (seq_len != 0 && !ref_id.empty()) {
                ref_dict[ref_id] = (uint32_t)ref_len.size();
                ref_len.push_back(seq_len);
                seq_len = 0;
            }
            size_t b = 0;  // id_line.split()[0][1:]
            while (b < len && py_space(line[b])) b++;
            size_t e = b;
            while (e < len && !py_space(line[e])) e++;
            ref_id.assign(line + b + 1, e - b - 1);
        } else {
            seq_len += len;
        }
        pos = nl ? end + 1 : text.size();
    }
    if (seq_len == 0) dies("SystemExit", "invalid fasta file: no sequence behind the last header (sam2overlaps.py:70-72)");
    ref_dict[ref_id] = (uint32_t)ref_len.size();
    ref_len.push_back(seq_len);
}

struct Line {  // one mapped line of a SAM file as the script's record (:182, :233)
    uint32_t aln;           // its hc_sam_aln
    const char* ref_name;
    size_t ref_name_len;
};

// one SAM file's lines (:141-183, :192-234): the mapped ones become alignments; ref is resolved later (:89-101)
void read_sam_lines(const std::string& text, const char* what, hc_sam& S, std::vector<Line>& out) {
    bool header = true;
    size_t pos = 0;
    uint64_t line_no = 0;
    while (pos < text.size()) {
        const char* nl = (const char*)memchr(text.data() + pos, '\n', text.size() - pos);
        const size_t end = nl ? (size_t)(nl - text.data()) : text.size();
        const char* line = text.data() + pos;
        const size_t len = end - pos;
        pos = nl ? end + 1 : text.size();
        line_no++;
        if (header && len && line[0] == '@') continue;
        header = false;
        const std::string at = std::string(" in line ") + std::to_string(line_no) + " of the " + what + " SAM file";
        const char* f[11];
        size_t fl[11];
        int nf = 0;
        size_t b = 0;
        for (size_t i = 0; i <= len && nf < 11; i++)
            if (i == len || line[i] == '\t') {
                f[nf] = line + b;
                fl[nf] = i - b;
                nf++;
                b = i + 1;
            }
        if (nf < 11) dies("ValueError", "fewer than 11 fields (sam2overlaps.py:149)" + at);
        int64_t flag, posv, tmp;
        if (!py_int(f[1], fl[1], flag)) dies("ValueError", "FLAG is not a number (sam2overlaps.py:151)" + at);
        const uint64_t bits = (uint64_t)(flag < 0 ? -flag : flag);  // power_find reads the binary digits of bin(n)
        if (bits & 4u) continue;                                    // unmapped
        // the CIGAR as runs of digits and of other characters (itertools.groupby(CIGAR, key=str.isdigit), :158)
        struct Run {
            size_t b, n;
            bool digits;
        };
        std::vector<Run> runs;
        for (size_t i = 0; i < fl[5];) {
            const bool dg = f[5][i] >= '0' && f[5][i] <= '9';
            size_t e = i;
            while (e < fl[5] && (f[5][e] >= '0' && f[5][e] <= '9') == dg) e++;
            runs.push_back(Run{i, e - i, dg});
            i = e;
        }
        if (runs.size() < 2) dies("IndexError", "a CIGAR without a count and a letter (sam2overlaps.py:162)" + at);
        auto run_is = [&](const Run& r, char c) { return r.n == 1 && f[5][r.b] == c; };
        auto run_int = [&](const Run& r) {
            int64_t v = 0;
            if (r.n > 10 || !py_int(f[5] + r.b, r.n, v) || v > 0x7FFFFFFFll) throw FatalError{HC_ERR_FORMAT, "a CIGAR count beyond 2^31 - 1" + at};
            return v;
        };
        hc_sam_aln a;
        memset(&a, 0, sizeof a);
        int64_t seq_len = (int64_t)fl[9];
        int64_t clip = 0;
        if (run_is(runs[1], 'S') || run_is(runs[1], 'H')) {  // (then runs[0] is the digits in front of it)
            if (!py_int(f[3], fl[3], posv)) dies("ValueError", "POS is not a number (sam2overlaps.py:164)" + at);
            clip = run_int(runs[0]);
            if (run_is(runs[1], 'H')) seq_len += clip;
        } else if (!py_int(f[3], fl[3], posv)) {
            dies("ValueError", "POS is not a number (sam2overlaps.py:174)" + at);
        }
        if (run_is(runs.back(), 'H')) seq_len += run_int(runs[runs.size() - 2]);
        if (!py_int(f[4], fl[4], tmp) || !py_int(f[7], fl[7], tmp) || !py_int(f[8], fl[8], tmp))
            dies("ValueError", "MAPQ, PNEXT or TLEN is not a number (sam2overlaps.py:182)" + at);
        if (seq_len > 0xFFFFFFFFll) throw FatalError{HC_ERR_FORMAT, "a sequence beyond 2^32 - 1 bases" + at};
        a.cpos = posv - clip;
        a.len = (uint32_t)seq_len;
        a.flag = (uint32_t)(bits & 0xFFFFFFFFu);
        a.ref = HC_SAM_NONE;
        a.op_first = (uint32_t)S.ops.size();
        // the operations, as compute_overlap_pos reads them: (runs[i], runs[i + 1]) for even i
        uint32_t marks = 0;
        if (!runs[0].digits) marks |= HC_SAM_CIGAR_VALUE_ERROR;       // int() of a letter, at the first operation
        else if (runs.size() % 2) marks |= HC_SAM_CIGAR_INDEX_ERROR;  // cigar[i + 1] behind the last count
        else {
            bool plain = true;
            for (size_t i = 0; i + 1 < runs.size(); i += 2) {
                const int64_t count = run_int(runs[i]);
                const Run& l = runs[i + 1];
                const char c = f[5][l.b];
                if (l.n != 1 || !((c >= 'A' && c <= 'Z') || c == '=') || count == 0) plain = false;
                S.ops.push_back(hc_sam_op{(uint32_t)count, l.n == 1 ? (uint32_t)(unsigned char)c : 0u});
            }
            if (plain) marks |= HC_SAM_CIGAR_PLAIN;
        }
        a.op_count = (uint32_t)(S.ops.size() - a.op_first);
        a.id_off = (uint32_t)S.id_text.size();
        a.id_len = (uint32_t)fl[0];
        S.id_text.append(f[0], fl[0]);
        if (fl[0] >= 1 && fl[0] <= 18 && (f[0][0] != '0' || fl[0] == 1)) {
            uint64_t v = 0;
            bool dg = true;
            for (size_t i = 0; i < fl[0]; i++) {
                dg = dg && f[0][i] >= '0' && f[0][i] <= '9';
                v = v * 10 + (uint64_t)(f[0][i] - '0');
            }
            if (dg) {
                marks |= HC_SAM_ID_PLAIN;
                a.id = v;
            }
        }
        a.marks = marks;
        if (S.id_text.size() > 0xFFFFFFFFull || S.ops.size() > 0xFFFFFFFFull || S.alns.size() >= HC_SAM_NONE)
            throw FatalError{HC_ERR_FORMAT, "more than 2^32 - 1 alignments, operations or id bytes"};
        out.push_back(Line{(uint32_t)S.alns.size(), f[2], fl[2]});
        S.alns.push_back(a);
    }
}

bool same_id(const hc_sam_view& v, uint32_t a, uint32_t b) {
    const hc_sam_aln &x = v.alns[a], &y = v.alns[b];
    if ((x.marks & y.marks & HC_SAM_ID_PLAIN) || !v.id_text) return x.id == y.id;  // (plain decimals are equal as texts iff equal as numbers)
    return x.id_len == y.id_len && memcmp(v.id_text + x.id_off, v.id_text + y.id_off, x.id_len) == 0;
}

void read_sam(const char* sam_s, const char* sam_p, const char* ref_fasta, hc_sam& S) {
    std::string fasta, text_s, text_p;
    if (!read_file(ref_fasta, fasta)) throw FatalError{HC_ERR_IO, std::string("cannot open ") + ref_fasta};
    std::map<std::string, uint32_t> ref_dict;
    read_fasta(fasta, S.ref_len, ref_dict);
    std::vector<Line> singles, mates;
    const bool have_s = sam_s && *sam_s, have_p = sam_p && *sam_p;
    if (have_s && !read_file(sam_s, text_s)) throw FatalError{HC_ERR_IO, std::string("cannot open ") + sam_s};
    if (have_s) read_sam_lines(text_s, "single-end", S, singles);
    if (have_p && !read_file(sam_p, text_p)) throw FatalError{HC_ERR_IO, std::string("cannot open ") + sam_p};
    if (have_p) read_sam_lines(text_p, "paired-end", S, mates);
    auto ref_of = [&](const Line& l) {  // ref_dict[ref_id], :93, :100
        const auto it = ref_dict.find(std::string(l.ref_name, l.ref_name_len));
        if (it == ref_dict.end()) dies("KeyError", "reference '" + std::string(l.ref_name, l.ref_name_len) + "' is not in the FASTA (sam2overlaps.py:93,100)");
        return it->second;
    };
    for (const Line& l : singles) S.recs.push_back(hc_sam_rec{l.aln, HC_SAM_NONE, 0, 0});
    S.n_singles = S.recs.size();
    // the paired file's state machine (:235-261): two consecutive mapped lines with equal ids
    const hc_sam_view v = S.view();
    bool held = false;
    uint32_t hold = 0;
    std::vector<const Line*> line_of(S.alns.size(), nullptr);
    for (const Line& l : mates) line_of[l.aln] = &l;
    for (const Line& l : mates) {
        if (!held) {
            hold = l.aln;
            held = true;
            continue;
        }
        if (!same_id(v, hold, l.aln)) {  // the older line goes, the newer stays (:241-244)
            hold = l.aln;
            continue;
        }
        held = false;
        const hc_sam_aln &a = S.alns[hold], &b = S.alns[l.aln];
        const bool ra = a.flag & 16u, rb = b.flag & 16u;
        if (a.cpos >= b.cpos) {
            if (ra && rb) S.recs.push_back(hc_sam_rec{l.aln, hold, 1, 0});  // reverse complement: [second, first, True]
        } else if (!ra && !rb) {
            S.recs.push_back(hc_sam_rec{hold, l.aln, 0, 0});
        }
    }
    for (const Line& l : singles) S.alns[l.aln].ref = ref_of(l);
    for (size_t k = S.n_singles; k < S.recs.size(); k++) S.alns[S.recs[k].first].ref = ref_of(*line_of[S.recs[k].first]);
}

// ---- the mirror: process_sam (:489-563) and get_overlaps (:372-481) as written -------------------------------------------------
[[noreturn]] void dies_in_pair(uint32_t err) {
    switch (err) {
        case kSamAssertCount: dies("AssertionError", "a CIGAR count of 0 (sam2overlaps.py:298)");
        case kSamAssertPerc: dies("AssertionError", "an overlap percentage outside 0 .. 100 (sam2overlaps.py:334,338)");
        case kSamZeroDivision: dies("ZeroDivisionError", "a read of length 0 (sam2overlaps.py:333)");
        case kSamCigarValue: dies("ValueError", "a CIGAR that starts with a letter (sam2overlaps.py:276,280)");
        case kSamCigarIndex: dies("IndexError", "a CIGAR that ends with a count (sam2overlaps.py:276,279)");
        default: throw FatalError{HC_ERR_FORMAT, "a position or length beyond 2^32 - 1 in an overlap line"};
    }
}

void records_to_lines(const hc_sam_view& v, int64_t mol, std::vector<hc_line_rec>& lines, std::vector<uint32_t>& src) {
    for (uint64_t k = 0; k < v.n_recs; k++) {
        const hc_sam_rec& r = v.recs[k];
        if (r.first >= v.n_alns || (r.second != HC_SAM_NONE && r.second >= v.n_alns) || v.alns[r.first].ref >= v.n_refs)
            throw FatalError{HC_ERR_ARG, "hc_host_sam_records_to_lines: a record points outside its arrays"};
    }
    for (uint64_t a = 0; a < v.n_alns; a++)
        if ((uint64_t)v.alns[a].op_first + v.alns[a].op_count > v.n_ops) throw FatalError{HC_ERR_ARG, "hc_host_sam_records_to_lines: operations outside the array"};
    std::vector<std::vector<uint32_t>> singles(v.n_refs), pairs(v.n_refs);  // :89-101
    for (uint64_t k = 0; k < v.n_recs; k++) (v.recs[k].second == HC_SAM_NONE ? singles : pairs)[v.alns[v.recs[k].first].ref].push_back((uint32_t)k);
    auto key = [&](uint32_t k) { return v.alns[v.recs[k].first].cpos; };
    for (uint64_t ref = 0; ref < v.n_refs; ref++) {
        std::vector<uint32_t>&s = singles[ref], &p = pairs[ref];
        if (s.empty() && p.empty()) continue;
        auto by_pos = [&](uint32_t a, uint32_t b) { return key(a) < key(b); };
        std::stable_sort(s.begin(), s.end(), by_pos);  // :493-494
        std::stable_sort(p.begin(), p.end(), by_pos);
        std::vector<uint32_t> merged;  // :496-519
        size_t k1 = 0, k2 = 0;
        while (k1 < s.size() && k2 < p.size()) merged.push_back(key(s[k1]) <= key(p[k2]) ? s[k1++] : p[k2++]);
        while (k1 < s.size()) merged.push_back(s[k1++]);
        while (k2 < p.size()) merged.push_back(p[k2++]);
        std::vector<uint32_t> active, next_active;  // :528
        size_t i = 0;
        int64_t cur_pos = key(merged[0]);
        while (cur_pos < (int64_t)v.ref_len[ref] && i < merged.size()) {  // :535
            const hc_sam_rec& rec = v.recs[merged[i]];
            const hc_sam_aln& R = v.alns[rec.first];
            cur_pos = R.cpos;
            next_active.clear();
            for (uint32_t q : active) {  // get_overlaps, :383-480
                const hc_sam_rec& read = v.recs[q];
                const hc_sam_aln& Q = v.alns[read.first];
                const int64_t overlap_pos = R.cpos - Q.cpos;
                if ((int64_t)Q.len - overlap_pos >= mol) next_active.push_back(q);  // :393
                hc_line_rec line;
                uint32_t from[2], err = 0;
                const bool both = rec.second != HC_SAM_NONE && read.second != HC_SAM_NONE;
                const SamPair a{rec.first, rec.second, rec.reverse}, b{read.first, read.second, read.reverse};
                const bool emitted = sam_pair_line(v.alns, v.ops, a, b, mol, both && same_id(v, read.first, rec.second), line, from, err);
                if (err) dies_in_pair(err);
                if (emitted) {
                    lines.push_back(line);
                    src.push_back(from[0]);
                    src.push_back(from[1]);
                }
            }
            active.swap(next_active);
            active.push_back(merged[i]);  // :542
            i++;
        }
    }
    if (v.n_recs == 0) dies("SystemExit", "no reads could be aligned to the reference (sam2overlaps.py:115-117)");
}

void lines_to_text(const hc_sam_view* v, const hc_line_rec* lines, const uint32_t* src, uint64_t n, std::string& out) {
    for (uint64_t k = 0; k < n; k++) {
        const hc_line_rec& l = lines[k];
        for (int side = 0; side < 2; side++) {
            if (src) {
                if (!v || src[2 * k + side] >= v->n_alns) throw FatalError{HC_ERR_ARG, "hc_host_sam_write_lines: a line's alignment is outside the view"};
                const hc_sam_aln& a = v->alns[src[2 * k + side]];
                out.append(v->id_text + a.id_off, a.id_len);
            } else {
                out += std::to_string(side ? l.id2 : l.id1);
            }
            out.push_back('\t');
        }
        char buf[160];
        const int k13 = snprintf(buf, sizeof buf, "%u\t%u\t%c\t%c\t%c\t%u\t%u\t%u\t%u\t%c\t%c\n", l.pos1, l.pos2, l.ord, l.ori1, l.ori2, l.perc1, l.perc2, l.len1,
                                 l.len2, l.type1, l.type2);
        out.append(buf, (size_t)k13);
    }
}

void write_text(const char* path, const std::string& text) {
    FILE* o = fopen(path, "wb");
    if (!o) throw FatalError{HC_ERR_IO, std::string("cannot write ") + path};
    const size_t w = fwrite(text.data(), 1, text.size(), o);
    if (fclose(o) != 0 || w != text.size()) throw FatalError{HC_ERR_IO, std::string("short write to ") + path};
}

}  // namespace

// for the stage (host/EdgeCalculator.cpp): the mirror's text in memory
void sam_view_to_overlaps_text(const hc_sam_view& v, int64_t min_overlap_len, std::string& out, uint64_t& n_lines) {
    std::vector<hc_line_rec> lines;
    std::vector<uint32_t> src;
    records_to_lines(v, min_overlap_len, lines, src);
    lines_to_text(&v, lines.data(), src.data(), lines.size(), out);
    n_lines = lines.size();
}

}  // namespace hc

using namespace hc;

extern "C" {

int hc_host_sam_read(hc_sam** out, const char* sam_s, const char* sam_p, const char* ref_fasta, hc_sam_view* view) {
    if (!out || !ref_fasta || !view) return set_last_error(HC_ERR_ARG, "hc_host_sam_read: null");
    *out = nullptr;
    hc_sam* S = new hc_sam();
    const int rc = guarded("sam2overlaps", [&] { read_sam(sam_s, sam_p, ref_fasta, *S); });
    if (rc) {
        delete S;
        return rc;
    }
    *view = S->view();
    *out = S;
    return HC_OK;
}

int hc_host_sam_free(hc_sam* s) {
    delete s;
    return HC_OK;
}

int hc_host_sam_records_to_lines(const hc_sam_view* view, int64_t min_overlap_len, hc_line_rec* lines, uint32_t* src, uint64_t cap, uint64_t* n_lines) {
    if (!view || !n_lines) return set_last_error(HC_ERR_ARG, "hc_host_sam_records_to_lines: null");
    return guarded("sam2overlaps", [&] {
        std::vector<hc_line_rec> l;
        std::vector<uint32_t> s;
        records_to_lines(*view, min_overlap_len, l, s);
        *n_lines = l.size();
        if (l.size() <= cap) {
            if (lines && !l.empty()) memcpy(lines, l.data(), l.size() * sizeof(hc_line_rec));
            if (src && !s.empty()) memcpy(src, s.data(), s.size() * sizeof(uint32_t));
        }
    });
}

int hc_host_sam_write_lines(const hc_sam_view* view, const hc_line_rec* lines, const uint32_t* src, uint64_t n, const char* out_path) {
    if (!out_path || (n && !lines) || (src && !view)) return set_last_error(HC_ERR_ARG, "hc_host_sam_write_lines: null");
    return guarded("sam2overlaps", [&] {
        std::string text;
        lines_to_text(view, lines, src, n, text);
        write_text(out_path, text);
    });
}

int hc_host_sam2overlaps(const char* sam_s, const char* sam_p, const char* ref_fasta, const char* out_path, int64_t min_overlap_len, uint64_t* n_lines) {
    if (!ref_fasta || !out_path) return set_last_error(HC_ERR_ARG, "hc_host_sam2overlaps: null path");
    return guarded("sam2overlaps", [&] {
        hc_sam S;
        read_sam(sam_s, sam_p, ref_fasta, S);
        std::string text;
        uint64_t n = 0;
        sam_view_to_overlaps_text(S.view(), min_overlap_len, text, n);
        write_text(out_path, text);
        if (n_lines) *n_lines = n;
    });
}

}  // extern "C"
