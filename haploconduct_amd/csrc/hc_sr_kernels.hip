// hc_sr_kernels.hip — super-read consensus on the device (include/hcsr.h): SRBuilder::consensus and consensus_pos
// (reference src/SRBuilder.cpp:289-535) for a batch of layouts against the read store.
//
// Two kernels.  sr_layout_kernel (one lane per layout) checks the layout, resolves every member to its oriented slot of the store and
// derives in closed form what the reference's serial loop carries: trim_pos (:430-450), the column where the suffix is cut (:479-482),
// the first column nobody covers (:507-510), a member shorter than its trimmed start (:490-494).  For a column c >= trim_pos a member is
// active exactly when pos <= c < pos + len: it was activated at `pos` (:468-472), started at trim_pos - pos when that lies before the trim
// (:452-459) and goes inactive with its last base (:501-503).  sr_column_kernel (one wave per layout, one lane per output column, 64
// consecutive columns at a time so that every member's symbols are read contiguously) adds the host-built log10 terms of the active
// members in list order in fp64 — the four sums are then the reference's, bit for bit — and takes the base by exact comparison in the
// reference's order A, T, C, G (:390-393).  The quality never comes from device transcendental functions (DESIGN.md "Super-read
// consensus"): columns of one or two members read it from a host-built table, a deeper column is finished here only where Phred 93
// follows from the sums by comparisons, and every other column is handed to the host as (layout, column, four sums).  The column's
// sums, its base, the table look-up and the output bytes are hc_sr_column.h's, which sr_self_merge_kernel uses too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_sr.h"
#include "hc_sr_column.h"

namespace hc {
namespace {

// (code, quality index) of a store symbol: hc_device.h.  code 0..3 = A, C, G, T, 4 = N, >= 5 = not a valid symbol.
__device__ inline void sr_decode(uint32_t sym, uint32_t symbytes, uint32_t lg, uint32_t& code, uint32_t& qidx) {
    if (symbytes == 1 && lg >= 6) {  // the wide 8-bit encodings: sym = qidx << 2 | base2, reserved indices below wide_first
        const uint32_t q = sym >> 2;
        if (q >= wide_first(lg)) {
            code = sym & 3u;
            qidx = q;
        } else {
            code = q == kWideN ? kCodeN : kCodeBadBase;
            qidx = 0;
        }
    } else {
        code = sym & 7u;
        qidx = symbytes == 2 ? sym >> 3 : (sym >> 3) & (lg == 3 ? 7u : 31u);
    }
}

__global__ __launch_bounds__(256) void sr_layout_kernel(StoreView st, const hc_sr_layout* __restrict__ layouts, uint64_t n_layouts,
                                                        const hc_sr_member* __restrict__ members, uint64_t n_members, uint32_t minimum_support,
                                                        uint32_t error_correction, SrMember* __restrict__ mem, SrLayoutInfo* __restrict__ info,
                                                        uint64_t* __restrict__ out_len) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > n_layouts) return;
    if (l == n_layouts) {  // the scan's last entry
        out_len[l] = 0;
        return;
    }
    const hc_sr_layout L = layouts[l];
    SrLayoutInfo o;
    o.ret = 0;
    o.status = HC_SR_BAD_LAYOUT;
    o.len = 0;
    o.trim = 0;
    out_len[l] = 0;
    bool ok = L.n_members != 0 && L.first_member <= n_members && L.n_members <= n_members - L.first_member && L.total_len >= 0;
    if (ok) {
        const hc_sr_member* m = members + L.first_member;
        SrMember* r = mem + L.first_member;
        int32_t prev = 0;
        for (uint32_t i = 0; i < L.n_members && ok; i++) {
            const hc_sr_member x = m[i];
            ok = x.read < st.n_reads && x.rev <= 1 && x.seq <= 2;
            if (!ok) break;
            const ReadDesc d = st.reads[x.read];
            const bool paired = (d.flags & kReadPaired) != 0;
            ok = paired ? x.seq != 0 : x.seq == 0;  // asserts of src/Read.h:145-149
            const uint32_t len = x.seq == 2 ? d.len2 : d.len1;
            ok = ok && (i == 0 ? x.pos == 0 : x.pos >= prev) && len != 0 && (uint64_t)x.pos + len <= (uint64_t)L.total_len;
            prev = x.pos;
            SrMember y;
            y.off = (x.seq == 2 ? d.off2 : d.off1) + (x.rev ? d.rc_delta : 0u);
            y.len = len;
            y.pos = x.pos;
            r[i] = y;
        }
    }
    if (!ok) {
        info[l] = o;
        return;
    }
    const SrMember* r = mem + L.first_member;
    const uint32_t n = L.n_members;
    int32_t trim = 0;
    if (error_correction) {  // :430-447: the iterator advances minimum_support - 1 times, or to the end
        const uint32_t it = minimum_support > 1 ? minimum_support - 1 : 0u;
        if (it >= n) {
            o.ret = -1;
            o.status = HC_SR_NO_SUPPORT;
            info[l] = o;
            return;
        }
        trim = r[it].pos;
    }
    o.trim = trim;
    // a member in front of the trim starts at trim - pos (:452-459): it is active at the first column whatever its length
    bool short_member = false;
    for (uint32_t i = 0; i < n; i++) short_member |= r[i].pos < trim && (uint32_t)(trim - r[i].pos) >= r[i].len;
    if (short_member && trim < L.total_len) {
        o.status = HC_SR_MEMBER_SHORT;
        info[l] = o;
        return;
    }
    // the suffix cut (:479-482): the first column at or after the last member's position, and the trim, with fewer than minimum_support
    // active members.  From there on all members have been activated, so the count only falls: a bisection.
    int32_t end = L.total_len;
    if (error_correction) {
        int32_t lo = max(trim, r[n - 1].pos), hi = L.total_len;  // the answer lies in [lo, hi]
        while (lo < hi) {
            const int32_t c = lo + (hi - lo) / 2;
            uint32_t cnt = 0;
            for (uint32_t i = 0; i < n; i++) cnt += (int64_t)r[i].pos + r[i].len > c;
            if (cnt < minimum_support) hi = c;
            else lo = c + 1;
        }
        end = lo;
    }
    // the first column >= trim that no member covers (:507-510): positions ascend, so a running maximum of the ends finds it
    int64_t reach = trim;
    int32_t gap = INT32_MAX;
    for (uint32_t i = 0; i < n; i++) {
        if (r[i].pos > reach) {
            gap = (int32_t)reach;
            break;
        }
        reach = max(reach, (int64_t)r[i].pos + r[i].len);
    }
    if (gap == INT32_MAX && reach < L.total_len) gap = (int32_t)reach;
    if (gap < end) {  // (at the same column the cut comes first: it is tested before the members are read)
        o.status = HC_SR_UNCOVERED;
        info[l] = o;
        return;
    }
    o.ret = trim;
    o.status = HC_SR_OK;
    o.len = end > trim ? (uint32_t)(end - trim) : 0u;
    info[l] = o;
    out_len[l] = o.len;
}

__global__ __launch_bounds__(256) void sr_column_kernel(StoreView st, uint32_t lg, const hc_sr_layout* __restrict__ layouts, uint64_t n_layouts,
                                                        const SrMember* __restrict__ mem, const SrLayoutInfo* __restrict__ info,
                                                        const uint64_t* __restrict__ out_off, const double* __restrict__ terms,
                                                        const uint8_t* __restrict__ qbyte, const uint8_t* __restrict__ table, uint32_t safe_region,
                                                        uint8_t* __restrict__ cons_seq, uint8_t* __restrict__ cons_qual,
                                                        uint32_t* __restrict__ late, SrHostColumn* __restrict__ host_cols, uint64_t host_cap,
                                                        unsigned long long* __restrict__ host_count) {
    __shared__ SrTerms T;
    __shared__ uint8_t q_of[sr::kQDim];
    T.load(terms);
    for (uint32_t i = threadIdx.x; i < sr::kQDim; i += blockDim.x) q_of[i] = qbyte[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint8_t* sym8 = (const uint8_t*)st.sym;
    const uint16_t* sym16 = (const uint16_t*)st.sym;
    // (the wave's number through readfirstlane: the layout, its members and the window are then wave-uniform values in scalar registers)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t l = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave; l < n_layouts; l += n_waves) {
        const SrLayoutInfo I = info[l];
        if (I.status != HC_SR_OK || I.len == 0) continue;  // (wave-uniform)
        const hc_sr_layout L = layouts[l];
        const SrMember* r = mem + L.first_member;
        const uint32_t n = L.n_members;
        const uint64_t o0 = out_off[l];
        const int32_t end = I.trim + (int32_t)I.len;
        // the members a block of 64 columns can meet lie in [first still active, last activated] of the position-sorted list
        uint32_t w_lo = 0, w_hi = 0;
        for (int32_t c0 = I.trim; c0 < end; c0 += 64) {
            const int32_t c = c0 + (int32_t)lane;
            const bool valid = c < end;
            while (w_hi < n && r[w_hi].pos < c0 + 64) w_hi++;
            while (w_lo < w_hi && (int64_t)r[w_lo].pos + r[w_lo].len <= c0) w_lo++;
            SrColumn col;
            bool bad = false;
            for (uint32_t i = w_lo; i < w_hi; i++) {
                const SrMember m = r[i];
                if (!(valid && c >= m.pos && (int64_t)c < (int64_t)m.pos + m.len)) continue;
                const uint64_t at = m.off + (uint32_t)(c - m.pos);
                const uint32_t sym = st.symbytes == 2 ? (uint32_t)sym16[at] : (uint32_t)sym8[at];
                uint32_t code, qi;
                sr_decode(sym, st.symbytes, lg, code, qi);
                if (code > kCodeN) {
                    bad = true;
                    code = kCodeN;
                }
                qi = code == kCodeN ? 0u : qi & (sr::kQDim - 1);
                const uint32_t q = code == kCodeN ? 0u : q_of[qi] & 127u;
                col.add(code, q, qi, T);
            }
            if (bad) atomicOr(&late[l], kSrLateBadSymbol);
            const double smax = col.max_sum();
            uint32_t entry = sr::kEntryN;  // Phred, kEntryN or kEntryNaN
            bool to_host = false;
            if (valid) {
                if (col.cnt == 1) entry = col.entry1(table);
                else if (col.cnt == 2) entry = col.entry2(table);
                else if (col.cnt >= 3) {
                    // Phred 93 without libm: the largest sum leads each of the other three by kSafeLead decades
                    const uint32_t led = (uint32_t)(smax - col.s0 >= sr::kSafeLead) + (uint32_t)(smax - col.s1 >= sr::kSafeLead) +
                                         (uint32_t)(smax - col.s2 >= sr::kSafeLead) + (uint32_t)(smax - col.s3 >= sr::kSafeLead);
                    if (safe_region && led == 3 && smax < 0.0 && smax > sr::kSafeFloor) entry = 93;
                    else to_host = true;
                }
                if (entry == sr::kEntryNaN) atomicOr(&late[l], kSrLateNaN);
            }
            const uint64_t o = o0 + (uint32_t)(c - I.trim);
            if (valid && !to_host) sr_put(entry, col.nuc(smax), cons_seq[o], cons_qual[o]);
            // the columns for the host: one atomic per wave
            const unsigned long long want = __ballot(to_host);
            if (want) {
                unsigned long long base = 0;
                if (lane == (uint32_t)__ffsll((long long)want) - 1u) base = atomicAdd(host_count, (unsigned long long)__popcll(want));
                base = __shfl(base, __ffsll((long long)want) - 1);
                const uint64_t at = base + __popcll(want & ((1ull << lane) - 1ull));
                if (to_host && at < host_cap) {
                    SrHostColumn h;
                    h.out = o;
                    h.n = col.cnt;
                    h.layout = (uint32_t)l;
                    h.s[0] = col.s0;
                    h.s[1] = col.s1;
                    h.s[2] = col.s2;
                    h.s[3] = col.s3;
                    host_cols[at] = h;
                }
            }
        }
    }
}

}  // namespace

hipError_t sr_launch_layouts(const StoreView& st, const hc_sr_layout* layouts, uint64_t n_layouts, const hc_sr_member* members, uint64_t n_members,
                             uint32_t minimum_support, uint32_t error_correction, SrMember* mem, SrLayoutInfo* info, uint64_t* out_len,
                             hipStream_t s) {
    const uint64_t blocks = (n_layouts + 1 + 255) / 256;
    hipLaunchKernelGGL(sr_layout_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, st, layouts, n_layouts, members, n_members, minimum_support,
                       error_correction, mem, info, out_len);
    return hipGetLastError();
}

hipError_t sr_launch_columns(const StoreView& st, uint32_t n_cu, const hc_sr_layout* layouts, uint64_t n_layouts, const SrMember* mem,
                             const SrLayoutInfo* info, const uint64_t* out_off, const double* terms, const uint8_t* qbyte, const uint8_t* table,
                             uint32_t safe_region, uint8_t* cons_seq, uint8_t* cons_qual, uint32_t* late, SrHostColumn* host_cols,
                             uint64_t host_cap, unsigned long long* host_count, hipStream_t s) {
    if (n_layouts == 0) return hipSuccess;
    const uint64_t want = (n_layouts + 3) / 4, most = (uint64_t)n_cu * 8;  // 4 waves a block, up to 32 waves a CU
    const uint32_t blocks = (uint32_t)(want < most ? want : most);
    hipLaunchKernelGGL(sr_column_kernel, dim3(blocks), dim3(256), 0, s, st, lut_lg(st.K), layouts, n_layouts, mem, info, out_off, terms, qbyte,
                       table, safe_region, cons_seq, cons_qual, late, host_cols, host_cap, host_count);
    return hipGetLastError();
}

}  // namespace hc
