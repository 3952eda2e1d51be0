// hc_sr_originals_kernels.hip — the device side of hc_sr_originals_init / _next / _write_text (include/hcsr.h): the original-read index maps
// of the next store from those of the current one (reference src/SRBuilder.cpp:750-806, :938-949, :1161-1216, :1312-1369) and the bytes of
// subreads.txt (:1449-1463).  Integer gathers, one lane per item — a source (a super-read's vertex or a graph vertex), a candidate entry, a
// kept entry, a new read — never a loop over a clique or a dict, so that one super-read of 10^4 originals costs what 10^4 pairs cost.  A lane
// finds its source, its super-read or its read by bisection over an exclusive sum.  The expressions are hc_sr_originals.h's, shared with the
// host mirror.  The only atomics are or-s into a new read's failure bits, issued by the entries that fail.
//
// or_init_kernel        read r -> its first_it entry (OverlapGraph.cpp:772-797).
// or_count_kernel       source j -> how many entries the dict of its read has; a trivial with none sets kBitEmpty.
// or_candidates_kernel  candidate t -> its source, the entry transformed, the key new id << 32 | original id.
// or_first_kernel       after the stable sort: the first of every run of equal keys wins (:762); a winner's failure bits go to its read.
// or_keep_kernel        a winner of a read without failure bits is kept.
// or_gather_kernel      after the ordered selection: kept entry u -> the new dict's entries, and its read for the offsets.
// or_offsets_kernel     new read r -> where its entries begin (bisection), and its status.
// or_text_sizes_kernel  item -> its characters: a line's id, or an entry; the line's last item owns the newline.
// or_text_write_kernel  after the sum: the characters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hc_device.h"
#include "hc_sr_originals.h"

namespace hc {
namespace orig {
namespace {

__device__ inline uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the largest j in [0, n) with a[j] <= x, for a[0] <= x < a[n] and ascending a
__device__ inline uint64_t owner(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void or_init_kernel(const ReadDesc* __restrict__ descs, uint32_t n_reads, uint64_t* __restrict__ off,
                                                      hc_sr_original* __restrict__ entries) {
    const uint64_t r = gid();
    if (r > n_reads) return;
    off[r] = r;
    if (r == n_reads) return;
    const ReadDesc d = descs[r];
    const bool paired = (d.flags & kReadPaired) != 0;
    entries[r] = hc_sr_original{(uint32_t)r, 0, 0, d.len1, paired ? d.len2 : 0u, (uint8_t)paired, 1, {0, 0}};
}

__global__ __launch_bounds__(256) void or_count_kernel(In I, Dict D, Work W) {
    const uint64_t j = gid(), n_src = I.n_sub + I.n_vertices;
    if (j > n_src) return;
    uint64_t n = 0;
    if (j < I.n_sub) {
        const uint64_t v = I.subreads[j].node;
        if (v < I.n_vertices) {
            const uint32_t r = I.vertex_read[v];
            if (r < D.n_reads) n = D.off[r + 1] - D.off[r];
        }
    } else if (j < n_src) {
        const uint64_t v = j - I.n_sub;
        if (I.vertex_state[v] == HC_SR_MN_V_TRIVIAL) {
            const uint32_t r = I.vertex_read[v];
            if (r < D.n_reads) n = D.off[r + 1] - D.off[r];
            const uint64_t id = I.nodes[v].id;
            if (n == 0 && id < I.n_new) atomicOr(&W.bits[id], kBitEmpty);  // assert (subreads.size() > 0), :1178
            if (id >= I.n_new) n = 0;
        }
    }
    W.cnt[j] = n;
}

__global__ __launch_bounds__(256) void or_candidates_kernel(In I, Dict D, Work W, uint64_t n_cand) {
    const uint64_t t = gid();
    if (t >= n_cand) return;
    const uint64_t n_src = I.n_sub + I.n_vertices;
    const uint64_t j = owner(W.cnt_off, n_src + 1, t);
    uint64_t v, id;
    Source s;
    if (j < I.n_sub) {
        const uint64_t k = owner(I.subread_off, I.n_srs + 1, j), c = I.sr_clique[k];
        const hc_fno_subread row = I.subreads[j];
        v = row.node;
        id = (uint32_t)I.new_id[c];
        s = sr_source(row, I.nodes[v], I.vertex_fwd[v], I.kind[c], I.overlap_pos[c], len2_of(I.first_layout, I.layouts, c), I.first_it);
    } else {
        v = j - I.n_sub;
        id = I.nodes[v].id;
        s = trivial_source(I.nodes[v], I.vertex_fwd[v]);
    }
    hc_sr_original e = D.entries[D.off[I.vertex_read[v]] + (t - W.cnt_off[j])];
    e.pad[0] = (uint8_t)transform(s, e);
    e.pad[1] = 0;
    W.cand[t] = e;
    W.key_in[t] = id << 32 | e.id;
    W.val_in[t] = (uint32_t)t;
}

__global__ __launch_bounds__(256) void or_first_kernel(Work W, uint64_t n_cand) {
    const uint64_t t = gid();
    if (t >= n_cand) return;
    const uint64_t key = W.key[t];
    const bool first = t == 0 || W.key[t - 1] != key;
    W.flag[t] = first;
    if (!first) return;
    const uint32_t b = W.cand[W.val[t]].pad[0];
    if (b) atomicOr(&W.bits[key >> 32], b);
}

__global__ __launch_bounds__(256) void or_keep_kernel(Work W, uint64_t n_cand) {
    const uint64_t t = gid();
    if (t >= n_cand) return;
    if (W.flag[t] && W.bits[W.key[t] >> 32]) W.flag[t] = 0;
}

__global__ __launch_bounds__(256) void or_gather_kernel(Work W, uint64_t n_cand) {
    const uint64_t u = gid();
    if (u >= n_cand || u >= *W.n_sel) return;
    const uint32_t t = W.sel[u];
    hc_sr_original e = W.cand[W.val[t]];
    e.pad[0] = 0;
    W.out_entries[u] = e;
    W.out_id[u] = (uint32_t)(W.key[t] >> 32);
}

__global__ __launch_bounds__(256) void or_offsets_kernel(In I, Work W) {
    const uint64_t r = gid();
    if (r > I.n_new) return;
    uint64_t lo = 0, hi = *W.n_sel;  // the first kept entry whose read is r or later
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (W.out_id[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    W.out_off[r] = lo;
    if (r < I.n_new) W.out_status[r] = status_of(W.bits[r]);
}

// items: read r's head (its id) at off[r] + r, its entries behind it; the line's last item — the head of a read without entries — also
// owns the newline; the last item is the sum's end
__global__ __launch_bounds__(256) void or_text_sizes_kernel(Dict D, uint64_t* __restrict__ sizes) {
    const uint64_t i = gid(), n_items = D.n_entries + D.n_reads;
    if (i > n_items) return;
    if (i == n_items) {
        sizes[i] = 0;
    } else if (i < D.n_entries) {
        const uint64_t r = owner(D.off, D.n_reads + 1, i);
        sizes[i + r + 1] = entry_chars(D.entries[i]) + (i + 1 == D.off[r + 1] ? 1u : 0u);
    } else {
        const uint64_t r = i - D.n_entries;
        sizes[D.off[r] + r] = dec_u32((uint32_t)r) + (D.off[r] == D.off[r + 1] ? 1u : 0u);
    }
}

__global__ __launch_bounds__(256) void or_text_write_kernel(Dict D, const uint64_t* __restrict__ pos, char* __restrict__ text) {
    const uint64_t i = gid(), n_items = D.n_entries + D.n_reads;
    if (i >= n_items) return;
    if (i < D.n_entries) {
        const uint64_t r = owner(D.off, D.n_reads + 1, i);
        char* p = put_entry(text + pos[i + r + 1], D.entries[i]);
        if (i + 1 == D.off[r + 1]) *p = '\n';
    } else {
        const uint64_t r = i - D.n_entries;
        char* p = put_u32(text + pos[D.off[r] + r], (uint32_t)r);
        if (D.off[r] == D.off[r + 1]) *p = '\n';
    }
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + 255) / 256 ? (n + 255) / 256 : 1)); }  // (n < 2^32)

}  // namespace

hipError_t launch_init(const void* descs, uint32_t n_reads, uint64_t* off, hc_sr_original* entries, hipStream_t stream) {
    hipLaunchKernelGGL(or_init_kernel, lanes((uint64_t)n_reads + 1), dim3(256), 0, stream, (const ReadDesc*)descs, n_reads, off, entries);
    return hipGetLastError();
}
hipError_t launch_count(In I, Dict D, Work W, hipStream_t stream) {
    hipLaunchKernelGGL(or_count_kernel, lanes(I.n_sub + I.n_vertices + 1), dim3(256), 0, stream, I, D, W);
    return hipGetLastError();
}
hipError_t launch_candidates(In I, Dict D, Work W, uint64_t n_cand, hipStream_t stream) {
    hipLaunchKernelGGL(or_candidates_kernel, lanes(n_cand), dim3(256), 0, stream, I, D, W, n_cand);
    return hipGetLastError();
}
hipError_t launch_first(Work W, uint64_t n_cand, hipStream_t stream) {
    hipLaunchKernelGGL(or_first_kernel, lanes(n_cand), dim3(256), 0, stream, W, n_cand);
    return hipGetLastError();
}
hipError_t launch_keep(Work W, uint64_t n_cand, hipStream_t stream) {
    hipLaunchKernelGGL(or_keep_kernel, lanes(n_cand), dim3(256), 0, stream, W, n_cand);
    return hipGetLastError();
}
hipError_t launch_gather(Work W, uint64_t n_cand, hipStream_t stream) {
    hipLaunchKernelGGL(or_gather_kernel, lanes(n_cand), dim3(256), 0, stream, W, n_cand);
    return hipGetLastError();
}
hipError_t launch_offsets(In I, Work W, hipStream_t stream) {
    hipLaunchKernelGGL(or_offsets_kernel, lanes(I.n_new + 1), dim3(256), 0, stream, I, W);
    return hipGetLastError();
}
hipError_t launch_text_sizes(Dict D, uint64_t* sizes, hipStream_t stream) {
    hipLaunchKernelGGL(or_text_sizes_kernel, lanes(D.n_entries + D.n_reads + 1), dim3(256), 0, stream, D, sizes);
    return hipGetLastError();
}
hipError_t launch_text_write(Dict D, const uint64_t* pos, char* text, hipStream_t stream) {
    hipLaunchKernelGGL(or_text_write_kernel, lanes(D.n_entries + D.n_reads), dim3(256), 0, stream, D, pos, text);
    return hipGetLastError();
}

}  // namespace orig
}  // namespace hc
