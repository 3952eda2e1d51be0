// hc_label_kernels.hip — OverlapGraph::vertexLabellingHeuristic (src/GraphAlgos.cpp:178-349) and checkDuplicateEdges
// (src/OverlapGraph.cpp:578-605) on the device graph, in a number of launches that does not depend on the graph's diameter
// (hc_label.h; the rules: include/hcedge.h, "vertex labelling on the device graph"):
//   components   union-find over the doubled vertex set (2 v + p = "v with parity p"): a record with ori1 == ori2 unites equal
//                parities of its ends, any other the crossed ones; v's component holds an odd cycle iff 2 v and 2 v + 1 share a
//                root.  The start vertex of a component (sortVerticesByIndegree's first member) is an atomicMin of
//                in-degree << 32 | v; in a consistent component label[v] = (root(2 v) == root(2 start)).
//   conflicts    one lane per record: the conflict mask over the tries is L[u] ^ L[v] ^ class; per try one ballot, one atomic per wave
//   replay       one lane per record: the tries in order on the record's current state (one step where the labels do not change)
//   rebuild      out-lists by one stable sort of new source << 32 | moved << 31 | old index; in-lists by the rank of an entry among
//                the equal values of its list against the number of records of that pair that leave, then the pushes in move order
#include <hip/hip_runtime.h>

#include "hc_label.h"
#include "hc_prims.h"
#include "host/Labelling.h"

namespace hc {
namespace label {

namespace {

constexpr unsigned kBlock = 256;
unsigned grid_for(uint64_t n) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}
#define HC_TRY(call)                      \
    do {                                  \
        const hipError_t e__ = (call);    \
        if (e__ != hipSuccess) return e__; \
    } while (0)

__device__ __forceinline__ void wave_count(bool pred, unsigned long long* counter) {
    const unsigned long long b = __ballot(pred);  // every lane of the wave is here: the loops that call this run in step
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (unsigned long long)__popcll(b));
}
// the number of grid-stride rounds every lane makes, so that ballots see whole waves
__device__ __forceinline__ uint32_t rounds(uint32_t n) {
    const uint32_t stride = gridDim.x * blockDim.x;
    return (n + stride - 1) / stride;
}

__global__ void k_extract(const hc_edge_rec* __restrict__ E, uint32_t n, uint32_t* __restrict__ src, uint32_t* __restrict__ tgt,
                          uint8_t* __restrict__ same) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        src[i] = (uint32_t)E[i].v1;
        tgt[i] = (uint32_t)E[i].v2;
        same[i] = (E[i].ori1 != 0) == (E[i].ori2 != 0);
    }
}

// a record that repeats the (target, class) of an earlier record of its list
__global__ void k_repeated(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ same,
                           const unsigned long long* __restrict__ out_off, uint32_t n, unsigned long long* __restrict__ place) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t u = src[i], base = (uint32_t)out_off[u], t = tgt[i];
        const uint8_t c = same[i];
        for (uint32_t q = base; q < i; q++)
            if (tgt[q] == t && same[q] == c) {
                atomicMin(place, (unsigned long long)u << 32 | (i - base));
                break;
            }
    }
}

__global__ void k_init(uint32_t* __restrict__ parent, unsigned long long* __restrict__ start, uint32_t n2) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n2; x += gridDim.x * blockDim.x) {
        parent[x] = x;
        start[x] = kNoPlace;
    }
}

// union-find as hc_trans_kernels.hip's: parent[x] <= x throughout (the larger root hooks under the smaller)
__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ uint32_t uf_root(uint32_t* parent, uint32_t v) {  // with path halving
    uint32_t curr = uf_load(parent + v);
    if (curr != v) {
        uint32_t prev = v, next;
        while (curr > (next = uf_load(parent + curr))) {
            __atomic_store_n(parent + prev, next, __ATOMIC_RELAXED);
            prev = curr;
            curr = next;
        }
    }
    return curr;
}
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t x, uint32_t y) {
    uint32_t a = uf_root(parent, x), b = uf_root(parent, y);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicCAS(parent + a, a, b);  // a > b: hook a under b if a is still a root
        if (old == a) break;
        a = uf_root(parent, old);
        b = uf_root(parent, b);
    }
}

__global__ void k_hook(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ same, uint32_t n,
                       uint32_t* parent) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t u = src[i], v = tgt[i], x = same[i] ? 0u : 1u;
        uf_unite(parent, 2 * u, 2 * v + x);
        uf_unite(parent, 2 * u + 1, 2 * v + (1 - x));
    }
}

// every element's root; a parent only ever moves towards the root, so writing in place cannot mislead another lane's walk
__global__ void k_compress(uint32_t* parent, uint32_t n2) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n2; x += gridDim.x * blockDim.x) {
        uint32_t r = x, nx;
        while ((nx = uf_load(parent + r)) != r) r = nx;
        __atomic_store_n(parent + x, r, __ATOMIC_RELAXED);
    }
}

__device__ __forceinline__ uint32_t slot_of(const uint32_t* parent, uint32_t v) {
    const uint32_t a = parent[2 * v], b = parent[2 * v + 1];
    return a < b ? a : b;
}

__global__ void k_start(const uint32_t* __restrict__ parent, const unsigned long long* __restrict__ in_off, uint32_t V,
                        unsigned long long* __restrict__ start) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x)
        atomicMin(start + slot_of(parent, v), (in_off[v + 1] - in_off[v]) << 32 | v);
}

__global__ void k_labels(const uint32_t* __restrict__ parent, const unsigned long long* __restrict__ start, uint32_t V,
                         unsigned long long* __restrict__ L, uint8_t* __restrict__ host_flag, unsigned long long* __restrict__ counters) {
    const uint32_t stride = gridDim.x * blockDim.x, R = rounds(V);
    uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t r = 0; r < R; r++, v += stride) {
        bool first = false, odd = false;
        if (v < V) {
            const uint32_t s = (uint32_t)start[slot_of(parent, v)];
            odd = parent[2 * v] == parent[2 * v + 1];
            first = s == v;
            const bool lab = !odd && parent[2 * v] == parent[2 * s];
            L[2 * v] = lab ? ~0ull : 0ull;
            L[2 * v + 1] = lab ? (1ull << 36) - 1 : 0ull;
            host_flag[v] = odd;
        }
        wave_count(first, counters + kComponents);
        wave_count(first && odd, counters + kInconsistent);
    }
}

__global__ void k_sub_counts(const uint32_t* __restrict__ host_vtx, uint32_t n, const unsigned long long* __restrict__ in_off,
                             const unsigned long long* __restrict__ out_off, uint32_t* __restrict__ lid, unsigned long long* __restrict__ sub_in_off,
                             unsigned long long* __restrict__ sub_out_off) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        if (i == n) {
            sub_in_off[i] = sub_out_off[i] = 0;
            continue;
        }
        const uint32_t v = host_vtx[i];
        lid[v] = i;
        sub_in_off[i] = in_off[v + 1] - in_off[v];
        sub_out_off[i] = out_off[v + 1] - out_off[v];
    }
}

// every neighbour of a flagged vertex is flagged (same component), so every id has its place in lid
__global__ void k_sub_fill(const uint32_t* __restrict__ host_vtx, uint32_t n, const unsigned long long* __restrict__ in_off,
                           const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ in_nodes, const uint32_t* __restrict__ tgt,
                           const uint8_t* __restrict__ same, const uint32_t* __restrict__ lid, const unsigned long long* __restrict__ sub_in_off,
                           const unsigned long long* __restrict__ sub_out_off, uint32_t* __restrict__ sub_in, uint32_t* __restrict__ sub_out,
                           uint8_t* __restrict__ sub_same) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t v = host_vtx[i];
        unsigned long long d = sub_in_off[i];
        for (unsigned long long p = in_off[v]; p < in_off[v + 1]; p++) sub_in[d++] = lid[in_nodes[p]];
        d = sub_out_off[i];
        for (unsigned long long p = out_off[v]; p < out_off[v + 1]; p++, d++) {
            sub_out[d] = lid[tgt[p]];
            sub_same[d] = same[p];
        }
    }
}

__global__ void k_scatter_bits(const uint32_t* __restrict__ host_vtx, uint32_t n, const unsigned long long* __restrict__ bits,
                               unsigned long long* __restrict__ L) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t v = host_vtx[i];
        L[2 * v] = bits[2 * i];
        L[2 * v + 1] = bits[2 * i + 1];
    }
}

// :318 for every try at once: a record conflicts where (ori1 == ori2) != (label[u] == label[v])
__global__ void k_conflicts(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ same,
                            const unsigned long long* __restrict__ L, const uint8_t* __restrict__ host_flag, uint32_t n, uint32_t n_tries,
                            unsigned long long* __restrict__ per_try) {
    const uint32_t stride = gridDim.x * blockDim.x, R = rounds(n);
    const unsigned long long hi_mask = n_tries > 64 ? (n_tries >= 128 ? ~0ull : (1ull << (n_tries - 64)) - 1) : 0ull;
    const unsigned long long lo_mask = n_tries >= 64 ? ~0ull : (1ull << n_tries) - 1;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t r = 0; r < R; r++, i += stride) {
        unsigned long long m0 = 0, m1 = 0;
        if (i < n && host_flag[src[i]]) {  // (a consistent component has no conflict)
            const uint32_t u = src[i], v = tgt[i];
            m0 = L[2 * u] ^ L[2 * v], m1 = L[2 * u + 1] ^ L[2 * v + 1];
            if (!same[i]) m0 = ~m0, m1 = ~m1;
            m0 &= lo_mask, m1 &= hi_mask;
        }
        if (__ballot((m0 | m1) != 0) == 0) continue;
        for (uint32_t t = 0; t < n_tries; t++) {
            const unsigned long long b = __ballot(((t < 64 ? m0 >> t : m1 >> (t - 64)) & 1) != 0);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(per_try + t, (unsigned long long)__popcll(b));
        }
    }
}

// :303-348 for the tries in order on the record's own state; what the best try listed; the out-list key of what stays in the graph
__global__ void k_replay(hc_edge_rec* E, const unsigned long long* __restrict__ L, const uint8_t* __restrict__ host_flag, uint32_t n, uint32_t V,
                         uint32_t n_tries, uint32_t best, uint8_t* __restrict__ rec_flag, uint32_t* __restrict__ mv, uint32_t* __restrict__ rm_in,
                         unsigned long long* __restrict__ out_cnt, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                         unsigned long long* __restrict__ counters) {
    const uint32_t stride = gridDim.x * blockDim.x, R = rounds(n);
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t r = 0; r < R; r++, i += stride) {
        uint8_t flag = kKeep;
        bool switched = false;
        if (i < n) {
            hc_edge_rec e = E[i], listed = e;
            const uint32_t u = (uint32_t)e.v1, v = (uint32_t)e.v2;
            const bool was = e.ori1 != 0;
            const unsigned long long a0 = L[2 * u], a1 = L[2 * u + 1], b0 = L[2 * v], b1 = L[2 * v + 1];
            // a consistent component has the same labels in every try: after the first, the record is ok (or moved again, the same copy)
            const uint32_t steps = host_flag[u] ? n_tries : 1;
            for (uint32_t t = 0; t < steps; t++) {
                const bool tu = ((t < 64 ? a0 >> t : a1 >> (t - 64)) & 1) != 0, tv = ((t < 64 ? b0 >> t : b1 >> (t - 64)) & 1) != 0;
                const bool o1 = e.ori1 != 0, o2 = e.ori2 != 0;
                uint8_t f = kKeep;
                if (o1 == tu && o2 == tv) {
                } else if ((o1 == o2) != (tu == tv)) {
                    f = kDelete;
                } else {
                    hc_edge_rec c = e;
                    if (switch_edge_orientation(c)) {
                        f = kMove;
                        if (t == best || steps == 1) listed = c;
                    } else {
                        e = c;
                    }
                }
                if (t == best || steps == 1) flag = f;
            }
            switched = flag == kKeep && (e.ori1 != 0) != was;
            const uint32_t new_src = flag == kMove ? v : u;
            if (flag == kMove) E[i] = listed;
            else if (switched || steps > 1) E[i] = e;
            rec_flag[i] = flag;
            mv[i] = flag == kMove;
            keys[i] = flag == kDelete ? (unsigned long long)V << 32 | i : (unsigned long long)new_src << 32 | (flag == kMove ? 1ull << 31 : 0) | i;
            vals[i] = i;
            if (flag != kDelete) atomicAdd(out_cnt + new_src, 1ull);
            if (flag != kKeep) atomicAdd(rm_in + v, 1u);
        }
        wave_count(flag == kMove, counters + kMoved);
        wave_count(flag == kDelete, counters + kDeleted);
        wave_count(switched, counters + kSwitched);
    }
}

// An in-entry x of adj_in[w] stays unless it is among the first k entries x of its list, k = records x -> w that leave
__global__ void k_in_keep(const uint32_t* __restrict__ in_nodes, const unsigned long long* __restrict__ in_off, const unsigned long long* __restrict__ out_off,
                          const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ rec_flag, const uint32_t* __restrict__ rm_in, uint32_t n, uint32_t V,
                          uint32_t* __restrict__ in_owner, uint32_t* __restrict__ keep) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = V;  // the last w with in_off[w] <= p
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (in_off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const uint32_t w = lo, x = in_nodes[p];
        in_owner[p] = w;
        uint32_t stays = 1;
        if (rm_in[w]) {
            uint32_t k = 0, rank = 0;
            for (unsigned long long q = out_off[x]; q < out_off[x + 1]; q++) k += tgt[q] == w && rec_flag[q] != kKeep;
            for (uint32_t q = (uint32_t)in_off[w]; q < p && rank < k; q++) rank += in_nodes[q] == x;
            stays = rank >= k;
        }
        keep[p] = stays;
    }
}

__global__ void k_in_counts(const unsigned long long* __restrict__ in_off, const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ keep_sum,
                            const uint32_t* __restrict__ mv_sum, uint32_t V, unsigned long long* __restrict__ in_cnt) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w <= V; w += gridDim.x * blockDim.x)
        in_cnt[w] = w == V ? 0 : (keep_sum[in_off[w + 1]] - keep_sum[in_off[w]]) + (mv_sum[out_off[w + 1]] - mv_sum[out_off[w]]);
}

// lane i writes in-entry i where it stays and, where record i moves (u -> v becomes v -> u), v behind what stays of adj_in[u]: the
// moves of one source are its list's records in list order, which is the order of the reference's pushes
__global__ void k_in_write(const uint32_t* __restrict__ in_nodes, const uint32_t* __restrict__ in_owner, const unsigned long long* __restrict__ in_off,
                           const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt,
                           const uint8_t* __restrict__ rec_flag, const uint32_t* __restrict__ keep_sum, const uint32_t* __restrict__ mv_sum, uint32_t n,
                           const unsigned long long* __restrict__ in_off_next, uint32_t* __restrict__ in_nodes_next) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (keep_sum[i + 1] != keep_sum[i]) {
            const uint32_t w = in_owner[i];
            in_nodes_next[in_off_next[w] + (keep_sum[i] - keep_sum[in_off[w]])] = in_nodes[i];
        }
        if (rec_flag[i] == kMove) {
            const uint32_t u = src[i];
            in_nodes_next[in_off_next[u] + (keep_sum[in_off[u + 1]] - keep_sum[in_off[u]]) + (mv_sum[i] - mv_sum[out_off[u]])] = tgt[i];
        }
    }
}

__global__ void k_gather(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ seq, const uint32_t* __restrict__ order, uint32_t n,
                         const unsigned long long* __restrict__ out_off_next, uint32_t V, hc_edge_rec* __restrict__ E_next, uint32_t* __restrict__ seq_next) {
    const unsigned long long live = out_off_next[V];  // (the records that left sort behind every list)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n && k < live; k += gridDim.x * blockDim.x) {
        E_next[k] = E[order[k]];
        seq_next[k] = seq[order[k]];
    }
}

__global__ void k_duplicates(const hc_edge_rec* __restrict__ E, const unsigned long long* __restrict__ out_off, uint32_t n,
                             unsigned long long* __restrict__ place) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const uint32_t u = (uint32_t)E[k].v1, base = (uint32_t)out_off[u];
        if (k > base && E[k - 1].v2 == E[k].v2) atomicMin(place, (unsigned long long)u << 32 | (k - base));
    }
}

__global__ void k_orient(const unsigned long long* __restrict__ L, uint32_t V, uint32_t best, uint8_t* __restrict__ orient) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x)
        orient[v] = (uint8_t)((L[2 * v + (best >> 6)] >> (best & 63)) & 1);
}

}  // namespace

size_t temp_bytes(uint64_t E, uint64_t V) {
    size_t b = prims::sort_temp_bytes(E, sizeof(uint64_t), sizeof(uint32_t));
    const size_t scan64 = prims::scan_temp_bytes(V + 1, sizeof(uint64_t)), scan32 = prims::scan_temp_bytes(E + 1, sizeof(uint32_t)),
                 sel = prims::select_temp_bytes(V);
    b = b > scan64 ? b : scan64;
    b = b > scan32 ? b : scan32;
    b = b > sel ? b : sel;
    return b ? b : 16;
}

hipError_t prepare(const trans::Graph& g, const Work& w, hipStream_t s) {
    HC_TRY(hipMemsetAsync(w.counters, 0, kCounters * 8, s));
    HC_TRY(hipMemsetAsync(w.counters + kRepeated, 0xff, 8, s));
    HC_TRY(hipMemsetAsync(w.counters + kDuplicate, 0xff, 8, s));
    if (!g.E) return hipSuccess;
    hipLaunchKernelGGL(k_extract, grid_for(g.E), kBlock, 0, s, g.edges, g.E, w.src, w.tgt, w.same);
    hipLaunchKernelGGL(k_repeated, grid_for(g.E), kBlock, 0, s, w.src, w.tgt, w.same, g.out_off, g.E, w.counters + kRepeated);
    return hipGetLastError();
}

hipError_t components(const trans::Graph& g, const Work& w, hipStream_t s) {
    if (!g.V) return hipSuccess;
    hipLaunchKernelGGL(k_init, grid_for(2ull * g.V), kBlock, 0, s, w.parent, w.start, 2 * g.V);
    if (g.E) hipLaunchKernelGGL(k_hook, grid_for(g.E), kBlock, 0, s, w.src, w.tgt, w.same, g.E, w.parent);
    hipLaunchKernelGGL(k_compress, grid_for(2ull * g.V), kBlock, 0, s, w.parent, 2 * g.V);
    hipLaunchKernelGGL(k_start, grid_for(g.V), kBlock, 0, s, w.parent, g.in_off, g.V, w.start);
    hipLaunchKernelGGL(k_labels, grid_for(g.V), kBlock, 0, s, w.parent, w.start, g.V, w.L, w.host_flag, w.counters);
    HC_TRY(hipGetLastError());
    return prims::select_flagged(w.temp, w.temp_bytes, w.host_flag, g.V, w.host_vtx, w.counters + kHostVertices, s);
}

hipError_t compact_subgraph(const trans::Graph& g, const Work& w, uint32_t n_host, hipStream_t s) {
    hipLaunchKernelGGL(k_sub_counts, grid_for(n_host + 1ull), kBlock, 0, s, w.host_vtx, n_host, g.in_off, g.out_off, w.lid, w.sub_in_off, w.sub_out_off);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, (const uint64_t*)w.sub_in_off, (uint64_t*)w.sub_in_off, n_host + 1ull, s));
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, (const uint64_t*)w.sub_out_off, (uint64_t*)w.sub_out_off, n_host + 1ull, s));
    hipLaunchKernelGGL(k_sub_fill, grid_for(n_host), kBlock, 0, s, w.host_vtx, n_host, g.in_off, g.out_off, g.in_nodes, w.tgt, w.same, w.lid, w.sub_in_off,
                       w.sub_out_off, w.sub_in, w.sub_out, w.sub_same);
    return hipGetLastError();
}

hipError_t scatter_bits(const Work& w, uint32_t n_host, hipStream_t s) {
    if (!n_host) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_bits, grid_for(n_host), kBlock, 0, s, w.host_vtx, n_host, w.bits, w.L);
    return hipGetLastError();
}

hipError_t conflicts(const trans::Graph& g, const Work& w, uint32_t n_tries, hipStream_t s) {
    if (!g.E) return hipSuccess;
    hipLaunchKernelGGL(k_conflicts, grid_for(g.E), kBlock, 0, s, w.src, w.tgt, w.same, w.L, w.host_flag, g.E, n_tries, w.counters + kTry0);
    return hipGetLastError();
}

hipError_t apply(const trans::Graph& g, trans::Graph& out, const Work& w, uint32_t n_tries, uint32_t best, hipStream_t s) {
    const uint32_t V = g.V, E = g.E;
    hipLaunchKernelGGL(k_orient, grid_for(V), kBlock, 0, s, w.L, V, best, w.orient);
    HC_TRY(hipGetLastError());
    if (!E) return hipSuccess;
    HC_TRY(hipMemsetAsync(out.out_off, 0, (V + 1ull) * 8, s));
    HC_TRY(hipMemsetAsync(w.rm_in, 0, (size_t)V * 4, s));
    HC_TRY(hipMemsetAsync(w.mv_sum + E, 0, 4, s));
    HC_TRY(hipMemsetAsync(w.keep_sum + E, 0, 4, s));
    hipLaunchKernelGGL(k_replay, grid_for(E), kBlock, 0, s, g.edges, w.L, w.host_flag, E, V, n_tries, best, w.rec_flag, w.mv_sum, w.rm_in, out.out_off,
                       w.keys_a, w.val_a, w.counters);
    hipLaunchKernelGGL(k_in_keep, grid_for(E), kBlock, 0, s, g.in_nodes, g.in_off, g.out_off, w.tgt, w.rec_flag, w.rm_in, E, V, w.in_owner, w.keep_sum);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, w.keep_sum, w.keep_sum, E + 1ull, s));
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, w.mv_sum, w.mv_sum, E + 1ull, s));
    hipLaunchKernelGGL(k_in_counts, grid_for(V + 1ull), kBlock, 0, s, g.in_off, g.out_off, w.keep_sum, w.mv_sum, V, out.in_off);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, (const uint64_t*)out.in_off, (uint64_t*)out.in_off, V + 1ull, s));
    hipLaunchKernelGGL(k_in_write, grid_for(E), kBlock, 0, s, g.in_nodes, w.in_owner, g.in_off, g.out_off, w.src, w.tgt, w.rec_flag, w.keep_sum, w.mv_sum, E,
                       out.in_off, out.in_nodes);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::exclusive_sum(w.temp, w.temp_bytes, (const uint64_t*)out.out_off, (uint64_t*)out.out_off, V + 1ull, s));
    int top = 33;  // the keys' sources reach V itself (the records that leave)
    while (top < 64 && ((unsigned long long)V >> (top - 32)) != 0) top++;
    HC_TRY(prims::sort_pairs(w.temp, w.temp_bytes, (const uint64_t*)w.keys_a, (uint64_t*)w.keys_b, w.val_a, w.val_b, E, 0, top, s));
    hipLaunchKernelGGL(k_gather, grid_for(E), kBlock, 0, s, g.edges, g.seq, w.val_b, E, out.out_off, V, out.edges, out.seq);
    return hipGetLastError();
}

hipError_t check_duplicates(const trans::Graph& g, const Work& w, hipStream_t s) {
    HC_TRY(hipMemsetAsync(w.counters + kDuplicate, 0xff, 8, s));
    if (!g.E) return hipSuccess;
    hipLaunchKernelGGL(k_duplicates, grid_for(g.E), kBlock, 0, s, g.edges, g.out_off, g.E, w.counters + kDuplicate);
    return hipGetLastError();
}

}  // namespace label
}  // namespace hc
