// hc_cycles_kernels.hip — what surrounds the host's depth-first walk of OverlapGraph::cycleRemovalHeuristic (src/GraphAlgos.cpp:352-541)
// on the device graph, in a number of launches that does not depend on the graph (hc_cycles.h; the rules: include/hcedge.h):
//   roots        sortVerticesByIndegree (:150-176): one radix sort of in-degree << 32 | vertex
//   columns      a try's neighbour order (:377-474).  Tries 1 - 4 are total orders over (key, target): a lane per record counts the
//                records of its own list that go before it, which is its place (the work is the sum of the squared list lengths),
//                while no list is longer than kRankMax; a graph with a longer list takes three stable radix sorts per column
//                (target, key, source) over (record index) instead.  Doubles go through an order-preserving transform of their bits that gives -0.0 and +0.0 one key;
//                descending orders take the complemented key.  Tries 5 - 20: a lane per record gathers through the host-built
//                permutation table of (try, list length).
//   components   weak components by union-find as hc_label_kernels.hip's (one hook pass, one compress pass), the ones that own a pair
//                of try 1 flagged, their vertices selected and their lists compacted and renumbered in ascending vertex order
//   find_records removeEdge's "first record u -> v" and "first u of adj_in[v]" (src/OverlapGraph.cpp:104-147): a wave per pair
#include <hip/hip_runtime.h>

#include "hc_cycles.h"
#include "hc_prims.h"

namespace hc {
namespace cycles {

namespace {

constexpr unsigned kBlock = 256;
unsigned grid_for(uint64_t n) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}
#define HC_TRY(call)                       \
    do {                                   \
        const hipError_t e__ = (call);     \
        if (e__ != hipSuccess) return e__; \
    } while (0)

// a double as an unsigned key in its own order; -0.0 and +0.0 share one (a == b in the reference's comparators, :409, :453)
__device__ __forceinline__ unsigned long long double_key(double x) {
    if (x == 0) x = 0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ unsigned long long int_key(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
// the key of try t = 1 .. 4: ascending keys are the reference's order
__device__ __forceinline__ unsigned long long try_key(const hc_edge_rec& e, uint32_t t) {
    return t == 1 ? int_key(e.pos1) : t == 2 ? ~double_key(e.score) : t == 3 ? 0xffffffffull - int_key(e.len0) : double_key(e.mismatch_rate);
}

__global__ void k_extract(const hc_edge_rec* __restrict__ E, const unsigned long long* __restrict__ out_off, uint32_t n, uint32_t* __restrict__ src,
                          uint32_t* __restrict__ tgt, unsigned long long* __restrict__ key, unsigned long long* __restrict__ nan_place) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const hc_edge_rec e = E[i];
        const uint32_t u = (uint32_t)e.v1;
        src[i] = u;
        tgt[i] = (uint32_t)e.v2;
        key[i] = try_key(e, 1);
        if (e.score != e.score || e.mismatch_rate != e.mismatch_rate) atomicMin(nan_place, (unsigned long long)u << 32 | (i - (uint32_t)out_off[u]));
    }
}

// col[off[u] + place] = tgt[i], place = the records of u's list before i in (key, target, position)
__global__ void k_rank(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, const unsigned long long* __restrict__ key,
                       const unsigned long long* __restrict__ off, uint32_t n, uint32_t* __restrict__ col) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t u = src[i], lo = (uint32_t)off[u], hi = (uint32_t)off[u + 1], t = tgt[i];
        const unsigned long long k = key[i];
        uint32_t place = 0;
        for (uint32_t q = lo; q < hi; q++) {
            const unsigned long long kq = key[q];
            const uint32_t tq = tgt[q];
            place += kq < k || (kq == k && (tq < t || (tq == t && q < i)));
        }
        col[lo + place] = t;
    }
}

__global__ void k_root_keys(const unsigned long long* __restrict__ in_off, uint32_t V, unsigned long long* __restrict__ keys) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) keys[v] = (in_off[v + 1] - in_off[v]) << 32 | v;
}

__global__ void k_uf_init(uint32_t* __restrict__ parent, uint8_t* __restrict__ root_flag, uint32_t V) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
        parent[v] = v;
        root_flag[v] = 0;
    }
}

// union-find as hc_label_kernels.hip's and hc_trans_kernels.hip's: parent[x] <= x throughout (the larger root hooks under the smaller)
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

__global__ void k_uf_hook(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, uint32_t n, uint32_t* parent) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) uf_unite(parent, src[i], tgt[i]);
}

// every vertex's root; a parent only ever moves towards the root, so writing in place cannot mislead another lane's walk
__global__ void k_uf_compress(uint32_t* parent, uint32_t V) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < V; x += gridDim.x * blockDim.x) {
        uint32_t r = x, nx;
        while ((nx = uf_load(parent + r)) != r) r = nx;
        __atomic_store_n(parent + x, r, __ATOMIC_RELAXED);
    }
}

__global__ void k_flag_roots(const uint32_t* __restrict__ pair_u, uint32_t n, const uint32_t* __restrict__ parent, uint8_t* __restrict__ root_flag) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) root_flag[parent[pair_u[i]]] = 1;
}

__global__ void k_flag_vertices(const uint32_t* __restrict__ parent, const uint8_t* __restrict__ root_flag, uint32_t V, uint8_t* __restrict__ vflag,
                                unsigned long long* __restrict__ n_components) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
        const uint32_t r = parent[v];
        vflag[v] = root_flag[r];
        if (r == v && root_flag[v]) atomicAdd(n_components, 1ull);  // (a handful)
    }
}

__global__ void k_sub_counts(const uint32_t* __restrict__ sub_vtx, uint32_t n, const unsigned long long* __restrict__ out_off, uint32_t* __restrict__ lid,
                             unsigned long long* __restrict__ sub_off) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        if (i == n) {
            sub_off[i] = 0;
            continue;
        }
        const uint32_t v = sub_vtx[i];
        lid[v] = i;
        sub_off[i] = out_off[v + 1] - out_off[v];
    }
}

// every target of a flagged vertex is flagged (same component), so every id has its place in lid.  A lane per record of the compact CSR:
// its owner by bisection of sub_off
__global__ void k_sub_fill(const hc_edge_rec* __restrict__ E, const uint32_t* __restrict__ sub_vtx, uint32_t n, const unsigned long long* __restrict__ out_off,
                           const uint32_t* __restrict__ lid, const unsigned long long* __restrict__ sub_off, uint64_t n_sub_edges, uint32_t* __restrict__ sub_src,
                           uint32_t* __restrict__ sub_tgt, unsigned long long* __restrict__ sub_key) {
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < n_sub_edges; d += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;  // the last i with sub_off[i] <= d (i < n because d < sub_off[n])
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (sub_off[mid] <= d) lo = mid;
            else hi = mid;
        }
        const uint32_t i = lo;
        const hc_edge_rec e = E[out_off[sub_vtx[i]] + (d - sub_off[i])];
        sub_src[d] = i;
        sub_tgt[d] = lid[(uint32_t)e.v2];
        sub_key[d] = try_key(e, 2);
        sub_key[n_sub_edges + d] = try_key(e, 3);
        sub_key[2 * n_sub_edges + d] = try_key(e, 4);
    }
}

// tries 5 .. 20: position j of a list of L records takes the target at position table[base + (t - 5) L + j] of the list
__global__ void k_shuffle(const uint32_t* __restrict__ sub_src, const uint32_t* __restrict__ sub_tgt, const unsigned long long* __restrict__ sub_off,
                          const unsigned long long* __restrict__ perm_base, const uint32_t* __restrict__ table, uint32_t n, uint32_t* __restrict__ cols) {
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < n; d += gridDim.x * blockDim.x) {
        const uint32_t i = sub_src[d];
        const unsigned long long lo = sub_off[i], L = sub_off[i + 1] - lo, base = perm_base[i], j = d - lo;
        for (uint32_t t = 0; t < 16; t++) cols[(size_t)(3 + t) * n + d] = sub_tgt[lo + table[base + t * L + j]];
    }
}

// a wave per pair: the first record u -> v of adj_out[u], the first u of adj_in[v]
__global__ void k_find_records(const hc_edge_rec* __restrict__ E, const unsigned long long* __restrict__ out_off, const uint32_t* __restrict__ in_nodes,
                               const unsigned long long* __restrict__ in_off, const unsigned long long* __restrict__ pairs, uint32_t n,
                               uint32_t* __restrict__ rec, uint32_t* __restrict__ in_pos, unsigned long long* __restrict__ missing) {
    const uint32_t lane = threadIdx.x & 63, n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < n; k += n_waves) {  // (k is the wave's: its lanes stay in step)
        const uint32_t u = (uint32_t)(pairs[k] >> 32), v = (uint32_t)pairs[k];
        uint32_t found = 0xffffffffu;
        for (unsigned long long base = out_off[u], hi = out_off[u + 1]; base < hi; base += 64) {
            const unsigned long long q = base + lane;
            const unsigned long long b = __ballot(q < hi && (uint32_t)E[q].v2 == v);
            if (b) {
                found = (uint32_t)base + (uint32_t)__ffsll((long long)b) - 1;
                break;
            }
        }
        uint32_t found_in = 0xffffffffu;
        for (unsigned long long base = in_off[v], hi = in_off[v + 1]; base < hi; base += 64) {
            const unsigned long long q = base + lane;
            const unsigned long long b = __ballot(q < hi && in_nodes[q] == u);
            if (b) {
                found_in = (uint32_t)base + (uint32_t)__ffsll((long long)b) - 1;
                break;
            }
        }
        if (lane == 0) {
            rec[k] = found;
            in_pos[k] = found_in;
            if (found == 0xffffffffu || found_in == 0xffffffffu) atomicAdd(missing, 1ull);
        }
    }
}

__global__ void k_long_list(const unsigned long long* __restrict__ out_off, uint32_t V, unsigned long long* __restrict__ longest) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
        const unsigned long long d = out_off[v + 1] - out_off[v];
        if (d > kRankMax) atomicMax(longest, d);  // (rare)
    }
}

// the radix form of a column: keys of the three stable passes, gathered through the order so far
__global__ void k_radix_start(const uint32_t* __restrict__ tgt, uint32_t n, uint32_t* __restrict__ k32, uint32_t* __restrict__ idx) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        k32[i] = tgt[i];
        idx[i] = i;
    }
}
__global__ void k_gather_key64(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ idx, uint32_t n, unsigned long long* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = key[idx[i]];
}
__global__ void k_gather_u32(const uint32_t* __restrict__ val, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = val[idx[i]];
}

__global__ void k_sort_prepare(const hc_edge_rec* __restrict__ E, uint32_t n, uint64_t n_reads, uint32_t* __restrict__ idx, unsigned long long* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        idx[i] = i;
        if (E[i].read1 >= n_reads || E[i].read2 >= n_reads) atomicAdd(bad, 1ull);
    }
}

__global__ void k_gather_seq(const uint32_t* __restrict__ seq, const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ seq_out) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) seq_out[k] = seq[order[k]];
}

}  // namespace

size_t temp_bytes(uint64_t E, uint64_t V) {
    size_t b = prims::sort_temp_bytes(V, sizeof(uint64_t), sizeof(uint32_t));
    const size_t scan64 = prims::scan_temp_bytes(V + 1, sizeof(uint64_t)), sel = prims::select_temp_bytes(V);
    b = b > scan64 ? b : scan64;
    b = b > sel ? b : sel;
    const size_t col = prims::sort_temp_bytes(E, sizeof(uint64_t), sizeof(uint32_t));  // the radix form of a column
    b = b > col ? b : col;
    return b ? b : 16;
}

namespace {
int bits_for(uint64_t n) {  // bits that hold every value below n (one at least)
    int b = 1;
    while (b < 64 && (n >> b) != 0) b++;
    return b;
}
// col = the targets in (source, key, target, position) order by three stable passes, least significant first; ids below n_ids.  The
// sorted order is the CSR's: position p of it is position p of the column.
hipError_t radix_column(const Work& w, const uint32_t* src, const uint32_t* tgt, const unsigned long long* key, uint32_t n, uint64_t n_ids, uint32_t* col,
                        hipStream_t s) {
    const int id_bits = bits_for(n_ids);
    hipLaunchKernelGGL(k_radix_start, grid_for(n), kBlock, 0, s, tgt, n, w.rs_k32a, w.rs_idx_a);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::sort_pairs(w.temp, w.temp_bytes, w.rs_k32a, w.rs_k32b, w.rs_idx_a, w.rs_idx_b, n, 0, id_bits, s));
    hipLaunchKernelGGL(k_gather_key64, grid_for(n), kBlock, 0, s, key, w.rs_idx_b, n, w.rs_k64a);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::sort_pairs(w.temp, w.temp_bytes, (const uint64_t*)w.rs_k64a, (uint64_t*)w.rs_k64b, w.rs_idx_b, w.rs_idx_a, n, 0, 64, s));
    hipLaunchKernelGGL(k_gather_u32, grid_for(n), kBlock, 0, s, src, w.rs_idx_a, n, w.rs_k32a);
    HC_TRY(hipGetLastError());
    HC_TRY(prims::sort_pairs(w.temp, w.temp_bytes, w.rs_k32a, w.rs_k32b, w.rs_idx_a, w.rs_idx_b, n, 0, id_bits, s));
    hipLaunchKernelGGL(k_gather_u32, grid_for(n), kBlock, 0, s, tgt, w.rs_idx_b, n, col);
    return hipGetLastError();
}
}  // namespace

hipError_t prepare(const trans::Graph& g, const Work& w, hipStream_t s) {
    HC_TRY(hipMemsetAsync(w.counters, 0, kCounters * 8, s));
    HC_TRY(hipMemsetAsync(w.counters + kNanPlace, 0xff, 8, s));
    if (!g.V) return hipSuccess;
    hipLaunchKernelGGL(k_long_list, grid_for(g.V), kBlock, 0, s, g.out_off, g.V, w.counters + kLongList);
    return hipGetLastError();
}

hipError_t first_try(const trans::Graph& g, const Work& w, bool radix, hipStream_t s) {
    if (g.E) {
        hipLaunchKernelGGL(k_extract, grid_for(g.E), kBlock, 0, s, g.edges, g.out_off, g.E, w.src, w.tgt, w.key, w.counters + kNanPlace);
        HC_TRY(hipGetLastError());
        if (radix) HC_TRY(radix_column(w, w.src, w.tgt, w.key, g.E, g.V, w.col1, s));
        else hipLaunchKernelGGL(k_rank, grid_for(g.E), kBlock, 0, s, w.src, w.tgt, w.key, g.out_off, g.E, w.col1);
    }
    if (!g.V) return hipGetLastError();
    hipLaunchKernelGGL(k_root_keys, grid_for(g.V), kBlock, 0, s, g.in_off, g.V, w.rk_a);
    HC_TRY(hipGetLastError());
    int top = 33;  // the in-degrees reach E
    while (top < 64 && ((unsigned long long)g.E >> (top - 32)) != 0) top++;
    return prims::sort_keys(w.temp, w.temp_bytes, (const uint64_t*)w.rk_a, (uint64_t*)w.rk_b, g.V, 0, top, s);
}

hipError_t components(const trans::Graph& g, const Work& w, uint32_t n_pairs, hipStream_t s) {
    hipLaunchKernelGGL(k_uf_init, grid_for(g.V), kBlock, 0, s, w.parent, w.root_flag, g.V);
    if (g.E) hipLaunchKernelGGL(k_uf_hook, grid_for(g.E), kBlock, 0, s, w.src, w.tgt, g.E, w.parent);
    hipLaunchKernelGGL(k_uf_compress, grid_for(g.V), kBlock, 0, s, w.parent, g.V);
    hipLaunchKernelGGL(k_flag_roots, grid_for(n_pairs), kBlock, 0, s, w.pair_u, n_pairs, w.parent, w.root_flag);
    hipLaunchKernelGGL(k_flag_vertices, grid_for(g.V), kBlock, 0, s, w.parent, w.root_flag, g.V, w.vflag, w.counters + kComponents);
    HC_TRY(hipGetLastError());
    return prims::select_flagged(w.temp, w.temp_bytes, w.vflag, g.V, w.sub_vtx, w.counters + kSubVertices, s);
}

hipError_t compact(const trans::Graph& g, const Work& w, uint32_t n_sub, hipStream_t s) {
    hipLaunchKernelGGL(k_sub_counts, grid_for(n_sub + 1ull), kBlock, 0, s, w.sub_vtx, n_sub, g.out_off, w.lid, w.sub_off);
    HC_TRY(hipGetLastError());
    return prims::exclusive_sum(w.temp, w.temp_bytes, (const uint64_t*)w.sub_off, (uint64_t*)w.sub_off, n_sub + 1ull, s);
}

hipError_t columns(const trans::Graph& g, const Work& w, uint32_t n_sub, uint64_t n_sub_edges, bool radix, hipStream_t s) {
    if (!n_sub_edges) return hipSuccess;
    const uint32_t n = (uint32_t)n_sub_edges;
    hipLaunchKernelGGL(k_sub_fill, grid_for(n), kBlock, 0, s, g.edges, w.sub_vtx, n_sub, g.out_off, w.lid, w.sub_off, n_sub_edges, w.sub_src, w.sub_tgt,
                       w.sub_key);
    HC_TRY(hipGetLastError());
    for (uint32_t t = 0; t < 3; t++) {
        if (radix) HC_TRY(radix_column(w, w.sub_src, w.sub_tgt, w.sub_key + t * n_sub_edges, n, n_sub, w.cols + t * n_sub_edges, s));
        else hipLaunchKernelGGL(k_rank, grid_for(n), kBlock, 0, s, w.sub_src, w.sub_tgt, w.sub_key + t * n_sub_edges, w.sub_off, n, w.cols + t * n_sub_edges);
    }
    hipLaunchKernelGGL(k_shuffle, grid_for(n), kBlock, 0, s, w.sub_src, w.sub_tgt, w.sub_off, w.perm_base, w.table, n, w.cols);
    return hipGetLastError();
}

hipError_t find_records(const trans::Graph& g, const Work& w, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_find_records, grid_for(64ull * n), kBlock, 0, s, g.edges, g.out_off, g.in_nodes, g.in_off, w.pairs, n, w.rec, w.in_pos,
                       w.counters + kMissing);
    return hipGetLastError();
}

hipError_t sort_prepare(const trans::Graph& g, uint32_t* idx, uint64_t n_reads, unsigned long long* bad, hipStream_t s) {
    HC_TRY(hipMemsetAsync(bad, 0, 8, s));
    if (!g.E) return hipSuccess;
    hipLaunchKernelGGL(k_sort_prepare, grid_for(g.E), kBlock, 0, s, g.edges, g.E, n_reads, idx, bad);
    return hipGetLastError();
}

hipError_t gather_seq(const uint32_t* seq, const uint32_t* order, uint32_t n, uint32_t* seq_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather_seq, grid_for(n), kBlock, 0, s, seq, order, n, seq_out);
    return hipGetLastError();
}

}  // namespace cycles
}  // namespace hc
