// kernels_genealogy.hip -- mhw_track_genealogy(): which part of day t - 1 of a selected object continues into which part
// of day t, and the split and merge counts taken from it.  The parts are those of kernels_parts.hip: the
// connected components of the object's footprint of the day under the K spatial neighbours nbr[c][K].  Part A of day
// t - 1 and part B of day t of one object are linked iff some cell lies in A on t - 1 and in B on t (overlap); the
// distinct links are the edges of the genealogy.  Entry offsets[i] + (t - time_start[i]) receives six counts over the
// parts of that day: n_parts, n_links (the sum of their in-degrees), n_born (in-degree 0), n_merged (in-degree >= 2),
// n_ended (out-degree 0) and n_split (out-degree >= 2).  The edges themselves go to the caller's buffer as
// (root of A << 32) | root of B, a root being the smallest voxel number of its part, in arbitrary order.
//
// Per voxel: parent, indeg, outdeg int32.  A hash set of `cap` 64-bit slots (cap a power of two, at least twice the
// number of keys the caller announces) deduplicates the (root, root) pairs; an empty slot is all ones, which no key
// equals because roots are below 2^31.
//
//   genealogy_init     lane = voxel / entry / table slot: parent[v] = v, the degrees and the six counts = 0, the table
//                      emptied.
//   parts_link         the union-find of kernels_parts.hip, launched there by launch_parts_union() (object_rows.h): lane
//   parts_flatten      = row, voxels of one day united; lane = voxel: parent[v] = find(v).
//   genealogy_pairs    lane = row.  For every day t of the row but its last the key (root(vox(r, t)), root(vox(r, t + 1)));
//                      where the next row holds the same cell and slot, is fit and starts on end + 1, the key across the
//                      two rows too.  Each key is put into the table by linear probing from a mixed hash, one 64-bit
//                      compare-and-swap per probe: an empty slot taken makes the lane the one winner of that distinct
//                      pair, the same key found ends the lane's work on it, another key sends it to the next slot.  The
//                      probe loop ends after `cap` probes at the latest and then raises *overflow: no lane waits for
//                      another lane's progress.  The winner adds 1 to outdeg[root A] and to indeg[root B].
//   genealogy_collect  lane = table slot: the slots in use are copied to edges[]; a wave takes its places from the cursor
//                      *n_edges with one atomic, and no place at or beyond edge_capacity is written.
//   genealogy_count    lane = row, walking its days as parts_count does: a voxel that is its own root adds to the six
//                      counters of its entry from its two degrees; integer atomics without a return value.
//
// Rows that are not fit (object_rows.h, fit_row<true>) are left out of every kernel and counted in *n_bad by
// genealogy_count.  Nothing outside entries 0..L-1, voxels 0..V-1, table slots 0..cap-1 and edges 0..edge_capacity-1 is ever written.  Every count
// is an integer sum and the set of edges is a set: exact, and the same under any schedule once the edges are sorted.
#include "device_common.h"
#include "kernels.h"
#include "object_rows.h"

namespace xmhw {

namespace {

using u64 = unsigned long long;
constexpr u64 kEmpty = ~0ull;

__global__ __launch_bounds__(kRowThreads) void genealogy_init(int64_t V, int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ indeg, int32_t* __restrict__ outdeg,
                                                              int64_t L, int32_t* __restrict__ counts, int64_t cap,
                                                              u64* __restrict__ table) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < V) {
        parent[i] = static_cast<int32_t>(i);
        indeg[i] = 0;
        outdeg[i] = 0;
    }
    if (i < L)
        for (int f = 0; f < kGenealogyFields; ++f) counts[f * L + i] = 0;
    if (i < cap) table[i] = kEmpty;
}

// both roots are voxels of fit rows: within [0, V), below 2^31
__device__ __forceinline__ void put_pair(int32_t ra, int32_t rb, u64* __restrict__ table, int64_t cap,
                                         int32_t* __restrict__ indeg, int32_t* __restrict__ outdeg,
                                         int32_t* __restrict__ overflow) {
    const u64 key = (static_cast<u64>(static_cast<uint32_t>(ra)) << 32) | static_cast<uint32_t>(rb);
    const u64 mask = static_cast<u64>(cap) - 1;
    u64 at = mix64(key) & mask;
    for (int64_t probe = 0; probe < cap; ++probe, at = (at + 1) & mask) {
        u64 seen = kEmpty;
        if (__hip_atomic_compare_exchange_strong(table + at, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
            atomicAdd(outdeg + ra, 1);               // the one winner of this distinct pair
            atomicAdd(indeg + rb, 1);
            return;
        }
        if (seen == key) return;                     // a duplicate
    }
    atomicOr(overflow, 1);                           // a full table: the caller announced too few keys
}

__global__ __launch_bounds__(kRowThreads) void genealogy_pairs(ObjectRows a, const int32_t* __restrict__ parent,
                                                               u64* __restrict__ table, int64_t cap,
                                                               int32_t* __restrict__ indeg, int32_t* __restrict__ outdeg,
                                                               int32_t* __restrict__ overflow) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    if (fit_row<true>(a, r, me) != 1) return;
    const int64_t days = static_cast<int64_t>(me.e) - me.s + 1;
    int32_t ra = parent[me.vox];                     // a root is a voxel of a fit row of the same day: within [0, V)
    for (int64_t d = 1; d < days; ++d) {
        const int32_t rb = parent[me.vox + d];
        put_pair(ra, rb, table, cap, indeg, outdeg, overflow);
        ra = rb;
    }
    if (r + 1 >= a.n || a.cell[r + 1] != me.c || a.slot[r + 1] != me.sl) return;
    ObjectRow next;                                    // the same cell goes on in the next row without a free day
    if (fit_row<true>(a, r + 1, next) != 1 || static_cast<int64_t>(next.s) != static_cast<int64_t>(me.e) + 1) return;
    put_pair(ra, parent[next.vox], table, cap, indeg, outdeg, overflow);
}

__global__ __launch_bounds__(kRowThreads) void genealogy_collect(const u64* __restrict__ table, int64_t cap,
                                                                 u64* __restrict__ edges, int64_t edge_capacity,
                                                                 u64* __restrict__ n_edges) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const u64 key = i < cap ? table[i] : kEmpty;     // every lane of the wave reaches the ballot
    const bool used = key != kEmpty;
    const u64 users = __ballot(used);
    if (users == 0) return;
    const int lane = static_cast<int>(__lane_id());
    const int leader = __ffsll(static_cast<long long>(users)) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(n_edges, static_cast<u64>(__popcll(users)));
    base = static_cast<u64>(__shfl(static_cast<long long>(base), leader, 64));
    if (!used) return;
    const u64 place = base + static_cast<u64>(__popcll(users & ((1ull << lane) - 1)));
    if (place < static_cast<u64>(edge_capacity)) edges[place] = key;
}

__global__ __launch_bounds__(kRowThreads) void genealogy_count(ObjectRows a, const int32_t* __restrict__ parent,
                                                               const int32_t* __restrict__ indeg,
                                                               const int32_t* __restrict__ outdeg,
                                                               int32_t* __restrict__ counts, int32_t* __restrict__ n_bad) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    const int fit = fit_row<true>(a, r, me);
    if (fit < 0) atomicAdd(n_bad, 1);
    if (fit != 1) return;
    const int64_t days = static_cast<int64_t>(me.e) - me.s + 1;
    for (int64_t d = 0; d < days; ++d) {
        const int64_t v = me.vox + d;
        if (parent[v] != v) continue;
        int32_t* at = counts + (me.entry + d);       // within [offsets[slot], offsets[slot + 1]), itself within [0, L)
        const int32_t in = indeg[v], out = outdeg[v];
        atomicAdd(at + kGenealogyParts * a.L, 1);
        if (in) atomicAdd(at + kGenealogyLinks * a.L, in);
        if (in == 0) atomicAdd(at + kGenealogyBorn * a.L, 1);
        if (in >= 2) atomicAdd(at + kGenealogyMerged * a.L, 1);
        if (out == 0) atomicAdd(at + kGenealogyEnded * a.L, 1);
        if (out >= 2) atomicAdd(at + kGenealogySplit * a.L, 1);
    }
}

}  // namespace

int64_t object_genealogy_table_slots(int64_t edge_capacity) {
    int64_t cap = 2;
    while (cap < 2 * (edge_capacity > 1 ? edge_capacity : 1)) cap *= 2;
    return cap;
}

size_t object_genealogy_scratch_bytes(int64_t V, int64_t edge_capacity) {
    return static_cast<size_t>(kGenealogySlotBytes) * static_cast<size_t>(object_genealogy_table_slots(edge_capacity)) +
           static_cast<size_t>(kGenealogyVoxelBytes) * static_cast<size_t>(V > 0 ? V : 1);
}

hipError_t launch_object_genealogy(const int32_t* start, const int32_t* end, const int32_t* slot,
                                   const int32_t* cell_of_row, int64_t n, const int64_t* row_offsets, int64_t C,
                                   const int32_t* nbr, int32_t K, const int64_t* vox_off, int64_t V,
                                   const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L,
                                   int32_t* counts, uint64_t* edges, int64_t edge_capacity, int64_t* n_edges,
                                   int32_t* n_bad, int32_t* overflow, void* scratch, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(overflow, 0, sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(n_edges, 0, sizeof(int64_t), stream);
    if (e != hipSuccess) return e;
    // the 64-bit table first (8-byte aligned), then the three 32-bit arrays
    const int64_t cap = object_genealogy_table_slots(edge_capacity);
    u64* table = static_cast<u64*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(table + cap);
    int32_t* indeg = parent + (V > 0 ? V : 0);
    int32_t* outdeg = indeg + (V > 0 ? V : 0);
    int64_t items = V > L ? V : L;
    items = cap > items ? cap : items;
    const dim3 b(kRowThreads);
    hipLaunchKernelGGL(genealogy_init, dim3(blocks_for(items)), b, 0, stream, V, parent, indeg, outdeg, L, counts, cap, table);
    if (n > 0 && n_slots > 0 && L > 0) {
        const ObjectRows rows{start, end, slot, cell_of_row, time_start, offsets, n, C, n_slots, L, vox_off, V};
        const dim3 g(blocks_for(n));
        if (V > 0) {
            launch_parts_union(rows, row_offsets, nbr, K, parent, V, stream);
            hipLaunchKernelGGL(genealogy_pairs, g, b, 0, stream, rows, static_cast<const int32_t*>(parent), table, cap, indeg,
                               outdeg, overflow);
            hipLaunchKernelGGL(genealogy_collect, dim3(blocks_for(cap)), b, 0, stream, static_cast<const u64*>(table), cap,
                               reinterpret_cast<u64*>(edges), edge_capacity, reinterpret_cast<u64*>(n_edges));
        }
        hipLaunchKernelGGL(genealogy_count, g, b, 0, stream, rows, static_cast<const int32_t*>(parent),
                           static_cast<const int32_t*>(indeg), static_cast<const int32_t*>(outdeg), counts, n_bad);
    }
    return hipGetLastError();
}

}  // namespace xmhw
