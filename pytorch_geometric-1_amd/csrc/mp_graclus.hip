// graclus on the device: the deterministic greedy matching of include/mi355_mp.h
// "Graclus" (PyG 1.4.3 nn.pool.graclus over torch_cluster 1.5 graclus_cluster [U],
// whose randomised propose / respond matching is replaced by a pure function of
// the graph).
//
// The caller hands over one node-sorted incidence list of the 2 * n_edges directed
// entries (mp_csr_build over cat(row, col) / cat(col, row)): row u of it holds
// every entry that touches u, whichever way it points.  mp_graclus_init computes
// the 64-bit priority word (wkey << 32) | h of every entry once, in incidence
// order, so a round reads nbr[j] and key[j] side by side and gathers only the
// neighbour's matched byte.
//
// A round is two launches.  k_graclus_point: every live node (unmatched, and it
// pointed at somebody last round) scans its row, skips loops and matched
// neighbours, keeps the entry of largest priority (key, min(u, v), max(u, v)) and
// writes the neighbour as its pointer, or -1 when nothing is left: it is then a
// singleton for good, as a node's unmatched neighbours only ever shrink.
// k_graclus_match: mutual pointers match, the larger end takes the smaller as its
// cluster, and the nodes that pointed in vain are counted as still live.  The
// priority is a strict order on pairs, so the pair that is largest among the
// entries with two unmatched ends is pointed at from both sides: it is the greedy
// matching's next choice, and every other mutual pair is one the greedy takes
// later without interference.  The handshake therefore equals the serial greedy
// walk exactly, whatever the launch shape or the order of the entries.
//
// One lane owns one node.  A row longer than kGraclusLongRow is not scanned by its
// lane: the wave takes such rows one at a time, all 64 lanes striding over the
// entries, and a butterfly of the (key, neighbour) pairs leaves the maximum with
// the owner, so a hub costs its wave len / 64 steps instead of len.
//
// No float atomics; the one atomic is the integer count of live nodes, one add
// per wave.  Rounds are separate launches: a round whose predecessor left nobody
// live returns at once (the host enqueues them in batches and reads the counts
// once per batch).  No grid is capped: one thread per node (n < 2^30) or entry
// (2 * n_edges < 2^31) in workgroups of 256 stays below 2^23 workgroups.
#include "mp_workspace.h"

namespace mp {

constexpr int kGraclusBlock = 256;
constexpr int kGraclusLongRow = 64;
constexpr int64_t kGraclusMaxSize = (int64_t)1 << 30;
constexpr int64_t kGraclusMaxRounds = 4096;

// counts (int64[4]): [0] rounds run, [1 + (r & 1)] nodes still live after round r
// (so [2] also holds the nodes live before round 0), [3] entries whose position or
// ends lie outside their range
__device__ __forceinline__ int64_t live_before(const int64_t* counts, int64_t r) { return counts[1 + ((r + 1) & 1)]; }

__device__ __forceinline__ uint64_t graclus_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// is entry (k1, v1) of node u above entry (k2, v2)?  Equal keys fall to the pair
// (min, max); two entries of one pair with one key are equal: false.
__device__ __forceinline__ bool graclus_above(uint64_t k1, int v1, uint64_t k2, int v2, int u) {
  if (k1 != k2) return k1 > k2;
  const int a1 = v1 < u ? v1 : u, b1 = v1 < u ? u : v1;
  const int a2 = v2 < u ? v2 : u, b2 = v2 < u ? u : v2;
  return a1 != a2 ? a1 > a2 : b1 > b2;
}

// one thread per incidence entry j: key[j] = (wkey << 32) | h of its pair, and
// ptr[u] = 0 (live) for the owner of every entry that is no loop
__global__ __launch_bounds__(kGraclusBlock) void k_graclus_keys(const int64_t* __restrict__ row,
                                                                const int64_t* __restrict__ col,
                                                                const int32_t* __restrict__ eid,
                                                                const float* __restrict__ weight, int64_t n,
                                                                int64_t n_edges, uint64_t seed_mix,
                                                                uint64_t* __restrict__ key, int32_t* __restrict__ ptr,
                                                                unsigned long long* __restrict__ counts) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < 2 * n_edges;
  bool bad = false;
  if (in) {
    const int64_t e = eid[j];
    uint64_t k = 0;
    bad = e < 0 || e >= 2 * n_edges;
    if (!bad) {
      const int64_t o = e < n_edges ? e : e - n_edges;
      const int64_t r = row[o], c = col[o];
      bad = r < 0 || r >= n || c < 0 || c >= n;
      if (!bad && r != c) {
        const uint64_t a = (uint64_t)(r < c ? r : c), b = (uint64_t)(r < c ? c : r);
        const uint64_t h = graclus_mix64(seed_mix ^ ((a << 32) | b)) >> 32;
        uint32_t wk = 0;
        if (weight) {
          const uint32_t u = __float_as_uint(weight[o]);
          wk = (u >> 31) ? ~u : (u | 0x80000000u);
        }
        k = ((uint64_t)wk << 32) | h;
        ptr[e < n_edges ? r : c] = 0;  // the row this entry was sorted into; every writer stores the same value
      }
    }
    key[j] = k;
  }
  const unsigned long long m = __ballot(bad);
  if (m != 0 && lane_id() == 0) atomicAdd(counts + 3, (unsigned long long)__popcll(m));
}

// one thread per node: cluster[u] = u, done[u] = 0, and the live nodes counted
__global__ __launch_bounds__(kGraclusBlock) void k_graclus_nodes(int64_t n, const int32_t* __restrict__ ptr,
                                                                 uint8_t* __restrict__ done,
                                                                 int64_t* __restrict__ cluster,
                                                                 unsigned long long* __restrict__ counts) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool live = false;
  if (u < n) {
    cluster[u] = u;
    done[u] = 0;
    live = ptr[u] == 0;
  }
  const unsigned long long m = __ballot(live);
  if (m != 0 && lane_id() == 0) atomicAdd(counts + 2, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kGraclusBlock) void k_graclus_point(const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ nbr,
                                                                 const uint64_t* __restrict__ key,
                                                                 const uint8_t* __restrict__ done, int n,
                                                                 int64_t n_entries, int64_t round,
                                                                 int32_t* __restrict__ ptr,
                                                                 int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) counts[1 + (round & 1)] = 0;  // this round's live count: k_graclus_match adds to it
  if (live_before(counts, round) == 0) return;
  const int u = t < n ? (int)t : -1;
  int64_t p0 = 0, p1 = 0;
  bool active = false;
  if (u >= 0 && !done[u] && ptr[u] >= 0) {
    p0 = rowptr[u];
    p1 = rowptr[u + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > n_entries) p1 = n_entries;
    active = true;
  }
  uint64_t bk = 0;
  int bv = -1;
  const bool is_long = active && p1 - p0 > kGraclusLongRow;
  if (active && !is_long) {
    for (int64_t j = p0; j < p1; ++j) {
      const int v = nbr[j];
      if (v == u || (unsigned)v >= (unsigned)n || done[v]) continue;
      const uint64_t k = key[j];
      if (bv < 0 || graclus_above(k, v, bk, bv, u)) {
        bk = k;
        bv = v;
      }
    }
  }
  // the wave's long rows, one at a time: 64 lanes stride over the entries
  unsigned long long todo = __ballot(is_long);
  const int lane = lane_id();
  while (todo) {
    const int l = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int uu = __shfl(u, l);
    const int64_t q0 = __shfl(p0, l), q1 = __shfl(p1, l);
    uint64_t ck = 0;
    int cv = -1;
    for (int64_t j = q0 + lane; j < q1; j += 64) {
      const int v = nbr[j];
      if (v == uu || (unsigned)v >= (unsigned)n || done[v]) continue;
      const uint64_t k = key[j];
      if (cv < 0 || graclus_above(k, v, ck, cv, uu)) {
        ck = k;
        cv = v;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const uint64_t ok = __shfl_xor(ck, off);
      const int ov = __shfl_xor(cv, off);
      if (ov >= 0 && (cv < 0 || graclus_above(ok, ov, ck, cv, uu))) {
        ck = ok;
        cv = ov;
      }
    }
    if (lane == l) bv = cv;
  }
  if (active) ptr[u] = bv;
}

__global__ __launch_bounds__(kGraclusBlock) void k_graclus_match(const int32_t* __restrict__ ptr, int n,
                                                                 int64_t round, uint8_t* __restrict__ done,
                                                                 int64_t* __restrict__ cluster,
                                                                 int64_t* __restrict__ counts) {
  if (live_before(counts, round) == 0) return;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) counts[0] = round + 1;
  bool still = false;
  if (t < n && !done[t]) {
    const int u = (int)t;
    const int p = ptr[u];
    if (p >= 0 && p < n) {
      if (ptr[p] == u) {
        done[u] = 1;
        if (p < u) cluster[u] = p;
      } else {
        still = true;
      }
    }
  }
  const unsigned long long m = __ballot(still);
  if (m != 0 && lane_id() == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(counts) + 1 + (round & 1), (unsigned long long)__popcll(m));
}

// ptr (>= 0: the node pointed at, or live before round 0; -1: nothing left) and
// the matched byte of every node, then the priority word of every incidence entry
struct GraclusWs : Carver {
  int64_t n, n_entries;
  int32_t* ptr = take<int32_t>(n);
  uint8_t* done = take<uint8_t>(n);
  uint64_t* key = take<uint64_t>(n_entries);
};

// the entry points return -(code); see the header
#define GRACLUS_CHECK_ARG(cond, ...)   \
  do {                                 \
    if (!(cond)) {                     \
      ::mp::set_error(__VA_ARGS__);    \
      return -(int64_t)MP_ERR_ARG;     \
    }                                  \
  } while (0)

#define GRACLUS_CHECK_EXTENT(fn, name, have, need)                                                  \
  GRACLUS_CHECK_ARG((size_t)(have) >= (size_t)(need), "%s: %s holds %zu bytes, the call needs %zu", \
                    fn, name, (size_t)(have), (size_t)(need))

#define GRACLUS_CHECK_HIP(expr)                                              \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      ::mp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                      __FILE__, __LINE__);                                   \
      return -(int64_t)MP_ERR_HIP;                                           \
    }                                                                        \
  } while (0)

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_graclus_workspace(int64_t n, int64_t n_edges) {
  return GraclusWs{nullptr, n, 2 * n_edges}.total(0);
}

int64_t mp_graclus_init(const int64_t* row, const int64_t* col, const float* weight, size_t weight_bytes,
                        int64_t n_edges, int64_t n, uint64_t seed, const int32_t* eid, size_t eid_bytes,
                        int64_t* cluster, size_t cluster_bytes, int64_t* counts, size_t counts_bytes, void* ws,
                        size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  GRACLUS_CHECK_ARG(n >= 0 && n < kGraclusMaxSize, "mp_graclus_init: n = %lld is negative or not below 2^30",
                    (long long)n);
  GRACLUS_CHECK_ARG(n_edges >= 0 && n_edges < kGraclusMaxSize,
                    "mp_graclus_init: n_edges = %lld is negative or not below 2^30", (long long)n_edges);
  GRACLUS_CHECK_ARG(counts, "mp_graclus_init: counts is NULL");
  GRACLUS_CHECK_ARG(ws, "mp_graclus_init: ws is NULL");
  GRACLUS_CHECK_ARG(n == 0 || cluster, "mp_graclus_init: cluster is NULL");
  GRACLUS_CHECK_ARG(n_edges == 0 || row, "mp_graclus_init: row is NULL");
  GRACLUS_CHECK_ARG(n_edges == 0 || col, "mp_graclus_init: col is NULL");
  GRACLUS_CHECK_ARG(n_edges == 0 || eid, "mp_graclus_init: eid is NULL");
  GRACLUS_CHECK_ARG(n_edges == 0 || n > 0, "mp_graclus_init: n_edges = %lld edges over no nodes", (long long)n_edges);
  if (weight) GRACLUS_CHECK_EXTENT("mp_graclus_init", "weight", weight_bytes, (size_t)n_edges * sizeof(float));
  GRACLUS_CHECK_EXTENT("mp_graclus_init", "eid", eid_bytes, (size_t)(2 * n_edges) * sizeof(int32_t));
  GRACLUS_CHECK_EXTENT("mp_graclus_init", "cluster", cluster_bytes, (size_t)n * sizeof(int64_t));
  GRACLUS_CHECK_EXTENT("mp_graclus_init", "counts", counts_bytes, 4 * sizeof(int64_t));
  const GraclusWs w{ws, n, 2 * n_edges};
  GRACLUS_CHECK_EXTENT("mp_graclus_init", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  int64_t launches = 0;
  GRACLUS_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s));
  if (n == 0) return launches;
  GRACLUS_CHECK_HIP(hipMemsetAsync(w.ptr, 0xFF, (size_t)n * sizeof(int32_t), s));  // -1: no entry but loops
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (n_edges > 0) {
    // mix64(seed) on the host: the same finaliser as the kernel's
    uint64_t z = seed + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    k_graclus_keys<<<(unsigned)ceil_div(2 * n_edges, kGraclusBlock), kGraclusBlock, 0, s>>>(
        row, col, eid, weight, n, n_edges, z, w.key, w.ptr, cnt);
    GRACLUS_CHECK_HIP(hipGetLastError());
    ++launches;
  }
  k_graclus_nodes<<<(unsigned)ceil_div(n, kGraclusBlock), kGraclusBlock, 0, s>>>(n, w.ptr, w.done, cluster, cnt);
  GRACLUS_CHECK_HIP(hipGetLastError());
  return launches + 1;
}

int64_t mp_graclus_rounds(const int32_t* rowptr, size_t rowptr_bytes, const int32_t* nbr, size_t nbr_bytes,
                          int64_t n_edges, int64_t n, int64_t first_round, int64_t n_rounds, int64_t* cluster,
                          size_t cluster_bytes, int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes,
                          void* stream) {
  MP_DEVICE_GUARD(stream);
  GRACLUS_CHECK_ARG(n >= 0 && n < kGraclusMaxSize, "mp_graclus_rounds: n = %lld is negative or not below 2^30",
                    (long long)n);
  GRACLUS_CHECK_ARG(n_edges >= 0 && n_edges < kGraclusMaxSize,
                    "mp_graclus_rounds: n_edges = %lld is negative or not below 2^30", (long long)n_edges);
  GRACLUS_CHECK_ARG(first_round >= 0, "mp_graclus_rounds: first_round = %lld is negative", (long long)first_round);
  GRACLUS_CHECK_ARG(n_rounds >= 0 && n_rounds <= kGraclusMaxRounds,
                    "mp_graclus_rounds: n_rounds = %lld is outside [0, %lld]", (long long)n_rounds,
                    (long long)kGraclusMaxRounds);
  GRACLUS_CHECK_ARG(counts, "mp_graclus_rounds: counts is NULL");
  GRACLUS_CHECK_ARG(ws, "mp_graclus_rounds: ws is NULL");
  GRACLUS_CHECK_ARG(n == 0 || rowptr, "mp_graclus_rounds: rowptr is NULL");
  GRACLUS_CHECK_ARG(n == 0 || cluster, "mp_graclus_rounds: cluster is NULL");
  GRACLUS_CHECK_ARG(n_edges == 0 || nbr, "mp_graclus_rounds: nbr is NULL");
  GRACLUS_CHECK_EXTENT("mp_graclus_rounds", "rowptr", rowptr_bytes, (size_t)(n + 1) * sizeof(int32_t));
  GRACLUS_CHECK_EXTENT("mp_graclus_rounds", "nbr", nbr_bytes, (size_t)(2 * n_edges) * sizeof(int32_t));
  GRACLUS_CHECK_EXTENT("mp_graclus_rounds", "cluster", cluster_bytes, (size_t)n * sizeof(int64_t));
  GRACLUS_CHECK_EXTENT("mp_graclus_rounds", "counts", counts_bytes, 4 * sizeof(int64_t));
  const GraclusWs w{ws, n, 2 * n_edges};
  GRACLUS_CHECK_EXTENT("mp_graclus_rounds", "ws", ws_bytes, w.total(0));
  if (n == 0 || n_edges == 0) return 0;
  hipStream_t s = as_stream(stream);
  const unsigned blocks = (unsigned)ceil_div(n, kGraclusBlock);
  for (int64_t r = first_round; r < first_round + n_rounds; ++r) {
    k_graclus_point<<<blocks, kGraclusBlock, 0, s>>>(rowptr, nbr, w.key, w.done, (int)n, 2 * n_edges, r, w.ptr,
                                                     counts);
    GRACLUS_CHECK_HIP(hipGetLastError());
    k_graclus_match<<<blocks, kGraclusBlock, 0, s>>>(w.ptr, (int)n, r, w.done, cluster, counts);
    GRACLUS_CHECK_HIP(hipGetLastError());
  }
  return n_rounds;
}

}  // extern "C"
