// Cluster pooling on the device (PyG 1.4.3 nn.pool voxel_grid / max_pool / avg_pool,
// torch_cluster 1.5 grid, torch_sparse 0.6.1 coalesce [U]; include/mi355_mp.h
// "Cluster pooling"): voxel keys, the consecutive relabelling of any int64 key
// vector, the per-cluster max / mean of x with the mean of pos and batch[perm],
// and pool_edge (relabel, drop loops, coalesce, sum the duplicates' attributes).
//
// One stable rocPRIM radix sort of (key, node index) gives the node side all it
// needs: equal keys are one run of the sorted order, a run's members ascend by
// node index (so the first-member tie rule of the max, the summation order of
// the mean and perm = the last member hold by construction), and an inclusive
// scan of the run heads numbers the clusters.  One stable sort of the relabelled
// edge keys inv[row] * M + inv[col] (loops and bad edges on a sentinel that
// sorts last) does the same for the edges: a run is one output edge, its
// members are the duplicates in ascending original position.
//
// Nothing here adds floats atomically; the one atomic is the integer count of
// edge ends outside the node range.  M and E' stay on the device: every kernel
// downstream of a sort is sized by its upper bound (n or E) and reads the count.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "mp_workspace.h"

namespace mp {

constexpr int kClusterBlock = 256;
// the row kernels (k_cluster_reduce, k_cluster_edge_attr) stride over their rows
// from at most this many workgroups: 8 per CU on 256 CUs is every wave slot of
// the chip (4 waves per workgroup, 8 per SIMD), and gridDim.x * blockDim.x
// stays far below 2^32 for any n < 2^31
constexpr int kClusterMaxBlocks = 2048;

static inline unsigned cluster_row_blocks(int64_t rows, int gl) {
  const int64_t waves = ceil_div(rows > 0 ? rows : 1, 64 / gl);
  const int64_t blocks = ceil_div(waves, kClusterBlock / 64);
  return (unsigned)(blocks < kClusterMaxBlocks ? blocks : kClusterMaxBlocks);
}

static inline unsigned cluster_flat_blocks(int64_t elems) {
  const int64_t blocks = ceil_div(elems > 0 ? elems : 1, kClusterBlock);
  return (unsigned)(blocks < kClusterMaxBlocks ? blocks : kClusterMaxBlocks);
}

__device__ __forceinline__ int64_t clamp_count(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- voxel keys --------------------------------------------------------------

// c_d = (int64) trunc(fl32(fl32(p_d - start_d) / size_d)), m_d the same of end_d,
// plus one; key = sum_d c_d * prod_{j<d} m_j in wrapping 64-bit arithmetic.  The
// unit is compiled with -ffp-contract=off and hipcc divides fp32 with correct
// rounding, so the quotient is the IEEE one torch computes on the CPU.
__global__ __launch_bounds__(kClusterBlock) void k_voxel_keys(const float* __restrict__ pos, int64_t ldp, int64_t n,
                                                              int D, const int64_t* __restrict__ batch,
                                                              const float* __restrict__ size,
                                                              const float* __restrict__ start,
                                                              const float* __restrict__ end,
                                                              int64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int Dt = D + (batch ? 1 : 0);
  uint64_t k = 0, mult = 1;
  for (int d = 0; d < Dt; ++d) {
    const float p = d < D ? pos[i * ldp + d] : (float)batch[i];
    const float s = start[d], z = size[d];
    const float q = (p - s) / z;
    const float qm = (end[d] - s) / z;
    const int64_t c = (int64_t)q;
    const int64_t m = (int64_t)qm + 1;
    k += (uint64_t)c * mult;
    mult *= (uint64_t)m;
  }
  key[i] = (int64_t)k;
}

// ---- consecutive clusters ------------------------------------------------------

struct RunHead {
  const int64_t* k;
  __host__ __device__ int operator()(int p) const { return (p == 0 || k[p] != k[p - 1]) ? 1 : 0; }
};

struct EdgeRunHead {
  const uint64_t* k;
  uint64_t sentinel;
  __host__ __device__ int operator()(int p) const {
    return (k[p] != sentinel && (p == 0 || k[p] != k[p - 1])) ? 1 : 0;
  }
};

using HeadIter = rocprim::transform_iterator<rocprim::counting_iterator<int>, RunHead, int>;
using EdgeHeadIter = rocprim::transform_iterator<rocprim::counting_iterator<int>, EdgeRunHead, int>;

__global__ __launch_bounds__(kClusterBlock) void k_cluster_emit(const int64_t* __restrict__ ks,
                                                                const int32_t* __restrict__ member,
                                                                const int32_t* __restrict__ cid, int64_t n,
                                                                int64_t* __restrict__ inv,
                                                                int32_t* __restrict__ rowptr,
                                                                int64_t* __restrict__ perm,
                                                                int64_t* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t c = (int64_t)cid[p] - 1;  // in [0, p]
  const int64_t node = member[p];         // the sort's own payload: in [0, n)
  const int64_t k = ks[p];
  if (c < 0 || c > p || node < 0 || node >= n) return;  // never for arrays this unit wrote
  inv[node] = c;
  if (p == 0 || ks[p - 1] != k) rowptr[c] = (int32_t)p;
  if (p == n - 1 || ks[p + 1] != k) perm[c] = node;  // the run's last member = its largest node index
  if (p == n - 1) {
    rowptr[c + 1] = (int32_t)n;
    counts[0] = c + 1;
  }
}

// temp bytes of mp_cluster_build's sort and of its scan
static hipError_t cluster_build_temp(int64_t n, size_t* sort_b, size_t* scan_b) {
  const size_t nn = (size_t)(n > 0 ? n : 1);
  HeadIter it(rocprim::counting_iterator<int>(0), RunHead{nullptr});
  const hipError_t e = rocprim::radix_sort_pairs((void*)nullptr, *sort_b, (const int64_t*)nullptr, (int64_t*)nullptr,
                                                 rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, nn, 0u,
                                                 64u, (hipStream_t)0, false);
  const hipError_t e2 = rocprim::inclusive_scan((void*)nullptr, *scan_b, it, (int32_t*)nullptr, nn,
                                                rocprim::plus<int>(), (hipStream_t)0, false);
  return e != hipSuccess ? e : e2;
}

// mp_cluster_build's workspace, then the temp the sort and the scan share (the larger of the two)
struct ClusterBuildWs : Carver {
  int64_t n;
  int64_t* ks = take<int64_t>(n);
  int32_t* cid = take<int32_t>(n);
};

// ---- per-cluster reduce ----------------------------------------------------------

// gl lanes (a power of two <= 64) own one cluster, 64 / gl clusters share a
// wave; a lane walks its cluster's members in ascending node order for each of
// its features f = sub, sub + gl, ...: rows are read coalesced across the group
__global__ __launch_bounds__(kClusterBlock) void k_cluster_reduce(
    const float* __restrict__ x, int64_t ldx, int F, int is_max, int mask, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ member, const int64_t* __restrict__ counts, int64_t n, float* __restrict__ x_out,
    int64_t ldo, int64_t* __restrict__ arg, const float* __restrict__ pos, int64_t ldp, int Dp,
    float* __restrict__ pos_out, int64_t ldpo, const int64_t* __restrict__ batch, const int64_t* __restrict__ perm,
    int64_t* __restrict__ batch_out, int gl) {
  const int64_t M = clamp_count(counts[0], n);
  const int lane = lane_id();
  const int cpw = 64 / gl;
  const int sub = lane & (gl - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (kClusterBlock / 64);
  for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w * cpw < M; w += n_waves) {
    const int64_t c = w * cpw + lane / gl;
    if (c >= M) continue;
    int64_t p0 = rowptr[c], p1 = rowptr[c + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > n) p1 = n;
    const float cnt = (float)(p1 - p0 > 1 ? p1 - p0 : 1);
    for (int f = sub; f < F; f += gl) {
      if (is_max) {
        float best = -3.402823466e+38f;  // lowest(): torch_scatter's start value
        int64_t a = n;
        for (int64_t p = p0; p < p1; ++p) {
          const int64_t node = member[p];
          if (node < 0 || node >= n) continue;
          const float v = x[node * ldx + f];
          if (v > best) {  // strict: the first (lowest-index) member keeps a tie
            best = v;
            a = node;
          }
        }
        if (a == n) best = 0.f;
        if (mask && best < -10000.f) best = 0.f;
        x_out[c * ldo + f] = best;
        if (arg) arg[c * (int64_t)F + f] = a;
      } else {
        float acc = 0.f;
        for (int64_t p = p0; p < p1; ++p) {
          const int64_t node = member[p];
          if (node < 0 || node >= n) continue;
          acc += x[node * ldx + f];
        }
        x_out[c * ldo + f] = acc / cnt;
      }
    }
    for (int d = sub; d < Dp; d += gl) {
      float acc = 0.f;
      for (int64_t p = p0; p < p1; ++p) {
        const int64_t node = member[p];
        if (node < 0 || node >= n) continue;
        acc += pos[node * ldp + d];
      }
      pos_out[c * ldpo + d] = acc / cnt;
    }
    if (batch_out && sub == 0) {
      const int64_t node = perm[c];
      batch_out[c] = (node >= 0 && node < n) ? batch[node] : 0;
    }
  }
}

// ---- pool_edge -----------------------------------------------------------------

__global__ __launch_bounds__(kClusterBlock) void k_cluster_edge_keys(const int64_t* __restrict__ row,
                                                                     const int64_t* __restrict__ col, int64_t n_edges,
                                                                     const int64_t* __restrict__ inv, int64_t n_nodes,
                                                                     uint64_t sentinel,
                                                                     uint64_t* __restrict__ keys,
                                                                     unsigned long long* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e < n_edges;
  const int64_t M = clamp_count((int64_t)counts[0], n_nodes);
  const int64_t r = in ? row[e] : 0, c = in ? col[e] : 0;
  const bool rbad = in && (r < 0 || r >= n_nodes), cbad = in && (c < 0 || c >= n_nodes);
  const unsigned long long bad = __ballot(rbad), bad2 = __ballot(cbad);
  if (lane_id() == 0 && (bad | bad2)) atomicAdd(counts + 2, (unsigned long long)(__popcll(bad) + __popcll(bad2)));
  if (!in) return;
  uint64_t k = sentinel;
  if (!rbad && !cbad) {
    const int64_t a = inv[r], b = inv[c];
    if (a >= 0 && a < M && b >= 0 && b < M && a != b) k = (uint64_t)a * (uint64_t)M + (uint64_t)b;
  }
  keys[e] = k;
}

__global__ __launch_bounds__(kClusterBlock) void k_cluster_edge_emit(
    const uint64_t* __restrict__ ks, const int32_t* __restrict__ seg_edge, const int32_t* __restrict__ slot1,
    int64_t n_edges, int64_t n_nodes, uint64_t sentinel, int64_t* __restrict__ out_row, int64_t* __restrict__ out_col,
    int64_t* __restrict__ edge_slot, int32_t* __restrict__ seg_ptr, int64_t* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_edges) return;
  const uint64_t k = ks[p];
  const int64_t e = seg_edge[p];  // the sort's own payload: in [0, n_edges)
  if (e < 0 || e >= n_edges) return;
  if (k == sentinel) {
    edge_slot[e] = -1;
    if (p == 0) seg_ptr[0] = 0;  // no edge survives; counts[1] keeps its 0
    return;
  }
  const int64_t s = (int64_t)slot1[p] - 1;
  if (s < 0 || s > p) return;  // never for arrays this unit wrote
  edge_slot[e] = s;
  if (p == 0 || ks[p - 1] != k) {
    int64_t M = clamp_count(counts[0], n_nodes);
    if (M < 1) M = 1;
    out_row[s] = (int64_t)(k / (uint64_t)M);
    out_col[s] = (int64_t)(k % (uint64_t)M);
    seg_ptr[s] = (int32_t)p;
  }
  if (p == n_edges - 1 || ks[p + 1] == sentinel) {
    seg_ptr[s + 1] = (int32_t)(p + 1);
    counts[1] = s + 1;
  }
}

static int cluster_key_log2(int64_t n) {
  int L = 0;
  while (((int64_t)1 << L) < n) ++L;
  return L;  // <= 31 for n < 2^31
}

// temp bytes of mp_cluster_edges' sort and of its scan
static hipError_t cluster_edges_temp(int64_t E, unsigned bits, size_t* sort_b, size_t* scan_b) {
  const size_t ee = (size_t)(E > 0 ? E : 1);
  EdgeHeadIter it(rocprim::counting_iterator<int>(0), EdgeRunHead{nullptr, 0});
  const hipError_t e = rocprim::radix_sort_pairs((void*)nullptr, *sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                 rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, ee, 0u,
                                                 bits, (hipStream_t)0, false);
  const hipError_t e2 = rocprim::inclusive_scan((void*)nullptr, *scan_b, it, (int32_t*)nullptr, ee,
                                                rocprim::plus<int>(), (hipStream_t)0, false);
  return e != hipSuccess ? e : e2;
}

// mp_cluster_edges' workspace (slot1: output slot + 1), then the temp the sort and the scan share
struct ClusterEdgesWs : Carver {
  int64_t n_edges;
  uint64_t* keys = take<uint64_t>(n_edges);
  uint64_t* ks = take<uint64_t>(n_edges);
  int32_t* slot1 = take<int32_t>(n_edges);
};

// attr_out[k, :] = ((0 + attr[e_0, :]) + attr[e_1, :]) + ... over the duplicates
// of output edge k in ascending original position
__global__ __launch_bounds__(kClusterBlock) void k_cluster_edge_attr(const float* __restrict__ attr, int64_t lda,
                                                                     int A, const int32_t* __restrict__ seg_ptr,
                                                                     const int32_t* __restrict__ seg_edge,
                                                                     const int64_t* __restrict__ counts,
                                                                     int64_t n_edges, float* __restrict__ out,
                                                                     int64_t ldo, int gl) {
  const int64_t K = clamp_count(counts[1], n_edges);
  const int lane = lane_id();
  const int cpw = 64 / gl;
  const int sub = lane & (gl - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (kClusterBlock / 64);
  for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w * cpw < K; w += n_waves) {
    const int64_t k = w * cpw + lane / gl;
    if (k >= K) continue;
    int64_t p0 = seg_ptr[k], p1 = seg_ptr[k + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > n_edges) p1 = n_edges;
    for (int a = sub; a < A; a += gl) {
      float acc = 0.f;
      for (int64_t p = p0; p < p1; ++p) {
        const int64_t e = seg_edge[p];
        if (e < 0 || e >= n_edges) continue;
        acc += attr[e * lda + a];
      }
      out[k * ldo + a] = acc;
    }
  }
}

// g_attr[e, :] = g[edge_slot[e], :], zeros for a dropped edge
__global__ __launch_bounds__(kClusterBlock) void k_cluster_edge_attr_bwd(const float* __restrict__ g, int64_t ldg,
                                                                         const int64_t* __restrict__ edge_slot,
                                                                         int64_t n_edges, int A, int64_t n_out,
                                                                         float* __restrict__ g_attr, int64_t ldga) {
  const int64_t total = n_edges * A;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const int64_t e = i / A;
    const int a = (int)(i - e * A);
    const int64_t s = edge_slot[e];
    g_attr[e * ldga + a] = (s >= 0 && s < n_out) ? g[s * ldg + a] : 0.f;
  }
}

}  // namespace mp

using namespace mp;

extern "C" {

int32_t mp_cluster_max_blocks(void) { return kClusterMaxBlocks; }

int mp_voxel_keys_f32(const float* pos, int64_t ldp, int64_t n, int32_t D, const int64_t* batch, const float* size,
                      const float* start, const float* end, int64_t* key, size_t key_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_voxel_keys_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(D >= 0 && D <= 8, "mp_voxel_keys_f32: D = %d is outside [0, 8]", D);
  MP_CHECK_ARG(D >= 1 || batch, "mp_voxel_keys_f32: D = 0 and batch is NULL");
  MP_CHECK_ARG(ldp >= D, "mp_voxel_keys_f32: ldp = %lld < D = %d", (long long)ldp, D);
  MP_CHECK_ARG(size, "mp_voxel_keys_f32: size is NULL");
  MP_CHECK_ARG(start, "mp_voxel_keys_f32: start is NULL");
  MP_CHECK_ARG(end, "mp_voxel_keys_f32: end is NULL");
  MP_CHECK_ARG(n == 0 || D == 0 || pos, "mp_voxel_keys_f32: pos is NULL");
  MP_CHECK_ARG(n == 0 || key, "mp_voxel_keys_f32: key is NULL");
  MP_CHECK_EXTENT("mp_voxel_keys_f32", "key", key_bytes, (size_t)n * sizeof(int64_t));
  if (n == 0) return MP_OK;
  k_voxel_keys<<<(unsigned)ceil_div(n, kClusterBlock), kClusterBlock, 0, as_stream(stream)>>>(pos, ldp, n, D, batch,
                                                                                              size, start, end, key);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

size_t mp_cluster_build_workspace(int64_t n) {
  size_t a = 0, b = 0;
  (void)cluster_build_temp(n, &a, &b);
  return ClusterBuildWs{nullptr, n}.total(a > b ? a : b);
}

int mp_cluster_build(const int64_t* key, int64_t n, int64_t* inv, size_t inv_bytes, int32_t* rowptr,
                     size_t rowptr_bytes, int32_t* member, size_t member_bytes, int64_t* perm, size_t perm_bytes,
                     int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_cluster_build: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(counts, "mp_cluster_build: counts is NULL");
  MP_CHECK_ARG(rowptr, "mp_cluster_build: rowptr is NULL");
  MP_CHECK_ARG(n == 0 || key, "mp_cluster_build: key is NULL");
  MP_CHECK_ARG(n == 0 || inv, "mp_cluster_build: inv is NULL");
  MP_CHECK_ARG(n == 0 || member, "mp_cluster_build: member is NULL");
  MP_CHECK_ARG(n == 0 || perm, "mp_cluster_build: perm is NULL");
  MP_CHECK_ARG(ws, "mp_cluster_build: ws is NULL");
  MP_CHECK_EXTENT("mp_cluster_build", "inv", inv_bytes, (size_t)n * sizeof(int64_t));
  MP_CHECK_EXTENT("mp_cluster_build", "rowptr", rowptr_bytes, (size_t)(n + 1) * sizeof(int32_t));
  MP_CHECK_EXTENT("mp_cluster_build", "member", member_bytes, (size_t)n * sizeof(int32_t));
  MP_CHECK_EXTENT("mp_cluster_build", "perm", perm_bytes, (size_t)n * sizeof(int64_t));
  const ClusterBuildWs w{ws, n};
  MP_CHECK_EXTENT("mp_cluster_build", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    MP_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t), s));
    MP_CHECK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t), s));
    return MP_OK;
  }
  size_t sort_b = 0, scan_b = 0;
  const hipError_t size_query = cluster_build_temp(n, &sort_b, &scan_b);
  MP_CHECK_EXTENT("mp_cluster_build", "ws", ws_bytes, w.total(std::max(sort_b, scan_b)));
  MP_CHECK_HIP(size_query);
  MP_CHECK_HIP(rocprim::radix_sort_pairs(w.rest(), sort_b, key, w.ks, rocprim::counting_iterator<int32_t>(0), member,
                                         (size_t)n, 0u, 64u, s, false));
  HeadIter heads(rocprim::counting_iterator<int>(0), RunHead{w.ks});
  MP_CHECK_HIP(rocprim::inclusive_scan(w.rest(), scan_b, heads, w.cid, (size_t)n, rocprim::plus<int>(), s, false));
  k_cluster_emit<<<(unsigned)ceil_div(n, kClusterBlock), kClusterBlock, 0, s>>>(w.ks, member, w.cid, n, inv, rowptr,
                                                                                perm, counts);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_cluster_reduce_f32(const float* x, int64_t ldx, int32_t F, int32_t reduce, int32_t flags,
                          const int32_t* rowptr, const int32_t* member, const int64_t* counts, int64_t n,
                          float* x_out, int64_t ldo, size_t x_out_bytes, int64_t* arg, size_t arg_bytes,
                          const float* pos, int64_t ldp, int32_t Dp, float* pos_out, size_t pos_out_bytes,
                          const int64_t* batch, const int64_t* perm, int64_t* batch_out, size_t batch_out_bytes,
                          void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_cluster_reduce_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(F >= 0, "mp_cluster_reduce_f32: F = %d", F);
  MP_CHECK_ARG(Dp >= 0, "mp_cluster_reduce_f32: Dp = %d", Dp);
  MP_CHECK_ARG(reduce == MP_REDUCE_MAX || reduce == MP_REDUCE_MEAN,
               "mp_cluster_reduce_f32: reduce = %d is neither MP_REDUCE_MAX nor MP_REDUCE_MEAN", reduce);
  MP_CHECK_ARG((flags & ~MP_FLAG_PYG_MASK) == 0, "mp_cluster_reduce_f32: unknown flags %d", flags);
  MP_CHECK_ARG(F == 0 || ldx >= F, "mp_cluster_reduce_f32: ldx = %lld < F = %d", (long long)ldx, F);
  MP_CHECK_ARG(F == 0 || ldo >= F, "mp_cluster_reduce_f32: ldo = %lld < F = %d", (long long)ldo, F);
  MP_CHECK_ARG(Dp == 0 || ldp >= Dp, "mp_cluster_reduce_f32: ldp = %lld < Dp = %d", (long long)ldp, Dp);
  MP_CHECK_ARG(counts, "mp_cluster_reduce_f32: counts is NULL");
  if (n == 0) return MP_OK;
  MP_CHECK_ARG(rowptr, "mp_cluster_reduce_f32: rowptr is NULL");
  MP_CHECK_ARG(member, "mp_cluster_reduce_f32: member is NULL");
  MP_CHECK_ARG(F == 0 || x, "mp_cluster_reduce_f32: x is NULL");
  MP_CHECK_ARG(F == 0 || x_out, "mp_cluster_reduce_f32: x_out is NULL");
  MP_CHECK_ARG(Dp == 0 || pos, "mp_cluster_reduce_f32: pos is NULL");
  MP_CHECK_ARG(Dp == 0 || pos_out, "mp_cluster_reduce_f32: pos_out is NULL");
  MP_CHECK_ARG(!batch_out || (batch && perm), "mp_cluster_reduce_f32: batch_out needs batch and perm");
  if (F > 0)
    MP_CHECK_EXTENT("mp_cluster_reduce_f32", "x_out", x_out_bytes,
                    ((size_t)(n - 1) * (size_t)ldo + (size_t)F) * sizeof(float));
  if (arg) MP_CHECK_EXTENT("mp_cluster_reduce_f32", "arg", arg_bytes, (size_t)n * (size_t)F * sizeof(int64_t));
  if (Dp > 0) MP_CHECK_EXTENT("mp_cluster_reduce_f32", "pos_out", pos_out_bytes, (size_t)n * (size_t)Dp * sizeof(float));
  if (batch_out) MP_CHECK_EXTENT("mp_cluster_reduce_f32", "batch_out", batch_out_bytes, (size_t)n * sizeof(int64_t));
  const int gl = group_lanes(F > Dp ? F : Dp);
  k_cluster_reduce<<<cluster_row_blocks(n, gl), kClusterBlock, 0, as_stream(stream)>>>(
      x, ldx, F, reduce == MP_REDUCE_MAX, (flags & MP_FLAG_PYG_MASK) ? 1 : 0, rowptr, member, counts, n, x_out, ldo,
      reduce == MP_REDUCE_MAX ? arg : nullptr, pos, ldp, Dp, pos_out, Dp, batch, perm, batch_out, gl);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

size_t mp_cluster_edges_workspace(int64_t n_edges, int64_t n_nodes) {
  size_t a = 0, b = 0;
  const unsigned bits = 2u * (unsigned)cluster_key_log2(n_nodes > 0 ? n_nodes : 1) + 1u;
  (void)cluster_edges_temp(n_edges, bits, &a, &b);
  return ClusterEdgesWs{nullptr, n_edges}.total(a > b ? a : b);
}

int mp_cluster_edges(const int64_t* row, const int64_t* col, int64_t n_edges, const int64_t* inv, int64_t n_nodes,
                     int64_t* counts, int64_t* out_row, int64_t* out_col, int64_t* edge_slot, size_t out_bytes,
                     int32_t* seg_ptr, size_t seg_ptr_bytes, int32_t* seg_edge, size_t seg_edge_bytes, void* ws,
                     size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_edges >= 0 && n_edges < (int64_t)INT32_MAX,
               "mp_cluster_edges: n_edges = %lld is negative or not below 2^31", (long long)n_edges);
  MP_CHECK_ARG(n_nodes >= 0 && n_nodes < (int64_t)INT32_MAX,
               "mp_cluster_edges: n_nodes = %lld is negative or not below 2^31", (long long)n_nodes);
  MP_CHECK_ARG(counts, "mp_cluster_edges: counts is NULL");
  MP_CHECK_ARG(seg_ptr, "mp_cluster_edges: seg_ptr is NULL");
  MP_CHECK_ARG(n_edges == 0 || row, "mp_cluster_edges: row is NULL");
  MP_CHECK_ARG(n_edges == 0 || col, "mp_cluster_edges: col is NULL");
  MP_CHECK_ARG(n_edges == 0 || n_nodes == 0 || inv, "mp_cluster_edges: inv is NULL");
  MP_CHECK_ARG(n_edges == 0 || out_row, "mp_cluster_edges: out_row is NULL");
  MP_CHECK_ARG(n_edges == 0 || out_col, "mp_cluster_edges: out_col is NULL");
  MP_CHECK_ARG(n_edges == 0 || edge_slot, "mp_cluster_edges: edge_slot is NULL");
  MP_CHECK_ARG(n_edges == 0 || seg_edge, "mp_cluster_edges: seg_edge is NULL");
  MP_CHECK_ARG(ws, "mp_cluster_edges: ws is NULL");
  MP_CHECK_EXTENT("mp_cluster_edges", "out_row / out_col / edge_slot", out_bytes, (size_t)n_edges * sizeof(int64_t));
  MP_CHECK_EXTENT("mp_cluster_edges", "seg_ptr", seg_ptr_bytes, (size_t)(n_edges + 1) * sizeof(int32_t));
  MP_CHECK_EXTENT("mp_cluster_edges", "seg_edge", seg_edge_bytes, (size_t)n_edges * sizeof(int32_t));
  const ClusterEdgesWs w{ws, n_edges};
  MP_CHECK_EXTENT("mp_cluster_edges", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  if (n_edges == 0) {
    MP_CHECK_HIP(hipMemsetAsync(counts + 1, 0, 2 * sizeof(int64_t), s));
    MP_CHECK_HIP(hipMemsetAsync(seg_ptr, 0, sizeof(int32_t), s));
    return MP_OK;
  }
  const int L = cluster_key_log2(n_nodes > 0 ? n_nodes : 1);
  const uint64_t sentinel = (uint64_t)1 << (2 * L);  // above every a * M + b < n^2 <= 2^(2L)
  const unsigned bits = 2u * (unsigned)L + 1u;
  size_t sort_b = 0, scan_b = 0;
  const hipError_t size_query = cluster_edges_temp(n_edges, bits, &sort_b, &scan_b);
  MP_CHECK_EXTENT("mp_cluster_edges", "ws", ws_bytes, w.total(std::max(sort_b, scan_b)));
  MP_CHECK_HIP(size_query);
  MP_CHECK_HIP(hipMemsetAsync(counts + 1, 0, 2 * sizeof(int64_t), s));
  const unsigned blocks = (unsigned)ceil_div(n_edges, kClusterBlock);
  k_cluster_edge_keys<<<blocks, kClusterBlock, 0, s>>>(row, col, n_edges, inv, n_nodes, sentinel, w.keys,
                                                       reinterpret_cast<unsigned long long*>(counts));
  MP_CHECK_LAUNCH();
  MP_CHECK_HIP(rocprim::radix_sort_pairs(w.rest(), sort_b, (const uint64_t*)w.keys, w.ks,
                                         rocprim::counting_iterator<int32_t>(0), seg_edge, (size_t)n_edges, 0u, bits,
                                         s, false));
  EdgeHeadIter heads(rocprim::counting_iterator<int>(0), EdgeRunHead{w.ks, sentinel});
  MP_CHECK_HIP(rocprim::inclusive_scan(w.rest(), scan_b, heads, w.slot1, (size_t)n_edges, rocprim::plus<int>(), s,
                                       false));
  k_cluster_edge_emit<<<blocks, kClusterBlock, 0, s>>>(w.ks, seg_edge, w.slot1, n_edges, n_nodes, sentinel, out_row,
                                                       out_col, edge_slot, seg_ptr, counts);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_cluster_edge_attr_f32(const float* attr, int64_t lda, int32_t A, const int32_t* seg_ptr,
                             const int32_t* seg_edge, const int64_t* counts, int64_t n_edges, float* out, int64_t ldo,
                             size_t out_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_edges >= 0 && n_edges < (int64_t)INT32_MAX,
               "mp_cluster_edge_attr_f32: n_edges = %lld is negative or not below 2^31", (long long)n_edges);
  MP_CHECK_ARG(A >= 1, "mp_cluster_edge_attr_f32: A = %d", A);
  MP_CHECK_ARG(lda >= A, "mp_cluster_edge_attr_f32: lda = %lld < A = %d", (long long)lda, A);
  MP_CHECK_ARG(ldo >= A, "mp_cluster_edge_attr_f32: ldo = %lld < A = %d", (long long)ldo, A);
  MP_CHECK_ARG(counts, "mp_cluster_edge_attr_f32: counts is NULL");
  if (n_edges == 0) return MP_OK;
  MP_CHECK_ARG(attr, "mp_cluster_edge_attr_f32: attr is NULL");
  MP_CHECK_ARG(seg_ptr, "mp_cluster_edge_attr_f32: seg_ptr is NULL");
  MP_CHECK_ARG(seg_edge, "mp_cluster_edge_attr_f32: seg_edge is NULL");
  MP_CHECK_ARG(out, "mp_cluster_edge_attr_f32: out is NULL");
  MP_CHECK_EXTENT("mp_cluster_edge_attr_f32", "out", out_bytes,
                  ((size_t)(n_edges - 1) * (size_t)ldo + (size_t)A) * sizeof(float));
  const int gl = group_lanes(A);
  k_cluster_edge_attr<<<cluster_row_blocks(n_edges, gl), kClusterBlock, 0, as_stream(stream)>>>(
      attr, lda, A, seg_ptr, seg_edge, counts, n_edges, out, ldo, gl);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_cluster_edge_attr_bwd_f32(const float* g, int64_t ldg, const int64_t* edge_slot, int64_t n_edges, int32_t A,
                                 int64_t n_out, float* g_attr, int64_t ldga, size_t g_attr_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_edges >= 0 && n_edges < (int64_t)INT32_MAX,
               "mp_cluster_edge_attr_bwd_f32: n_edges = %lld is negative or not below 2^31", (long long)n_edges);
  MP_CHECK_ARG(A >= 1, "mp_cluster_edge_attr_bwd_f32: A = %d", A);
  MP_CHECK_ARG(n_out >= 0 && n_out <= n_edges, "mp_cluster_edge_attr_bwd_f32: n_out = %lld is outside [0, n_edges]",
               (long long)n_out);
  MP_CHECK_ARG(ldg >= A, "mp_cluster_edge_attr_bwd_f32: ldg = %lld < A = %d", (long long)ldg, A);
  MP_CHECK_ARG(ldga >= A, "mp_cluster_edge_attr_bwd_f32: ldga = %lld < A = %d", (long long)ldga, A);
  if (n_edges == 0) return MP_OK;
  MP_CHECK_ARG(n_out == 0 || g, "mp_cluster_edge_attr_bwd_f32: g is NULL");
  MP_CHECK_ARG(edge_slot, "mp_cluster_edge_attr_bwd_f32: edge_slot is NULL");
  MP_CHECK_ARG(g_attr, "mp_cluster_edge_attr_bwd_f32: g_attr is NULL");
  MP_CHECK_EXTENT("mp_cluster_edge_attr_bwd_f32", "g_attr", g_attr_bytes,
                  ((size_t)(n_edges - 1) * (size_t)ldga + (size_t)A) * sizeof(float));
  k_cluster_edge_attr_bwd<<<cluster_flat_blocks(n_edges * A), kClusterBlock, 0, as_stream(stream)>>>(
      g, ldg, edge_slot, n_edges, A, n_out, g_attr, ldga);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // extern "C"
