// Shard-plan build on the device (SURVEY 8e / 8f-2 "halo maps"): for rank p
// owning the key rows [lo, hi) of a destination-range partition,
//   edge_pos     = positions of the edges whose key lies in [lo, hi), in the
//                  global edge order (rocPRIM stable select),
//   halo_nodes   = the sorted unique remote `other` endpoints of those edges,
//   local ids    = key - lo, and other - lo (owned) or n_own + halo index,
//   recv_counts  = halo nodes per owner rank (halo_nodes are sorted, so they
//                  are grouped by owner).
// No sort: remote endpoints are flagged in an [N] array and an exclusive scan
// of the flags is both the halo index of every node and, read at the cut
// points, the per-owner counts -- O(E + N), deterministic.
// Replaces the torch-op plan of mi355_mp.dist.ShardPlan (nonzero / unique /
// searchsorted) for device edge lists.
#include <rocprim/device/device_scan.hpp>

#include "mp_workspace.h"

namespace mp {

__global__ void k_plan_flags(const int64_t* __restrict__ key, const int64_t* __restrict__ other, int64_t n,
                             int64_t n_nodes, int64_t lo, int64_t hi, uint8_t* __restrict__ keep,
                             int32_t* __restrict__ flag, int32_t* __restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t k = key[e];
  const bool mine = k >= lo && k < hi;
  keep[e] = mine ? 1 : 0;
  if (mine) {
    const int64_t o = other[e];
    if (o < 0 || o >= n_nodes) {
      *bad = 1;  // reported through counts[1] = -1
    } else if (o < lo || o >= hi) {
      flag[o] = 1;  // every writer stores the same value
    }
  }
}

__global__ void k_plan_halo(const int32_t* __restrict__ flag, const int32_t* __restrict__ hidx, int64_t n_nodes,
                            int64_t* __restrict__ halo_nodes) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_nodes && flag[v]) halo_nodes[hidx[v]] = v;
}

// local ids of the selected edges; n_sel is read on the device (the grid
// covers the upper bound n_edges)
__global__ void k_plan_local(const int64_t* __restrict__ key, const int64_t* __restrict__ other,
                             const int64_t* __restrict__ edge_pos, const unsigned long long* __restrict__ n_sel,
                             int64_t n_nodes, int64_t lo, int64_t hi, const int32_t* __restrict__ hidx,
                             int64_t* __restrict__ local_key, int64_t* __restrict__ local_other) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)*n_sel) return;
  const int64_t p = edge_pos[k];
  const int64_t o = other[p];
  local_key[k] = key[p] - lo;
  local_other[k] = (o >= lo && o < hi) ? o - lo : (o >= 0 && o < n_nodes) ? (hi - lo) + (int64_t)hidx[o] : -1;
}

// counts[0] = selected edges, counts[1] = halo nodes (-1: an `other` index of
// a selected edge lies outside [0, n_nodes)), counts[2 + q] = halo nodes owned
// by rank q (cuts[q] <= v < cuts[q + 1])
__global__ void k_plan_counts(const int32_t* __restrict__ flag, const int32_t* __restrict__ hidx, int64_t n_nodes,
                              const int64_t* __restrict__ cuts, int32_t world,
                              const unsigned long long* __restrict__ n_sel, const int32_t* __restrict__ bad,
                              int64_t* __restrict__ counts) {
  const int q = (int)threadIdx.x;
  const int64_t total = n_nodes > 0 ? (int64_t)hidx[n_nodes - 1] + flag[n_nodes - 1] : 0;
  auto before = [&](int64_t c) -> int64_t { return c >= n_nodes ? total : (c <= 0 ? 0 : (int64_t)hidx[c]); };
  if (q == 0) {
    counts[0] = (int64_t)*n_sel;
    counts[1] = *bad ? -1 : total;
  }
  if (q < world) counts[2 + q] = before(cuts[q + 1]) - before(cuts[q]);
}

static hipError_t plan_scan_bytes(int64_t n, size_t* bytes) {
  return rocprim::exclusive_scan((void*)nullptr, *bytes, (const int32_t*)nullptr, (int32_t*)nullptr, 0,
                                 (size_t)(n > 0 ? n : 1), rocprim::plus<int32_t>(), (hipStream_t)0, false);
}

// mp_shard_plan's workspace, then the temp the select and the scan share (the larger of the two)
struct ShardPlanWs : Carver {
  int64_t n_edges, n_nodes;
  uint8_t* keep = take<uint8_t>(n_edges);
  int32_t* flag = take<int32_t>(n_nodes);
  int32_t* hidx = take<int32_t>(n_nodes);
  unsigned long long* n_sel = take<unsigned long long>(1);
  int32_t* bad = take<int32_t>(1);
};

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_shard_plan_workspace(int64_t n_edges, int64_t n_nodes) {
  size_t sel_bytes = 0, scan_bytes = 0;
  (void)select_positions_bytes(n_edges, &sel_bytes);
  (void)plan_scan_bytes(n_nodes, &scan_bytes);
  return ShardPlanWs{nullptr, n_edges, n_nodes}.total(std::max(sel_bytes, scan_bytes));
}

int mp_shard_plan(const int64_t* key, const int64_t* other, int64_t n_edges, int64_t n_nodes, const int64_t* cuts,
                  int32_t world, int32_t rank, int64_t lo, int64_t hi, int64_t* edge_pos, int64_t* local_key,
                  int64_t* local_other, int64_t* halo_nodes, int64_t* counts, void* ws, size_t ws_bytes,
                  void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && n_nodes < (int64_t)INT32_MAX, "mp_shard_plan: bad sizes");
  MP_CHECK_ARG(world >= 1 && world <= 1024 && rank >= 0 && rank < world, "mp_shard_plan: bad rank / world");
  MP_CHECK_ARG(0 <= lo && lo <= hi && hi <= n_nodes, "mp_shard_plan: [lo, hi) outside [0, n_nodes)");
  MP_CHECK_ARG(cuts && counts, "mp_shard_plan: null cuts / counts");
  MP_CHECK_ARG(n_edges == 0 || (key && other && edge_pos && local_key && local_other),
               "mp_shard_plan: null edge array");
  MP_CHECK_ARG(n_nodes == 0 || halo_nodes, "mp_shard_plan: null halo_nodes");
  const ShardPlanWs w{ws, n_edges, n_nodes};
  size_t sel_bytes = 0, scan_bytes = 0;
  const hipError_t sel_query = select_positions_bytes(n_edges, &sel_bytes);
  const hipError_t scan_query = plan_scan_bytes(n_nodes, &scan_bytes);
  MP_CHECK_ARG(ws && ws_bytes >= w.total(std::max(sel_bytes, scan_bytes)), "mp_shard_plan: workspace too small");
  MP_CHECK_HIP(sel_query);
  MP_CHECK_HIP(scan_query);
  hipStream_t s = as_stream(stream);
  const int B = 256;
  MP_CHECK_HIP(hipMemsetAsync(w.n_sel, 0, 8, s));
  MP_CHECK_HIP(hipMemsetAsync(w.bad, 0, 4, s));
  if (n_nodes > 0) MP_CHECK_HIP(hipMemsetAsync(w.flag, 0, (size_t)n_nodes * 4, s));
  if (n_edges > 0) {
    k_plan_flags<<<ceil_div(n_edges, B), B, 0, s>>>(key, other, n_edges, n_nodes, lo, hi, w.keep, w.flag, w.bad);
    MP_CHECK_LAUNCH();
    rocprim::counting_iterator<int64_t> it(0);
    MP_CHECK_HIP(rocprim::select(w.rest(), sel_bytes, it, w.keep, edge_pos, w.n_sel, (size_t)n_edges, s, false));
  }
  if (n_nodes > 0) {
    MP_CHECK_HIP(rocprim::exclusive_scan(w.rest(), scan_bytes, w.flag, w.hidx, 0, (size_t)n_nodes,
                                         rocprim::plus<int32_t>(), s, false));
    k_plan_halo<<<ceil_div(n_nodes, B), B, 0, s>>>(w.flag, w.hidx, n_nodes, halo_nodes);
    MP_CHECK_LAUNCH();
  }
  if (n_edges > 0) {
    k_plan_local<<<ceil_div(n_edges, B), B, 0, s>>>(key, other, edge_pos, w.n_sel, n_nodes, lo, hi, w.hidx,
                                                    local_key, local_other);
    MP_CHECK_LAUNCH();
  }
  k_plan_counts<<<1, 1024, 0, s>>>(w.flag, w.hidx, n_nodes, cuts, world, w.n_sel, w.bad, counts);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // extern "C"
