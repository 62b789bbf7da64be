// TopKPooling on the device (PyG 1.4.3 nn.pool.topk_pool [U]; include/mi355_mp.h
// "TopKPooling"): node score, per-graph top-k select, gather + gate, the
// ordered compaction behind filter_adj and the min_score path, and the two
// backward passes.
//
// Select ranks a graph's nodes by counting, rank(i) = #{j : key_j > key_i or
// (key_j == key_i and j < i)}, from keys held on chip: a wave's registers for
// graphs of up to 64 nodes (the reference's ENZYMES batches average 33), LDS
// for graphs of up to MP_TUNE_TOPK_WG_LIMIT nodes.  Every node gets a distinct
// rank, the tie rule (lower index first) holds by construction and nothing is
// sorted.  Larger graphs sort the 64-bit composite (key << 32 | ~local index)
// with rocPRIM: the composites are distinct, so the order does not depend on
// the sort being stable.  Keys are the usual order-preserving map of the fp32
// bits to uint32 with -0 folded onto +0 and every NaN onto the top key.
//
// Nothing here adds floats atomically: the only atomics are the two integer
// counters and the integer maximum documented in the header.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "mp_workspace.h"

namespace mp {

constexpr int kPoolBlock = 256;
constexpr int kScoreBwdMaxParts = 512;

static inline unsigned pool_row_blocks(int64_t rows, int gl) {
  const int64_t waves = ceil_div(rows, 64 / gl);
  return (unsigned)ceil_div(waves, kPoolBlock / 64);
}

__device__ __forceinline__ int64_t pool_wave_id() {
  return ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
}

// ||w||_2, the same bits in every wave: lane-strided squares, then the DPP tree
__device__ __forceinline__ float pool_wnorm(const float* __restrict__ w, int F) {
  float t = 0.f;
  for (int f = lane_id(); f < F; f += 64) t += w[f] * w[f];
  return sqrtf(group_sum(t, 64));
}

// <attn[row, :], w> by the row's lane group (all lanes of the wave take part)
__device__ __forceinline__ float pool_row_dot(const float* __restrict__ a, const float* __restrict__ w, int F, int sub,
                                              int gl) {
  float t = 0.f;
  for (int f = sub; f < F; f += gl) t += a[f] * w[f];
  return group_sum(t, gl);
}

__global__ __launch_bounds__(kPoolBlock) void k_pool_score(const float* __restrict__ attn, int64_t ld, int64_t n, int F,
                                                           const float* __restrict__ w, int flags, int gl,
                                                           float* __restrict__ score) {
  const int lane = lane_id();
  const int64_t row = pool_wave_id() * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  const bool raw = flags & MP_POOL_SCORE_RAW;
  const float nrm = raw ? 1.f : pool_wnorm(w, F);
  const bool valid = row < n;
  const float z = pool_row_dot(attn + (valid ? row : 0) * ld, w, F, sub, gl);
  const float u = raw ? z : z / nrm;
  const float s = (flags & MP_POOL_SCORE_TANH) ? tanhf(u) : u;
  if (valid && sub == 0) score[row] = s;
}

// backward, pass 1: du and z of every row, and the g_attn rows
__global__ __launch_bounds__(kPoolBlock) void k_pool_score_bwd_rows(
    const float* __restrict__ attn, int64_t ld, int64_t n, int F, const float* __restrict__ w, int flags, int gl,
    const float* __restrict__ score, const float* __restrict__ g_score, float* __restrict__ g_attn, int64_t ldg,
    float* __restrict__ du_out, float* __restrict__ z_out) {
  const int lane = lane_id();
  const int64_t row = pool_wave_id() * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  const bool raw = flags & MP_POOL_SCORE_RAW;
  const float nrm = raw ? 1.f : pool_wnorm(w, F);
  const bool valid = row < n;
  const float z = pool_row_dot(attn + (valid ? row : 0) * ld, w, F, sub, gl);
  if (!valid) return;
  float du = g_score[row];
  if (flags & MP_POOL_SCORE_TANH) {
    const float s = score[row];
    du = du * (1.f - s * s);
  }
  if (sub == 0) {
    du_out[row] = du;
    z_out[row] = z;
  }
  if (g_attn) {
    const float c = raw ? du : du / nrm;
    for (int f = sub; f < F; f += gl) g_attn[row * ldg + f] = c * w[f];
  }
}

// pass 2: part[p, c] = sum over the rows of chunk p of du * (c < F ? attn[., c] : z);
// a lane owns a column, the block's four waves take every fourth row and are
// added in wave order
__global__ __launch_bounds__(kPoolBlock) void k_pool_score_bwd_parts(const float* __restrict__ attn, int64_t ld,
                                                                    int64_t n, int F, int64_t chunk,
                                                                    const float* __restrict__ du,
                                                                    const float* __restrict__ z,
                                                                    float* __restrict__ part) {
  __shared__ float sh[kPoolBlock / 64][64];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
  float acc = 0.f;
  if (c <= F) {
    for (int64_t r = r0 + wv; r < r1; r += kPoolBlock / 64) {
      const float v = c < F ? attn[r * ld + c] : z[r];
      acc += du[r] * v;
    }
  }
  sh[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && c <= F) {
    float t = sh[0][lane];
    for (int k = 1; k < kPoolBlock / 64; ++k) t += sh[k][lane];
    part[(int64_t)blockIdx.x * (F + 1) + c] = t;
  }
}

// pass 3: the partials in chunk order, then g_w
__global__ __launch_bounds__(kPoolBlock) void k_pool_score_bwd_finish(const float* __restrict__ part, int n_parts,
                                                                     int F, const float* __restrict__ w, int flags,
                                                                     float* __restrict__ g_w) {
  const bool raw = flags & MP_POOL_SCORE_RAW;
  const float nrm = raw ? 1.f : pool_wnorm(w, F);
  float sz = 0.f;
  if (!raw)
    for (int p = 0; p < n_parts; ++p) sz += part[(int64_t)p * (F + 1) + F];
  for (int f = threadIdx.x; f < F; f += kPoolBlock) {
    float s = 0.f;
    for (int p = 0; p < n_parts; ++p) s += part[(int64_t)p * (F + 1) + f];
    g_w[f] = raw ? s : s / nrm - (sz * w[f]) / (nrm * nrm * nrm);
  }
}

// ---- batch vector ----------------------------------------------------------

__global__ void k_batch_stats(const int64_t* __restrict__ batch, int64_t n, unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const int64_t b = in ? batch[i] : 0;
  const int64_t prev = in && i > 0 ? batch[i - 1] : b;
  const bool bad = in && (b < prev || (i == 0 && b < 0));
  long long len = 0;
  if (in && (i == 0 || b != prev)) {
    int64_t lo = i, hi = n;  // batch[lo] <= b; the first index past the run (exact for a sorted batch)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (batch[mid] <= b) lo = mid;
      else hi = mid;
    }
    len = hi - i;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const long long o = __shfl_xor(len, d);
    len = o > len ? o : len;
  }
  const unsigned long long nbad = __ballot(bad);
  if (lane_id() == 0 && len > 0) atomicMax(stats + 1, (unsigned long long)len);
  if (lane_id() == 0 && nbad) atomicAdd(stats + 2, (unsigned long long)__popcll(nbad));
  if (in && i == n - 1) stats[0] = (unsigned long long)(b + 1);
}

__global__ void k_batch_starts(const int64_t* __restrict__ batch, int64_t n, int64_t G, int64_t* __restrict__ starts) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > G) return;
  int64_t lo = 0, hi = n;  // first i with batch[i] >= g
  if (g == G) lo = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (batch[mid] < g) lo = mid + 1;
    else hi = mid;
  }
  starts[g] = g == 0 ? 0 : lo;
}

// ---- select ----------------------------------------------------------------

// k_g = min(n_g, ceil(fl32(ratio * fl32(n_g)))): one fp32 multiply (upstream's
// (ratio * num_nodes.to(torch.float)).ceil()); the min guards n_g > 2^24, where
// fl32(n_g) may round up past n_g
__device__ __forceinline__ int64_t topk_k(float ratio, int64_t n) {
  if (n <= 0) return 0;
  const float p = ratio * (float)n;
  int64_t k = (int64_t)ceilf(p);
  if (k > n) k = n;
  return k < 0 ? 0 : k;
}

// order-preserving uint32 key: -0 -> +0, every NaN -> the top key
__device__ __forceinline__ uint32_t topk_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  uint32_t b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int64_t pool_seg_of(const int64_t* __restrict__ starts, int64_t G, int64_t i) {
  int64_t lo = 0, hi = G;  // starts[lo] <= i < starts[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (starts[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// out_starts = exclusive scan of k_g in one workgroup (integer: exact in any
// order); counts[0] = K, or -1 when a graph is larger than max_n
__global__ __launch_bounds__(1024) void k_topk_plan(const int64_t* __restrict__ starts, int64_t G, float ratio,
                                                    int64_t max_n, int64_t* __restrict__ out_starts,
                                                    int64_t* __restrict__ counts) {
  __shared__ long long wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long carry = 0;
  int over = 0;
  for (int64_t base = 0; base < G; base += 1024) {
    const int64_t g = base + tid;
    int64_t n_g = g < G ? starts[g + 1] - starts[g] : 0;
    if (n_g < 0) n_g = 0;
    if (n_g > max_n) over = 1;
    const long long k = topk_k(ratio, n_g);
    long long v = k;
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(v, d);
      if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    long long woff = 0, total = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < wv) woff += wsum[q];
      total += wsum[q];
    }
    if (g < G) out_starts[g] = carry + woff + v - k;
    carry += total;
    __syncthreads();
  }
  over = __syncthreads_or(over);
  if (tid == 0) {
    out_starts[G] = carry;
    counts[0] = over ? -1 : carry;
  }
}

__device__ __forceinline__ void topk_emit(int64_t node, int64_t rank, int64_t o0, int64_t k,
                                          int64_t* __restrict__ perm, int64_t* __restrict__ inv) {
  const bool keep = rank < k;
  inv[node] = keep ? o0 + rank : -1;
  if (keep) perm[o0 + rank] = node;
}

// graphs of 1..64 nodes: one wave each, keys in registers
__global__ __launch_bounds__(kPoolBlock) void k_topk_wave(const float* __restrict__ score,
                                                          const int64_t* __restrict__ starts, int64_t G,
                                                          const int64_t* __restrict__ out_starts,
                                                          int64_t* __restrict__ perm, int64_t* __restrict__ inv) {
  const int64_t g = pool_wave_id();
  if (g >= G) return;
  const int64_t s0 = starts[g];
  const int64_t n64 = starts[g + 1] - s0;
  if (n64 <= 0 || n64 > 64) return;
  const int n = uni((int)n64);
  const int lane = lane_id();
  const int64_t o0 = out_starts[g], k = out_starts[g + 1] - o0;
  const uint32_t key = lane < n ? topk_key(score[s0 + lane]) : 0u;
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t kj = (uint32_t)readlane((int)key, j);
    rank += (kj > key || (kj == key && j < lane)) ? 1 : 0;
  }
  if (lane < n) topk_emit(s0 + lane, rank, o0, k, perm, inv);
}

// graphs of 65..cap nodes: one workgroup each (256 threads, or 1024 when the
// batch holds a graph of more than 256 nodes: the count is quadratic and a
// batch of few large graphs has few workgroups), keys in LDS (cap * 4 bytes)
__global__ __launch_bounds__(1024) void k_topk_block(const float* __restrict__ score,
                                                           const int64_t* __restrict__ starts,
                                                           const int64_t* __restrict__ out_starts,
                                                           int64_t* __restrict__ perm, int64_t* __restrict__ inv,
                                                           int cap) {
  extern __shared__ uint32_t keys[];
  const int64_t g = blockIdx.x;
  const int64_t s0 = starts[g];
  const int64_t n64 = starts[g + 1] - s0;
  if (n64 <= 64 || n64 > cap) return;
  const int n = (int)n64;
  const int64_t o0 = out_starts[g], k = out_starts[g + 1] - o0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) keys[i] = topk_key(score[s0 + i]);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const uint32_t key = keys[i];
    int rank = 0;
    for (int j = 0; j < i; ++j) rank += keys[j] >= key ? 1 : 0;
    for (int j = i + 1; j < n; ++j) rank += keys[j] > key ? 1 : 0;
    topk_emit(s0 + i, rank, o0, k, perm, inv);
  }
}

// sorted path: the composite of every node of an over-limit graph (0 for the rest)
__global__ void k_topk_sort_keys(const float* __restrict__ score, int64_t n, const int64_t* __restrict__ starts,
                                 int64_t G, int cap, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t g = G == 1 ? 0 : pool_seg_of(starts, G, i);
  const int64_t s0 = starts[g];
  uint64_t key = 0;
  if (starts[g + 1] - s0 > cap) key = ((uint64_t)topk_key(score[i]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(i - s0));
  keys[i] = key;
}

__global__ void k_topk_segments(const int64_t* __restrict__ starts, int64_t G, int cap, int64_t* __restrict__ begin,
                                int64_t* __restrict__ end) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t s0 = starts[g], s1 = starts[g + 1];
  begin[g] = s0;
  end[g] = s1 - s0 > cap ? s1 : s0;
}

__global__ void k_topk_sort_emit(const uint64_t* __restrict__ sorted, int64_t n, const int64_t* __restrict__ starts,
                                 int64_t G, int cap, const int64_t* __restrict__ out_starts,
                                 int64_t* __restrict__ perm, int64_t* __restrict__ inv) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t g = G == 1 ? 0 : pool_seg_of(starts, G, p);
  const int64_t s0 = starts[g], n_g = starts[g + 1] - s0;
  if (n_g <= cap) return;
  const int64_t local = (int64_t)(0xFFFFFFFFu - (uint32_t)sorted[p]);
  if (local >= n_g) return;  // never for keys this unit wrote; keeps any store inside the graph
  const int64_t o0 = out_starts[g];
  topk_emit(s0 + local, p - s0, o0, out_starts[g + 1] - o0, perm, inv);
}

static hipError_t topk_sort_bytes(int64_t n, int64_t G, size_t* bytes) {
  const size_t size = (size_t)(n > 0 ? n : 1);
  if (G == 1)
    return rocprim::radix_sort_keys_desc((void*)nullptr, *bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, size, 0u,
                                         64u, (hipStream_t)0, false);
  return rocprim::segmented_radix_sort_keys_desc((void*)nullptr, *bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, size,
                                                 (unsigned)G, (const int64_t*)nullptr, (const int64_t*)nullptr, 0u,
                                                 64u, (hipStream_t)0, false);
}

// mp_topk_select_f32's workspace on the sorted path: the composites, their sorted
// copy and the segment bounds, then the sort's temp.  The on-chip paths use no
// workspace; the caller still passes kTopkOnChipWs bytes.
constexpr size_t kTopkOnChipWs = 256;
struct TopkSortWs : Carver {
  int64_t n, G;
  uint64_t* keys = take<uint64_t>(n);
  uint64_t* keys_out = take<uint64_t>(n);
  int64_t* seg_begin = take<int64_t>(G);
  int64_t* seg_end = take<int64_t>(G);
};

// mp_pool_score_bwd_f32's workspace: du and z of every row, the per-chunk partials
struct ScoreBwdWs : Carver {
  int64_t n, F;
  float* du = take<float>(n);
  float* z = take<float>(n);
  float* part = take<float>(mp_pool_score_bwd_parts(n) * ((F > 0 ? F : 1) + 1));
};

// ---- gate ------------------------------------------------------------------

template <int VEC>
__global__ __launch_bounds__(kPoolBlock) void k_pool_gate(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ score,
                                                          const int64_t* __restrict__ batch,
                                                          const int64_t* __restrict__ perm, int64_t k, int64_t n,
                                                          int FE, float mult, int use_mult, int gl,
                                                          float* __restrict__ x_out, int64_t ldo,
                                                          int64_t* __restrict__ batch_out,
                                                          float* __restrict__ score_out) {
  const int lane = lane_id();
  const int64_t r = pool_wave_id() * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  if (r >= k) return;
  const int64_t node = perm[r];
  const bool ok = node >= 0 && node < n;  // a perm of this engine always is; a foreign one never reads outside x
  const float s = ok ? score[node] : 0.f;
  for (int e = sub; e < FE; e += gl) {
    Frag<VEC> v;
    if (ok) {
      v = load_frag<VEC>(x + node * ldx + (int64_t)e * VEC);
    } else {
#pragma unroll
      for (int q = 0; q < VEC; ++q) v.v[q] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      v.v[q] = v.v[q] * s;
      if (use_mult) v.v[q] = mult * v.v[q];
    }
    store_frag<VEC>(x_out + r * ldo + (int64_t)e * VEC, v);
  }
  if (sub == 0) {
    score_out[r] = s;
    if (batch_out) batch_out[r] = ok && batch ? batch[node] : 0;
  }
}

// A fragment of VEC floats by one vector access (ALIGNED: 16-byte aligned rows) or by VEC scalar ones
template <int VEC, bool ALIGNED>
__device__ __forceinline__ Frag<VEC> pool_load(const float* p) {
  if constexpr (ALIGNED) {
    return load_frag<VEC>(p);
  } else {
    Frag<VEC> r;
#pragma unroll
    for (int q = 0; q < VEC; ++q) r.v[q] = p[q];
    return r;
  }
}

template <int VEC, bool ALIGNED>
__device__ __forceinline__ void pool_store(float* p, const Frag<VEC>& f) {
  if constexpr (ALIGNED) {
    store_frag<VEC>(p, f);
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q) p[q] = f.v[q];
  }
}

// g_s[i] = mult * <g_y[r, :], x[i, :]> is a sum: its order is fixed by VEC (a lane adds its VEC
// consecutive features, then the lane group is added), so VEC follows F alone (4 when F % 4 == 0)
// and rows that are not 16-byte aligned (a column slice of a wider tensor) keep VEC and only
// change how a fragment is moved: the gradient does not depend on where x lies in memory
template <int VEC, bool ALIGNED>
__global__ __launch_bounds__(kPoolBlock) void k_pool_gate_bwd(const float* __restrict__ g_y, int64_t ldgy,
                                                              const float* __restrict__ g_t,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ score,
                                                              const int64_t* __restrict__ inv, int64_t k, int64_t n,
                                                              int FE, float mult, int use_mult, int gl,
                                                              float* __restrict__ g_x, int64_t ldgx,
                                                              float* __restrict__ g_s) {
  const int lane = lane_id();
  const int64_t i = pool_wave_id() * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  const bool valid = i < n;
  const int64_t r = valid ? inv[i] : -1;
  const bool kept = r >= 0 && r < k;
  const float s = valid ? score[i] : 0.f;
  const float c = use_mult ? mult * s : s;
  float dot = 0.f;
  for (int e = sub; e < FE; e += gl) {
    Frag<VEC> o;
    if (kept) {
      const Frag<VEC> gy = pool_load<VEC, ALIGNED>(g_y + r * ldgy + (int64_t)e * VEC);
      const Frag<VEC> xv = pool_load<VEC, ALIGNED>(x + i * ldx + (int64_t)e * VEC);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        dot += gy.v[q] * xv.v[q];
        o.v[q] = c * gy.v[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < VEC; ++q) o.v[q] = 0.f;
    }
    if (valid) pool_store<VEC, ALIGNED>(g_x + i * ldgx + (int64_t)e * VEC, o);
  }
  dot = group_sum(dot, gl);
  if (valid && sub == 0) {
    float v = 0.f;
    if (kept) {
      v = use_mult ? mult * dot : dot;
      if (g_t) v += g_t[r];
    }
    g_s[i] = v;
  }
}

static inline bool pool_vec4_ok(int F, const void* a, int64_t lda, const void* b, int64_t ldb) {
  return F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0;
}

// ---- filter_adj --------------------------------------------------------------

__global__ void k_pool_inverse(const int64_t* __restrict__ perm, int64_t k, const int64_t* __restrict__ k_dev,
                               int64_t n, int64_t* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= k || (k_dev && r >= *k_dev)) return;
  const int64_t node = perm[r];
  if (node >= 0 && node < n) inv[node] = r;
}

// keep[e] = both ends kept; counts[2] += edge ends outside [0, n_nodes)
__global__ void k_pool_edge_flags(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t n_edges,
                                  const int64_t* __restrict__ inv, int64_t n_nodes, uint8_t* __restrict__ keep,
                                  unsigned long long* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e < n_edges;
  const int64_t r = in ? row[e] : 0, c = in ? col[e] : 0;
  const bool rbad = in && (r < 0 || r >= n_nodes), cbad = in && (c < 0 || c >= n_nodes);
  const unsigned long long bad = __ballot(rbad), bad2 = __ballot(cbad);
  if (lane_id() == 0 && (bad | bad2)) atomicAdd(counts + 2, (unsigned long long)(__popcll(bad) + __popcll(bad2)));
  if (in) keep[e] = (!rbad && !cbad && inv[r] >= 0 && inv[c] >= 0) ? 1 : 0;
}

// the relabelled kept edges; n_kept is read from the device
__global__ void k_pool_edge_emit(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                 const int64_t* __restrict__ inv, const int64_t* __restrict__ pos,
                                 const int64_t* __restrict__ n_kept, int64_t n_edges, int64_t* __restrict__ out_row,
                                 int64_t* __restrict__ out_col) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_edges || k >= *n_kept) return;
  const int64_t p = pos[k];
  out_row[k] = inv[row[p]];
  out_col[k] = inv[col[p]];
}

// mp_pool_filter_adj's workspace: keep flag per edge, then the select's temp
// (mp_pool_compact's is the select's temp alone: a bare Carver)
struct FilterAdjWs : Carver {
  int64_t n_edges;
  uint8_t* keep = take<uint8_t>(n_edges);
};

}  // namespace mp

using namespace mp;

extern "C" {

int mp_topk_path(int64_t n_g) {
  if (n_g <= 64) return 0;
  return n_g <= tuned_topk_wg_limit() ? 1 : 2;
}

int mp_batch_stats(const int64_t* batch, int64_t n, int64_t* stats, size_t stats_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_batch_stats: n = %lld is negative or not below 2^31", (long long)n);
  MP_CHECK_ARG(stats, "mp_batch_stats: stats is NULL");
  MP_CHECK_ARG(n == 0 || batch, "mp_batch_stats: batch is NULL");
  MP_CHECK_EXTENT("mp_batch_stats", "stats", stats_bytes, 3 * sizeof(int64_t));
  hipStream_t s = as_stream(stream);
  MP_CHECK_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(int64_t), s));
  if (n == 0) return MP_OK;
  k_batch_stats<<<(unsigned)ceil_div(n, kPoolBlock), kPoolBlock, 0, s>>>(batch, n,
                                                                        reinterpret_cast<unsigned long long*>(stats));
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_batch_starts(const int64_t* batch, int64_t n, int64_t n_graphs, int64_t* starts, size_t starts_bytes,
                    void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_batch_starts: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(n_graphs >= 0 && n_graphs < (int64_t)INT32_MAX,
               "mp_batch_starts: n_graphs = %lld is negative or not below 2^31", (long long)n_graphs);
  MP_CHECK_ARG(starts, "mp_batch_starts: starts is NULL");
  MP_CHECK_ARG(n == 0 || batch, "mp_batch_starts: batch is NULL");
  MP_CHECK_EXTENT("mp_batch_starts", "starts", starts_bytes, (size_t)(n_graphs + 1) * sizeof(int64_t));
  k_batch_starts<<<(unsigned)ceil_div(n_graphs + 1, kPoolBlock), kPoolBlock, 0, as_stream(stream)>>>(batch, n, n_graphs,
                                                                                                    starts);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_pool_score_f32(const float* attn, int64_t ld, int64_t n, int32_t F, const float* w, int32_t flags,
                      float* score, size_t score_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_score_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(F >= 1, "mp_pool_score_f32: F = %d", F);
  MP_CHECK_ARG(ld >= F, "mp_pool_score_f32: ld = %lld < F = %d", (long long)ld, F);
  MP_CHECK_ARG((flags & ~(MP_POOL_SCORE_TANH | MP_POOL_SCORE_RAW)) == 0, "mp_pool_score_f32: unknown flags %d", flags);
  MP_CHECK_ARG(w, "mp_pool_score_f32: w is NULL");
  MP_CHECK_ARG(n == 0 || attn, "mp_pool_score_f32: attn is NULL");
  MP_CHECK_ARG(n == 0 || score, "mp_pool_score_f32: score is NULL");
  MP_CHECK_EXTENT("mp_pool_score_f32", "score", score_bytes, (size_t)n * sizeof(float));
  if (n == 0) return MP_OK;
  const int gl = group_lanes(F);
  k_pool_score<<<pool_row_blocks(n, gl), kPoolBlock, 0, as_stream(stream)>>>(attn, ld, n, F, w, flags, gl, score);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int32_t mp_pool_score_bwd_parts(int64_t n) {
  const int64_t p = ceil_div(n > 0 ? n : 1, 256);
  return (int32_t)(p < kScoreBwdMaxParts ? p : kScoreBwdMaxParts);
}

size_t mp_pool_score_bwd_workspace(int64_t n, int32_t F) {
  return ScoreBwdWs{nullptr, n, F}.off;
}

int mp_pool_score_bwd_f32(const float* attn, int64_t ld, int64_t n, int32_t F, const float* w, int32_t flags,
                          const float* score, const float* g_score, float* g_attn, int64_t ldg, float* g_w,
                          size_t g_w_bytes, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_score_bwd_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(F >= 1, "mp_pool_score_bwd_f32: F = %d", F);
  MP_CHECK_ARG(ld >= F, "mp_pool_score_bwd_f32: ld = %lld < F = %d", (long long)ld, F);
  MP_CHECK_ARG(!g_attn || ldg >= F, "mp_pool_score_bwd_f32: ldg = %lld < F = %d", (long long)ldg, F);
  MP_CHECK_ARG((flags & ~(MP_POOL_SCORE_TANH | MP_POOL_SCORE_RAW)) == 0, "mp_pool_score_bwd_f32: unknown flags %d",
               flags);
  MP_CHECK_ARG(w, "mp_pool_score_bwd_f32: w is NULL");
  MP_CHECK_ARG(g_w, "mp_pool_score_bwd_f32: g_w is NULL");
  MP_CHECK_ARG(n == 0 || attn, "mp_pool_score_bwd_f32: attn is NULL");
  MP_CHECK_ARG(n == 0 || g_score, "mp_pool_score_bwd_f32: g_score is NULL");
  MP_CHECK_ARG(n == 0 || score || !(flags & MP_POOL_SCORE_TANH), "mp_pool_score_bwd_f32: score is NULL");
  MP_CHECK_ARG(ws, "mp_pool_score_bwd_f32: ws is NULL");
  MP_CHECK_EXTENT("mp_pool_score_bwd_f32", "g_w", g_w_bytes, (size_t)F * sizeof(float));
  const ScoreBwdWs l{ws, n, F};
  MP_CHECK_EXTENT("mp_pool_score_bwd_f32", "ws", ws_bytes, l.off);
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    MP_CHECK_HIP(hipMemsetAsync(g_w, 0, (size_t)F * sizeof(float), s));
    return MP_OK;
  }
  const int gl = group_lanes(F);
  k_pool_score_bwd_rows<<<pool_row_blocks(n, gl), kPoolBlock, 0, s>>>(attn, ld, n, F, w, flags, gl, score, g_score,
                                                                     g_attn, ldg, l.du, l.z);
  MP_CHECK_LAUNCH();
  const int parts = mp_pool_score_bwd_parts(n);
  const int64_t chunk = ceil_div(n, parts);
  k_pool_score_bwd_parts<<<dim3((unsigned)parts, (unsigned)ceil_div(F + 1, 64)), kPoolBlock, 0, s>>>(
      attn, ld, n, F, chunk, l.du, l.z, l.part);
  MP_CHECK_LAUNCH();
  k_pool_score_bwd_finish<<<1, kPoolBlock, 0, s>>>(l.part, parts, F, w, flags, g_w);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_topk_counts(const int64_t* starts, int64_t n_graphs, float ratio, int64_t max_n, int64_t* out_starts,
                   size_t out_starts_bytes, int64_t* counts, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_graphs >= 0 && n_graphs < (int64_t)INT32_MAX,
               "mp_topk_counts: n_graphs = %lld is negative or not below 2^31", (long long)n_graphs);
  MP_CHECK_ARG(ratio > 0.f && ratio <= 1.f, "mp_topk_counts: ratio = %g is outside (0, 1]", (double)ratio);
  MP_CHECK_ARG(max_n >= 0, "mp_topk_counts: max_n = %lld", (long long)max_n);
  MP_CHECK_ARG(starts, "mp_topk_counts: starts is NULL");
  MP_CHECK_ARG(out_starts, "mp_topk_counts: out_starts is NULL");
  MP_CHECK_ARG(counts, "mp_topk_counts: counts is NULL");
  MP_CHECK_EXTENT("mp_topk_counts", "out_starts", out_starts_bytes, (size_t)(n_graphs + 1) * sizeof(int64_t));
  k_topk_plan<<<1, 1024, 0, as_stream(stream)>>>(starts, n_graphs, ratio, max_n, out_starts, counts);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

size_t mp_topk_workspace(int64_t n, int64_t n_graphs, int64_t max_n) {
  if (max_n <= tuned_topk_wg_limit()) return kTopkOnChipWs;
  size_t sort = 0;
  (void)topk_sort_bytes(n, n_graphs, &sort);
  return TopkSortWs{nullptr, n, n_graphs}.total(sort);
}

int mp_topk_select_f32(const float* score, int64_t n, const int64_t* starts, int64_t n_graphs, int64_t max_n,
                       float ratio, int64_t* perm, size_t perm_bytes, int64_t* out_starts, size_t out_starts_bytes,
                       int64_t* inv, size_t inv_bytes, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_topk_select_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(n_graphs >= 0 && n_graphs < (int64_t)INT32_MAX,
               "mp_topk_select_f32: n_graphs = %lld is negative or not below 2^31", (long long)n_graphs);
  MP_CHECK_ARG(n == 0 || n_graphs > 0, "mp_topk_select_f32: %lld nodes but n_graphs = 0", (long long)n);
  MP_CHECK_ARG(ratio > 0.f && ratio <= 1.f, "mp_topk_select_f32: ratio = %g is outside (0, 1]", (double)ratio);
  MP_CHECK_ARG(max_n >= 0 && max_n <= n, "mp_topk_select_f32: max_n = %lld is outside [0, n]", (long long)max_n);
  MP_CHECK_ARG(starts, "mp_topk_select_f32: starts is NULL");
  MP_CHECK_ARG(out_starts, "mp_topk_select_f32: out_starts is NULL");
  MP_CHECK_ARG(counts, "mp_topk_select_f32: counts is NULL");
  MP_CHECK_ARG(n == 0 || score, "mp_topk_select_f32: score is NULL");
  MP_CHECK_ARG(n == 0 || perm, "mp_topk_select_f32: perm is NULL");
  MP_CHECK_ARG(n == 0 || inv, "mp_topk_select_f32: inv is NULL");
  MP_CHECK_ARG(ws, "mp_topk_select_f32: ws is NULL");
  MP_CHECK_EXTENT("mp_topk_select_f32", "perm", perm_bytes, (size_t)n * sizeof(int64_t));
  MP_CHECK_EXTENT("mp_topk_select_f32", "inv", inv_bytes, (size_t)n * sizeof(int64_t));
  MP_CHECK_EXTENT("mp_topk_select_f32", "out_starts", out_starts_bytes, (size_t)(n_graphs + 1) * sizeof(int64_t));
  const int64_t limit = tuned_topk_wg_limit();
  const bool sorted = max_n > limit;
  const TopkSortWs w{ws, n, n_graphs};
  MP_CHECK_EXTENT("mp_topk_select_f32", "ws", ws_bytes, sorted ? w.off : kTopkOnChipWs);
  size_t sort_bytes = 0;
  if (sorted) {
    const hipError_t size_query = topk_sort_bytes(n, n_graphs, &sort_bytes);
    MP_CHECK_EXTENT("mp_topk_select_f32", "ws", ws_bytes, w.total(sort_bytes));
    MP_CHECK_HIP(size_query);
  }
  hipStream_t s = as_stream(stream);
  k_topk_plan<<<1, 1024, 0, s>>>(starts, n_graphs, ratio, max_n, out_starts, counts);
  MP_CHECK_LAUNCH();
  if (n == 0) return MP_OK;
  const int cap = (int)(max_n < limit ? max_n : limit);  // keys a workgroup holds
  k_topk_wave<<<(unsigned)ceil_div(n_graphs, kPoolBlock / 64), kPoolBlock, 0, s>>>(score, starts, n_graphs, out_starts,
                                                                                   perm, inv);
  MP_CHECK_LAUNCH();
  if (max_n > 64) {
    k_topk_block<<<(unsigned)n_graphs, cap > 256 ? 1024 : kPoolBlock, (size_t)cap * sizeof(uint32_t), s>>>(
        score, starts, out_starts, perm, inv, cap);
    MP_CHECK_LAUNCH();
  }
  if (sorted) {
    k_topk_sort_keys<<<(unsigned)ceil_div(n, kPoolBlock), kPoolBlock, 0, s>>>(score, n, starts, n_graphs, cap, w.keys);
    MP_CHECK_LAUNCH();
    if (n_graphs == 1) {
      MP_CHECK_HIP(rocprim::radix_sort_keys_desc(w.rest(), sort_bytes, w.keys, w.keys_out, (size_t)n, 0u, 64u, s,
                                                 false));
    } else {
      k_topk_segments<<<(unsigned)ceil_div(n_graphs, kPoolBlock), kPoolBlock, 0, s>>>(starts, n_graphs, cap,
                                                                                      w.seg_begin, w.seg_end);
      MP_CHECK_LAUNCH();
      MP_CHECK_HIP(rocprim::segmented_radix_sort_keys_desc(w.rest(), sort_bytes, w.keys, w.keys_out, (size_t)n,
                                                           (unsigned)n_graphs, w.seg_begin, w.seg_end, 0u, 64u, s,
                                                           false));
    }
    k_topk_sort_emit<<<(unsigned)ceil_div(n, kPoolBlock), kPoolBlock, 0, s>>>(w.keys_out, n, starts, n_graphs, cap,
                                                                              out_starts, perm, inv);
    MP_CHECK_LAUNCH();
  }
  return MP_OK;
}

int mp_pool_gate_f32(const float* x, int64_t ldx, const float* score, const int64_t* batch, const int64_t* perm,
                     int64_t k, int64_t n, int32_t F, float multiplier, float* x_out, int64_t ldo,
                     size_t x_out_bytes, int64_t* batch_out, float* score_out, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_gate_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(k >= 0 && k <= n, "mp_pool_gate_f32: k = %lld is outside [0, n]", (long long)k);
  MP_CHECK_ARG(F >= 1, "mp_pool_gate_f32: F = %d", F);
  MP_CHECK_ARG(ldx >= F, "mp_pool_gate_f32: ldx = %lld < F = %d", (long long)ldx, F);
  MP_CHECK_ARG(ldo >= F, "mp_pool_gate_f32: ldo = %lld < F = %d", (long long)ldo, F);
  if (k == 0) return MP_OK;
  MP_CHECK_ARG(x, "mp_pool_gate_f32: x is NULL");
  MP_CHECK_ARG(score, "mp_pool_gate_f32: score is NULL");
  MP_CHECK_ARG(perm, "mp_pool_gate_f32: perm is NULL");
  MP_CHECK_ARG(x_out, "mp_pool_gate_f32: x_out is NULL");
  MP_CHECK_ARG(score_out, "mp_pool_gate_f32: score_out is NULL");
  MP_CHECK_EXTENT("mp_pool_gate_f32", "x_out", x_out_bytes, ((size_t)(k - 1) * (size_t)ldo + (size_t)F) * sizeof(float));
  hipStream_t s = as_stream(stream);
  const int use_mult = multiplier != 1.f;
  if (pool_vec4_ok(F, x, ldx, x_out, ldo)) {
    const int gl = group_lanes(F / 4);
    k_pool_gate<4><<<pool_row_blocks(k, gl), kPoolBlock, 0, s>>>(x, ldx, score, batch, perm, k, n, F / 4, multiplier,
                                                                use_mult, gl, x_out, ldo, batch_out, score_out);
  } else {
    const int gl = group_lanes(F);
    k_pool_gate<1><<<pool_row_blocks(k, gl), kPoolBlock, 0, s>>>(x, ldx, score, batch, perm, k, n, F, multiplier,
                                                                use_mult, gl, x_out, ldo, batch_out, score_out);
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_pool_gate_bwd_f32(const float* g_y, int64_t ldgy, const float* g_t, const float* x, int64_t ldx,
                         const float* score, const int64_t* inv, int64_t k, int64_t n, int32_t F, float multiplier,
                         float* g_x, int64_t ldgx, size_t g_x_bytes, float* g_s, size_t g_s_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_gate_bwd_f32: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(k >= 0 && k <= n, "mp_pool_gate_bwd_f32: k = %lld is outside [0, n]", (long long)k);
  MP_CHECK_ARG(F >= 1, "mp_pool_gate_bwd_f32: F = %d", F);
  MP_CHECK_ARG(ldx >= F, "mp_pool_gate_bwd_f32: ldx = %lld < F = %d", (long long)ldx, F);
  MP_CHECK_ARG(ldgy >= F, "mp_pool_gate_bwd_f32: ldgy = %lld < F = %d", (long long)ldgy, F);
  MP_CHECK_ARG(ldgx >= F, "mp_pool_gate_bwd_f32: ldgx = %lld < F = %d", (long long)ldgx, F);
  if (n == 0) return MP_OK;
  MP_CHECK_ARG(k == 0 || g_y, "mp_pool_gate_bwd_f32: g_y is NULL");
  MP_CHECK_ARG(x, "mp_pool_gate_bwd_f32: x is NULL");
  MP_CHECK_ARG(score, "mp_pool_gate_bwd_f32: score is NULL");
  MP_CHECK_ARG(inv, "mp_pool_gate_bwd_f32: inv is NULL");
  MP_CHECK_ARG(g_x, "mp_pool_gate_bwd_f32: g_x is NULL");
  MP_CHECK_ARG(g_s, "mp_pool_gate_bwd_f32: g_s is NULL");
  MP_CHECK_EXTENT("mp_pool_gate_bwd_f32", "g_x", g_x_bytes, ((size_t)(n - 1) * (size_t)ldgx + (size_t)F) * sizeof(float));
  MP_CHECK_EXTENT("mp_pool_gate_bwd_f32", "g_s", g_s_bytes, (size_t)n * sizeof(float));
  hipStream_t s = as_stream(stream);
  const int use_mult = multiplier != 1.f;
  if (F % 4 == 0) {
    const int gl = group_lanes(F / 4);
    if (pool_vec4_ok(F, x, ldx, g_x, ldgx) && ldgy % 4 == 0 && (uintptr_t)g_y % 16 == 0) {
      k_pool_gate_bwd<4, true><<<pool_row_blocks(n, gl), kPoolBlock, 0, s>>>(
          g_y, ldgy, g_t, x, ldx, score, inv, k, n, F / 4, multiplier, use_mult, gl, g_x, ldgx, g_s);
    } else {
      k_pool_gate_bwd<4, false><<<pool_row_blocks(n, gl), kPoolBlock, 0, s>>>(
          g_y, ldgy, g_t, x, ldx, score, inv, k, n, F / 4, multiplier, use_mult, gl, g_x, ldgx, g_s);
    }
  } else {
    const int gl = group_lanes(F);
    k_pool_gate_bwd<1, true><<<pool_row_blocks(n, gl), kPoolBlock, 0, s>>>(g_y, ldgy, g_t, x, ldx, score, inv, k, n, F,
                                                                          multiplier, use_mult, gl, g_x, ldgx, g_s);
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_pool_inverse(const int64_t* perm, int64_t k, const int64_t* k_dev, int64_t n, int64_t* inv, size_t inv_bytes,
                    void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_inverse: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(k >= 0, "mp_pool_inverse: k = %lld", (long long)k);
  MP_CHECK_ARG(k == 0 || perm, "mp_pool_inverse: perm is NULL");
  MP_CHECK_ARG(n == 0 || inv, "mp_pool_inverse: inv is NULL");
  MP_CHECK_EXTENT("mp_pool_inverse", "inv", inv_bytes, (size_t)n * sizeof(int64_t));
  if (n == 0) return MP_OK;
  hipStream_t s = as_stream(stream);
  MP_CHECK_HIP(hipMemsetAsync(inv, 0xff, (size_t)n * sizeof(int64_t), s));  // -1
  if (k == 0) return MP_OK;
  k_pool_inverse<<<(unsigned)ceil_div(k, kPoolBlock), kPoolBlock, 0, s>>>(perm, k, k_dev, n, inv);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

size_t mp_pool_compact_workspace(int64_t n) {
  size_t sel = 0;
  (void)select_positions_bytes(n, &sel);
  return Carver(nullptr).total(sel);
}

int mp_pool_compact(const uint8_t* keep, int64_t n, int64_t* out_pos, size_t out_pos_bytes, int64_t* count_dev,
                    void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_pool_compact: n = %lld is negative or not below 2^31",
               (long long)n);
  MP_CHECK_ARG(count_dev, "mp_pool_compact: count_dev is NULL");
  MP_CHECK_ARG(n == 0 || keep, "mp_pool_compact: keep is NULL");
  MP_CHECK_ARG(n == 0 || out_pos, "mp_pool_compact: out_pos is NULL");
  MP_CHECK_ARG(ws, "mp_pool_compact: ws is NULL");
  MP_CHECK_EXTENT("mp_pool_compact", "out_pos", out_pos_bytes, (size_t)n * sizeof(int64_t));
  const Carver w(ws);
  MP_CHECK_EXTENT("mp_pool_compact", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    MP_CHECK_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
    return MP_OK;
  }
  size_t sel = 0;
  const hipError_t size_query = select_positions_bytes(n, &sel);
  MP_CHECK_EXTENT("mp_pool_compact", "ws", ws_bytes, w.total(sel));
  MP_CHECK_HIP(size_query);
  rocprim::counting_iterator<int64_t> it(0);
  MP_CHECK_HIP(rocprim::select(w.rest(), sel, it, keep, out_pos, reinterpret_cast<unsigned long long*>(count_dev),
                               (size_t)n, s, false));
  return MP_OK;
}

size_t mp_pool_filter_workspace(int64_t n_edges) {
  size_t sel = 0;
  (void)select_positions_bytes(n_edges, &sel);
  return FilterAdjWs{nullptr, n_edges}.total(sel);
}

int mp_pool_filter_adj(const int64_t* row, const int64_t* col, int64_t n_edges, const int64_t* inv, int64_t n_nodes,
                       int64_t* out_row, int64_t* out_col, int64_t* out_pos, size_t out_bytes, int64_t* counts,
                       void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(n_edges >= 0 && n_edges < (int64_t)INT32_MAX,
               "mp_pool_filter_adj: n_edges = %lld is negative or not below 2^31", (long long)n_edges);
  MP_CHECK_ARG(n_nodes >= 0, "mp_pool_filter_adj: n_nodes = %lld", (long long)n_nodes);
  MP_CHECK_ARG(counts, "mp_pool_filter_adj: counts is NULL");
  MP_CHECK_ARG(n_edges == 0 || row, "mp_pool_filter_adj: row is NULL");
  MP_CHECK_ARG(n_edges == 0 || col, "mp_pool_filter_adj: col is NULL");
  MP_CHECK_ARG(n_edges == 0 || n_nodes == 0 || inv, "mp_pool_filter_adj: inv is NULL");
  MP_CHECK_ARG(n_edges == 0 || out_row, "mp_pool_filter_adj: out_row is NULL");
  MP_CHECK_ARG(n_edges == 0 || out_col, "mp_pool_filter_adj: out_col is NULL");
  MP_CHECK_ARG(n_edges == 0 || out_pos, "mp_pool_filter_adj: out_pos is NULL");
  MP_CHECK_ARG(ws, "mp_pool_filter_adj: ws is NULL");
  MP_CHECK_EXTENT("mp_pool_filter_adj", "out_row / out_col / out_pos", out_bytes, (size_t)n_edges * sizeof(int64_t));
  const FilterAdjWs w{ws, n_edges};
  MP_CHECK_EXTENT("mp_pool_filter_adj", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  MP_CHECK_HIP(hipMemsetAsync(counts + 1, 0, 2 * sizeof(int64_t), s));
  if (n_edges == 0) return MP_OK;
  size_t sel = 0;
  const hipError_t size_query = select_positions_bytes(n_edges, &sel);
  MP_CHECK_EXTENT("mp_pool_filter_adj", "ws", ws_bytes, w.total(sel));
  MP_CHECK_HIP(size_query);
  const unsigned blocks = (unsigned)ceil_div(n_edges, kPoolBlock);
  k_pool_edge_flags<<<blocks, kPoolBlock, 0, s>>>(row, col, n_edges, inv, n_nodes, w.keep,
                                                  reinterpret_cast<unsigned long long*>(counts));
  MP_CHECK_LAUNCH();
  rocprim::counting_iterator<int64_t> it(0);
  MP_CHECK_HIP(rocprim::select(w.rest(), sel, it, w.keep, out_pos, reinterpret_cast<unsigned long long*>(counts + 1),
                               (size_t)n_edges, s, false));
  k_pool_edge_emit<<<blocks, kPoolBlock, 0, s>>>(row, col, inv, out_pos, counts + 1, n_edges, out_row, out_col);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // extern "C"
