// Point sets on the device (include/mi355_mp.h "Point sets"): farthest point
// sampling, the fixed-radius neighbour search and PointConv's per-edge feature
// matrix -- the geometry of PyG 1.4.3's PointNet++ set abstraction (nn.fps /
// nn.radius over torch_cluster 1.5, nn.conv.PointConv [U]).
//
// fps is k_g dependent steps per graph, so one graph is one workgroup (or one wave)
// and what counts is the latency of a step: update the m values a thread owns
// against the last selection, reduce to the next argmax, hand its coordinates to
// everybody.  The argmax is ONE unsigned 64-bit maximum: m >= 0, so its fp32 bits
// order as an integer, and (bits(m) << 32) | (0xFFFFFFFF - local index) is largest
// for the largest distance with the lowest index.  In a wave it is four DPP steps
// and two cross-row swaps; across waves every wave leaves its word and the winner's
// coordinates in one of two LDS slots that alternate between steps, so a step has
// one barrier: the slot a step writes was last read two steps ago, before the
// barrier between.  Three paths by graph size (mp_fps_path):
//   0  n_g <= kFpsWaveLimit: one wave, points and m in registers, the selection
//      broadcast with readlane; no LDS, no barrier;
//   1  n_g <= kFpsBlockLimit: one workgroup (256, 512 or 1024 threads by the batch's
//      largest graph), points and m in registers;
//   2  larger: one workgroup of 1024 that strides over the graph, m in the global
//      workspace (a thread reads back only what it wrote itself: no fence).
//
// radius is brute force inside a graph on purpose: "the first cap hits in index
// order" is the semantics.  One wave per query; its lanes test 64 consecutive
// candidates, the ballot is the hit mask, the popcount below a lane its slot, so
// the hits come out ascending without a sort, and the wave stops at the cap.  When
// the four queries of a workgroup search the same rows (the usual case: queries are
// sorted by graph) the workgroup stages tiles of 256 candidates in LDS and every
// wave tests from there.  Hits go to a slab of cap entries per query, the counts
// are scanned (rocPRIM, integers), the caller reads E and mp_radius_fill compacts
// the slab in order.  Against a count pass and a fill pass: those read every
// candidate twice (n_y * n_g * D * 4 bytes each, and the distance arithmetic with
// them), the slab costs at most 2 * E * 4 bytes more than the output itself.
//
// Nothing here adds floats atomically; the one atomic is the integer count of
// rejected starts.
#include <rocprim/device/device_scan.hpp>

#include "mp_workspace.h"

// thresholds between the fps paths (tools/ab_tune.py variants: make variant DEFS=-D...)
#ifndef MP_FPS_WAVE_LIMIT
#define MP_FPS_WAVE_LIMIT 256
#endif
#ifndef MP_FPS_BLOCK_LIMIT
#define MP_FPS_BLOCK_LIMIT 8192
#endif
// path 1's workgroup by the batch's largest graph: 256 threads up to MP_FPS_T256_LIMIT points,
// 512 up to MP_FPS_T512_LIMIT, else 1024 (fewer waves make the barrier cheaper, more points a
// thread make the update longer; measured)
#ifndef MP_FPS_T256_LIMIT
#define MP_FPS_T256_LIMIT 1024
#endif
#ifndef MP_FPS_T512_LIMIT
#define MP_FPS_T512_LIMIT 4096
#endif

namespace mp {

constexpr int kPointBlock = 256;
constexpr int kFpsWaveLimit = MP_FPS_WAVE_LIMIT;
constexpr int kFpsBlockLimit = MP_FPS_BLOCK_LIMIT;
constexpr int kFpsWavePpt = kFpsWaveLimit / 64;      // points a lane owns on path 0
constexpr int kFpsBlockPpt = kFpsBlockLimit / 1024;  // points a thread owns on path 1
constexpr int kFpsT256Limit = MP_FPS_T256_LIMIT;
constexpr int kFpsT512Limit = MP_FPS_T512_LIMIT;
constexpr int kPointMaxD = 8;
constexpr size_t kFpsOnChipWs = 256;
static_assert(kFpsWaveLimit % 64 == 0 && kFpsWaveLimit >= 64 && kFpsWaveLimit <= 512, "MP_FPS_WAVE_LIMIT");
static_assert(kFpsBlockLimit % 1024 == 0 && kFpsBlockLimit > kFpsWaveLimit && kFpsBlockLimit <= 16384,
              "MP_FPS_BLOCK_LIMIT");
static_assert(kFpsT256Limit >= 0 && kFpsT256Limit <= 256 * kFpsBlockPpt, "MP_FPS_T256_LIMIT");
static_assert(kFpsT512Limit >= kFpsT256Limit && kFpsT512Limit <= 512 * kFpsBlockPpt, "MP_FPS_T512_LIMIT");

// the squared distance of the header: every operation rounded (-ffp-contract=off), left to right
template <int D>
__device__ __forceinline__ float point_d2(const float (&a)[D], const float (&b)[D]) {
  float t = a[0] - b[0];
  float acc = t * t;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    t = a[d] - b[d];
    acc = acc + t * t;
  }
  return acc;
}

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}

// the maximum over each row of 16 lanes, in every lane of the row (all lanes active)
__device__ __forceinline__ uint64_t row_max64(uint64_t v) {
  v = umax64(v, dpp64<0xB1>(v));   // quad_perm(1,0,3,2)
  v = umax64(v, dpp64<0x4E>(v));   // quad_perm(2,3,0,1)
  v = umax64(v, dpp64<0x141>(v));  // row_half_mirror
  v = umax64(v, dpp64<0x140>(v));  // row_mirror
  return v;
}

// ... and over the wave
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
  v = row_max64(v);
  v = umax64(v, (uint64_t)__shfl_xor((unsigned long long)v, 16));
  v = umax64(v, (uint64_t)__shfl_xor((unsigned long long)v, 32));
  return v;
}

__device__ __forceinline__ uint64_t fps_word(float m, int local) {
  return ((uint64_t)__float_as_uint(m) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)local);
}

// the local index a word names, kept inside the graph whatever the word
__device__ __forceinline__ int fps_local(uint64_t word, int n_g) {
  const uint32_t l = 0xFFFFFFFFu - (uint32_t)word;
  return l < (uint32_t)n_g ? (int)l : 0;
}

// One graph's rows of pos and idx, every bound taken from device memory clamped:
// rows [s0, s0 + n_g) within [0, n), outputs [o0, o0 + k) within [0, idx_cap)
struct FpsGraph {
  int64_t s0, o0;
  int n_g, k, first;
  bool bad_start;
};

__device__ __forceinline__ FpsGraph fps_graph(const int64_t* __restrict__ starts,
                                              const int64_t* __restrict__ out_starts,
                                              const int64_t* __restrict__ start, int64_t g, int64_t n,
                                              int64_t idx_cap) {
  FpsGraph q;
  int64_t s0 = starts[g], s1 = starts[g + 1];
  s0 = s0 < 0 ? 0 : (s0 > n ? n : s0);
  s1 = s1 < s0 ? s0 : (s1 > n ? n : s1);
  int64_t o0 = out_starts[g], o1 = out_starts[g + 1];
  o0 = o0 < 0 ? 0 : (o0 > idx_cap ? idx_cap : o0);
  o1 = o1 < o0 ? o0 : (o1 > idx_cap ? idx_cap : o1);
  q.s0 = s0;
  q.o0 = o0;
  q.n_g = (int)(s1 - s0);  // n < 2^31
  q.k = (int)(o1 - o0);
  const int64_t f = start ? start[g] : 0;
  q.bad_start = q.n_g > 0 && (f < 0 || f >= q.n_g);
  q.first = q.bad_start || q.n_g == 0 ? 0 : (int)f;
  return q;
}

// ---- fps, path 0: one wave per graph ---------------------------------------------------------

template <int D>
__global__ __launch_bounds__(kPointBlock) void k_fps_wave(const float* __restrict__ pos, int64_t ldp, int64_t n,
                                                          const int64_t* __restrict__ starts, int64_t G,
                                                          const int64_t* __restrict__ out_starts,
                                                          const int64_t* __restrict__ start,
                                                          int64_t* __restrict__ idx, int64_t idx_cap,
                                                          unsigned long long* __restrict__ counts) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (g >= G) return;
  const FpsGraph q = fps_graph(starts, out_starts, start, g, n, idx_cap);
  if (q.n_g < 1 || q.n_g > kFpsWaveLimit) return;
  const int lane = lane_id();
  if (q.bad_start && lane == 0) atomicAdd(counts + 1, 1ull);
  if (q.k < 1) return;
  const int n_g = uni(q.n_g);
  float p[kFpsWavePpt][D], m[kFpsWavePpt];
#pragma unroll
  for (int s = 0; s < kFpsWavePpt; ++s) {
    const int i = s * 64 + lane;
    const float* row = pos + (q.s0 + (i < n_g ? i : 0)) * ldp;
#pragma unroll
    for (int d = 0; d < D; ++d) p[s][d] = row[d];
    m[s] = INFINITY;
  }
  int cur = uni(q.first);
  if (lane == 0) idx[q.o0] = q.s0 + cur;
  for (int t = 1; t < q.k; ++t) {
    // the selection's coordinates: its owner's registers, read by every lane
    const int slot = cur >> 6, owner = cur & 63;
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float v = p[0][d];
#pragma unroll
      for (int s = 1; s < kFpsWavePpt; ++s) v = slot == s ? p[s][d] : v;
      c[d] = readlane(v, owner);
    }
    uint64_t best = 0;
#pragma unroll
    for (int s = 0; s < kFpsWavePpt; ++s) {
      const int i = s * 64 + lane;
      if (s * 64 < n_g && i < n_g) {
        const float d2 = point_d2<D>(p[s], c);
        m[s] = d2 < m[s] ? d2 : m[s];
        best = umax64(best, fps_word(m[s], i));
      }
    }
    best = wave_max64(best);
    cur = uni(fps_local(best, n_g));
    if (lane == 0) idx[q.o0 + t] = q.s0 + cur;
  }
}

// ---- fps, paths 1 and 2: one workgroup per graph ------------------------------------------------

// The workgroup's maximum of the waves' words.  Every wave has left its word in
// skey[0 .. n_waves); n_waves is a power of two <= 16, so the 16 lanes of a DPP row
// read all of them between them.
__device__ __forceinline__ uint64_t fps_block_max(const uint64_t* skey, int n_waves) {
  return row_max64(skey[lane_id() & (n_waves - 1)]);
}

template <int D>
__global__ __launch_bounds__(1024) void k_fps_block(const float* __restrict__ pos, int64_t ldp, int64_t n,
                                                    const int64_t* __restrict__ starts,
                                                    const int64_t* __restrict__ out_starts,
                                                    const int64_t* __restrict__ start, int64_t* __restrict__ idx,
                                                    int64_t idx_cap, unsigned long long* __restrict__ counts) {
  __shared__ uint64_t skey[2][16];
  __shared__ float scoord[2][16][kPointMaxD];
  const FpsGraph q = fps_graph(starts, out_starts, start, blockIdx.x, n, idx_cap);
  const int T = blockDim.x, tid = threadIdx.x, wv = tid >> 6, n_waves = T >> 6;
  if (q.n_g <= kFpsWaveLimit || q.n_g > kFpsBlockLimit || q.n_g > T * kFpsBlockPpt) return;
  if (q.bad_start && tid == 0) atomicAdd(counts + 1, 1ull);
  if (q.k < 1) return;
  const int n_g = q.n_g;
  const int shift = __ffs(T) - 1;  // T is a power of two: point i is slot i >> shift of thread i & (T - 1)
  float p[kFpsBlockPpt][D], m[kFpsBlockPpt];
#pragma unroll
  for (int s = 0; s < kFpsBlockPpt; ++s) {
    const int i = s * T + tid;
    const float* row = pos + (q.s0 + (i < n_g ? i : 0)) * ldp;
#pragma unroll
    for (int d = 0; d < D; ++d) p[s][d] = row[d];
    m[s] = INFINITY;
  }
  int cur = q.first;
  float c[D];
#pragma unroll
  for (int d = 0; d < D; ++d) c[d] = pos[(q.s0 + cur) * ldp + d];
  if (tid == 0) idx[q.o0] = q.s0 + cur;
  for (int t = 1; t < q.k; ++t) {
    uint64_t best = 0;
#pragma unroll
    for (int s = 0; s < kFpsBlockPpt; ++s) {
      const int i = s * T + tid;
      if (s * T < n_g && i < n_g) {
        const float d2 = point_d2<D>(p[s], c);
        m[s] = d2 < m[s] ? d2 : m[s];
        best = umax64(best, fps_word(m[s], i));
      }
    }
    best = wave_max64(best);
    const int buf = t & 1;
    // the wave's winner belongs to one of its own threads: that thread leaves the word and its coordinates
    const int wl = fps_local(best, n_g);
    if (best != 0) {
      if ((wl & (T - 1)) == tid) {
        const int slot = wl >> shift;
        skey[buf][wv] = best;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          float v = p[0][d];
#pragma unroll
          for (int s = 1; s < kFpsBlockPpt; ++s) v = slot == s ? p[s][d] : v;
          scoord[buf][wv][d] = v;
        }
      }
    } else if ((tid & 63) == 0) {
      skey[buf][wv] = 0;  // a wave past the end of the graph
    }
    __syncthreads();
    cur = fps_local(fps_block_max(skey[buf], n_waves), n_g);
    const int ow = (cur & (T - 1)) >> 6;
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = scoord[buf][ow][d];
    if (tid == 0) idx[q.o0 + t] = q.s0 + cur;
  }
}

template <int D>
__global__ __launch_bounds__(1024) void k_fps_global(const float* __restrict__ pos, int64_t ldp, int64_t n,
                                                     const int64_t* __restrict__ starts,
                                                     const int64_t* __restrict__ out_starts,
                                                     const int64_t* __restrict__ start, float* __restrict__ mws,
                                                     int64_t* __restrict__ idx, int64_t idx_cap,
                                                     unsigned long long* __restrict__ counts) {
  __shared__ uint64_t skey[2][16];
  const FpsGraph q = fps_graph(starts, out_starts, start, blockIdx.x, n, idx_cap);
  const int T = blockDim.x, tid = threadIdx.x, wv = tid >> 6, n_waves = T >> 6;
  if (q.n_g <= kFpsBlockLimit) return;
  if (q.bad_start && tid == 0) atomicAdd(counts + 1, 1ull);
  if (q.k < 1) return;
  const int n_g = q.n_g;
  int cur = q.first;
  if (tid == 0) idx[q.o0] = q.s0 + cur;
  for (int t = 1; t < q.k; ++t) {
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = pos[(q.s0 + cur) * ldp + d];
    uint64_t best = 0;
    for (int i = tid; i < n_g; i += T) {
      float a[D];
#pragma unroll
      for (int d = 0; d < D; ++d) a[d] = pos[(q.s0 + i) * ldp + d];
      const float d2 = point_d2<D>(a, c);
      float mi = t == 1 ? INFINITY : mws[q.s0 + i];  // a thread reads back only its own stores
      mi = d2 < mi ? d2 : mi;
      mws[q.s0 + i] = mi;
      best = umax64(best, fps_word(mi, i));
    }
    best = wave_max64(best);
    const int buf = t & 1;
    if ((tid & 63) == 0) skey[buf][wv] = best;
    __syncthreads();
    cur = fps_local(fps_block_max(skey[buf], n_waves), n_g);
    if (tid == 0) idx[q.o0 + t] = q.s0 + cur;
  }
}

// mp_fps_f32's workspace on path 2: m of every point (the on-chip paths use none;
// the caller still passes kFpsOnChipWs bytes)
struct FpsWs : Carver {
  int64_t n;
  float* m = take<float>(n);
};

// ---- radius ------------------------------------------------------------------------------------

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// one tile of 64 candidates of a query's wave: hit = the lane's candidate lies within
// r2; returns true once the query holds cap hits
__device__ __forceinline__ bool radius_take(bool hit, int64_t cand, int cap, int32_t* __restrict__ mine, int& count) {
  const unsigned long long mask = __ballot(hit);
  if (hit) {
    const int slot = count + lanes_below(mask);
    if (slot < cap) mine[slot] = (int32_t)cand;
  }
  count += __popcll(mask);
  if (count >= cap) {
    count = cap;
    return true;
  }
  return false;
}

template <int D>
__global__ __launch_bounds__(kPointBlock) void k_radius_search(const float* __restrict__ x, int64_t ldx, int64_t n_x,
                                                               const float* __restrict__ y, int64_t ldy, int64_t n_y,
                                                               const int64_t* __restrict__ batch_y,
                                                               const int64_t* __restrict__ starts_x, int64_t G_x,
                                                               float r2, int cap, int64_t* __restrict__ cnt,
                                                               int32_t* __restrict__ slab) {
  __shared__ float tile[D][kPointBlock];
  __shared__ long long srange[2];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * (kPointBlock / 64) + wv;
  const bool live = j < n_y;
  int64_t c0 = 0, c1 = 0;
  float qy[D];
#pragma unroll
  for (int d = 0; d < D; ++d) qy[d] = 0.f;
  if (live) {
    const int64_t g = batch_y ? batch_y[j] : 0;
    if (g >= 0 && g < G_x) {
      c0 = starts_x[g];
      c1 = starts_x[g + 1];
      c0 = c0 < 0 ? 0 : (c0 > n_x ? n_x : c0);
      c1 = c1 < c0 ? c0 : (c1 > n_x ? n_x : c1);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) qy[d] = y[j * ldy + d];
  }
  if (threadIdx.x == 0) {
    srange[0] = c0;
    srange[1] = c1;
  }
  __syncthreads();
  const int64_t b0 = srange[0], b1 = srange[1];
  const int staged = __syncthreads_and(!live || (c0 == b0 && c1 == b1));
  int32_t* mine = slab + (live ? j : 0) * cap;
  int count = 0;
  bool done = !live || c0 >= c1;
  if (staged) {
    // every live query of the workgroup searches rows [b0, b1): tiles of 256 candidates through LDS
    for (int64_t base = b0; base < b1; base += kPointBlock) {
      if (__syncthreads_and(done)) break;  // also: everybody is through with the last tile
      const int64_t cl = base + threadIdx.x;
      if (cl < b1) {
#pragma unroll
        for (int d = 0; d < D; ++d) tile[d][threadIdx.x] = x[cl * ldx + d];
      }
      __syncthreads();
      if (!done) {
        for (int sub = 0; sub < kPointBlock / 64 && base + sub * 64 < b1; ++sub) {
          const int64_t cand = base + sub * 64 + lane;
          bool hit = false;
          if (cand < b1) {
            float a[D];
#pragma unroll
            for (int d = 0; d < D; ++d) a[d] = tile[d][sub * 64 + lane];
            hit = point_d2<D>(a, qy) <= r2;
          }
          if (radius_take(hit, cand, cap, mine, count)) {
            done = true;
            break;
          }
        }
      }
    }
  } else if (!done) {
    for (int64_t base = c0; base < c1; base += 64) {
      const int64_t cand = base + lane;
      bool hit = false;
      if (cand < c1) {
        float a[D];
#pragma unroll
        for (int d = 0; d < D; ++d) a[d] = x[cand * ldx + d];
        hit = point_d2<D>(a, qy) <= r2;
      }
      if (radius_take(hit, cand, cap, mine, count)) break;
    }
  }
  if (live && lane == 0) cnt[j] = count;
}

// one thread per slab entry: entry s of query j goes to position off[j] + s
__global__ __launch_bounds__(kPointBlock) void k_radius_fill(const int64_t* __restrict__ cnt,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ slab, int64_t n_y, int cap,
                                                             int64_t n_edges, int64_t* __restrict__ out_y,
                                                             int64_t* __restrict__ out_x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_y * cap) return;
  const int64_t j = t / cap, s = t - j * cap;
  if (s >= cnt[j]) return;
  const int64_t o = off[j] + s;
  if (o < 0 || o >= n_edges) return;  // never for counts this unit wrote; keeps any store inside the output
  out_y[o] = j;
  out_x[o] = slab[t];
}

__global__ void k_radius_total(const int64_t* __restrict__ off, int64_t n_y, int64_t* __restrict__ counts) {
  counts[0] = off[n_y];
}

// the hit counts (one more entry, 0, so that the exclusive scan ends with E), their
// scan, the slab of cap candidates per query; then the scan's temp
struct RadiusWs : Carver {
  int64_t n_y, cap;
  int64_t* cnt = take<int64_t>(n_y + 1);
  int64_t* off = take<int64_t>(n_y + 1);
  int32_t* slab = take<int32_t>(n_y * cap);
};

static inline hipError_t radius_scan_bytes(int64_t n_y, size_t* bytes) {
  return rocprim::exclusive_scan((void*)nullptr, *bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0,
                                 (size_t)(n_y + 1), rocprim::plus<int64_t>(), (hipStream_t)0, false);
}

// ---- edge features -------------------------------------------------------------------------------

// A lane group per edge; its units are the FE fragments of VEC features of the x row,
// then the D coordinate differences.  ALIGNED: out rows take vector stores.
template <int VEC, bool ALIGNED>
__global__ __launch_bounds__(kPointBlock) void k_point_edge_features(
    const float* __restrict__ x_src, int64_t ldx, int FE, const float* __restrict__ pos_src, int64_t ldps,
    int64_t n_src, const float* __restrict__ pos_dst, int64_t ldpd, int64_t n_dst, int D,
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t n_edges, int gl,
    float* __restrict__ out, int64_t ldo) {
  const int lane = lane_id();
  const int64_t e = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  if (e >= n_edges) return;
  const int64_t s = src[e], t = dst[e];
  const bool ok = s >= 0 && s < n_src && t >= 0 && t < n_dst;
  float* row = out + e * ldo;
  for (int u = sub; u < FE + D; u += gl) {
    if (u < FE) {
      Frag<VEC> v;
      if (ok) {
        v = load_frag<VEC>(x_src + s * ldx + (int64_t)u * VEC);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v.v[k] = 0.f;
      }
      if constexpr (ALIGNED) {
        store_frag<VEC>(row + (int64_t)u * VEC, v);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) row[(int64_t)u * VEC + k] = v.v[k];
      }
    } else {
      const int d = u - FE;
      row[(int64_t)FE * VEC + d] = ok ? pos_src[s * ldps + d] - pos_dst[t * ldpd + d] : 0.f;
    }
  }
}

// run `call` with D as a template argument
#define POINT_FOR_D(D, call) \
  switch (D) {               \
    case 1: { constexpr int kD = 1; call; } break; \
    case 2: { constexpr int kD = 2; call; } break; \
    case 3: { constexpr int kD = 3; call; } break; \
    case 4: { constexpr int kD = 4; call; } break; \
    case 5: { constexpr int kD = 5; call; } break; \
    case 6: { constexpr int kD = 6; call; } break; \
    case 7: { constexpr int kD = 7; call; } break; \
    default: { constexpr int kD = 8; call; } break; \
  }

// the entry points return the launches enqueued, or -(code); see the header
#define POINT_CHECK_ARG(cond, ...)     \
  do {                                 \
    if (!(cond)) {                     \
      ::mp::set_error(__VA_ARGS__);    \
      return -(int64_t)MP_ERR_ARG;     \
    }                                  \
  } while (0)

#define POINT_CHECK_EXTENT(fn, name, have, need)                                                  \
  POINT_CHECK_ARG((size_t)(have) >= (size_t)(need), "%s: %s holds %zu bytes, the call needs %zu", \
                  fn, name, (size_t)(have), (size_t)(need))

#define POINT_CHECK_HIP(expr)                                                \
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

int64_t mp_fps_path(int64_t n_g) {
  if (n_g <= kFpsWaveLimit) return 0;
  return n_g <= kFpsBlockLimit ? 1 : 2;
}

size_t mp_fps_workspace(int64_t n, int64_t max_n) {
  if (max_n <= kFpsBlockLimit) return kFpsOnChipWs;
  return FpsWs{nullptr, n}.off;
}

int64_t mp_fps_f32(const float* pos, int64_t ldp, int64_t n, int32_t D, const int64_t* starts, int64_t n_graphs,
                   int64_t max_n, const int64_t* out_starts, const int64_t* start, int64_t* idx, size_t idx_bytes,
                   int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  POINT_CHECK_ARG(n >= 0 && n < (int64_t)INT32_MAX, "mp_fps_f32: n = %lld is negative or not below 2^31", (long long)n);
  POINT_CHECK_ARG(D >= 1 && D <= kPointMaxD, "mp_fps_f32: D = %d is outside [1, 8]", D);
  POINT_CHECK_ARG(ldp >= D, "mp_fps_f32: ldp = %lld < D = %d", (long long)ldp, D);
  POINT_CHECK_ARG(n_graphs >= 0 && n_graphs < (int64_t)INT32_MAX,
                  "mp_fps_f32: n_graphs = %lld is negative or not below 2^31", (long long)n_graphs);
  POINT_CHECK_ARG(n == 0 || n_graphs > 0, "mp_fps_f32: %lld points but n_graphs = 0", (long long)n);
  POINT_CHECK_ARG(max_n >= 0 && max_n <= n, "mp_fps_f32: max_n = %lld is outside [0, n]", (long long)max_n);
  POINT_CHECK_ARG(starts, "mp_fps_f32: starts is NULL");
  POINT_CHECK_ARG(out_starts, "mp_fps_f32: out_starts is NULL");
  POINT_CHECK_ARG(counts, "mp_fps_f32: counts is NULL");
  POINT_CHECK_ARG(ws, "mp_fps_f32: ws is NULL");
  POINT_CHECK_ARG(n == 0 || pos, "mp_fps_f32: pos is NULL");
  POINT_CHECK_ARG(n == 0 || idx, "mp_fps_f32: idx is NULL");
  POINT_CHECK_EXTENT("mp_fps_f32", "counts", counts_bytes, 4 * sizeof(int64_t));
  const bool global = max_n > kFpsBlockLimit;
  const FpsWs w{ws, n};
  POINT_CHECK_EXTENT("mp_fps_f32", "ws", ws_bytes, global ? w.off : kFpsOnChipWs);
  hipStream_t s = as_stream(stream);
  POINT_CHECK_HIP(hipMemsetAsync(counts + 1, 0, sizeof(int64_t), s));
  if (n == 0 || n_graphs == 0) return 0;
  const int64_t idx_cap = (int64_t)(idx_bytes / sizeof(int64_t));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  POINT_FOR_D(D, (k_fps_wave<kD><<<(unsigned)ceil_div(n_graphs, kPointBlock / 64), kPointBlock, 0, s>>>(
                     pos, ldp, n, starts, n_graphs, out_starts, start, idx, idx_cap, cnt)));
  POINT_CHECK_HIP(hipGetLastError());
  int64_t launches = 1;
  if (max_n > kFpsWaveLimit) {
    const int T = max_n <= kFpsT256Limit ? 256 : (max_n <= kFpsT512Limit ? 512 : 1024);
    POINT_FOR_D(D, (k_fps_block<kD><<<(unsigned)n_graphs, T, 0, s>>>(pos, ldp, n, starts, out_starts, start, idx,
                                                                     idx_cap, cnt)));
    POINT_CHECK_HIP(hipGetLastError());
    ++launches;
  }
  if (global) {
    POINT_FOR_D(D, (k_fps_global<kD><<<(unsigned)n_graphs, 1024, 0, s>>>(pos, ldp, n, starts, out_starts, start, w.m,
                                                                         idx, idx_cap, cnt)));
    POINT_CHECK_HIP(hipGetLastError());
    ++launches;
  }
  return launches;
}

size_t mp_radius_workspace(int64_t n_y, int64_t cap) {
  size_t scan = 0;
  (void)radius_scan_bytes(n_y > 0 ? n_y : 0, &scan);
  return RadiusWs{nullptr, n_y, cap}.total(scan);
}

int64_t mp_radius_search_f32(const float* x, int64_t ldx, int64_t n_x, const float* y, int64_t ldy, int64_t n_y,
                             int32_t D, const int64_t* batch_y, const int64_t* starts_x, int64_t n_graphs_x, float r,
                             int64_t cap, int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes,
                             void* stream) {
  MP_DEVICE_GUARD(stream);
  POINT_CHECK_ARG(n_x >= 0 && n_x < (int64_t)INT32_MAX,
                  "mp_radius_search_f32: n_x = %lld is negative or not below 2^31", (long long)n_x);
  POINT_CHECK_ARG(n_y >= 0 && n_y < (int64_t)INT32_MAX,
                  "mp_radius_search_f32: n_y = %lld is negative or not below 2^31", (long long)n_y);
  POINT_CHECK_ARG(D >= 1 && D <= kPointMaxD, "mp_radius_search_f32: D = %d is outside [1, 8]", D);
  POINT_CHECK_ARG(ldx >= D, "mp_radius_search_f32: ldx = %lld < D = %d", (long long)ldx, D);
  POINT_CHECK_ARG(ldy >= D, "mp_radius_search_f32: ldy = %lld < D = %d", (long long)ldy, D);
  POINT_CHECK_ARG(n_graphs_x >= 0 && n_graphs_x < (int64_t)INT32_MAX,
                  "mp_radius_search_f32: n_graphs_x = %lld is negative or not below 2^31", (long long)n_graphs_x);
  POINT_CHECK_ARG(r >= 0.f && r <= 3.4028234663852886e38f, "mp_radius_search_f32: r = %g is negative or not finite",
                  (double)r);
  POINT_CHECK_ARG(cap >= 1 && cap < (int64_t)INT32_MAX, "mp_radius_search_f32: cap = %lld is outside [1, 2^31)",
                  (long long)cap);
  POINT_CHECK_ARG(n_y == 0 || cap < (int64_t)INT32_MAX / n_y,
                  "mp_radius_search_f32: n_y * cap = %lld * %lld is not below 2^31", (long long)n_y, (long long)cap);
  POINT_CHECK_ARG(starts_x, "mp_radius_search_f32: starts_x is NULL");
  POINT_CHECK_ARG(counts, "mp_radius_search_f32: counts is NULL");
  POINT_CHECK_ARG(ws, "mp_radius_search_f32: ws is NULL");
  POINT_CHECK_ARG(n_x == 0 || x, "mp_radius_search_f32: x is NULL");
  POINT_CHECK_ARG(n_y == 0 || y, "mp_radius_search_f32: y is NULL");
  POINT_CHECK_EXTENT("mp_radius_search_f32", "counts", counts_bytes, 4 * sizeof(int64_t));
  const RadiusWs w{ws, n_y, cap};
  POINT_CHECK_EXTENT("mp_radius_search_f32", "ws", ws_bytes, w.total(0));
  size_t scan = 0;
  const hipError_t size_query = radius_scan_bytes(n_y, &scan);
  POINT_CHECK_EXTENT("mp_radius_search_f32", "ws", ws_bytes, w.total(scan));
  POINT_CHECK_HIP(size_query);
  hipStream_t s = as_stream(stream);
  POINT_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t), s));
  if (n_y == 0) return 0;
  POINT_CHECK_HIP(hipMemsetAsync(w.cnt + n_y, 0, sizeof(int64_t), s));
  const float r2 = r * r;
  POINT_FOR_D(D, (k_radius_search<kD><<<(unsigned)ceil_div(n_y, kPointBlock / 64), kPointBlock, 0, s>>>(
                     x, ldx, n_x, y, ldy, n_y, batch_y, starts_x, n_graphs_x, r2, (int)cap, w.cnt, w.slab)));
  POINT_CHECK_HIP(hipGetLastError());
  POINT_CHECK_HIP(rocprim::exclusive_scan(w.rest(), scan, (const int64_t*)w.cnt, w.off, (int64_t)0, (size_t)(n_y + 1),
                                          rocprim::plus<int64_t>(), s, false));
  k_radius_total<<<1, 1, 0, s>>>(w.off, n_y, counts);
  POINT_CHECK_HIP(hipGetLastError());
  return 2;  // the search and the total; the scan's launches are rocPRIM's
}

int64_t mp_radius_fill(int64_t n_y, int64_t cap, int64_t n_edges, int64_t* out_y, int64_t* out_x, size_t out_bytes,
                       void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  POINT_CHECK_ARG(n_y >= 0 && n_y < (int64_t)INT32_MAX, "mp_radius_fill: n_y = %lld is negative or not below 2^31",
                  (long long)n_y);
  POINT_CHECK_ARG(cap >= 1 && cap < (int64_t)INT32_MAX, "mp_radius_fill: cap = %lld is outside [1, 2^31)",
                  (long long)cap);
  POINT_CHECK_ARG(n_y == 0 || cap < (int64_t)INT32_MAX / n_y,
                  "mp_radius_fill: n_y * cap = %lld * %lld is not below 2^31", (long long)n_y, (long long)cap);
  POINT_CHECK_ARG(n_edges >= 0 && n_edges <= n_y * cap, "mp_radius_fill: n_edges = %lld is outside [0, n_y * cap]",
                  (long long)n_edges);
  POINT_CHECK_ARG(ws, "mp_radius_fill: ws is NULL");
  POINT_CHECK_ARG(n_edges == 0 || out_y, "mp_radius_fill: out_y is NULL");
  POINT_CHECK_ARG(n_edges == 0 || out_x, "mp_radius_fill: out_x is NULL");
  POINT_CHECK_EXTENT("mp_radius_fill", "out_y / out_x", out_bytes, (size_t)n_edges * sizeof(int64_t));
  const RadiusWs w{ws, n_y, cap};
  POINT_CHECK_EXTENT("mp_radius_fill", "ws", ws_bytes, w.total(0));
  if (n_edges == 0) return 0;
  k_radius_fill<<<(unsigned)ceil_div(n_y * cap, kPointBlock), kPointBlock, 0, as_stream(stream)>>>(
      w.cnt, w.off, w.slab, n_y, (int)cap, n_edges, out_y, out_x);
  POINT_CHECK_HIP(hipGetLastError());
  return 1;
}

int64_t mp_point_edge_features_f32(const float* x_src, int64_t ldx, int32_t F, const float* pos_src, int64_t ldps,
                                   int64_t n_src, const float* pos_dst, int64_t ldpd, int64_t n_dst, int32_t D,
                                   const int64_t* src, const int64_t* dst, int64_t n_edges, float* out, int64_t ldo,
                                   size_t out_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  POINT_CHECK_ARG(n_edges >= 0 && n_edges < (int64_t)INT32_MAX,
                  "mp_point_edge_features_f32: n_edges = %lld is negative or not below 2^31", (long long)n_edges);
  POINT_CHECK_ARG(n_src >= 0 && n_src < (int64_t)INT32_MAX,
                  "mp_point_edge_features_f32: n_src = %lld is negative or not below 2^31", (long long)n_src);
  POINT_CHECK_ARG(n_dst >= 0 && n_dst < (int64_t)INT32_MAX,
                  "mp_point_edge_features_f32: n_dst = %lld is negative or not below 2^31", (long long)n_dst);
  POINT_CHECK_ARG(F >= 0, "mp_point_edge_features_f32: F = %d", F);
  POINT_CHECK_ARG(D >= 1 && D <= kPointMaxD, "mp_point_edge_features_f32: D = %d is outside [1, 8]", D);
  POINT_CHECK_ARG(F == 0 || ldx >= F, "mp_point_edge_features_f32: ldx = %lld < F = %d", (long long)ldx, F);
  POINT_CHECK_ARG(ldps >= D, "mp_point_edge_features_f32: ldps = %lld < D = %d", (long long)ldps, D);
  POINT_CHECK_ARG(ldpd >= D, "mp_point_edge_features_f32: ldpd = %lld < D = %d", (long long)ldpd, D);
  POINT_CHECK_ARG(ldo >= (int64_t)F + D, "mp_point_edge_features_f32: ldo = %lld < F + D = %d", (long long)ldo, F + D);
  if (n_edges == 0) return 0;
  POINT_CHECK_ARG(F == 0 || n_src == 0 || x_src, "mp_point_edge_features_f32: x_src is NULL");
  POINT_CHECK_ARG(n_src == 0 || pos_src, "mp_point_edge_features_f32: pos_src is NULL");
  POINT_CHECK_ARG(n_dst == 0 || pos_dst, "mp_point_edge_features_f32: pos_dst is NULL");
  POINT_CHECK_ARG(src, "mp_point_edge_features_f32: src is NULL");
  POINT_CHECK_ARG(dst, "mp_point_edge_features_f32: dst is NULL");
  POINT_CHECK_ARG(out, "mp_point_edge_features_f32: out is NULL");
  POINT_CHECK_EXTENT("mp_point_edge_features_f32", "out", out_bytes,
                     ((size_t)(n_edges - 1) * (size_t)ldo + (size_t)(F + D)) * sizeof(float));
  hipStream_t s = as_stream(stream);
  const bool vec4 = F > 0 && F % 4 == 0 && ldx % 4 == 0 && (uintptr_t)x_src % 16 == 0;
  const int FE = vec4 ? F / 4 : F;
  const int gl = group_lanes(FE + D);
  const unsigned blocks = (unsigned)ceil_div(ceil_div(n_edges, 64 / gl), kPointBlock / 64);
#define POINT_EF(VEC, ALIGNED)                                                                                    \
  k_point_edge_features<VEC, ALIGNED><<<blocks, kPointBlock, 0, s>>>(x_src, ldx, FE, pos_src, ldps, n_src, pos_dst, \
                                                                     ldpd, n_dst, D, src, dst, n_edges, gl, out, ldo)
  if (!vec4) {
    POINT_EF(1, true);
  } else if (ldo % 4 == 0 && (uintptr_t)out % 16 == 0) {
    POINT_EF(4, true);
  } else {
    POINT_EF(4, false);
  }
#undef POINT_EF
  POINT_CHECK_HIP(hipGetLastError());
  return 1;
}

}  // extern "C"
