// k nearest neighbours on the device (include/mi355_mp.h "Nearest neighbours"):
// the search behind knn / knn_graph / nearest and the inverse-distance
// interpolation of knn_interpolate -- the other half of torch_cluster 1.5 /
// PyG 1.4.3's point-set functions (nn.knn, nn.knn_graph, nn.nearest,
// nn.unpool.knn_interpolate [U]); mp_point.hip holds fps and radius.
//
// Like radius the search is brute force inside a graph, one wave per query, its
// lanes testing 64 consecutive candidates.  radius keeps the first cap hits in
// index order (a ballot and a popcount); knn keeps the k best, an ordered
// selection that lives across the wave: lane l holds the l-th smallest key found
// so far.  A key is ONE unsigned 64-bit word, (bits(d2) << 32) | in-graph index:
// d2 >= +0, so its fp32 bits order as an integer, and equal distances go to the
// lower index (fps's trick, here as a minimum).  Empty slots hold ~0, which no
// candidate's key reaches (its index is below 2^31).  A candidate survives when its
// key is below the current k-th key; the ballot gives the survivors, and each is
// inserted by one wave shift of the keys above it: pos = the number of keys below
// the newcomer (keys are distinct, so that is a popcount of a ballot), lanes above
// pos take their lower neighbour's key.  After every insertion the survivors are
// balloted again against the new k-th key, so a tile costs as many shifts as it
// really improves the selection: about k * ln(n / k) in all on random input, n when
// the candidates arrive in descending distance.
//
// Two paths by width (mp_knn_path):
//   0  D <= 8, a template: query and candidate in registers.  When the four queries
//      of a workgroup search the same rows (the usual case: queries are sorted by
//      graph) tiles of 256 candidates are staged in LDS between two barriers, as in
//      the radius kernel; otherwise a wave reads its candidates directly.
//   1  D <= MP_KNN_MAX_D: the query rows in LDS; candidates come through LDS in tiles of
//      256 rows x 32 columns when the workgroup's queries search the same rows, a lane
//      keeping its candidates' running sums across the column chunks (still left to
//      right), otherwise every lane walks its candidate's row from memory.  A
//      correctness path: no performance bar.
//
// The selection goes to a slab of k (index, d2) pairs per query with a count;
// the counts are scanned (rocPRIM, integers) and mp_knn_fill compacts the slab to
// [2, E] in order, optionally with the normalised interpolation weight of every
// pair.  mp_knn_interpolate_f32 runs straight from the slab and never needs E.
//
// Nothing here adds floats atomically, and there is no atomic at all.
#include <rocprim/device/device_scan.hpp>

#include "mp_workspace.h"

// the widest row the general path takes (a build knob: make variant DEFS=-DMP_KNN_MAX_D=...)
#ifndef MP_KNN_MAX_D
#define MP_KNN_MAX_D 256
#endif

namespace mp {

constexpr int kKnnBlock = 256;
constexpr int kKnnWaves = kKnnBlock / 64;
constexpr int kKnnMaxK = 64;  // one slot per lane
constexpr int kKnnRegD = 8;   // path 0: the widths that are template arguments
constexpr int kKnnChunk = 32;  // path 1: columns of a candidate tile in LDS
constexpr int kKnnMaxD = MP_KNN_MAX_D;
constexpr uint64_t kKnnEmpty = ~0ull;
constexpr float kKnnClamp = 1e-16f;  // upstream's clamp(min=1e-16) of the squared distance
static_assert(kKnnMaxD >= 256 && kKnnMaxD <= 2048, "MP_KNN_MAX_D");  // path 1 keeps 4 query rows in static LDS
static_assert(kKnnChunk == 32, "a chunk of the query is half a wave's registers; the tile's padding assumes 32");

// the squared distance of the header: every operation rounded (-ffp-contract=off), left to right
template <int D>
__device__ __forceinline__ float knn_d2(const float (&a)[D], const float (&b)[D]) {
  float t = a[0] - b[0];
  float acc = t * t;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    t = a[d] - b[d];
    acc = acc + t * t;
  }
  return acc;
}

__device__ __forceinline__ uint64_t knn_readlane64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t knn_key(float d2, int64_t local) {
  return ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)(uint32_t)local;
}

// One tile of 64 candidates of a query's wave (all 64 lanes active).  key: lane l's
// slot of the selection, ascending; kth: slot k - 1, the key a candidate has to beat.
__device__ __forceinline__ void knn_take(bool valid, uint64_t ckey, int k, uint64_t& key, uint64_t& kth) {
  const int lane = lane_id();
  bool pending = valid;
  for (;;) {
    const unsigned long long mask = __ballot(pending && ckey < kth);
    if (!mask) break;
    const int s = uni(__ffsll(mask) - 1);
    const uint64_t ck = knn_readlane64(ckey, s);
    const int pos = __popcll(__ballot(key < ck));  // the keys are distinct and ascending: a prefix of the lanes
    const uint64_t up = (uint64_t)__shfl_up((unsigned long long)key, 1);
    key = lane < pos ? key : (lane == pos ? ck : up);
    kth = knn_readlane64(key, k - 1);
    if (lane == s) pending = false;
  }
}

// rows [c0, c1) of x that query j searches, every bound taken from device memory clamped
__device__ __forceinline__ void knn_range(const int64_t* __restrict__ batch_y, const int64_t* __restrict__ starts_x,
                                          int64_t G_x, int64_t n_x, int64_t j, int64_t& c0, int64_t& c1) {
  c0 = c1 = 0;
  const int64_t g = batch_y ? batch_y[j] : 0;
  if (g >= 0 && g < G_x) {
    c0 = starts_x[g];
    c1 = starts_x[g + 1];
    c0 = c0 < 0 ? 0 : (c0 > n_x ? n_x : c0);
    c1 = c1 < c0 ? c0 : (c1 > n_x ? n_x : c1);
  }
}

// the wave's selection to the slab: min(k, n_g) pairs in ascending key
__device__ __forceinline__ void knn_store(int64_t j, int k, uint64_t key, int64_t c0, int64_t c1,
                                          int64_t* __restrict__ cnt, int32_t* __restrict__ slab_i,
                                          float* __restrict__ slab_d) {
  const int lane = lane_id();
  const int64_t n_g = c1 - c0;  // n_x < 2^31
  const int count = n_g < k ? (int)n_g : k;
  if (lane < count) {
    uint32_t local = (uint32_t)key;
    local = (int64_t)local < n_g ? local : 0u;  // never for a key this unit made; keeps the index inside the graph
    slab_i[j * k + lane] = (int32_t)(c0 + local);
    slab_d[j * k + lane] = __uint_as_float((uint32_t)(key >> 32));
  }
  if (lane == 0) cnt[j] = count;
}

// ---- path 0: D <= 8 ------------------------------------------------------------------------------

template <int D>
__global__ __launch_bounds__(kKnnBlock) void k_knn_search(const float* __restrict__ x, int64_t ldx, int64_t n_x,
                                                          const float* __restrict__ y, int64_t ldy, int64_t n_y,
                                                          const int64_t* __restrict__ batch_y,
                                                          const int64_t* __restrict__ starts_x, int64_t G_x, int k,
                                                          int64_t* __restrict__ cnt, int32_t* __restrict__ slab_i,
                                                          float* __restrict__ slab_d) {
  __shared__ float tile[D][kKnnBlock];
  __shared__ long long srange[2];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kKnnWaves + wv;
  const bool live = j < n_y;
  int64_t c0 = 0, c1 = 0;
  float qy[D];
#pragma unroll
  for (int d = 0; d < D; ++d) qy[d] = 0.f;
  if (live) {
    knn_range(batch_y, starts_x, G_x, n_x, j, c0, c1);
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
  uint64_t key = kKnnEmpty, kth = kKnnEmpty;
  if (staged) {
    // every live query of the workgroup searches rows [b0, b1): tiles of 256 candidates through LDS
    for (int64_t base = b0; base < b1; base += kKnnBlock) {
      if (base != b0) __syncthreads();  // everybody is through with the last tile
      const int64_t cl = base + threadIdx.x;
      if (cl < b1) {
#pragma unroll
        for (int d = 0; d < D; ++d) tile[d][threadIdx.x] = x[cl * ldx + d];
      }
      __syncthreads();
      if (live) {
        for (int sub = 0; sub < kKnnWaves && base + sub * 64 < b1; ++sub) {
          const int64_t cand = base + sub * 64 + lane;
          const bool valid = cand < b1;
          float a[D];
#pragma unroll
          for (int d = 0; d < D; ++d) a[d] = tile[d][sub * 64 + lane];  // past b1: stale, and not valid
          knn_take(valid, knn_key(knn_d2<D>(a, qy), cand - b0), k, key, kth);
        }
      }
    }
  } else if (live) {
    for (int64_t base = c0; base < c1; base += 64) {
      const int64_t cand = base + lane;
      const bool valid = cand < c1;
      float a[D];
#pragma unroll
      for (int d = 0; d < D; ++d) a[d] = valid ? x[cand * ldx + d] : 0.f;
      knn_take(valid, knn_key(knn_d2<D>(a, qy), cand - c0), k, key, kth);
    }
  }
  if (live) knn_store(j, k, key, c0, c1, cnt, slab_i, slab_d);
}

// ---- path 1: D <= MP_KNN_MAX_D ---------------------------------------------------------------------

// The query rows of the workgroup's four waves sit in LDS.  When the four search the
// same rows, tiles of 256 candidates x kKnnChunk columns go through LDS between two
// barriers (rows padded to kKnnChunk + 1 floats: lane l reads row l, 33 l mod 64 are
// distinct banks); a lane keeps the running sum of each of its four candidates across
// the chunks, so every distance is still summed left to right, and the chunk of the
// query a wave needs is one register, lane c holding column c, read with readlane.
// acc starts at +0: 0 + t * t is t * t bit for bit (t * t is never -0), and the padding
// columns past D add (0 - 0)^2 = +0.  Otherwise every lane walks its candidate's row
// from memory.
__global__ __launch_bounds__(kKnnBlock) void k_knn_search_wide(const float* __restrict__ x, int64_t ldx, int64_t n_x,
                                                               const float* __restrict__ y, int64_t ldy, int64_t n_y,
                                                               int D, const int64_t* __restrict__ batch_y,
                                                               const int64_t* __restrict__ starts_x, int64_t G_x,
                                                               int k, int64_t* __restrict__ cnt,
                                                               int32_t* __restrict__ slab_i,
                                                               float* __restrict__ slab_d) {
  __shared__ float sq[kKnnWaves][kKnnMaxD];
  __shared__ float tile[kKnnBlock][kKnnChunk + 1];
  __shared__ long long srange[2];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kKnnWaves + wv;
  const bool live = j < n_y;
  int64_t c0 = 0, c1 = 0;
  if (live) {
    knn_range(batch_y, starts_x, G_x, n_x, j, c0, c1);
    for (int d = lane; d < D; d += 64) sq[wv][d] = y[j * ldy + d];
  }
  if (threadIdx.x == 0) {
    srange[0] = c0;
    srange[1] = c1;
  }
  __syncthreads();
  const int64_t b0 = srange[0], b1 = srange[1];
  const int staged = __syncthreads_and(!live || (c0 == b0 && c1 == b1));
  const float* q = sq[wv];
  uint64_t key = kKnnEmpty, kth = kKnnEmpty;
  if (staged) {
    for (int64_t base = b0; base < b1; base += kKnnBlock) {
      float acc[kKnnWaves];
#pragma unroll
      for (int sub = 0; sub < kKnnWaves; ++sub) acc[sub] = 0.f;
      for (int dc = 0; dc < D; dc += kKnnChunk) {
        __syncthreads();  // everybody is through with the last chunk
        for (int e = threadIdx.x; e < kKnnBlock * kKnnChunk; e += kKnnBlock) {
          const int r = e / kKnnChunk, c = e % kKnnChunk;
          const int64_t cl = base + r;
          if (cl < b1) tile[r][c] = dc + c < D ? x[cl * ldx + dc + c] : 0.f;
        }
        __syncthreads();
        if (live) {
          const int qc = dc + (lane & (kKnnChunk - 1));
          const float qv = qc < D ? q[qc] : 0.f;
#pragma unroll
          for (int sub = 0; sub < kKnnWaves; ++sub) {
            if (base + sub * 64 < b1) {
              const float* row = tile[sub * 64 + lane];  // past b1: stale, and not valid
#pragma unroll
              for (int c = 0; c < kKnnChunk; ++c) {
                const float t = row[c] - readlane(qv, c);
                acc[sub] = acc[sub] + t * t;
              }
            }
          }
        }
      }
      if (live) {
#pragma unroll
        for (int sub = 0; sub < kKnnWaves; ++sub) {
          if (base + sub * 64 < b1) {
            const int64_t cand = base + sub * 64 + lane;
            knn_take(cand < b1, knn_key(acc[sub], cand - b0), k, key, kth);
          }
        }
      }
    }
  } else if (live) {
    for (int64_t base = c0; base < c1; base += 64) {
      const int64_t cand = base + lane;
      const bool valid = cand < c1;
      const float* row = x + (valid ? cand : c0) * ldx;
      float t = row[0] - q[0];
      float acc = t * t;
      for (int d = 1; d < D; ++d) {
        t = row[d] - q[d];
        acc = acc + t * t;
      }
      knn_take(valid, knn_key(acc, cand - c0), k, key, kth);
    }
  }
  if (live) knn_store(j, k, key, c0, c1, cnt, slab_i, slab_d);
}

// ---- the slab to [2, E] ----------------------------------------------------------------------------

__device__ __forceinline__ float knn_weight(float d2) { return 1.f / fmaxf(d2, kKnnClamp); }

// one thread per slab entry: entry s of query j goes to position off[j] + s; out_w (or NULL): w_s / W_j,
// W_j = the weights of query j summed in slab order
__global__ __launch_bounds__(kKnnBlock) void k_knn_fill(const int64_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ slab_i,
                                                        const float* __restrict__ slab_d, int64_t n_y, int k,
                                                        int64_t n_edges, int64_t* __restrict__ out_y,
                                                        int64_t* __restrict__ out_x, float* __restrict__ out_w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_y * k) return;
  const int64_t j = t / k, s = t - j * k;
  int64_t c = cnt[j];
  c = c < 0 ? 0 : (c > k ? k : c);
  if (s >= c) return;
  const int64_t o = off[j] + s;
  if (o < 0 || o >= n_edges) return;  // never for counts this unit wrote; keeps any store inside the output
  out_y[o] = j;
  out_x[o] = slab_i[t];
  if (out_w) {
    float W = 0.f;
    for (int64_t u = 0; u < c; ++u) W = W + knn_weight(slab_d[j * k + u]);
    out_w[o] = knn_weight(slab_d[t]) / W;
  }
}

__global__ void k_knn_total(const int64_t* __restrict__ off, int64_t n_y, int64_t* __restrict__ counts) {
  counts[0] = off[n_y];
}

// ---- interpolation from the slab -------------------------------------------------------------------

// A lane group per row of y; its units are the FE fragments of VEC features.  Both sums
// run over the slab's entries in order, every operation rounded.
template <int VEC>
__global__ __launch_bounds__(kKnnBlock) void k_knn_interpolate(const float* __restrict__ x, int64_t ldx, int64_t n_x,
                                                               int FE, int64_t n_y, int k,
                                                               const int64_t* __restrict__ cnt,
                                                               const int32_t* __restrict__ slab_i,
                                                               const float* __restrict__ slab_d, int gl,
                                                               float* __restrict__ out, int64_t ldo) {
  const int lane = lane_id();
  const int64_t j = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * (64 / gl) + lane / gl;
  const int sub = lane & (gl - 1);
  if (j >= n_y) return;
  int64_t c = cnt[j];
  c = c < 0 ? 0 : (c > k ? k : c);
  const int32_t* idx = slab_i + j * k;
  const float* dd = slab_d + j * k;
  float* row = out + j * ldo;
  for (int u = sub; u < FE; u += gl) {
    Frag<VEC> num;
#pragma unroll
    for (int v = 0; v < VEC; ++v) num.v[v] = 0.f;
    float W = 0.f;
    for (int t = 0; t < (int)c; ++t) {
      const float w = knn_weight(dd[t]);
      const int64_t i = idx[t];
      W = W + w;
      if (i < 0 || i >= n_x) continue;  // never for a slab this unit wrote
      const Frag<VEC> xv = load_frag<VEC>(x + i * ldx + (int64_t)u * VEC);
#pragma unroll
      for (int v = 0; v < VEC; ++v) num.v[v] = num.v[v] + w * xv.v[v];
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) num.v[v] = c > 0 ? num.v[v] / W : 0.f;  // a graph without x: zeros
    store_frag<VEC>(row + (int64_t)u * VEC, num);
  }
}

// the selection counts (one more entry, 0, so that the exclusive scan ends with E), their
// scan, the slab of k (index, d2) pairs per query; then the scan's temp
struct KnnWs : Carver {
  int64_t n_y, k;
  int64_t* cnt = take<int64_t>(n_y + 1);
  int64_t* off = take<int64_t>(n_y + 1);
  int32_t* slab_i = take<int32_t>(n_y * k);
  float* slab_d = take<float>(n_y * k);
};

static inline hipError_t knn_scan_bytes(int64_t n_y, size_t* bytes) {
  return rocprim::exclusive_scan((void*)nullptr, *bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0,
                                 (size_t)(n_y + 1), rocprim::plus<int64_t>(), (hipStream_t)0, false);
}

// run `call` with D (1 .. 8) as a template argument
#define KNN_FOR_D(D, call) \
  switch (D) {             \
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
#define KNN_CHECK_ARG(cond, ...)       \
  do {                                 \
    if (!(cond)) {                     \
      ::mp::set_error(__VA_ARGS__);    \
      return -(int64_t)MP_ERR_ARG;     \
    }                                  \
  } while (0)

#define KNN_CHECK_EXTENT(fn, name, have, need)                                                  \
  KNN_CHECK_ARG((size_t)(have) >= (size_t)(need), "%s: %s holds %zu bytes, the call needs %zu", \
                fn, name, (size_t)(have), (size_t)(need))

#define KNN_CHECK_HIP(expr)                                                  \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      ::mp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                      __FILE__, __LINE__);                                   \
      return -(int64_t)MP_ERR_HIP;                                           \
    }                                                                        \
  } while (0)

// n_y and k of a slab, as every entry point that carves one checks them
#define KNN_CHECK_SLAB(fn, n_y, k)                                                                                  \
  KNN_CHECK_ARG((n_y) >= 0 && (n_y) < (int64_t)INT32_MAX, "%s: n_y = %lld is negative or not below 2^31", fn,       \
                (long long)(n_y));                                                                                  \
  KNN_CHECK_ARG((k) >= 1 && (k) <= kKnnMaxK, "%s: k = %lld is outside [1, %d]", fn, (long long)(k), kKnnMaxK);      \
  KNN_CHECK_ARG((n_y) == 0 || (k) < (int64_t)INT32_MAX / (n_y), "%s: n_y * k = %lld * %lld is not below 2^31", fn,  \
                (long long)(n_y), (long long)(k))

}  // namespace mp

using namespace mp;

extern "C" {

int64_t mp_knn_max_k(void) { return kKnnMaxK; }

int64_t mp_knn_max_d(void) { return kKnnMaxD; }

int64_t mp_knn_path(int32_t D) {
  KNN_CHECK_ARG(D >= 1 && D <= kKnnMaxD, "mp_knn_path: D = %d is outside [1, %d]", D, kKnnMaxD);
  return D <= kKnnRegD ? 0 : 1;
}

size_t mp_knn_workspace(int64_t n_y, int64_t k) {
  size_t scan = 0;
  (void)knn_scan_bytes(n_y > 0 ? n_y : 0, &scan);
  return KnnWs{nullptr, n_y, k}.total(scan);
}

int64_t mp_knn_search_f32(const float* x, int64_t ldx, int64_t n_x, const float* y, int64_t ldy, int64_t n_y,
                          int32_t D, const int64_t* batch_y, const int64_t* starts_x, int64_t n_graphs_x, int64_t k,
                          int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  KNN_CHECK_ARG(n_x >= 0 && n_x < (int64_t)INT32_MAX, "mp_knn_search_f32: n_x = %lld is negative or not below 2^31",
                (long long)n_x);
  KNN_CHECK_SLAB("mp_knn_search_f32", n_y, k);
  KNN_CHECK_ARG(D >= 1 && D <= kKnnMaxD, "mp_knn_search_f32: D = %d is outside [1, %d]", D, kKnnMaxD);
  KNN_CHECK_ARG(ldx >= D, "mp_knn_search_f32: ldx = %lld < D = %d", (long long)ldx, D);
  KNN_CHECK_ARG(ldy >= D, "mp_knn_search_f32: ldy = %lld < D = %d", (long long)ldy, D);
  KNN_CHECK_ARG(n_graphs_x >= 0 && n_graphs_x < (int64_t)INT32_MAX,
                "mp_knn_search_f32: n_graphs_x = %lld is negative or not below 2^31", (long long)n_graphs_x);
  KNN_CHECK_ARG(starts_x, "mp_knn_search_f32: starts_x is NULL");
  KNN_CHECK_ARG(counts, "mp_knn_search_f32: counts is NULL");
  KNN_CHECK_ARG(ws, "mp_knn_search_f32: ws is NULL");
  KNN_CHECK_ARG(n_x == 0 || x, "mp_knn_search_f32: x is NULL");
  KNN_CHECK_ARG(n_y == 0 || y, "mp_knn_search_f32: y is NULL");
  KNN_CHECK_EXTENT("mp_knn_search_f32", "counts", counts_bytes, 4 * sizeof(int64_t));
  const KnnWs w{ws, n_y, k};
  KNN_CHECK_EXTENT("mp_knn_search_f32", "ws", ws_bytes, w.total(0));
  size_t scan = 0;
  const hipError_t size_query = knn_scan_bytes(n_y, &scan);
  KNN_CHECK_EXTENT("mp_knn_search_f32", "ws", ws_bytes, w.total(scan));
  KNN_CHECK_HIP(size_query);
  hipStream_t s = as_stream(stream);
  KNN_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t), s));
  if (n_y == 0) return 0;
  KNN_CHECK_HIP(hipMemsetAsync(w.cnt + n_y, 0, sizeof(int64_t), s));
  const unsigned blocks = (unsigned)ceil_div(n_y, kKnnWaves);
  if (D <= kKnnRegD) {
    KNN_FOR_D(D, (k_knn_search<kD><<<blocks, kKnnBlock, 0, s>>>(x, ldx, n_x, y, ldy, n_y, batch_y, starts_x,
                                                                 n_graphs_x, (int)k, w.cnt, w.slab_i, w.slab_d)));
  } else {
    k_knn_search_wide<<<blocks, kKnnBlock, 0, s>>>(x, ldx, n_x, y, ldy, n_y, D, batch_y, starts_x, n_graphs_x, (int)k,
                                                   w.cnt, w.slab_i, w.slab_d);
  }
  KNN_CHECK_HIP(hipGetLastError());
  KNN_CHECK_HIP(rocprim::exclusive_scan(w.rest(), scan, (const int64_t*)w.cnt, w.off, (int64_t)0, (size_t)(n_y + 1),
                                        rocprim::plus<int64_t>(), s, false));
  k_knn_total<<<1, 1, 0, s>>>(w.off, n_y, counts);
  KNN_CHECK_HIP(hipGetLastError());
  return 2;  // the search and the total; the scan's launches are rocPRIM's
}

int64_t mp_knn_fill(int64_t n_y, int64_t k, int64_t n_edges, int64_t* out_y, int64_t* out_x, size_t out_bytes,
                    float* out_w, size_t out_w_bytes, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  KNN_CHECK_SLAB("mp_knn_fill", n_y, k);
  KNN_CHECK_ARG(n_edges >= 0 && n_edges <= n_y * k, "mp_knn_fill: n_edges = %lld is outside [0, n_y * k]",
                (long long)n_edges);
  KNN_CHECK_ARG(ws, "mp_knn_fill: ws is NULL");
  KNN_CHECK_ARG(n_edges == 0 || out_y, "mp_knn_fill: out_y is NULL");
  KNN_CHECK_ARG(n_edges == 0 || out_x, "mp_knn_fill: out_x is NULL");
  KNN_CHECK_EXTENT("mp_knn_fill", "out_y / out_x", out_bytes, (size_t)n_edges * sizeof(int64_t));
  if (out_w) KNN_CHECK_EXTENT("mp_knn_fill", "out_w", out_w_bytes, (size_t)n_edges * sizeof(float));
  const KnnWs w{ws, n_y, k};
  KNN_CHECK_EXTENT("mp_knn_fill", "ws", ws_bytes, w.total(0));
  if (n_edges == 0) return 0;
  k_knn_fill<<<(unsigned)ceil_div(n_y * k, kKnnBlock), kKnnBlock, 0, as_stream(stream)>>>(
      w.cnt, w.off, w.slab_i, w.slab_d, n_y, (int)k, n_edges, out_y, out_x, out_w);
  KNN_CHECK_HIP(hipGetLastError());
  return 1;
}

int64_t mp_knn_interpolate_f32(const float* x, int64_t ldx, int64_t n_x, int32_t C, int64_t n_y, int64_t k, void* ws,
                               size_t ws_bytes, float* out, int64_t ldo, size_t out_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  KNN_CHECK_ARG(n_x >= 0 && n_x < (int64_t)INT32_MAX,
                "mp_knn_interpolate_f32: n_x = %lld is negative or not below 2^31", (long long)n_x);
  KNN_CHECK_SLAB("mp_knn_interpolate_f32", n_y, k);
  KNN_CHECK_ARG(C >= 1, "mp_knn_interpolate_f32: C = %d is below 1", C);
  KNN_CHECK_ARG(ldx >= C, "mp_knn_interpolate_f32: ldx = %lld < C = %d", (long long)ldx, C);
  KNN_CHECK_ARG(ldo >= C, "mp_knn_interpolate_f32: ldo = %lld < C = %d", (long long)ldo, C);
  KNN_CHECK_ARG(ws, "mp_knn_interpolate_f32: ws is NULL");
  KNN_CHECK_ARG(n_x == 0 || x, "mp_knn_interpolate_f32: x is NULL");
  KNN_CHECK_ARG(n_y == 0 || out, "mp_knn_interpolate_f32: out is NULL");
  if (n_y > 0) {
    KNN_CHECK_EXTENT("mp_knn_interpolate_f32", "out", out_bytes,
                     ((size_t)(n_y - 1) * (size_t)ldo + (size_t)C) * sizeof(float));
  }
  const KnnWs w{ws, n_y, k};
  KNN_CHECK_EXTENT("mp_knn_interpolate_f32", "ws", ws_bytes, w.total(0));
  if (n_y == 0) return 0;
  hipStream_t s = as_stream(stream);
  const bool vec4 = C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int FE = vec4 ? C / 4 : C;
  const int gl = group_lanes(FE);
  const unsigned blocks = (unsigned)ceil_div(ceil_div(n_y, 64 / gl), kKnnWaves);
  if (vec4) {
    k_knn_interpolate<4><<<blocks, kKnnBlock, 0, s>>>(x, ldx, n_x, FE, n_y, (int)k, w.cnt, w.slab_i, w.slab_d, gl, out,
                                                      ldo);
  } else {
    k_knn_interpolate<1><<<blocks, kKnnBlock, 0, s>>>(x, ldx, n_x, FE, n_y, (int)k, w.cnt, w.slab_i, w.slab_d, gl, out,
                                                      ldo);
  }
  KNN_CHECK_HIP(hipGetLastError());
  return 1;
}

}  // extern "C"
