// Link prediction (GAE / VGAE): the edge-parallel inner-product decoder, the fused
// reconstruction loss, the gradient of z over an unscheduled CSR and the negative
// sampler (gfx950).
//
// Upstream (PyG 1.4.x nn.models.autoencoder) decodes with (z[row] * z[col]).sum(1):
// two [E, C] gathers, and two index_select backwards that scatter with float
// atomics; its negative_sampling copies the edge keys to the host, draws with
// random.sample and retries through np.isin.  Here a group of G lanes serves one
// edge and reads the two rows in place, the per-edge loss coefficient is written by
// the forward, the gradient is a row-wise sum in slot order, and a sample is the
// r-th key that is NOT in the sorted key table, found by one binary search -- no
// [E, C] array, no float atomics, no retry and no host read anywhere.
#include "mp_workspace.h"

namespace mp {

constexpr int LINK_BLOCK = 256;
constexpr float LINK_EPS = 1e-15f;   // upstream's EPS
// N * N (the full mode's key space) must stay below 2^63
constexpr int64_t LINK_MAX_N = 3037000499LL;

// ---------------------------------------------------------------------------
// the dot product of two rows by a group of G lanes
// ---------------------------------------------------------------------------

// Lane `sub` of the group sums the products of columns sub * VEC + k (+ G * VEC per
// pass) in column order, then the group adds its lanes in group_sum's fixed tree:
// the value depends on C, G, VEC and the two rows, not on where the edge sits.
// Every lane of the wave must call this (the tree is cross-lane); `live` guards
// the loads.
template <int VEC>
__device__ __forceinline__ float edge_dot(const float* __restrict__ zi, const float* __restrict__ zj, int C, int sub,
                                          int G, bool live) {
  float acc = 0.f;
  if (live) {
    for (int c = sub * VEC; c < C; c += G * VEC) {
      const Frag<VEC> a = load_frag<VEC>(zi + c), b = load_frag<VEC>(zj + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc += a.v[k] * b.v[k];
    }
  }
  return group_sum(acc, G);
}

__device__ __forceinline__ float link_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// one edge per group: its two rows (or live = false: past the end, or an index
// outside [0, N) -- such an edge scores NaN and nothing is read for it)
struct EdgeRows {
  int64_t e;
  int sub;
  bool in_list, live;
  const float *zi, *zj;
};

__device__ __forceinline__ EdgeRows edge_rows(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                              int64_t E, const float* __restrict__ z, int64_t ldz, int64_t N, int G) {
  EdgeRows r;
  r.e = (int64_t)blockIdx.x * (LINK_BLOCK / G) + threadIdx.x / G;
  r.sub = threadIdx.x & (G - 1);
  r.in_list = r.e < E;
  r.live = false;
  r.zi = r.zj = z;
  if (r.in_list) {
    const int64_t i = row[r.e], j = col[r.e];
    if (i >= 0 && i < N && j >= 0 && j < N) {
      r.live = true;
      r.zi = z + i * ldz;
      r.zj = z + j * ldz;
    }
  }
  return r;
}

template <int VEC>
__global__ __launch_bounds__(LINK_BLOCK) void k_edge_score(const int64_t* __restrict__ row,
                                                           const int64_t* __restrict__ col, int64_t E,
                                                           const float* __restrict__ z, int64_t ldz, int64_t N, int C,
                                                           int G, int sigmoid, float* __restrict__ v) {
  const EdgeRows r = edge_rows(row, col, E, z, ldz, N, G);
  const float d = edge_dot<VEC>(r.zi, r.zj, C, r.sub, G, r.live);
  if (r.in_list && r.sub == 0) v[r.e] = !r.live ? __builtin_nanf("") : sigmoid ? link_sigmoid(d) : d;
}

// The score, upstream's loss term t and d(mean t)/dv per edge; the block's terms
// are added in fp64 by a fixed tree over the block's edges and go to partial[block].
template <int VEC>
__global__ __launch_bounds__(LINK_BLOCK) void k_link_loss(const int64_t* __restrict__ row,
                                                          const int64_t* __restrict__ col, int64_t E,
                                                          const float* __restrict__ z, int64_t ldz, int64_t N, int C,
                                                          int G, int positive, float e_f, float* __restrict__ coef,
                                                          double* __restrict__ partial) {
  __shared__ double st[LINK_BLOCK];
  const EdgeRows r = edge_rows(row, col, E, z, ldz, N, G);
  const float d = edge_dot<VEC>(r.zi, r.zj, C, r.sub, G, r.live);
  if (r.sub == 0) {
    double t = 0.0;
    if (r.in_list) {
      float tf, cf;
      if (!r.live) {
        tf = cf = __builtin_nanf("");
      } else {
        // q = 1 - p, formed as sigmoid(-v): the same quantity without the cancellation
        // that leaves 1.f - p a few ulp of ONE wrong once p nears 1
        const float p = link_sigmoid(d), q = link_sigmoid(-d);
        const float pq = p * q;
        if (positive) {
          tf = -logf(p + LINK_EPS);
          cf = -pq / (p + LINK_EPS) / e_f;
        } else {
          tf = -logf(q + LINK_EPS);
          cf = pq / (q + LINK_EPS) / e_f;
        }
      }
      coef[r.e] = cf;
      t = (double)tf;
    }
    st[threadIdx.x / G] = t;
  }
  __syncthreads();
  for (int s = (LINK_BLOCK / G) >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) st[threadIdx.x] += st[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = st[0];
}

// One block: lane t adds partials t, t + 256, ... in index order, the lanes are
// added by a fixed tree, and the mean is rounded once to fp32.  E = 0: nan, as
// torch.mean of an empty tensor.
__global__ __launch_bounds__(LINK_BLOCK) void k_link_loss_finish(const double* __restrict__ partial, int64_t n_part,
                                                                 int64_t E, float* __restrict__ loss) {
  __shared__ double st[LINK_BLOCK];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += LINK_BLOCK) a += partial[i];
  st[threadIdx.x] = a;
  __syncthreads();
  for (int s = LINK_BLOCK >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) st[threadIdx.x] += st[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = E > 0 ? (float)(st[0] / (double)E) : __builtin_nanf("");
}

// ---------------------------------------------------------------------------
// the gradient of z over an unscheduled CSR
// ---------------------------------------------------------------------------

// dz[r, :] (+)= sum over row r's slots s, in slot order, of coef[eid[s] mod n_coef] *
// z[col[s], :]: one lane group per row, the sum in registers.  A slot whose column
// is outside [0, N) is skipped (mp_csr_build keeps such a value as it came).
template <int VEC>
__global__ __launch_bounds__(LINK_BLOCK) void k_link_grad_rows(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const int32_t* __restrict__ eid, int64_t n_rows,
                                                               int64_t n_slots, int64_t n_coef,
                                                               const float* __restrict__ coef,
                                                               const float* __restrict__ z, int64_t ldz, int64_t N,
                                                               int C, int G, int init_from_out,
                                                               float* __restrict__ dz, int64_t lddz) {
  const int64_t r = (int64_t)blockIdx.x * (LINK_BLOCK / G) + threadIdx.x / G;
  const int sub = threadIdx.x & (G - 1);
  if (r >= n_rows) return;
  int64_t s0 = rowptr[r], s1 = rowptr[r + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > n_slots ? n_slots : s1;
  for (int c = sub * VEC; c < C; c += G * VEC) {
    Frag<VEC> acc;
    if (init_from_out) {
      acc = load_frag<VEC>(dz + r * lddz + c);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
    }
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t j = col[s];
      int64_t e = eid[s];
      if (e >= n_coef) e -= n_coef;
      if (j < 0 || j >= N || e < 0 || e >= n_coef) continue;
      const float w = coef[e];
      const Frag<VEC> x = load_frag<VEC>(z + j * ldz + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc.v[k] += w * x.v[k];
    }
    store_frag<VEC>(dz + r * lddz + c, acc);
  }
}

// ---------------------------------------------------------------------------
// the negative sampler
// ---------------------------------------------------------------------------

// splitmix64 finaliser (mi355_mp.ops._mix64); a draw's bits are mix(mix(seed) ^ s)
__device__ __forceinline__ uint64_t link_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t link_draw(uint64_t seed, uint64_t s, uint64_t m) {
  return __umul64hi(link_mix64(link_mix64(seed) ^ s), m);
}

// The r-th (from 0) non-negative integer missing from the sorted distinct keys
// k[0..n), each taken minus `base`: k[j] - base - j counts the missing values below
// k[j] and never decreases, so with j the smallest index where it exceeds r (n when
// none does) the answer is r + j.
__device__ __forceinline__ uint64_t kth_missing(const int64_t* __restrict__ k, int64_t n, int64_t base, uint64_t r) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((uint64_t)(k[mid] - base - mid) > r) hi = mid;
    else lo = mid + 1;
  }
  return r + (uint64_t)lo;
}

// t = j (j - 1) / 2 + i, i < j: the double sqrt gives j to within one step near
// 2^61, the two loops settle it exactly
__device__ __forceinline__ void tri_inverse(uint64_t t, uint64_t* i, uint64_t* j) {
  uint64_t g = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
  if (g < 1) g = 1;
  while (g > 1 && g * (g - 1) / 2 > t) --g;
  while ((g + 1) * g / 2 <= t) ++g;
  *j = g;
  *i = t - g * (g - 1) / 2;
}

// mode 0: keys row * N + col over T = N * N; mode 1: keys of the strict upper
// triangle over T = N (N - 1) / 2, the sample written twice, [i | j ; j | i].
// M = T - U <= 0 (nothing to draw from) or a key table that does not fit T: -1.
__global__ __launch_bounds__(LINK_BLOCK) void k_neg_sample(const int64_t* __restrict__ keys, int64_t cap,
                                                           const int64_t* __restrict__ n_keys, int64_t N, int mode,
                                                           uint64_t seed, int64_t n, int64_t* __restrict__ out_row,
                                                           int64_t* __restrict__ out_col) {
  const int64_t s = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x;
  if (s >= n) return;
  int64_t U = n_keys[0];
  U = U < 0 ? 0 : (U > cap ? cap : U);
  const uint64_t T = mode == 0 ? (uint64_t)N * (uint64_t)N : (uint64_t)N * (uint64_t)(N - 1) / 2;
  int64_t a = -1, b = -1;
  if ((uint64_t)U < T) {
    const uint64_t t = kth_missing(keys, U, 0, link_draw(seed, (uint64_t)s, T - (uint64_t)U));
    if (t < T) {
      uint64_t i, j;
      if (mode == 0) {
        i = t / (uint64_t)N;
        j = t % (uint64_t)N;
      } else {
        tri_inverse(t, &i, &j);
      }
      a = (int64_t)i;
      b = (int64_t)j;
    }
  }
  out_row[s] = a;
  out_col[s] = b;
  if (mode != 0) {
    out_row[n + s] = b;
    out_col[n + s] = a;
  }
}

// For edge e with i = row[e]: the r-th column of row i that is not among row i's
// keys (two lower bounds over the table), r drawn below N - d_i; a full row, or an
// i outside [0, N): -1.
__global__ __launch_bounds__(LINK_BLOCK) void k_neg_sample_rows(const int64_t* __restrict__ keys, int64_t cap,
                                                                const int64_t* __restrict__ n_keys, int64_t N,
                                                                uint64_t seed, const int64_t* __restrict__ row,
                                                                int64_t E, int64_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x;
  if (e >= E) return;
  int64_t U = n_keys[0];
  U = U < 0 ? 0 : (U > cap ? cap : U);
  const int64_t i = row[e];
  int64_t k = -1;
  if (i >= 0 && i < N) {
    int64_t b[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t want = (i + q) * N;
      int64_t lo = 0, hi = U;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      b[q] = lo;
    }
    const int64_t d = b[1] - b[0];
    if (d < N) {
      const uint64_t c = kth_missing(keys + b[0], d, i * N, link_draw(seed, (uint64_t)e, (uint64_t)(N - d)));
      if (c < (uint64_t)N) k = (int64_t)c;
    }
  }
  out[e] = k;
}

// mp_link_loss_f32's workspace: one fp64 partial per block of the widest mapping
// (64 lanes per edge: four edges per block)
struct LinkLossWs : Carver {
  int64_t n_edges;
  double* partial = take<double>(ceil_div(n_edges > 0 ? n_edges : 0, LINK_BLOCK / 64) + 1);
};

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// 16-byte loads when the rows allow them
static bool link_vec4(const float* z, int64_t ldz, int32_t C) { return C % 4 == 0 && ldz % 4 == 0 && aligned16(z); }

// 16-byte loads: at most LINK_VEC4_LANES lanes an edge, looping beyond -- with 4 Mi edges
// over a z of 2^20 rows, C = 128 scores in 0.57 ms at 16 lanes against 0.73 at 32 and
// 1.31 at 64, C = 64 within 5 % from 4 to 16 lanes, C = 16 fastest at its natural 4
// (tools/bench_link.py, profiles/link_bench.json): more edges a wave keep more row
// loads in flight than a wider group gains.
constexpr int LINK_VEC4_LANES = 16;

static int link_group(int32_t C, bool vec4, int32_t lanes) {
  if (lanes > 0) return lanes;
  if (!vec4) return group_lanes(C);
  const int g = group_lanes((C + 3) / 4);
  return g < LINK_VEC4_LANES ? g : LINK_VEC4_LANES;
}

static bool lanes_ok(int32_t lanes) { return lanes == 0 || (lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0); }

}  // namespace mp

using namespace mp;

#define LINK_CHECK(cond, ...)        \
  do {                               \
    if (!(cond)) {                   \
      ::mp::set_error(__VA_ARGS__);  \
      return -(int64_t)MP_ERR_ARG;   \
    }                                \
  } while (0)
#define LINK_EXTENT(fn, name, have, need)                                                                           \
  LINK_CHECK((size_t)(have) >= (size_t)(need), "%s: %s holds %zu bytes, the call needs %zu", fn, name, (size_t)(have), \
             (size_t)(need))
#define LINK_HIP(expr)                                                                                    \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess) {                                                                               \
      ::mp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);         \
      return -(int64_t)MP_ERR_HIP;                                                                        \
    }                                                                                                     \
  } while (0)

// the checks the score and the loss share
#define LINK_CHECK_EDGES(fn)                                                                                         \
  LINK_CHECK(E >= 0 && E < (int64_t)INT32_MAX, "%s: E = %lld is outside [0, 2^31 - 1)", fn, (long long)E);            \
  LINK_CHECK(N >= 0 && N < (int64_t)INT32_MAX, "%s: N = %lld is outside [0, 2^31 - 1)", fn, (long long)N);            \
  LINK_CHECK(C >= 1, "%s: C = %d, need C >= 1", fn, (int)C);                                                         \
  LINK_CHECK(ldz >= C, "%s: ldz = %lld < C = %d", fn, (long long)ldz, (int)C);                                       \
  LINK_CHECK(lanes_ok(lanes), "%s: lanes = %d is not 0 or a power of two up to 64", fn, (int)lanes);                 \
  LINK_CHECK(E == 0 || row, "%s: row is NULL", fn);                                                                  \
  LINK_CHECK(E == 0 || col, "%s: col is NULL", fn);                                                                  \
  LINK_CHECK(E == 0 || N == 0 || z, "%s: z is NULL", fn);                                                            \
  LINK_CHECK(aligned4(z), "%s: z is not 4-byte aligned", fn)

extern "C" {

int64_t mp_link_lanes(int32_t C, int32_t vec4) {
  LINK_CHECK(C >= 1, "mp_link_lanes: C = %d, need C >= 1", (int)C);
  return link_group(C, vec4 != 0 && C % 4 == 0, 0);
}

int64_t mp_edge_score_f32(const int64_t* row, const int64_t* col, int64_t E, const float* z, int64_t ldz, int64_t N,
                          int32_t C, int32_t sigmoid, int32_t lanes, float* v, size_t v_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  LINK_CHECK_EDGES("mp_edge_score_f32");
  LINK_CHECK(E == 0 || v, "mp_edge_score_f32: v is NULL");
  LINK_EXTENT("mp_edge_score_f32", "v", v_bytes, (size_t)E * sizeof(float));
  if (E == 0) return 0;
  const bool v4 = link_vec4(z, ldz, C);
  const int G = link_group(C, v4, lanes);
  const int64_t blocks = ceil_div(E, LINK_BLOCK / G);
  hipStream_t s = as_stream(stream);
  if (v4) k_edge_score<4><<<blocks, LINK_BLOCK, 0, s>>>(row, col, E, z, ldz, N, C, G, sigmoid, v);
  else k_edge_score<1><<<blocks, LINK_BLOCK, 0, s>>>(row, col, E, z, ldz, N, C, G, sigmoid, v);
  LINK_HIP(hipGetLastError());
  return 1;
}

size_t mp_link_loss_workspace(int64_t E) { return LinkLossWs{nullptr, E}.total(0); }

int64_t mp_link_loss_f32(const int64_t* row, const int64_t* col, int64_t E, const float* z, int64_t ldz, int64_t N,
                         int32_t C, int32_t positive, int32_t lanes, float* coef, size_t coef_bytes, float* loss,
                         size_t loss_bytes, void* ws, size_t ws_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  LINK_CHECK_EDGES("mp_link_loss_f32");
  LINK_CHECK(positive == 0 || positive == 1, "mp_link_loss_f32: positive = %d is not 0 or 1", (int)positive);
  LINK_CHECK(E == 0 || coef, "mp_link_loss_f32: coef is NULL");
  LINK_CHECK(loss, "mp_link_loss_f32: loss is NULL");
  LINK_CHECK(ws, "mp_link_loss_f32: ws is NULL");
  LINK_CHECK(aligned16(ws), "mp_link_loss_f32: ws is not 16-byte aligned");
  LINK_EXTENT("mp_link_loss_f32", "coef", coef_bytes, (size_t)E * sizeof(float));
  LINK_EXTENT("mp_link_loss_f32", "loss", loss_bytes, sizeof(float));
  const LinkLossWs w{ws, E};
  LINK_EXTENT("mp_link_loss_f32", "ws", ws_bytes, w.total(0));
  hipStream_t s = as_stream(stream);
  int64_t blocks = 0, launches = 1;
  if (E > 0) {
    const bool v4 = link_vec4(z, ldz, C);
    const int G = link_group(C, v4, lanes);
    blocks = ceil_div(E, LINK_BLOCK / G);
    const float e_f = (float)E;
    if (v4) k_link_loss<4><<<blocks, LINK_BLOCK, 0, s>>>(row, col, E, z, ldz, N, C, G, positive, e_f, coef, w.partial);
    else k_link_loss<1><<<blocks, LINK_BLOCK, 0, s>>>(row, col, E, z, ldz, N, C, G, positive, e_f, coef, w.partial);
    LINK_HIP(hipGetLastError());
    launches = 2;
  }
  k_link_loss_finish<<<1, LINK_BLOCK, 0, s>>>(w.partial, blocks, E, loss);
  LINK_HIP(hipGetLastError());
  return launches;
}

int64_t mp_link_grad_rows_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t n_rows,
                              int64_t n_slots, const float* coef, int64_t n_coef, const float* z, int64_t ldz,
                              int64_t N, int32_t C, int32_t init_from_out, float* dz, int64_t lddz, size_t dz_bytes,
                              void* stream) {
  MP_DEVICE_GUARD(stream);
  const char* fn = "mp_link_grad_rows_f32";
  LINK_CHECK(n_rows >= 0 && n_rows < (int64_t)INT32_MAX, "%s: n_rows = %lld is outside [0, 2^31 - 1)", fn,
             (long long)n_rows);
  LINK_CHECK(n_slots >= 0 && n_slots < (int64_t)INT32_MAX, "%s: n_slots = %lld is outside [0, 2^31 - 1)", fn,
             (long long)n_slots);
  LINK_CHECK(n_coef >= 0 && n_coef <= n_slots && 2 * n_coef >= n_slots,
             "%s: n_coef = %lld, need n_slots / 2 <= n_coef <= n_slots = %lld", fn, (long long)n_coef,
             (long long)n_slots);
  LINK_CHECK(N >= 0 && N < (int64_t)INT32_MAX, "%s: N = %lld is outside [0, 2^31 - 1)", fn, (long long)N);
  LINK_CHECK(C >= 1, "%s: C = %d, need C >= 1", fn, (int)C);
  LINK_CHECK(ldz >= C, "%s: ldz = %lld < C = %d", fn, (long long)ldz, (int)C);
  LINK_CHECK(lddz >= C, "%s: lddz = %lld < C = %d", fn, (long long)lddz, (int)C);
  LINK_CHECK(init_from_out == 0 || init_from_out == 1, "%s: init_from_out = %d is not 0 or 1", fn, (int)init_from_out);
  LINK_CHECK(rowptr, "%s: rowptr is NULL", fn);
  LINK_CHECK(n_slots == 0 || col, "%s: col is NULL", fn);
  LINK_CHECK(n_slots == 0 || eid, "%s: eid is NULL", fn);
  LINK_CHECK(n_slots == 0 || coef, "%s: coef is NULL", fn);
  LINK_CHECK(n_slots == 0 || z, "%s: z is NULL", fn);
  LINK_CHECK(n_rows == 0 || dz, "%s: dz is NULL", fn);
  LINK_CHECK(aligned4(z) && aligned4(dz), "%s: z or dz is not 4-byte aligned", fn);
  LINK_EXTENT(fn, "dz", dz_bytes, n_rows == 0 ? 0 : ((size_t)(n_rows - 1) * (size_t)lddz + (size_t)C) * sizeof(float));
  if (n_rows == 0) return 0;
  const bool v4 = link_vec4(z, ldz, C) && lddz % 4 == 0 && aligned16(dz);
  const int G = link_group(C, v4, 0);
  const int64_t blocks = ceil_div(n_rows, LINK_BLOCK / G);
  hipStream_t s = as_stream(stream);
  if (v4)
    k_link_grad_rows<4><<<blocks, LINK_BLOCK, 0, s>>>(rowptr, col, eid, n_rows, n_slots, n_coef, coef, z, ldz, N, C, G,
                                                      init_from_out, dz, lddz);
  else
    k_link_grad_rows<1><<<blocks, LINK_BLOCK, 0, s>>>(rowptr, col, eid, n_rows, n_slots, n_coef, coef, z, ldz, N, C, G,
                                                      init_from_out, dz, lddz);
  LINK_HIP(hipGetLastError());
  return 1;
}

int64_t mp_neg_sample(const int64_t* keys, size_t keys_bytes, const int64_t* n_keys, int64_t N, int32_t mode,
                      uint64_t seed, int64_t n_samples, int64_t* out_row, int64_t* out_col, size_t out_bytes,
                      void* stream) {
  MP_DEVICE_GUARD(stream);
  const char* fn = "mp_neg_sample";
  LINK_CHECK(mode == 0 || mode == 1, "%s: mode = %d is not 0 (full) or 1 (upper)", fn, (int)mode);
  LINK_CHECK(N >= 0 && N <= LINK_MAX_N, "%s: N = %lld is outside [0, %lld]", fn, (long long)N, (long long)LINK_MAX_N);
  LINK_CHECK(n_samples >= 0 && n_samples < (int64_t)INT32_MAX, "%s: n_samples = %lld is outside [0, 2^31 - 1)", fn,
             (long long)n_samples);
  LINK_CHECK(keys || keys_bytes < sizeof(int64_t), "%s: keys is NULL", fn);
  LINK_CHECK(n_keys, "%s: n_keys is NULL", fn);
  LINK_CHECK(n_samples == 0 || out_row, "%s: out_row is NULL", fn);
  LINK_CHECK(n_samples == 0 || out_col, "%s: out_col is NULL", fn);
  LINK_EXTENT(fn, "out_row / out_col", out_bytes, (size_t)n_samples * (mode ? 2 : 1) * sizeof(int64_t));
  if (n_samples == 0) return 0;
  k_neg_sample<<<ceil_div(n_samples, LINK_BLOCK), LINK_BLOCK, 0, as_stream(stream)>>>(
      keys, (int64_t)(keys_bytes / sizeof(int64_t)), n_keys, N, mode, seed, n_samples, out_row, out_col);
  LINK_HIP(hipGetLastError());
  return 1;
}

int64_t mp_neg_sample_rows(const int64_t* keys, size_t keys_bytes, const int64_t* n_keys, int64_t N, uint64_t seed,
                           const int64_t* row, int64_t E, int64_t* out, size_t out_bytes, void* stream) {
  MP_DEVICE_GUARD(stream);
  const char* fn = "mp_neg_sample_rows";
  LINK_CHECK(N >= 0 && N <= LINK_MAX_N, "%s: N = %lld is outside [0, %lld]", fn, (long long)N, (long long)LINK_MAX_N);
  LINK_CHECK(E >= 0 && E < (int64_t)INT32_MAX, "%s: E = %lld is outside [0, 2^31 - 1)", fn, (long long)E);
  LINK_CHECK(keys || keys_bytes < sizeof(int64_t), "%s: keys is NULL", fn);
  LINK_CHECK(n_keys, "%s: n_keys is NULL", fn);
  LINK_CHECK(E == 0 || row, "%s: row is NULL", fn);
  LINK_CHECK(E == 0 || out, "%s: out is NULL", fn);
  LINK_EXTENT(fn, "out", out_bytes, (size_t)E * sizeof(int64_t));
  if (E == 0) return 0;
  k_neg_sample_rows<<<ceil_div(E, LINK_BLOCK), LINK_BLOCK, 0, as_stream(stream)>>>(
      keys, (int64_t)(keys_bytes / sizeof(int64_t)), n_keys, N, seed, row, E, out);
  LINK_HIP(hipGetLastError());
  return 1;
}

}  // extern "C"
