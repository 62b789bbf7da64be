// The dense family (gfx950): dense_diff_pool forward and backward, the dense
// mean aggregation of DenseSAGEConv, and the to_dense_batch / to_dense_adj fills.
//
// dense_diff_pool, per graph b with x [N, F], adj [N, N], s [N, C], mask [N]:
//   P = softmax(s, -1) * mask          T = adj P           V = adj^T P
//   out = P^T x   out_adj = P^T T      q_b = sum_ij (adj_ij - p_i . p_j)^2
//   h_b = sum_ic -p log(p + 1e-15)
//   link = sqrt(sum_b q_b) / (B N N)   ent = sum_b h_b / (B N)
// (P's masked rows are zero, so P^T x is P^T (x * mask) term for term.)  The
// residual is formed entry by entry; nothing of size [B, N, N] is allocated.
// P, T and V ([B, N, C] each) are saved: the backward never reads adj.
//
// Forms, mp_diff_pool_path(N, C, F):
//   0  one workgroup per graph: P, T and V live in LDS ([N, C | 1] each, odd
//      row stride), adj is staged in chunks of dp_chunk_rows(N) rows, and T, V
//      and the residual are formed from each staged chunk: one pass over adj,
//      one launch, plus the launch that adds the B per-graph partials.
//   1  row tiles: a softmax kernel writes P, and T, V, the residual, out and
//      out_adj are tiles of one batched fp32 GEMM core (64 x 64 x 32, a 4 x 4
//      register block per lane, LDS-staged); the residual's tile partials and
//      the rows' entropies go to the workspace and are added per graph in a
//      fixed order.
// The backward is the same GEMM core over [N, C]-sized operands, then one wave
// per row for the loss terms and the softmax backward.
// No atomics on floats and every sum in a fixed order: the same input gives the
// same bits.  Products are fused (fmaf) explicitly; the unit is compiled with
// contraction off like the rest.
#include "mp_workspace.h"

#include <math.h>

namespace mp {

constexpr int kDnTile = 64;     // GEMM tile rows and columns
constexpr int kDnK = 32;        // GEMM tile depth
constexpr int kDnPad = 4;       // LDS row padding (keeps 16-byte alignment)
constexpr int kDpMaxN0 = 128;   // form 0: the largest graph one workgroup takes
constexpr int kDpLds0 = 60 * 1024;  // form 0: LDS budget in bytes (below the 64 KiB a plain launch may ask for)
constexpr float kDpEps = 1e-15f;

enum { kEpiStore = 0, kEpiDeg = 1, kEpiSqRes = 2 };

// rows of adj staged at a time by form 0: about 16 KiB
__host__ __device__ static inline int dp_chunk_rows(int64_t N) {
  const int64_t np = N | 1;
  int64_t r = 4096 / np;
  if (r < 1) r = 1;
  return (int)(r < N ? r : N);
}
__host__ __device__ static inline int64_t dp_lds_bytes(int64_t N, int32_t C) {
  const int64_t cp = (int64_t)C | 1, np = N | 1;
  return (3 * N * cp + (int64_t)dp_chunk_rows(N) * np) * (int64_t)sizeof(float);
}
__host__ __device__ static inline int dp_path(int64_t N, int32_t C) {
  return (N <= kDpMaxN0 && dp_lds_bytes(N, C) <= kDpLds0) ? 0 : 1;
}
static inline int64_t dn_tiles(int64_t n) { return ceil_div(n, kDnTile); }

// Forward workspace: the per-graph partials (q_b, h_b), and for form 1 the
// residual's tile partials [B, tiles(N)^2] and the rows' entropies [B, N].
struct DiffPoolWs : Carver {
  float *qb, *hb, *qpart, *hrow;
  DiffPoolWs(void* ws, int64_t B, int64_t N, int32_t C)
      : Carver(ws),
        qb(take<float>(B)),
        hb(take<float>(B)),
        qpart(take<float>(dp_path(N, C) == 1 ? B * dn_tiles(N) * dn_tiles(N) : 0)),
        hrow(take<float>(dp_path(N, C) == 1 ? B * N : 0)) {}
};
// Backward workspace: G = P^T P per graph, [B, C, C].
struct DiffPoolBwdWs : Carver {
  float* G;
  DiffPoolBwdWs(void* ws, int64_t B, int32_t C) : Carver(ws), G(take<float>(B * (int64_t)C * C)) {}
};
// to_dense_adj with edge_attr: the winning edge (its index + 1) of every cell.
struct DenseAdjWs : Carver {
  unsigned long long* win;
  DenseAdjWs(void* ws, int64_t B, int64_t Nmax, int32_t D)
      : Carver(ws), win(take<unsigned long long>(D > 0 ? B * Nmax * Nmax : 0)) {}
};

// sum over the 256 threads of a workgroup in a fixed tree; red: 256 floats of LDS
__device__ __forceinline__ float dn_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// One wave: the row softmax(srow) * live into prow (global) and lrow (LDS, or
// NULL); returns the row's entropy sum_c -p log(p + eps) in every lane.
__device__ __forceinline__ float dp_softmax_row(const float* __restrict__ srow, int C, bool live,
                                                float* __restrict__ prow, float* lrow) {
  const int lane = lane_id();
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, srow[c]);
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += expf(srow[c] - m);
  sum = group_sum(sum, 64);
  float h = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float p = live ? expf(srow[c] - m) / sum : 0.f;
    prow[c] = p;
    if (lrow) lrow[c] = p;
    h -= p * logf(p + kDpEps);
  }
  return group_sum(h, 64);
}

struct DpFwd {
  const float* x;
  const float* adj;
  const float* s;
  const uint8_t* mask;
  float *out, *out_adj, *P, *T, *V, *qb, *hb;
  int32_t N, C, F;
};

// form 0: one workgroup per graph
__global__ __launch_bounds__(256) void k_dp_fwd_graph(DpFwd a) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];
  __shared__ float red[256];
  const int N = a.N, C = a.C, F = a.F, Cp = C | 1, Np = N | 1;
  const int RJ = dp_chunk_rows(N);
  float* sP = dp_lds;
  float* sT = sP + N * Cp;
  float* sV = sT + N * Cp;
  float* sA = sV + N * Cp;
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, wave = uni(tid >> 6);
  const float* xb = a.x + b * N * F;
  const float* ab = a.adj + b * N * N;
  const float* sb = a.s + b * N * C;
  const uint8_t* mb = a.mask ? a.mask + b * N : nullptr;
  float* Pb = a.P + b * N * C;
  float* Tb = a.T + b * N * C;
  float* Vb = a.V + b * N * C;

  float h = 0.f;
  for (int i = wave; i < N; i += 4) {
    const bool live = !mb || mb[i] != 0;
    const float hr = dp_softmax_row(sb + (int64_t)i * C, C, live, Pb + (int64_t)i * C, sP + i * Cp);
    if (lane_id() == 0) h += hr;
  }
  for (int idx = tid; idx < N * Cp; idx += 256) sV[idx] = 0.f;
  __syncthreads();

  float q = 0.f;
  for (int r0 = 0; r0 < N; r0 += RJ) {
    const int rows = N - r0 < RJ ? N - r0 : RJ;
    for (int idx = tid; idx < rows * N; idx += 256) {
      const int r = idx / N, j = idx - r * N;
      sA[r * Np + j] = ab[(int64_t)(r0 + r) * N + j];
    }
    __syncthreads();
    // T rows of the chunk
    for (int idx = tid; idx < rows * C; idx += 256) {
      const int r = idx / C, c = idx - r * C;
      const float* ar = sA + r * Np;
      float acc = 0.f;
      for (int j = 0; j < N; ++j) acc = fmaf(ar[j], sP[j * Cp + c], acc);
      sT[(r0 + r) * Cp + c] = acc;
      Tb[(int64_t)(r0 + r) * C + c] = acc;
    }
    // the chunk's rows into every V row
    for (int idx = tid; idx < N * C; idx += 256) {
      const int j = idx / C, c = idx - j * C;
      float acc = sV[j * Cp + c];
      for (int r = 0; r < rows; ++r) acc = fmaf(sA[r * Np + j], sP[(r0 + r) * Cp + c], acc);
      sV[j * Cp + c] = acc;
    }
    // the residual of the chunk's entries
    for (int idx = tid; idx < rows * N; idx += 256) {
      const int r = idx / N, j = idx - r * N;
      const float* pi = sP + (r0 + r) * Cp;
      const float* pj = sP + j * Cp;
      float d = 0.f;
      for (int c = 0; c < C; ++c) d = fmaf(pi[c], pj[c], d);
      const float e = sA[r * Np + j] - d;
      q = fmaf(e, e, q);
    }
    __syncthreads();
  }
  for (int idx = tid; idx < N * C; idx += 256) {
    const int j = idx / C, c = idx - j * C;
    Vb[idx] = sV[j * Cp + c];
  }
  float* ob = a.out + b * C * F;
  for (int idx = tid; idx < C * F; idx += 256) {
    const int c = idx / F, f = idx - c * F;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc = fmaf(sP[n * Cp + c], xb[(int64_t)n * F + f], acc);
    ob[idx] = acc;
  }
  float* oab = a.out_adj + b * C * C;
  for (int idx = tid; idx < C * C; idx += 256) {
    const int c = idx / C, c2 = idx - c * C;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc = fmaf(sP[n * Cp + c], sT[n * Cp + c2], acc);
    oab[idx] = acc;
  }
  q = dn_block_sum(q, red);
  h = dn_block_sum(h, red);
  if (tid == 0) {
    a.qb[b] = q;
    a.hb[b] = h;
  }
}

// form 1: P and the rows' entropies, a wave per row of [B * N]
__global__ __launch_bounds__(256) void k_dp_softmax(const float* __restrict__ s, const uint8_t* __restrict__ mask,
                                                    int64_t rows, int32_t C, float* __restrict__ P,
                                                    float* __restrict__ hrow) {
  const int wave = uni((int)(threadIdx.x >> 6));
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const bool live = !mask || mask[r] != 0;
    const float h = dp_softmax_row(s + r * C, C, live, P + r * C, nullptr);
    if (lane_id() == 0) hrow[r] = h;
  }
}

// form 1: q_b and h_b from the workspace partials, a workgroup per graph
__global__ __launch_bounds__(256) void k_dp_reduce(const float* __restrict__ qpart, int64_t nq,
                                                   const float* __restrict__ hrow, int64_t N, float* __restrict__ qb,
                                                   float* __restrict__ hb) {
  __shared__ float red[256];
  const int64_t b = blockIdx.x;
  float q = 0.f, h = 0.f;
  for (int64_t i = threadIdx.x; i < nq; i += 256) q += qpart[b * nq + i];
  for (int64_t i = threadIdx.x; i < N; i += 256) h += hrow[b * N + i];
  q = dn_block_sum(q, red);
  h = dn_block_sum(h, red);
  if (threadIdx.x == 0) {
    qb[b] = q;
    hb[b] = h;
  }
}

// loss = (link, ent, sum q_b, sum h_b): one workgroup
__global__ __launch_bounds__(256) void k_dp_finalize(const float* __restrict__ qb, const float* __restrict__ hb,
                                                     int64_t B, int64_t N, float* __restrict__ loss) {
  __shared__ float red[256];
  float q = 0.f, h = 0.f;
  for (int64_t i = threadIdx.x; i < B; i += 256) {
    q += qb[i];
    h += hb[i];
  }
  q = dn_block_sum(q, red);
  h = dn_block_sum(h, red);
  if (threadIdx.x == 0) {
    const float bn = (float)B * (float)N;
    loss[0] = sqrtf(q) / (bn * (float)N);
    loss[1] = h / bn;
    loss[2] = q;
    loss[3] = h;
  }
}

// ---------------------------------------------------------------------------
// the batched GEMM core:  Out[b] (M x N) = alpha * A[b] (M x K) . B[b] (K x N)
// ---------------------------------------------------------------------------
struct DnGemm {
  const float* A;
  int64_t a_batch, a_m, a_k;  // A(b, m, k) = A[b * a_batch + m * a_m + k * a_k]
  const float* Bm;
  int64_t b_batch, b_k, b_n;
  float* Out;
  int64_t o_batch, o_m;       // Out(b, m, n) = Out[b * o_batch + m * o_m + n]
  int32_t M, N, K;
  int32_t epi;
  int32_t diag_one;           // A(m, m) is read as 1
  int32_t accumulate;         // Out += instead of Out =
  const float* bscale;        // [b, K] or NULL: B(k, :) is divided by max(bscale[k], 1)
  float* deg;                 // kEpiDeg: [b, M], the row sums of A; Out = acc / max(deg, 1)
  const float* aux;           // kEpiSqRes: the matrix [b, M, N] the product is taken from
  float* part;                // kEpiSqRes: [b, tiles] sums of (aux - acc)^2
  const float* k_gl;          // not NULL: alpha = 2 gl / (sqrt(q) k_den), 0 when q is 0
  const float* k_q;
  float k_den;
};

__global__ __launch_bounds__(256) void k_dense_gemm(DnGemm g) {
  __shared__ __attribute__((aligned(16))) float sA[kDnK][kDnTile + kDnPad];
  __shared__ __attribute__((aligned(16))) float sB[kDnK][kDnTile + kDnPad];
  __shared__ float red[256];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t b = blockIdx.z;
  const int m0 = blockIdx.x * kDnTile, n0 = blockIdx.y * kDnTile;
  const float* A = g.A + b * g.a_batch;
  const float* Bp = g.Bm + b * g.b_batch;
  const float* bs = g.bscale ? g.bscale + b * g.K : nullptr;
  const bool a_kc = g.a_k == 1, b_nc = g.b_n == 1;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  float deg = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += kDnK) {
#pragma unroll
    for (int e = 0; e < kDnTile * kDnK / 256; ++e) {
      const int lin = tid + e * 256;
      int m, k;
      if (a_kc) {
        k = lin & (kDnK - 1);
        m = lin / kDnK;
      } else {
        m = lin & (kDnTile - 1);
        k = lin / kDnTile;
      }
      const int gm = m0 + m, gk = k0 + k;
      float v = 0.f;
      if (gm < g.M && gk < g.K) {
        v = A[(int64_t)gm * g.a_m + (int64_t)gk * g.a_k];
        if (g.diag_one && gm == gk) v = 1.f;
      }
      sA[k][m] = v;
    }
#pragma unroll
    for (int e = 0; e < kDnTile * kDnK / 256; ++e) {
      const int lin = tid + e * 256;
      int n, k;
      if (b_nc) {
        n = lin & (kDnTile - 1);
        k = lin / kDnTile;
      } else {
        k = lin & (kDnK - 1);
        n = lin / kDnK;
      }
      const int gn = n0 + n, gk = k0 + k;
      float v = 0.f;
      if (gn < g.N && gk < g.K) {
        v = Bp[(int64_t)gk * g.b_k + (int64_t)gn * g.b_n];
        if (bs) v = v / fmaxf(bs[gk], 1.f);
      }
      sB[k][n] = v;
    }
    __syncthreads();
    if (g.epi == kEpiDeg && tid < kDnTile) {
#pragma unroll
      for (int k = 0; k < kDnK; ++k) deg += sA[k][tid];
    }
#pragma unroll
    for (int k = 0; k < kDnK; ++k) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&sA[k][ty * 4]);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&sB[k][tx * 4]);
      const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
    }
    __syncthreads();
  }
  if (g.epi == kEpiSqRes) {
    const float* aux = g.aux + b * (int64_t)g.M * g.N;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + ty * 4 + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + tx * 4 + j;
        if (m < g.M && n < g.N) {
          const float e = aux[(int64_t)m * g.N + n] - acc[i][j];
          q = fmaf(e, e, q);
        }
      }
    }
    q = dn_block_sum(q, red);
    if (tid == 0)
      g.part[b * (int64_t)gridDim.x * gridDim.y + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = q;
    return;
  }
  float alpha = 1.f;
  if (g.k_gl) {
    const float qv = *g.k_q;
    alpha = qv > 0.f ? 2.f * *g.k_gl / (sqrtf(qv) * g.k_den) : 0.f;
  }
  if (g.epi == kEpiDeg) {
    if (tid < kDnTile) red[tid] = deg;
    __syncthreads();
    if (blockIdx.y == 0 && tid < kDnTile && m0 + tid < g.M) g.deg[b * g.M + m0 + tid] = deg;
  }
  float* O = g.Out + b * g.o_batch;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= g.M) continue;
    const float dv = g.epi == kEpiDeg ? fmaxf(red[ty * 4 + i], 1.f) : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx * 4 + j;
      if (n >= g.N) continue;
      float v = g.epi == kEpiDeg ? acc[i][j] / dv : alpha * acc[i][j];
      float* o = O + (int64_t)m * g.o_m + n;
      if (g.accumulate) v += *o;
      *o = v;
    }
  }
}

static DnGemm dn_gemm(const float* A, int64_t a_batch, int64_t a_m, int64_t a_k, const float* Bm, int64_t b_batch,
                      int64_t b_k, int64_t b_n, float* Out, int64_t o_batch, int64_t o_m, int64_t M, int64_t N,
                      int64_t K) {
  DnGemm g;
  g.A = A, g.a_batch = a_batch, g.a_m = a_m, g.a_k = a_k;
  g.Bm = Bm, g.b_batch = b_batch, g.b_k = b_k, g.b_n = b_n;
  g.Out = Out, g.o_batch = o_batch, g.o_m = o_m;
  g.M = (int32_t)M, g.N = (int32_t)N, g.K = (int32_t)K;
  g.epi = kEpiStore, g.diag_one = 0, g.accumulate = 0;
  g.bscale = nullptr, g.deg = nullptr, g.aux = nullptr, g.part = nullptr, g.k_gl = nullptr, g.k_q = nullptr;
  g.k_den = 1.f;
  return g;
}

static void dn_launch(const DnGemm& g, int64_t B, hipStream_t st) {
  const dim3 grid((unsigned)dn_tiles(g.M), (unsigned)dn_tiles(g.N), (unsigned)B);
  hipLaunchKernelGGL(k_dense_gemm, grid, dim3(256), 0, st, g);
}

// the loss terms and the softmax backward, a wave per row of [B * N]; ds holds
// x gOut^T + T gOA^T + V gOA + 2k P G on entry
__global__ __launch_bounds__(256) void k_dp_bwd_rows(const float* __restrict__ P, const float* __restrict__ T,
                                                     const float* __restrict__ V, float* __restrict__ ds,
                                                     const float* __restrict__ g_loss,
                                                     const float* __restrict__ loss, int64_t rows, int32_t C,
                                                     float k_den, float e_den) {
  const int wave = uni((int)(threadIdx.x >> 6)), lane = lane_id();
  float k = 0.f, ec = 0.f;
  if (g_loss) {
    const float qv = loss[2];
    k = qv > 0.f ? g_loss[0] / (sqrtf(qv) * k_den) : 0.f;
    ec = g_loss[1] / e_den;
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const float* p = P + r * C;
    const float* t = T + r * C;
    const float* v = V + r * C;
    float* d = ds + r * C;
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float pc = p[c];
      const float dp = d[c] - k * (t[c] + v[c]) - ec * (logf(pc + kDpEps) + pc / (pc + kDpEps));
      dot = fmaf(dp, pc, dot);
    }
    dot = group_sum(dot, 64);
    for (int c = lane; c < C; c += 64) {
      const float pc = p[c];
      const float dp = d[c] - k * (t[c] + v[c]) - ec * (logf(pc + kDpEps) + pc / (pc + kDpEps));
      d[c] = pc * (dp - dot);
    }
  }
}

// ---------------------------------------------------------------------------
// to_dense_batch / to_dense_adj
// ---------------------------------------------------------------------------

// SCATTER: dense[g, i, :] = i < n_g ? x[starts[g] + i, :] : fill, mask[g, i] = i < n_g
// else (the backward): dx[starts[g] + i, :] = dense[g, i, :]
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_dense_rows(const float* __restrict__ src, int32_t F,
                                                    const int64_t* __restrict__ starts, int64_t B, int64_t Nmax,
                                                    float fill, float* __restrict__ dst, uint8_t* __restrict__ mask) {
  const int64_t total = B * Nmax * F;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / F, f = idx - row * F;
    const int64_t g = row / Nmax, i = row - g * Nmax;
    const int64_t s = starts[g], cnt = starts[g + 1] - s;
    const bool live = i < cnt;
    if (SCATTER) {
      dst[idx] = live ? src[(s + i) * F + f] : fill;
      if (f == 0) mask[row] = live ? 1 : 0;
    } else if (live) {
      dst[(s + i) * F + f] = src[idx];
    }
  }
}

// the cell of edge e, or -1: both ends in graph batch[row], inside [0, Nmax)
__device__ __forceinline__ int64_t dn_edge_cell(const int64_t* row, const int64_t* col, const int64_t* batch,
                                                const int64_t* starts, int64_t n, int64_t B, int64_t Nmax,
                                                int64_t e) {
  const int64_t r = row[e], c = col[e];
  if (r < 0 || r >= n) return -1;
  const int64_t g = batch ? batch[r] : 0;
  if (g < 0 || g >= B) return -1;
  const int64_t i = r - starts[g], j = c - starts[g];
  if (i < 0 || i >= Nmax || j < 0 || j >= Nmax) return -1;
  return (g * Nmax + i) * Nmax + j;
}

// PASS 0: out[cell] = 1; PASS 1: win[cell] = max(e + 1) (an integer maximum: the
// last edge of a cell, whatever the order the lanes run in); PASS 2: the winner
// writes its D attributes
template <int PASS>
__global__ __launch_bounds__(256) void k_dense_adj(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                   int64_t E, const float* __restrict__ attr, int32_t D,
                                                   const int64_t* __restrict__ batch,
                                                   const int64_t* __restrict__ starts, int64_t n, int64_t B,
                                                   int64_t Nmax, float* __restrict__ out,
                                                   unsigned long long* __restrict__ win) {
  const int64_t per = PASS == 2 ? D : 1, total = E * per;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t e = idx / per, d = idx - e * per;
    const int64_t cell = dn_edge_cell(row, col, batch, starts, n, B, Nmax, e);
    if (cell < 0) continue;
    if (PASS == 0) {
      out[cell] = 1.f;
    } else if (PASS == 1) {
      atomicMax(win + cell, (unsigned long long)(e + 1));
    } else if (win[cell] == (unsigned long long)(e + 1)) {
      out[cell * D + d] = attr[e * D + d];
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static inline bool dn_al(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

#define DN_CHECK_PTR(fn, name, p) \
  MP_CHECK_ARG((p) != nullptr && dn_al((p), 4), "%s: %s is %s", fn, name, (p) ? "not 4-byte aligned" : "NULL")
#define DN_CHECK_OPT(fn, name, p) MP_CHECK_ARG(dn_al((p), 4), "%s: %s is not 4-byte aligned", fn, name)

static unsigned dn_blocks(int64_t items, int per_block) {
  const int64_t b = ceil_div(items > 0 ? items : 1, per_block);
  return (unsigned)(b < (1 << 18) ? b : (1 << 18));
}

// shapes every diff-pool call takes: all >= 1, and grids within HIP's limits (a
// launch holds fewer than 2^24 workgroups; B rides in gridDim.z)
static int dp_shape(const char* fn, int64_t B, int64_t N, int32_t C, int32_t F) {
  MP_CHECK_ARG(B >= 1, "%s: B = %lld < 1", fn, (long long)B);
  MP_CHECK_ARG(N >= 1, "%s: N = %lld < 1", fn, (long long)N);
  MP_CHECK_ARG(C >= 1, "%s: C = %d < 1", fn, C);
  MP_CHECK_ARG(F >= 1, "%s: F = %d < 1", fn, F);
  const int64_t tn = dn_tiles(N), tc = dn_tiles(C), tf = dn_tiles(F);
  MP_CHECK_ARG(B <= 65535 && N <= ((int64_t)1 << 22) && tc <= 65535 && tf <= 65535 &&
                   B * tn * tn < ((int64_t)1 << 24) && B * tn * (tc > tf ? tc : tf) < ((int64_t)1 << 24),
               "%s: grid too large (B %lld, N %lld, C %d, F %d): B <= 65535 and fewer than 2^24 tiles of 64 x 64 "
               "per launch",
               fn, (long long)B, (long long)N, C, F);
  return MP_OK;
}

static int diff_pool_fwd(const float* x, const float* adj, const float* s, const uint8_t* mask, int64_t B, int64_t N,
                         int32_t C, int32_t F, float* out, size_t out_bytes, float* out_adj, size_t out_adj_bytes,
                         float* loss, size_t loss_bytes, float* P, size_t P_bytes, float* T, size_t T_bytes, float* V,
                         size_t V_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_dense_diff_pool_f32";
  if (int rc = dp_shape(fn, B, N, C, F)) return rc;
  DN_CHECK_PTR(fn, "x", x);
  DN_CHECK_PTR(fn, "adj", adj);
  DN_CHECK_PTR(fn, "s", s);
  DN_CHECK_PTR(fn, "out", out);
  DN_CHECK_PTR(fn, "out_adj", out_adj);
  DN_CHECK_PTR(fn, "loss", loss);
  DN_CHECK_PTR(fn, "P", P);
  DN_CHECK_PTR(fn, "T", T);
  DN_CHECK_PTR(fn, "V", V);
  MP_CHECK_ARG(ws != nullptr && dn_al(ws, 16), "%s: ws is %s", fn, ws ? "not 16-byte aligned" : "NULL");
  const size_t nc = (size_t)B * N * C * sizeof(float);
  MP_CHECK_EXTENT(fn, "out", out_bytes, (size_t)B * C * F * sizeof(float));
  MP_CHECK_EXTENT(fn, "out_adj", out_adj_bytes, (size_t)B * C * C * sizeof(float));
  MP_CHECK_EXTENT(fn, "loss", loss_bytes, 4 * sizeof(float));
  MP_CHECK_EXTENT(fn, "P", P_bytes, nc);
  MP_CHECK_EXTENT(fn, "T", T_bytes, nc);
  MP_CHECK_EXTENT(fn, "V", V_bytes, nc);
  const DiffPoolWs w(ws, B, N, C);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  if (dp_path(N, C) == 0) {
    const DpFwd a{x, adj, s, mask, out, out_adj, P, T, V, w.qb, w.hb, (int32_t)N, C, F};
    hipLaunchKernelGGL(k_dp_fwd_graph, dim3((unsigned)B), dim3(256), (size_t)dp_lds_bytes(N, C), st, a);
    *launches = 1;
  } else {
    const int64_t nc1 = N * (int64_t)C, nn = N * N, tn = dn_tiles(N);
    hipLaunchKernelGGL(k_dp_softmax, dim3(dn_blocks(B * N, 4)), dim3(256), 0, st, s, mask, B * N, C, P, w.hrow);
    dn_launch(dn_gemm(adj, nn, N, 1, P, nc1, C, 1, T, nc1, C, N, C, N), B, st);          // T = adj P
    dn_launch(dn_gemm(adj, nn, 1, N, P, nc1, C, 1, V, nc1, C, N, C, N), B, st);          // V = adj^T P
    DnGemm gq = dn_gemm(P, nc1, C, 1, P, nc1, 1, C, nullptr, 0, 0, N, N, C);             // (adj - P P^T)^2
    gq.epi = kEpiSqRes, gq.aux = adj, gq.part = w.qpart;
    dn_launch(gq, B, st);
    dn_launch(dn_gemm(P, nc1, 1, C, x, N * (int64_t)F, F, 1, out, (int64_t)C * F, F, C, F, N), B, st);   // P^T x
    dn_launch(dn_gemm(P, nc1, 1, C, T, nc1, C, 1, out_adj, (int64_t)C * C, C, C, C, N), B, st);          // P^T T
    hipLaunchKernelGGL(k_dp_reduce, dim3((unsigned)B), dim3(256), 0, st, w.qpart, tn * tn, w.hrow, N, w.qb, w.hb);
    *launches = 7;
  }
  hipLaunchKernelGGL(k_dp_finalize, dim3(1), dim3(256), 0, st, w.qb, w.hb, B, N, loss);
  ++*launches;
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int diff_pool_bwd(const float* g_out, const float* g_oa, const float* g_loss, const float* x, const float* P,
                         const float* T, const float* V, const float* loss, int64_t B, int64_t N, int32_t C,
                         int32_t F, float* dx, size_t dx_bytes, float* ds, size_t ds_bytes, void* ws, size_t ws_bytes,
                         void* stream, int64_t* launches) {
  const char* fn = "mp_dense_diff_pool_bwd_f32";
  if (int rc = dp_shape(fn, B, N, C, F)) return rc;
  DN_CHECK_OPT(fn, "g_out", g_out);
  DN_CHECK_OPT(fn, "g_oa", g_oa);
  DN_CHECK_OPT(fn, "g_loss", g_loss);
  DN_CHECK_PTR(fn, "x", x);
  DN_CHECK_PTR(fn, "P", P);
  DN_CHECK_PTR(fn, "T", T);
  DN_CHECK_PTR(fn, "V", V);
  DN_CHECK_PTR(fn, "loss", loss);
  DN_CHECK_OPT(fn, "dx", dx);
  DN_CHECK_PTR(fn, "ds", ds);
  MP_CHECK_ARG(ws != nullptr && dn_al(ws, 16), "%s: ws is %s", fn, ws ? "not 16-byte aligned" : "NULL");
  if (dx) MP_CHECK_EXTENT(fn, "dx", dx_bytes, (size_t)B * N * F * sizeof(float));
  MP_CHECK_EXTENT(fn, "ds", ds_bytes, (size_t)B * N * C * sizeof(float));
  const DiffPoolBwdWs w(ws, B, C);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  const int64_t nc = N * (int64_t)C, nf = N * (int64_t)F, cc = (int64_t)C * C, cf = (int64_t)C * F;
  const float k_den = (float)B * (float)N * (float)N, e_den = (float)B * (float)N;
  *launches = 0;
  bool have = false;   // ds holds a term already
  if (g_out) {         // x gOut^T
    dn_launch(dn_gemm(x, nf, F, 1, g_out, cf, 1, F, ds, nc, C, N, C, F), B, st);
    have = true, ++*launches;
  }
  if (g_oa) {          // T gOA^T + V gOA
    DnGemm a = dn_gemm(T, nc, C, 1, g_oa, cc, 1, C, ds, nc, C, N, C, C);
    a.accumulate = have;
    dn_launch(a, B, st);
    DnGemm b = dn_gemm(V, nc, C, 1, g_oa, cc, C, 1, ds, nc, C, N, C, C);
    b.accumulate = 1;
    dn_launch(b, B, st);
    have = true, *launches += 2;
  }
  if (g_loss) {        // 2k P (P^T P)
    dn_launch(dn_gemm(P, nc, 1, C, P, nc, C, 1, w.G, cc, C, C, C, N), B, st);
    DnGemm a = dn_gemm(P, nc, C, 1, w.G, cc, C, 1, ds, nc, C, N, C, C);
    a.accumulate = have, a.k_gl = g_loss, a.k_q = loss + 2, a.k_den = k_den;
    dn_launch(a, B, st);
    have = true, *launches += 2;
  }
  if (!have) {
    MP_CHECK_HIP(hipMemsetAsync(ds, 0, (size_t)B * N * C * sizeof(float), st));
    ++*launches;
  }
  hipLaunchKernelGGL(k_dp_bwd_rows, dim3(dn_blocks(B * N, 4)), dim3(256), 0, st, P, T, V, ds, g_loss, loss, B * N, C,
                     k_den, e_den);
  ++*launches;
  if (dx) {            // mask (P gOut): P's masked rows are zero
    if (g_out) {
      dn_launch(dn_gemm(P, nc, C, 1, g_out, cf, F, 1, dx, nf, F, N, F, C), B, st);
    } else {
      MP_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)B * N * F * sizeof(float), st));
    }
    ++*launches;
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int dense_mean_agg(const float* adj, const float* x, int64_t B, int64_t N, int32_t F, int32_t add_loop,
                          int32_t transpose, const float* deg_in, float* out, size_t out_bytes, float* deg_out,
                          size_t deg_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_dense_mean_agg_f32";
  if (int rc = dp_shape(fn, B, N, 1, F)) return rc;
  DN_CHECK_PTR(fn, "adj", adj);
  DN_CHECK_PTR(fn, "x", x);
  DN_CHECK_PTR(fn, "out", out);
  MP_CHECK_ARG(add_loop == 0 || add_loop == 1, "%s: add_loop = %d (0 or 1)", fn, add_loop);
  MP_CHECK_ARG(transpose == 0 || transpose == 1, "%s: transpose = %d (0 or 1)", fn, transpose);
  if (transpose) {
    DN_CHECK_PTR(fn, "deg_in", deg_in);
    MP_CHECK_ARG(deg_out == nullptr, "%s: deg_out is the forward's output (transpose = 0)", fn);
  } else {
    DN_CHECK_PTR(fn, "deg_out", deg_out);
    MP_CHECK_ARG(deg_in == nullptr, "%s: deg_in belongs to the transposed call", fn);
    MP_CHECK_EXTENT(fn, "deg_out", deg_bytes, (size_t)B * N * sizeof(float));
  }
  MP_CHECK_EXTENT(fn, "out", out_bytes, (size_t)B * N * F * sizeof(float));
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  const int64_t nn = N * N, nf = N * (int64_t)F;
  DnGemm g = transpose ? dn_gemm(adj, nn, 1, N, x, nf, F, 1, out, nf, F, N, F, N)
                       : dn_gemm(adj, nn, N, 1, x, nf, F, 1, out, nf, F, N, F, N);
  g.diag_one = add_loop;
  if (transpose) {
    g.bscale = deg_in;
  } else {
    g.epi = kEpiDeg, g.deg = deg_out;
  }
  dn_launch(g, B, st);
  *launches = 1;
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int dense_rows(const char* fn, bool scatter, const float* src, int64_t n, int32_t F, const int64_t* starts,
                      int64_t B, int64_t Nmax, float fill, float* dst, size_t dst_bytes, uint8_t* mask,
                      size_t mask_bytes, void* stream, int64_t* launches) {
  MP_CHECK_ARG(n >= 0, "%s: n = %lld < 0", fn, (long long)n);
  MP_CHECK_ARG(F >= 1, "%s: F = %d < 1", fn, F);
  MP_CHECK_ARG(B >= 0, "%s: B = %lld < 0", fn, (long long)B);
  MP_CHECK_ARG(Nmax >= 0, "%s: Nmax = %lld < 0", fn, (long long)Nmax);
  MP_CHECK_ARG(starts != nullptr && dn_al(starts, 8), "%s: starts is %s", fn, starts ? "not 8-byte aligned" : "NULL");
  const int64_t dense = B * Nmax;
  MP_CHECK_ARG((scatter ? n == 0 : dense == 0) || (src != nullptr && dn_al(src, 4)), "%s: %s is %s", fn,
               scatter ? "x" : "g", src ? "not 4-byte aligned" : "NULL");
  MP_CHECK_ARG((scatter ? dense == 0 : n == 0) || (dst != nullptr && dn_al(dst, 4)), "%s: %s is %s", fn,
               scatter ? "out" : "dx", dst ? "not 4-byte aligned" : "NULL");
  MP_CHECK_EXTENT(fn, scatter ? "out" : "dx", dst_bytes, (size_t)(scatter ? dense : n) * F * sizeof(float));
  if (scatter) {
    MP_CHECK_ARG(dense == 0 || mask != nullptr, "%s: mask is NULL", fn);
    MP_CHECK_EXTENT(fn, "mask", mask_bytes, (size_t)dense);
  }
  *launches = 0;
  if (dense == 0) return MP_OK;
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  const dim3 grid(dn_blocks(dense * F, 256));
  if (scatter) {
    hipLaunchKernelGGL(k_dense_rows<true>, grid, dim3(256), 0, st, src, F, starts, B, Nmax, fill, dst, mask);
  } else {
    hipLaunchKernelGGL(k_dense_rows<false>, grid, dim3(256), 0, st, src, F, starts, B, Nmax, fill, dst, mask);
  }
  *launches = 1;
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int dense_adj(const int64_t* row, const int64_t* col, int64_t E, const float* attr, int32_t D,
                     const int64_t* batch, int64_t n, const int64_t* starts, int64_t B, int64_t Nmax, float* out,
                     size_t out_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_to_dense_adj_f32";
  MP_CHECK_ARG(E >= 0, "%s: E = %lld < 0", fn, (long long)E);
  MP_CHECK_ARG(D >= 0, "%s: D = %d < 0", fn, D);
  MP_CHECK_ARG(n >= 0, "%s: n = %lld < 0", fn, (long long)n);
  MP_CHECK_ARG(B >= 0, "%s: B = %lld < 0", fn, (long long)B);
  MP_CHECK_ARG(Nmax >= 0, "%s: Nmax = %lld < 0", fn, (long long)Nmax);
  MP_CHECK_ARG((D > 0) == (attr != nullptr), "%s: edge_attr %s with D = %d", fn, attr ? "given" : "NULL", D);
  DN_CHECK_OPT(fn, "edge_attr", attr);
  MP_CHECK_ARG(E == 0 || (row != nullptr && dn_al(row, 8)), "%s: row is %s", fn, row ? "not 8-byte aligned" : "NULL");
  MP_CHECK_ARG(E == 0 || (col != nullptr && dn_al(col, 8)), "%s: col is %s", fn, col ? "not 8-byte aligned" : "NULL");
  MP_CHECK_ARG(dn_al(batch, 8), "%s: batch is not 8-byte aligned", fn);
  MP_CHECK_ARG(starts != nullptr && dn_al(starts, 8), "%s: starts is %s", fn, starts ? "not 8-byte aligned" : "NULL");
  MP_CHECK_ARG(batch != nullptr || B <= 1, "%s: batch is NULL with B = %lld graphs", fn, (long long)B);
  const int64_t cells = B * Nmax * Nmax, per = D > 0 ? D : 1;
  MP_CHECK_ARG(cells == 0 || (out != nullptr && dn_al(out, 4)), "%s: out is %s", fn,
               out ? "not 4-byte aligned" : "NULL");
  MP_CHECK_EXTENT(fn, "out", out_bytes, (size_t)cells * per * sizeof(float));
  const DenseAdjWs w(ws, B, Nmax, D);
  MP_CHECK_ARG(ws != nullptr && dn_al(ws, 16), "%s: ws is %s", fn, ws ? "not 16-byte aligned" : "NULL");
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  *launches = 0;
  if (cells == 0) return MP_OK;
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  MP_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)cells * per * sizeof(float), st));
  ++*launches;
  if (E > 0 && D == 0) {
    hipLaunchKernelGGL(k_dense_adj<0>, dim3(dn_blocks(E, 256)), dim3(256), 0, st, row, col, E, attr, D, batch, starts,
                       n, B, Nmax, out, w.win);
    ++*launches;
  } else if (E > 0) {
    MP_CHECK_HIP(hipMemsetAsync(w.win, 0, (size_t)cells * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_dense_adj<1>, dim3(dn_blocks(E, 256)), dim3(256), 0, st, row, col, E, attr, D, batch, starts,
                       n, B, Nmax, out, w.win);
    hipLaunchKernelGGL(k_dense_adj<2>, dim3(dn_blocks(E * D, 256)), dim3(256), 0, st, row, col, E, attr, D, batch,
                       starts, n, B, Nmax, out, w.win);
    *launches += 3;
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_diff_pool_path(int64_t N, int32_t C, int32_t F) {
  if (N < 1 || C < 1 || F < 1) {
    set_error("mp_diff_pool_path: N = %lld, C = %d, F = %d (each >= 1)", (long long)N, C, F);
    return -(int64_t)MP_ERR_ARG;
  }
  return dp_path(N, C);
}

extern "C" size_t mp_diff_pool_workspace(int64_t B, int64_t N, int32_t C, int32_t F) {
  (void)F;
  if (B < 1 || N < 1 || C < 1) return DiffPoolWs{nullptr, 1, 1, 1}.total(0);
  return DiffPoolWs{nullptr, B, N, C}.total(0);
}

extern "C" size_t mp_diff_pool_bwd_workspace(int64_t B, int64_t N, int32_t C, int32_t F) {
  (void)N, (void)F;
  if (B < 1 || C < 1) return DiffPoolBwdWs{nullptr, 1, 1}.total(0);
  return DiffPoolBwdWs{nullptr, B, C}.total(0);
}

extern "C" int64_t mp_dense_diff_pool_f32(const float* x, const float* adj, const float* s, const uint8_t* mask,
                                          int64_t B, int64_t N, int32_t C, int32_t F, float* out, size_t out_bytes,
                                          float* out_adj, size_t out_adj_bytes, float* loss, size_t loss_bytes,
                                          float* P, size_t P_bytes, float* T, size_t T_bytes, float* V, size_t V_bytes,
                                          void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = diff_pool_fwd(x, adj, s, mask, B, N, C, F, out, out_bytes, out_adj, out_adj_bytes, loss, loss_bytes,
                               P, P_bytes, T, T_bytes, V, V_bytes, ws, ws_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_dense_diff_pool_bwd_f32(const float* g_out, const float* g_oa, const float* g_loss,
                                              const float* x, const float* P, const float* T, const float* V,
                                              const float* loss, int64_t B, int64_t N, int32_t C, int32_t F,
                                              float* dx, size_t dx_bytes, float* ds, size_t ds_bytes, void* ws,
                                              size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = diff_pool_bwd(g_out, g_oa, g_loss, x, P, T, V, loss, B, N, C, F, dx, dx_bytes, ds, ds_bytes, ws,
                               ws_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_dense_mean_agg_f32(const float* adj, const float* x, int64_t B, int64_t N, int32_t F,
                                         int32_t add_loop, int32_t transpose, const float* deg_in, float* out,
                                         size_t out_bytes, float* deg_out, size_t deg_out_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dense_mean_agg(adj, x, B, N, F, add_loop, transpose, deg_in, out, out_bytes, deg_out, deg_out_bytes,
                                stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_to_dense_batch_f32(const float* x, int64_t n, int32_t F, const int64_t* starts, int64_t B,
                                         int64_t Nmax, float fill, float* out, size_t out_bytes, uint8_t* mask,
                                         size_t mask_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dense_rows("mp_to_dense_batch_f32", true, x, n, F, starts, B, Nmax, fill, out, out_bytes, mask,
                            mask_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_to_dense_batch_bwd_f32(const float* g, int64_t n, int32_t F, const int64_t* starts, int64_t B,
                                             int64_t Nmax, float* dx, size_t dx_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dense_rows("mp_to_dense_batch_bwd_f32", false, g, n, F, starts, B, Nmax, 0.f, dx, dx_bytes, nullptr,
                            0, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" size_t mp_to_dense_adj_workspace(int64_t B, int64_t Nmax, int32_t D) {
  if (B < 0 || Nmax < 0 || D < 0) return DenseAdjWs{nullptr, 0, 0, 0}.total(0);
  return DenseAdjWs{nullptr, B, Nmax, D}.total(0);
}

extern "C" int64_t mp_to_dense_adj_f32(const int64_t* row, const int64_t* col, int64_t E, const float* edge_attr,
                                       int32_t D, const int64_t* batch, int64_t n, const int64_t* starts, int64_t B,
                                       int64_t Nmax, float* out, size_t out_bytes, void* ws, size_t ws_bytes,
                                       void* stream) {
  int64_t launches = 0;
  const int rc = dense_adj(row, col, E, edge_attr, D, batch, n, starts, B, Nmax, out, out_bytes, ws, ws_bytes, stream,
                           &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}
