// GMMConv's aggregation (gfx950): the Gaussian mixture weights of MoNet are
// evaluated inside the segmented pass, so no per-edge coefficient array exists.
//
// Per edge e = (j -> i) with pseudo-coordinates p_e in R^D the shared-Gaussian
// layer's message is m_e = sum_k w_k(p_e) Y[j, k, :], Y = (x g).view(N, K, M),
//   w_k(p) = exp(sum_d -0.5 (p_d - mu_kd)^2 * iv_kd),  iv_kd = 1 / (1e-15f + sigma_kd^2)
// With G'[(k, c), m] = g[c, k*M + m] the per-edge step is reordered like NNConv's:
//   bins form    Z[i, k*Cin + c] = scale[i] * sum_{e -> i} w_k(p_e) * x[j, c]
//                then out = Z @ G'                                  (aggregate first)
//   gather form  out[i, f] = scale[i] * sum_{e -> i} sum_k w_k(p_e) * Y[j, k*F + f] (+ bias)
//                                                                   (transform first)
// and the backward needs, besides the same two over the transposed CSR, the
// gradients of mu, sigma and pseudo: with dw[e, k] = sum_c dZ[i_e, k*Cin + c] *
// x[j_e, c] and t = dw * w (w recomputed; no [E, K] array is written or read),
//   dmu[k, d]     = sum_e t * (p_d - mu_kd) * iv_kd
//   dsigma[k, d]  = sum_e t * ((p_d - mu_kd)^2 * iv_kd) * (sigma_kd * iv_kd)
//   dpseudo[e, d] = -sum_k t * (p_d - mu_kd) * iv_kd
// pseudo is [n_p_edges, ldp >= D] in ORIGINAL edge order, read through eid.
//
// Every workgroup stages mu and -0.5 * iv ([K, D] each, K * D <= 1024: 8 KiB)
// in LDS once; the slot loops read the table from there.  Both aggregate
// kernels walk rowptr / col / eid only; one owner per output entry visits its
// row's slots in slot order and adds left to right (the gather form: k = 0..K-1
// inside a slot): deterministic, no atomics, bitwise reproducible.  Lane mappings:
//   bins, Cin < 32   ("flat"): lanes run over the flattened q = k*Cin + c, a
//       row owned by g = min(64, pow2 >= K*Cin) lanes and 64/g rows per wave,
//       wider rows tiled by 64 over blockIdx.y.  Each lane evaluates the weight
//       of its own k: one evaluation per (slot, k) per lane group when Cin = 1.
//   bins, Cin >= 32  ("columns"): one wave per (row, 64 columns c, 16 values
//       of k).  The row is wave-uniform, so a slot's weights are too: the wave
//       takes four slots at a time, lane l evaluates the weight of (slot l / 16,
//       k0 + l % 16), and the accumulation reads them back with readlane -- one
//       exp per (slot, k) per wave instead of one per lane.
//   gather: lanes map to f (g = min(64, pow2 >= F) lanes per row, 64/g rows
//       per wave, F tiled by 64).  A row's (slot, k) pairs are taken g at a
//       time: lane l of the group evaluates pair l of the batch, the batch is
//       handed round by readlane (g = 64, scalar) or a group-wide shuffle, and
//       eight y loads are in flight per lane.
//   param grad: a workgroup per chunk of edges; a lane per (edge, k) (64 / K
//       edges per wave step, k strided by 64 above K = 64) forms dw serially
//       over c (16-byte loads where Cin and the strides allow), and adds its
//       2 D terms into its own LDS accumulators; dpseudo sums over k in k order
//       through an LDS row of t.  The accumulator sets are added in a fixed
//       order into the chunk's partial, the partials in chunk order by a second
//       kernel: the result does not depend on the grid.
// An (edge, k) whose weight underflows to 0 contributes exactly 0 to every
// gradient (upstream's autograd yields NaN there: 0 * inf).
// Rows of any length are summed serially by their owner; hub rows are not split.
#include "mp_workspace.h"

namespace mp {

constexpr int64_t kGmmMaxRow = 1 << 20;   // floats in one row of Z or Y (4 MiB)
constexpr int kGmmMaxTable = 1024;        // K * D: mu and iv staged in LDS, 8 KiB
constexpr int kGmmColumnsMinCin = 32;     // bins: lanes over c from here on
constexpr int kGmmKTile = 16;             // bins, columns mapping: accumulators per lane
constexpr int kGmmSlotBatch = 64 / kGmmKTile;  // bins, columns mapping: slots whose weights one wave evaluates at once
constexpr int kGmmGatherInFlight = 8;     // gather: y loads in flight per lane
constexpr int64_t kGmmGradMinChunk = 1024;     // param grad: edges per stage-1 workgroup, at least
constexpr int64_t kGmmGradMaxChunks = 4096;    // and chunks at most (fewer at a large K * D)
constexpr int64_t kGmmGradMaxPartFloats = 1 << 21;  // the chunk partials: at most 8 MiB
constexpr float kGmmEps = 1e-15f;

static inline int gmm_group_log2(int64_t n) {
  int gl = 0;
  while ((1 << gl) < n && gl < 6) ++gl;
  return gl;
}

__device__ __forceinline__ float gmm_inv_var(float s) { return __fdiv_rn(1.f, __fadd_rn(kGmmEps, __fmul_rn(s, s))); }

// tab[0 .. KD): mu, tab[KD .. 2 KD): -0.5 * iv; every thread of the workgroup calls it
__device__ __forceinline__ void gmm_stage(float* tab, const float* __restrict__ mu, const float* __restrict__ sigma,
                                          int KD) {
  for (int i = threadIdx.x; i < KD; i += blockDim.x) {
    tab[i] = mu[i];
    tab[KD + i] = __fmul_rn(-0.5f, gmm_inv_var(sigma[i]));
  }
  __syncthreads();
}

// w_k(p): q adds d = 0..D-1 in order
__device__ __forceinline__ float gmm_weight(const float* tab, int KD, int k, int D, const float* __restrict__ p) {
  const float* m = tab + k * D;
  float q = 0.f;
  for (int d = 0; d < D; ++d) {
    const float t = __fsub_rn(p[d], m[d]);
    q = __fadd_rn(q, __fmul_rn(__fmul_rn(t, t), m[KD + d]));
  }
  return __expf(q);
}

// ---------------------------------------------------------------------------
// bins form, lanes over the flattened (k, c)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gmm_bins_flat(const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ eid, int64_t n_rows,
                                                       const float* __restrict__ pseudo, int64_t ldp, int32_t D,
                                                       const float* __restrict__ mu, const float* __restrict__ sigma,
                                                       int32_t K, const float* __restrict__ x, int64_t ldx, int32_t Cin,
                                                       int32_t glog, const float* __restrict__ row_scale,
                                                       float* __restrict__ out, int64_t ldo) {
  extern __shared__ float tab[];
  const int KD = K * D;
  gmm_stage(tab, mu, sigma, KD);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int q = blockIdx.y * 64 + fl;
  if (r >= n_rows || q >= K * Cin) return;
  const int kk = q / Cin;
  const int c = q - kk * Cin;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc = 0.f;
  int32_t nc = 0, ne = 0;
  if (b < e) {
    nc = col[b];
    ne = eid[b];
  }
  for (int k = b; k < e; ++k) {
    const int32_t cc = nc;
    const int64_t id = ne;
    if (k + 1 < e) {
      nc = col[k + 1];
      ne = eid[k + 1];
    }
    const float xv = x[(int64_t)cc * ldx + c];
    const float w = gmm_weight(tab, KD, kk, D, pseudo + id * ldp);
    acc = __fadd_rn(acc, __fmul_rn(w, xv));
  }
  if (row_scale) acc = __fmul_rn(acc, row_scale[r]);
  out[r * ldo + q] = acc;
}

// ---------------------------------------------------------------------------
// bins form, lanes over c; wave = (row, 64 columns, kGmmKTile values of k).
// Every lane stays active to the end: lanes beyond Cin still evaluate weights.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gmm_bins_cols(const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ eid, int64_t n_rows,
                                                       const float* __restrict__ pseudo, int64_t ldp, int32_t D,
                                                       const float* __restrict__ mu, const float* __restrict__ sigma,
                                                       int32_t K, const float* __restrict__ x, int64_t ldx, int32_t Cin,
                                                       const float* __restrict__ row_scale, float* __restrict__ out,
                                                       int64_t ldo) {
  constexpr int T = kGmmKTile;
  constexpr int S = kGmmSlotBatch;
  extern __shared__ float tab[];
  const int KD = K * D;
  gmm_stage(tab, mu, sigma, KD);
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
  const int c = blockIdx.y * 64 + lane;
  const int k0 = blockIdx.z * T;
  if (r >= n_rows) return;  // wave-uniform
  const bool has_c = c < Cin;
  const int ws = lane / T;        // the slot of the batch and
  const int wk = k0 + lane % T;   // the k whose weight this lane evaluates
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  for (int k = b; k < e; k += S) {
    float wv = 0.f;
    if (k + ws < e && wk < K) wv = gmm_weight(tab, KD, wk, D, pseudo + (int64_t)eid[k + ws] * ldp);
    float xv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) xv[s] = (k + s < e && has_c) ? x[(int64_t)col[k + s] * ldx + c] : 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (k + s < e) {  // wave-uniform
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __fadd_rn(acc[t], __fmul_rn(readlane(wv, s * T + t), xv[s]));
      }
    }
  }
  if (!has_c) return;
  const float sc = row_scale ? row_scale[r] : 1.f;
  float* o = out + r * ldo + c;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int kk = k0 + t;
    if (kk < K) o[(int64_t)kk * Cin] = row_scale ? __fmul_rn(acc[t], sc) : acc[t];
  }
}

// ---------------------------------------------------------------------------
// gather form: y is [n_cols, K, F].  UNI: one row per wave (g = 64), the batch's
// weights are read back as scalars; U: y loads in flight per lane.  Every lane
// of a live row group stays active to the end (its weights are read by the group).
// ---------------------------------------------------------------------------
template <bool UNI, int U>
__global__ __launch_bounds__(256) void k_gmm_gather(const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col,
                                                    const int32_t* __restrict__ eid, int64_t n_rows,
                                                    const float* __restrict__ pseudo, int64_t ldp, int32_t D,
                                                    const float* __restrict__ mu, const float* __restrict__ sigma,
                                                    int32_t K, const float* __restrict__ y, int64_t ldy, int32_t F,
                                                    int32_t glog, const float* __restrict__ row_scale,
                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                    int64_t ldo) {
  extern __shared__ float tab[];
  const int KD = K * D;
  gmm_stage(tab, mu, sigma, KD);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int g = UNI ? 64 : (1 << glog);
  const int sub = UNI ? 0 : (lane >> glog);
  const int fl = lane & (g - 1);
  const int base = lane - fl;  // the group's first lane
  const int64_t r = UNI ? (int64_t)blockIdx.x * 4 + uni(wave) : ((((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub);
  const int f = blockIdx.y * 64 + fl;
  if (r >= n_rows) return;  // a whole group
  const bool has_f = f < F;
  const int b = rowptr[r], e = rowptr[r + 1];
  const int64_t total = (int64_t)(e - b) * K;  // the row's (slot, k) pairs
  // the pair this lane evaluates in the current batch, and its step from batch to batch
  int64_t ps = b + fl / K;
  int pk = fl % K;
  const int gq = g / K, gr = g % K;
  // the pair being accumulated
  int cs = b, ck = 0;
  int32_t cc = 0, nc = 0;
  if (b < e) {
    cc = col[b];
    if (b + 1 < e) nc = col[b + 1];
  }
  float acc = 0.f;
  for (int64_t p0 = 0; p0 < total; p0 += g) {
    float wv = 0.f;
    if (ps < e) wv = gmm_weight(tab, KD, pk, D, pseudo + (int64_t)eid[ps] * ldp);
    ps += gq;
    pk += gr;
    if (pk >= K) {
      pk -= K;
      ++ps;
    }
    const int n = total - p0 < g ? (int)(total - p0) : g;
    for (int i0 = 0; i0 < n; i0 += U) {
      float wu[U], yu[U];
      bool lv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u;
        lv[u] = i < n;
        float w;
        if constexpr (UNI) w = readlane(wv, uni(i & 63));
        else w = __shfl(wv, base + (i & (g - 1)));
        wu[u] = w;
        yu[u] = (lv[u] && has_f) ? y[(int64_t)cc * ldy + (int64_t)ck * F + f] : 0.f;
        if (lv[u] && ++ck == K) {  // the next slot; its column was loaded a slot ahead
          ck = 0;
          ++cs;
          cc = nc;
          if (cs + 1 < e) nc = col[cs + 1];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (lv[u]) acc = __fadd_rn(acc, __fmul_rn(wu[u], yu[u]));
      }
    }
  }
  if (!has_f) return;
  if (row_scale) acc = __fmul_rn(acc, row_scale[r]);
  if (bias) acc = __fadd_rn(acc, bias[f]);
  out[r * ldo + f] = acc;
}

// ---------------------------------------------------------------------------
// param grad, stage 1: one workgroup per chunk of edges
// ---------------------------------------------------------------------------

// edges one wave takes per step: a lane per (edge, k); the accumulator sets (4 waves * nE * 2 K D floats) stay
// within 32 KiB
static inline int gmm_grad_edges_per_wave(int K, int D) {
  if (K >= 64) return 1;
  const int by_lanes = 64 / K, by_lds = kGmmMaxTable / (K * D);
  const int n = by_lanes < by_lds ? by_lanes : by_lds;
  return n < 1 ? 1 : n;
}
static inline size_t gmm_grad_lds_bytes(int K, int D) {
  const int KD = K * D, nE = gmm_grad_edges_per_wave(K, D);
  return ((size_t)3 * KD + (size_t)4 * nE * 2 * KD + (size_t)4 * (K > 64 ? K : 64)) * sizeof(float);
}

// V = 4: 16-byte loads of dz and x (Cin, the strides and the base pointers multiples of four floats); V = 1
// otherwise.  dw adds c = 0..Cin-1 in order whatever V: the two are bitwise equal.
template <int V>
__global__ __launch_bounds__(256) void k_gmm_grad_part(const int64_t* __restrict__ rows,
                                                       const int64_t* __restrict__ cols, int64_t n_edges,
                                                       int64_t chunk, const float* __restrict__ pseudo, int64_t ldp,
                                                       int32_t D, const float* __restrict__ mu,
                                                       const float* __restrict__ sigma, int32_t K,
                                                       const float* __restrict__ dz, int64_t lddz,
                                                       const float* __restrict__ x, int64_t ldx, int32_t Cin,
                                                       int32_t nE, float* __restrict__ dpseudo, int64_t lddp,
                                                       float* __restrict__ part) {
  extern __shared__ float sm[];
  const int KD = K * D;
  const int tw = K > 64 ? K : 64;
  float* tmu = sm;                    // mu
  float* tiv = sm + KD;               // iv
  float* tsv = sm + 2 * KD;           // sigma * iv
  float* acc = sm + 3 * KD;           // [4 waves * nE][dmu K D | dsigma K D]
  float* tb = acc + 4 * nE * 2 * KD;  // [4 waves][tw]: t of the wave's edges, for dpseudo
  for (int i = threadIdx.x; i < KD; i += 256) {
    const float s = sigma[i];
    const float iv = gmm_inv_var(s);
    tmu[i] = mu[i];
    tiv[i] = iv;
    tsv[i] = __fmul_rn(s, iv);
  }
  for (int i = threadIdx.x; i < 4 * nE * 2 * KD; i += 256) acc[i] = 0.f;
  __syncthreads();
  const int lane = lane_id();
  const int wave = uni((int)(threadIdx.x >> 6));
  const int gw = K < 64 ? K : 64;  // lanes of one edge
  const int es = lane / gw;
  const int kl = lane - es * gw;
  const bool lane_ok = es < nE;
  float* my = acc + (size_t)(wave * nE + (lane_ok ? es : 0)) * 2 * KD;
  float* tbw = tb + wave * tw + (lane_ok ? es : 0) * (K < 64 ? K : 0);
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n_edges ? lo + chunk : n_edges;
  for (int64_t e0 = lo + (int64_t)wave * nE; e0 < hi; e0 += 4 * nE) {  // wave-uniform
    const int64_t e = e0 + es;
    const bool live = lane_ok && e < hi;
    const float* pr = pseudo + (live ? e : lo) * ldp;
    if (live) {
      const float* dr = dz + rows[e] * lddz;
      const float* xr = x + cols[e] * ldx;
      for (int k = kl; k < K; k += 64) {  // one pass up to K = 64
        const float* m = tmu + k * D;
        const float* iv = tiv + k * D;
        float q = 0.f;
        for (int d = 0; d < D; ++d) {
          const float df = __fsub_rn(pr[d], m[d]);
          q = __fadd_rn(q, __fmul_rn(__fmul_rn(df, df), __fmul_rn(-0.5f, iv[d])));
        }
        const float w = __expf(q);
        float t = 0.f;
        if (w != 0.f) {  // an underflowed weight contributes exactly zero
          const float* dk = dr + (int64_t)k * Cin;
          float dw = 0.f;
          if constexpr (V == 4) {
            for (int c = 0; c < Cin; c += 4) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(dk + c);
              const f32x4 b = *reinterpret_cast<const f32x4*>(xr + c);
              dw = __fadd_rn(dw, __fmul_rn(a.x, b.x));
              dw = __fadd_rn(dw, __fmul_rn(a.y, b.y));
              dw = __fadd_rn(dw, __fmul_rn(a.z, b.z));
              dw = __fadd_rn(dw, __fmul_rn(a.w, b.w));
            }
          } else {
            for (int c = 0; c < Cin; ++c) dw = __fadd_rn(dw, __fmul_rn(dk[c], xr[c]));
          }
          t = __fmul_rn(dw, w);
          const float* sv = tsv + k * D;
          float* am = my + k * D;
          for (int d = 0; d < D; ++d) {
            const float df = __fsub_rn(pr[d], m[d]);
            const float a = __fmul_rn(df, iv[d]);
            am[d] = __fadd_rn(am[d], __fmul_rn(t, a));
            am[KD + d] = __fadd_rn(am[KD + d], __fmul_rn(__fmul_rn(t, __fmul_rn(df, a)), sv[d]));
          }
        }
        if (dpseudo) tbw[k] = t;
      }
    }
    if (dpseudo) {
      __builtin_amdgcn_wave_barrier();  // LDS ops of one wave run in order: the reads below see the stores
      if (live) {
        for (int d = kl; d < D; d += gw) {
          const float pd = pr[d];
          float s = 0.f;
          for (int k = 0; k < K; ++k) {
            const float t = tbw[k];
            if (t != 0.f) s = __fadd_rn(s, __fmul_rn(t, __fmul_rn(__fsub_rn(pd, tmu[k * D + d]), tiv[k * D + d])));
          }
          dpseudo[e * lddp + d] = -s;
        }
      }
      __builtin_amdgcn_wave_barrier();  // the next step's stores follow these reads
    }
  }
  __syncthreads();
  // the accumulator sets in set order: (wave, edge of the step) ascending
  float* po = part + (int64_t)blockIdx.x * 2 * KD;
  for (int i = threadIdx.x; i < 2 * KD; i += 256) {
    float s = 0.f;
    for (int j = 0; j < 4 * nE; ++j) s = __fadd_rn(s, acc[(size_t)j * 2 * KD + i]);
    po[i] = s;
  }
}

// stage 2: the chunk partials in chunk order (zeros without edges)
__global__ __launch_bounds__(256) void k_gmm_grad_sum(const float* __restrict__ part, int64_t n_chunks, int32_t KD,
                                                      float* __restrict__ dmu, float* __restrict__ dsigma) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * KD) return;
  float s = 0.f;
#pragma unroll 8
  for (int64_t j = 0; j < n_chunks; ++j) s = __fadd_rn(s, part[j * 2 * KD + i]);
  if (i < KD) dmu[i] = s; else dsigma[i - KD] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// (K, D) and one channel count C of the fused path: a table of K * D entries, a row of K * C floats
static int gmm_shape(const char* fn, int32_t K, int32_t D, int32_t C, const char* cname) {
  MP_CHECK_ARG(K >= 1, "%s: K = %d < 1", fn, K);
  MP_CHECK_ARG(D >= 1, "%s: D = %d < 1", fn, D);
  MP_CHECK_ARG(C >= 1, "%s: %s = %d < 1", fn, cname, C);
  MP_CHECK_ARG((int64_t)K * D <= kGmmMaxTable, "%s: K * D = %lld above the limit K * D <= %d", fn,
               (long long)((int64_t)K * D), kGmmMaxTable);
  MP_CHECK_ARG((int64_t)K * C <= kGmmMaxRow, "%s: K * %s = %lld above the limit K * C <= %lld", fn, cname,
               (long long)((int64_t)K * C), (long long)kGmmMaxRow);
  return MP_OK;
}

static int gmm_csr(const char* fn, const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp, int32_t D,
                   const float* mu, const float* sigma) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the GMMConv passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (pseudo is read in original edge order)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  MP_CHECK_ARG(n_p_edges >= ids, "%s: eid indexes %lld edges, pseudo holds n_p_edges = %lld rows", fn, (long long)ids,
               (long long)n_p_edges);
  MP_CHECK_ARG(ldp >= D, "%s: ldp = %lld < D = %d", fn, (long long)ldp, D);
  MP_CHECK_ARG(pseudo != nullptr || g->n_edges == 0, "%s: pseudo is NULL", fn);
  MP_CHECK_ARG(mu != nullptr, "%s: mu is NULL", fn);
  MP_CHECK_ARG(sigma != nullptr, "%s: sigma is NULL", fn);
  return MP_OK;
}

static inline int64_t gmm_grad_chunk(int64_t n_edges, int32_t K, int32_t D) {
  const int64_t by_ws = kGmmGradMaxPartFloats / (2 * (int64_t)K * D);
  const int64_t max_chunks = by_ws < kGmmGradMaxChunks ? by_ws : kGmmGradMaxChunks;
  const int64_t c = ceil_div(ceil_div(n_edges > 0 ? n_edges : 0, max_chunks), 256) * 256;
  return c < kGmmGradMinChunk ? kGmmGradMinChunk : c;
}

// part [n_chunks, 2 K D] of one mp_gmm_param_grad_f32 call
struct GmmGradWs : Carver {
  int64_t chunk, n_chunks;
  float* part;
  GmmGradWs(void* ws, int64_t n_edges, int32_t K, int32_t D)
      : Carver(ws),
        chunk(gmm_grad_chunk(n_edges, K, D)),
        n_chunks(ceil_div(n_edges > 0 ? n_edges : 0, chunk)),
        part(take<float>(n_chunks * 2 * K * D)) {}
};

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_gmm_ok(int32_t K, int32_t D, int32_t Cin, int32_t Cout) {
  const char* fn = "mp_gmm_ok";
  return gmm_shape(fn, K, D, Cin, "Cin") == MP_OK && gmm_shape(fn, K, D, Cout, "Cout") == MP_OK ? 1 : 0;
}

static int gmm_bins(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp, int32_t D, const float* mu,
                    const float* sigma, int32_t K, const float* x, int64_t ldx, int32_t Cin, const float* row_scale,
                    float* out, int64_t ldo, void* stream) {
  const char* fn = "mp_gmm_aggregate_bins_f32";
  if (int rc = gmm_shape(fn, K, D, Cin, "Cin")) return rc;
  if (int rc = gmm_csr(fn, g, pseudo, n_p_edges, ldp, D, mu, sigma)) return rc;
  const int64_t Q = (int64_t)K * Cin;
  MP_CHECK_ARG(ldx >= Cin, "%s: ldx = %lld < Cin = %d", fn, (long long)ldx, Cin);
  MP_CHECK_ARG(ldo >= Q, "%s: ldo = %lld < K * Cin = %lld", fn, (long long)ldo, (long long)Q);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  const size_t lds = (size_t)2 * K * D * sizeof(float);
  if (Cin < kGmmColumnsMinCin) {
    const int glog = gmm_group_log2(Q);
    const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
    const int64_t by = ceil_div(Q, 64);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, K * Cin %lld)", fn,
                 (long long)g->n_rows, (long long)Q);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_gmm_bins_flat, dim3((unsigned)bx, (unsigned)by), dim3(256), lds, as_stream(stream), g->rowptr,
                       g->col, g->eid, g->n_rows, pseudo, ldp, D, mu, sigma, K, x, ldx, Cin, glog, row_scale, out, ldo);
  } else {
    const int64_t bx = ceil_div(g->n_rows, 4);
    const int64_t by = ceil_div(Cin, 64);
    const int64_t bz = ceil_div(K, kGmmKTile);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535 && bz <= 65535, "%s: grid too large (n_rows %lld, K %d, Cin %d)", fn,
                 (long long)g->n_rows, K, Cin);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_gmm_bins_cols, dim3((unsigned)bx, (unsigned)by, (unsigned)bz), dim3(256), lds,
                       as_stream(stream), g->rowptr, g->col, g->eid, g->n_rows, pseudo, ldp, D, mu, sigma, K, x, ldx,
                       Cin, row_scale, out, ldo);
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int gmm_gather(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp, int32_t D, const float* mu,
                      const float* sigma, int32_t K, const float* y, int64_t ldy, int32_t F, const float* row_scale,
                      const float* bias, float* out, int64_t ldo, void* stream) {
  const char* fn = "mp_gmm_aggregate_gather_f32";
  if (int rc = gmm_shape(fn, K, D, F, "F")) return rc;
  if (int rc = gmm_csr(fn, g, pseudo, n_p_edges, ldp, D, mu, sigma)) return rc;
  const int64_t Q = (int64_t)K * F;
  MP_CHECK_ARG(ldy >= Q, "%s: ldy = %lld < K * F = %lld", fn, (long long)ldy, (long long)Q);
  MP_CHECK_ARG(ldo >= F, "%s: ldo = %lld < F = %d", fn, (long long)ldo, F);
  MP_CHECK_ARG(y != nullptr, "%s: y is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  const size_t lds = (size_t)2 * K * D * sizeof(float);
  const int glog = gmm_group_log2(F);
  const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
  const int64_t by = ceil_div(F, 64);
  MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, F %d)", fn, (long long)g->n_rows, F);
  MP_DEVICE_GUARD(stream);
  auto kern = glog == 6 ? k_gmm_gather<true, kGmmGatherInFlight>
                        : (glog >= 3 ? k_gmm_gather<false, kGmmGatherInFlight> : k_gmm_gather<false, 1>);
  hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)by), dim3(256), lds, as_stream(stream), g->rowptr, g->col,
                     g->eid, g->n_rows, pseudo, ldp, D, mu, sigma, K, y, ldy, F, glog, row_scale, bias, out, ldo);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int gmm_param_grad(const int64_t* rows, const int64_t* cols, int64_t n_edges, const float* pseudo, int64_t ldp,
                          int32_t D, const float* mu, const float* sigma, int32_t K, const float* dz, int64_t lddz,
                          const float* x, int64_t ldx, int32_t Cin, float* dmu, float* dsigma, float* dpseudo,
                          int64_t lddp, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_gmm_param_grad_f32";
  if (int rc = gmm_shape(fn, K, D, Cin, "Cin")) return rc;
  MP_CHECK_ARG(n_edges >= 0, "%s: n_edges < 0", fn);
  MP_CHECK_ARG(n_edges <= 0x7fffffff, "%s: n_edges too large", fn);
  MP_CHECK_ARG(ldp >= D, "%s: ldp = %lld < D = %d", fn, (long long)ldp, D);
  MP_CHECK_ARG(lddz >= (int64_t)K * Cin, "%s: lddz = %lld < K * Cin = %lld", fn, (long long)lddz,
               (long long)((int64_t)K * Cin));
  MP_CHECK_ARG(ldx >= Cin, "%s: ldx = %lld < Cin = %d", fn, (long long)ldx, Cin);
  MP_CHECK_ARG(dpseudo == nullptr || lddp >= D, "%s: lddp = %lld < D = %d", fn, (long long)lddp, D);
  MP_CHECK_ARG(mu != nullptr, "%s: mu is NULL", fn);
  MP_CHECK_ARG(sigma != nullptr, "%s: sigma is NULL", fn);
  MP_CHECK_ARG(dmu != nullptr, "%s: dmu is NULL", fn);
  MP_CHECK_ARG(dsigma != nullptr, "%s: dsigma is NULL", fn);
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  GmmGradWs w(ws, n_edges, K, D);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  if (n_edges > 0) {
    MP_CHECK_ARG(rows != nullptr, "%s: rows is NULL", fn);
    MP_CHECK_ARG(cols != nullptr, "%s: cols is NULL", fn);
    MP_CHECK_ARG(pseudo != nullptr, "%s: pseudo is NULL", fn);
    MP_CHECK_ARG(dz != nullptr, "%s: dz is NULL", fn);
    MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  }
  const int KD = K * D;
  MP_DEVICE_GUARD(stream);
  if (n_edges > 0) {
    const bool vec4 = Cin % 4 == 0 && lddz % 4 == 0 && ldx % 4 == 0 && (uintptr_t)dz % 16 == 0 && (uintptr_t)x % 16 == 0;
    hipLaunchKernelGGL(vec4 ? k_gmm_grad_part<4> : k_gmm_grad_part<1>, dim3((unsigned)w.n_chunks), dim3(256), gmm_grad_lds_bytes(K, D),
                       as_stream(stream), rows, cols, n_edges, w.chunk, pseudo, ldp, D, mu, sigma, K, dz, lddz, x, ldx,
                       Cin, gmm_grad_edges_per_wave(K, D), dpseudo, lddp, w.part);
    MP_CHECK_LAUNCH();
    ++*launches;
  }
  hipLaunchKernelGGL(k_gmm_grad_sum, dim3((unsigned)ceil_div(2 * KD, 256)), dim3(256), 0, as_stream(stream), w.part,
                     w.n_chunks, KD, dmu, dsigma);
  MP_CHECK_LAUNCH();
  ++*launches;
  return MP_OK;
}

// The entry points return int64_t like the NNConv ones: the launches enqueued
// (0 for an empty problem), or -(MP_ERR_* code).
static inline int64_t gmm_result(int rc, int64_t launches) { return rc != MP_OK ? -(int64_t)rc : launches; }

extern "C" int64_t mp_gmm_aggregate_bins_f32(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp,
                                             int32_t D, const float* mu, const float* sigma, int32_t K, const float* x,
                                             int64_t ldx, int32_t Cin, const float* row_scale, float* out, int64_t ldo,
                                             void* stream) {
  return gmm_result(gmm_bins(g, pseudo, n_p_edges, ldp, D, mu, sigma, K, x, ldx, Cin, row_scale, out, ldo, stream),
                    g != nullptr && g->n_rows > 0 ? 1 : 0);
}

extern "C" int64_t mp_gmm_aggregate_gather_f32(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp,
                                               int32_t D, const float* mu, const float* sigma, int32_t K,
                                               const float* y, int64_t ldy, int32_t F, const float* row_scale,
                                               const float* bias, float* out, int64_t ldo, void* stream) {
  return gmm_result(
      gmm_gather(g, pseudo, n_p_edges, ldp, D, mu, sigma, K, y, ldy, F, row_scale, bias, out, ldo, stream),
      g != nullptr && g->n_rows > 0 ? 1 : 0);
}

extern "C" int64_t mp_gmm_grad_chunk(int64_t n_edges, int32_t K, int32_t D) {
  if (n_edges < 0 || K < 1 || D < 1 || (int64_t)K * D > kGmmMaxTable) {
    set_error("mp_gmm_grad_chunk: n_edges = %lld, K = %d, D = %d outside n_edges >= 0, K, D >= 1, K * D <= %d",
              (long long)n_edges, K, D, kGmmMaxTable);
    return -(int64_t)MP_ERR_ARG;
  }
  return gmm_grad_chunk(n_edges, K, D);
}

extern "C" size_t mp_gmm_param_grad_workspace(int64_t n_edges, int32_t K, int32_t D) {
  if (n_edges < 0 || K < 1 || D < 1 || (int64_t)K * D > kGmmMaxTable) return GmmGradWs{nullptr, 0, 1, 1}.total(0);
  return GmmGradWs{nullptr, n_edges, K, D}.total(0);
}

extern "C" int64_t mp_gmm_param_grad_f32(const int64_t* rows, const int64_t* cols, int64_t n_edges,
                                         const float* pseudo, int64_t ldp, int32_t D, const float* mu,
                                         const float* sigma, int32_t K, const float* dz, int64_t lddz, const float* x,
                                         int64_t ldx, int32_t Cin, float* dmu, float* dsigma, float* dpseudo,
                                         int64_t lddp, void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = gmm_param_grad(rows, cols, n_edges, pseudo, ldp, D, mu, sigma, K, dz, lddz, x, ldx, Cin, dmu, dsigma,
                                dpseudo, lddp, ws, ws_bytes, stream, &launches);
  return gmm_result(rc, launches);
}
