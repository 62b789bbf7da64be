// SplineConv's aggregation (gfx950): open / closed B-spline bases of degree
// 1..3 over 1..3 pseudo-coordinate dimensions, fused into the gather ->
// weight -> segment-reduce pass of a destination-sorted CSR.
//
// Per edge e = (j -> i) with pseudo-coordinates u[e, 0..D) in [0, 1], kernel
// sizes ks[d], open flags op[d], degree M and S = (M+1)^D:
//   v_d = u[e,d] * float(ks[d] - M*op[d])          (one fp32 multiply)
//   f_d = v_d - floor(v_d)
//   for s in 0..S, with k_d the d-th base-(M+1) digit of s:
//     basis[e,s] = prod_d B_M(f_d, k_d)
//     wi[e,s]    = sum_d ((floor(v_d) + k_d) mod ks[d]) * prod_{d' < d} ks[d']
// and the layer's message is m_e = sum_s basis[e,s] * x_j W[wi[e,s]], W of shape
// [K = prod ks, Fin, Fout].  The per-edge step (E x S x Fin x Fout) is reordered
// into ONE segmented pass plus one dense GEMM:
//   bins form    A[i, k*F + f] = scale[i] * sum_{e -> i} sum_{s: wi = k} basis * x[j, f]
//                then out = A @ W.view(K*Fin, Fout)                (aggregate first)
//   gather form  out[i, f] = scale[i] * sum_{e -> i} sum_s basis * XW[j, wi*F + f] (+ bias)
//                with XW = x @ W laid out [n, K, Fout]             (transform first)
// Neither form keeps a basis or index array in memory: every slot's basis is
// recomputed from pseudo[eid[slot]] (original edge order, no permuted copy).
//
// Both walk rowptr / col / eid only (no wave schedule).  A row belongs to one
// group of g = min(64, pow2 >= F) lanes -- a wave carries 64/g rows, so the
// Fin = 1 first layer of a superpixel model fills its lanes -- and a wider F is
// tiled over blockIdx.y (the basis is recomputed per tile).  The owner visits
// its row's slots in slot order (= original edge order) and adds left to
// right: deterministic, no atomics, bitwise reproducible.  The bins form keeps
// a wave's accumulators in LDS (K bins x 64 lanes, lane-private columns: bank
// conflict free, no barrier), because a slot's bins are indexed dynamically.
//
// Rows of any length are summed serially by their owner; splitting hub rows
// is out of scope.  Such a pass runs as long as its most loaded wave: with
// rows at thousands of slots against a median of tens it is expected to run
// 1.5-3x longer than an evenly loaded one at equal bytes, and the remedy is to
// split slot lists longer than a quarter of one wave's share of the slots into
// chunks summed by separate waves, added in chunk order by a further pass.
#include "mp_common.h"

namespace mp {

constexpr int kSplineMaxDim = 3;
constexpr int kSplineMaxDegree = 3;
constexpr int kSplineMaxBins = 256;  // one wave's bins (K x 256 B) fit a 64 KiB workgroup

struct SplineGeom {
  int32_t ks[kSplineMaxDim];
  float span[kSplineMaxDim];  // float(ks[d] - M * op[d])
};

template <int M>
__device__ __forceinline__ float bspline(float f, int k) {
  if constexpr (M == 1) {
    return k == 0 ? 1.f - f : f;
  } else if constexpr (M == 2) {
    // (1-f)^2/2 and 1/2 + f(1-f): the expanded forms f^2/2 - f + 1/2 and -f^2 + f + 1/2
    // cancel near f = 1, where the value is tiny and a bin may hold nothing else
    if (k == 0) return 0.5f * (1.f - f) * (1.f - f);
    if (k == 1) return 0.5f + f * (1.f - f);
    return 0.5f * f * f;
  } else {
    if (k == 0) return (1.f - f) * (1.f - f) * (1.f - f) / 6.f;
    if (k == 1) return (3.f * f * f * f - 6.f * f * f + 4.f) / 6.f;
    if (k == 2) return (-3.f * f * f * f + 3.f * f * f + 3.f * f + 1.f) / 6.f;
    return f * f * f / 6.f;
  }
}

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

// Per-dimension tables of one edge: the M+1 basis values and the M+1 bin
// offsets.  Every index below is a constant after unrolling (registers only).
// Whatever the coordinate holds (outside [0, 1], NaN), every offset stays in
// [0, ks[d]) * stride: no bin or gathered column is ever out of range.
template <int D, int M>
struct EdgeBasis {
  static constexpr int S = ipow(M + 1, D);
  float b[D][M + 1];
  int32_t w[D][M + 1];

  __device__ __forceinline__ void set(const float (&u)[D], const SplineGeom& gm) {
    int off = 1;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int ks = gm.ks[d];
      const float v = __fmul_rn(u[d], gm.span[d]);
      const float fl = floorf(v);
      const float f = v - fl;
      int i0 = (int)fminf(fmaxf(fl, -1.0e9f), 1.0e9f) % ks;
      if (i0 < 0) i0 += ks;
#pragma unroll
      for (int k = 0; k <= M; ++k) {
        b[d][k] = bspline<M>(f, k);
        w[d][k] = ((i0 + k) % ks) * off;
      }
      off *= ks;
    }
  }
  __device__ __forceinline__ float basis(int s) const {
    float r = b[0][s % (M + 1)];
    if constexpr (D > 1) r = __fmul_rn(r, b[1][s / (M + 1) % (M + 1)]);
    if constexpr (D > 2) r = __fmul_rn(r, b[2][s / ((M + 1) * (M + 1))]);
    return r;
  }
  __device__ __forceinline__ int index(int s) const {
    int r = w[0][s % (M + 1)];
    if constexpr (D > 1) r += w[1][s / (M + 1) % (M + 1)];
    if constexpr (D > 2) r += w[2][s / ((M + 1) * (M + 1))];
    return r;
  }
};

// ---------------------------------------------------------------------------
// standalone basis, original edge order
// ---------------------------------------------------------------------------
template <int D, int M>
__global__ __launch_bounds__(256) void k_spline_basis(const float* __restrict__ pseudo, int64_t n_edges,
                                                      SplineGeom gm, float* __restrict__ basis,
                                                      int64_t* __restrict__ wi) {
  constexpr int S = EdgeBasis<D, M>::S;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  float u[D];
#pragma unroll
  for (int d = 0; d < D; ++d) u[d] = pseudo[e * D + d];
  EdgeBasis<D, M> eb;
  eb.set(u, gm);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    basis[e * S + s] = eb.basis(s);
    wi[e * S + s] = eb.index(s);
  }
}

// One slot's operands, loaded one slot ahead of their use.
template <int D>
struct SlotOps {
  float u[D];
  int32_t c;
};

template <int D>
__device__ __forceinline__ SlotOps<D> load_slot(const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
                                                const float* __restrict__ pseudo, int k) {
  SlotOps<D> o;
  o.c = col[k];
  const int64_t id = eid[k];
#pragma unroll
  for (int d = 0; d < D; ++d) o.u[d] = pseudo[id * D + d];
  return o;
}

// ---------------------------------------------------------------------------
// bins form.  Block = W waves (W * K * 256 B of LDS <= 64 KiB); wave w of block
// bx owns rows ((bx * W + w) << rsh) .. + (64 >> glog) - 1, lane group `sub` the
// row, lane `fl` of the group feature blockIdx.y * 64 + fl.  DISTINCT: every
// ks[d] > M, so a slot's S bins are pairwise different and their
// read-modify-writes are issued together.
// ---------------------------------------------------------------------------
template <int D, int M, bool DISTINCT>
__global__ __launch_bounds__(256) void k_spline_bins(const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col,
                                                     const int32_t* __restrict__ eid, int64_t n_rows,
                                                     const float* __restrict__ pseudo, SplineGeom gm, int32_t K,
                                                     const float* __restrict__ x, int64_t ldx, int32_t F,
                                                     int32_t glog, const float* __restrict__ row_scale,
                                                     float* __restrict__ out, int64_t ldo) {
  constexpr int S = EdgeBasis<D, M>::S;
  extern __shared__ __attribute__((aligned(16))) float spline_bins[];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  float* bins = spline_bins + (size_t)wave * K * 64 + lane;  // bin k of this lane: bins[k * 64]
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * waves + wave) << (6 - glog)) + sub;
  const int f = blockIdx.y * 64 + fl;
  const bool live = r < n_rows && f < F;
  if (!live) return;  // lane-private columns: no barrier follows
  for (int k = 0; k < K; ++k) bins[k * 64] = 0.f;
  const int b = rowptr[r], e = rowptr[r + 1];
  SlotOps<D> nxt;
  if (b < e) nxt = load_slot<D>(col, eid, pseudo, b);
  for (int k = b; k < e; ++k) {
    const SlotOps<D> cur = nxt;
    const float xv = x[(int64_t)cur.c * ldx + f];
    if (k + 1 < e) nxt = load_slot<D>(col, eid, pseudo, k + 1);
    EdgeBasis<D, M> eb;
    eb.set(cur.u, gm);
    if constexpr (DISTINCT) {
      float acc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = bins[eb.index(s) * 64];
#pragma unroll
      for (int s = 0; s < S; ++s) bins[eb.index(s) * 64] = __fadd_rn(acc[s], __fmul_rn(eb.basis(s), xv));
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        float* p = bins + eb.index(s) * 64;
        *p = __fadd_rn(*p, __fmul_rn(eb.basis(s), xv));
      }
    }
  }
  float* o = out + r * ldo + f;
  if (row_scale) {
    const float sc = row_scale[r];
    for (int k = 0; k < K; ++k) o[(int64_t)k * F] = __fmul_rn(bins[k * 64], sc);
  } else {
    for (int k = 0; k < K; ++k) o[(int64_t)k * F] = bins[k * 64];
  }
}

// ---------------------------------------------------------------------------
// gather form: x is [n_cols, K, F]; the S gathers of a slot are independent
// and issued together, then added in s order.
// ---------------------------------------------------------------------------
template <int D, int M>
__global__ __launch_bounds__(256) void k_spline_gather(const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ eid, int64_t n_rows,
                                                       const float* __restrict__ pseudo, SplineGeom gm,
                                                       const float* __restrict__ x, int64_t ldx, int32_t F,
                                                       int32_t glog, const float* __restrict__ row_scale,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       int64_t ldo) {
  constexpr int S = EdgeBasis<D, M>::S;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int f = blockIdx.y * 64 + fl;
  if (r >= n_rows || f >= F) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc = 0.f;
  SlotOps<D> nxt;
  if (b < e) nxt = load_slot<D>(col, eid, pseudo, b);
  for (int k = b; k < e; ++k) {
    const SlotOps<D> cur = nxt;
    if (k + 1 < e) nxt = load_slot<D>(col, eid, pseudo, k + 1);
    EdgeBasis<D, M> eb;
    eb.set(cur.u, gm);
    const float* xr = x + (int64_t)cur.c * ldx + f;
    float xv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) xv[s] = xr[(int64_t)eb.index(s) * F];
#pragma unroll
    for (int s = 0; s < S; ++s) acc = __fadd_rn(acc, __fmul_rn(eb.basis(s), xv[s]));
  }
  if (row_scale) acc = __fmul_rn(acc, row_scale[r]);
  if (bias) acc = __fadd_rn(acc, bias[f]);
  out[r * ldo + f] = acc;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Validates (D, degree, ks, open) and fills the geometry; K = prod ks.
static int spline_geom(const char* fn, int32_t D, int32_t degree, const int32_t* ks, const int32_t* open,
                       SplineGeom* gm, int32_t* K_out, bool* distinct) {
  MP_CHECK_ARG(D >= 1 && D <= kSplineMaxDim, "%s: D = %d outside [1, %d]", fn, D, kSplineMaxDim);
  MP_CHECK_ARG(degree >= 1 && degree <= kSplineMaxDegree, "%s: degree = %d outside [1, %d]", fn, degree,
               kSplineMaxDegree);
  MP_CHECK_ARG(ks != nullptr, "%s: kernel_size is NULL", fn);
  MP_CHECK_ARG(open != nullptr, "%s: is_open is NULL", fn);
  int64_t K = 1;
  *distinct = true;
  for (int d = 0; d < kSplineMaxDim; ++d) {
    gm->ks[d] = 1;
    gm->span[d] = 0.f;
  }
  for (int d = 0; d < D; ++d) {
    const int32_t o = open[d] != 0 ? 1 : 0;
    MP_CHECK_ARG(ks[d] >= 1 && ks[d] - degree * o >= 1,
                 "%s: kernel_size[%d] = %d leaves kernel_size - degree * is_open = %d < 1", fn, d, ks[d],
                 ks[d] - degree * o);
    MP_CHECK_ARG(ks[d] <= kSplineMaxBins, "%s: kernel_size[%d] = %d above the limit K <= %d", fn, d, ks[d],
                 kSplineMaxBins);
    K *= ks[d];
    MP_CHECK_ARG(K <= kSplineMaxBins, "%s: K = prod kernel_size = %lld above the limit K <= %d", fn, (long long)K,
                 kSplineMaxBins);
    gm->ks[d] = ks[d];
    gm->span[d] = (float)(ks[d] - degree * o);
    if (ks[d] <= degree) *distinct = false;
  }
  *K_out = (int32_t)K;
  return MP_OK;
}

static int spline_csr(const char* fn, const mp_csr* g, int64_t n_pseudo_edges) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the spline passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (pseudo is read in original edge order)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  MP_CHECK_ARG(n_pseudo_edges >= ids, "%s: eid indexes %lld edges, pseudo holds n_pseudo_edges = %lld rows", fn,
               (long long)ids, (long long)n_pseudo_edges);
  return MP_OK;
}

static inline int group_log2(int32_t F) {
  int gl = 0;
  while ((1 << gl) < F && gl < 6) ++gl;
  return gl;
}

#define MP_SPLINE_DISPATCH_DM(D, M, ...)                         \
  switch ((D) * 4 + (M)) {                                         \
    case 1 * 4 + 1: { constexpr int D_ = 1, M_ = 1; __VA_ARGS__; } break; \
    case 1 * 4 + 2: { constexpr int D_ = 1, M_ = 2; __VA_ARGS__; } break; \
    case 1 * 4 + 3: { constexpr int D_ = 1, M_ = 3; __VA_ARGS__; } break; \
    case 2 * 4 + 1: { constexpr int D_ = 2, M_ = 1; __VA_ARGS__; } break; \
    case 2 * 4 + 2: { constexpr int D_ = 2, M_ = 2; __VA_ARGS__; } break; \
    case 2 * 4 + 3: { constexpr int D_ = 2, M_ = 3; __VA_ARGS__; } break; \
    case 3 * 4 + 1: { constexpr int D_ = 3, M_ = 1; __VA_ARGS__; } break; \
    case 3 * 4 + 2: { constexpr int D_ = 3, M_ = 2; __VA_ARGS__; } break; \
    default: { constexpr int D_ = 3, M_ = 3; __VA_ARGS__; } break;        \
  }

}  // namespace mp

using namespace mp;

extern "C" int mp_spline_ok(int32_t D, int32_t degree, const int32_t* kernel_size, const int32_t* is_open,
                            int32_t F) {
  SplineGeom gm;
  int32_t K;
  bool distinct;
  if (F < 1) {
    set_error("mp_spline_ok: F = %d < 1", F);
    return 0;
  }
  return spline_geom("mp_spline_ok", D, degree, kernel_size, is_open, &gm, &K, &distinct) == MP_OK ? 1 : 0;
}

extern "C" int mp_spline_basis_f32(const float* pseudo, int64_t n_edges, int32_t D, const int32_t* kernel_size,
                                   const int32_t* is_open, int32_t degree, float* basis, size_t basis_bytes,
                                   int64_t* weight_index, size_t weight_index_bytes, void* stream) {
  const char* fn = "mp_spline_basis_f32";
  SplineGeom gm;
  int32_t K;
  bool distinct;
  if (int rc = spline_geom(fn, D, degree, kernel_size, is_open, &gm, &K, &distinct)) return rc;
  MP_CHECK_ARG(n_edges >= 0, "%s: n_edges < 0", fn);
  int64_t S = 1;
  for (int d = 0; d < D; ++d) S *= degree + 1;
  MP_CHECK_EXTENT(fn, "basis", basis_bytes, (size_t)n_edges * S * sizeof(float));
  MP_CHECK_EXTENT(fn, "weight_index", weight_index_bytes, (size_t)n_edges * S * sizeof(int64_t));
  if (n_edges == 0) return MP_OK;
  MP_CHECK_ARG(pseudo != nullptr, "%s: pseudo is NULL", fn);
  MP_CHECK_ARG(basis != nullptr, "%s: basis is NULL", fn);
  MP_CHECK_ARG(weight_index != nullptr, "%s: weight_index is NULL", fn);
  const int64_t blocks = ceil_div(n_edges, 256);
  MP_CHECK_ARG(blocks <= 0x7fffffff, "%s: n_edges too large", fn);
  MP_DEVICE_GUARD(stream);
  MP_SPLINE_DISPATCH_DM(D, degree,
                        hipLaunchKernelGGL((k_spline_basis<D_, M_>), dim3((unsigned)blocks), dim3(256), 0,
                                            as_stream(stream), pseudo, n_edges, gm, basis, weight_index));
  MP_CHECK_LAUNCH();
  return MP_OK;
}

extern "C" int mp_spline_aggregate_bins_f32(const mp_csr* g, const float* pseudo, int64_t n_pseudo_edges, int32_t D,
                                            const int32_t* kernel_size, const int32_t* is_open, int32_t degree,
                                            const float* x, int64_t ldx, int32_t F, const float* row_scale,
                                            float* out, int64_t ldo, void* stream) {
  const char* fn = "mp_spline_aggregate_bins_f32";
  SplineGeom gm;
  int32_t K;
  bool distinct;
  if (int rc = spline_csr(fn, g, n_pseudo_edges)) return rc;
  if (int rc = spline_geom(fn, D, degree, kernel_size, is_open, &gm, &K, &distinct)) return rc;
  MP_CHECK_ARG(F >= 1, "%s: F = %d < 1", fn, F);
  MP_CHECK_ARG(ldx >= F, "%s: ldx = %lld < F = %d", fn, (long long)ldx, F);
  MP_CHECK_ARG(ldo >= (int64_t)K * F, "%s: ldo = %lld < K * F = %lld", fn, (long long)ldo, (long long)K * F);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  MP_CHECK_ARG(pseudo != nullptr || g->n_edges == 0, "%s: pseudo is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  const int glog = group_log2(F);
  int waves = 65536 / (K * 256);
  waves = waves > 4 ? 4 : waves;  // K <= 256: at least one
  const int64_t rows_per_block = (int64_t)waves << (6 - glog);
  const int64_t bx = ceil_div(g->n_rows, rows_per_block);
  const int64_t by = ceil_div(F, 64);
  MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, F %d)", fn, (long long)g->n_rows,
               F);
  const size_t lds = (size_t)waves * K * 256;
  MP_DEVICE_GUARD(stream);
#define MP_SPLINE_BINS(DIST)                                                                                       \
  MP_SPLINE_DISPATCH_DM(D, degree,                                                                                 \
                        hipLaunchKernelGGL((k_spline_bins<D_, M_, DIST>), dim3((unsigned)bx, (unsigned)by),        \
                                            dim3(64 * waves), lds, as_stream(stream), g->rowptr, g->col, g->eid,   \
                                            g->n_rows, pseudo, gm, K, x, ldx, F, glog, row_scale, out, ldo))
  if (distinct) {
    MP_SPLINE_BINS(true);
  } else {
    MP_SPLINE_BINS(false);
  }
#undef MP_SPLINE_BINS
  MP_CHECK_LAUNCH();
  return MP_OK;
}

extern "C" int mp_spline_aggregate_gather_f32(const mp_csr* g, const float* pseudo, int64_t n_pseudo_edges,
                                              int32_t D, const int32_t* kernel_size, const int32_t* is_open,
                                              int32_t degree, const float* x, int64_t ldx, int32_t F,
                                              const float* row_scale, const float* bias, float* out, int64_t ldo,
                                              void* stream) {
  const char* fn = "mp_spline_aggregate_gather_f32";
  SplineGeom gm;
  int32_t K;
  bool distinct;
  if (int rc = spline_csr(fn, g, n_pseudo_edges)) return rc;
  if (int rc = spline_geom(fn, D, degree, kernel_size, is_open, &gm, &K, &distinct)) return rc;
  MP_CHECK_ARG(F >= 1, "%s: F = %d < 1", fn, F);
  MP_CHECK_ARG(ldx >= (int64_t)K * F, "%s: ldx = %lld < K * F = %lld", fn, (long long)ldx, (long long)K * F);
  MP_CHECK_ARG(ldo >= F, "%s: ldo = %lld < F = %d", fn, (long long)ldo, F);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  MP_CHECK_ARG(pseudo != nullptr || g->n_edges == 0, "%s: pseudo is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  const int glog = group_log2(F);
  const int64_t rows_per_block = (int64_t)4 << (6 - glog);
  const int64_t bx = ceil_div(g->n_rows, rows_per_block);
  const int64_t by = ceil_div(F, 64);
  MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, F %d)", fn, (long long)g->n_rows,
               F);
  MP_DEVICE_GUARD(stream);
  MP_SPLINE_DISPATCH_DM(D, degree,
                        hipLaunchKernelGGL((k_spline_gather<D_, M_>), dim3((unsigned)bx, (unsigned)by), dim3(256), 0,
                                            as_stream(stream), g->rowptr, g->col, g->eid, g->n_rows, pseudo, gm, x,
                                            ldx, F, glog, row_scale, bias, out, ldo));
  MP_CHECK_LAUNCH();
  return MP_OK;
}
