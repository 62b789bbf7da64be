// AGNNConv's cosine attention in one gather pass, with its backward (gfx950).
//
//   xn    = x / max(|x|_2, 1e-12)
//   s_ij  = beta <xn_i, xn_j>
//   a_ij  = exp(s_ij - m_i) / (sum_j exp(s_ij - m_i) + 1e-16),  m_i = max_j s_ij
//   out_i = sum_j a_ij x_j
// The row that gives the score is the row that is the message: one gathered x_j
// feeds the dot product and, from the same registers, the weighted sum.  No [E, F]
// array exists; between the two backward passes sit two scalars per edge.
//
// Lane mapping.  A group of g lanes owns one unit (a row, or a merge-path task).
// A lane holds NV elements of W floats of a row, element (fl + u * g) at features
// [(fl + u * g) * W, +W): W = 4 (one dwordx4 per element) where F % 4 == 0 and
// every operand is 16-byte aligned with a row stride that is a multiple of 4,
// W = 1 otherwise (rows of such an F are not 16-byte aligned).  g is the smallest
// power of two that covers the row's elements, at most 64; wider rows take
// NV = ceil(elements / 64) elements per lane, up to 16 floats: F <= 1024.  A dot
// product is the lanes' partial products summed by the DPP butterfly group_sum.
// Every kernel uses this mapping and the same expression for the score, so a
// recomputed score has the forward's bits.  fp32, deterministic, no atomics.
//
// Slots are walked in CSR order in batches of U: the batch's columns were loaded
// one batch ahead (every lane of the group loads the same address: one broadcast
// transaction), its U rows are in flight together.  The forward takes the batch's
// largest score first and rescales (m, l, acc) once per batch, not once per slot.
//
//   rnorm         rn[k] = 1 / max(|x_k|, 1e-12), once per call, reused by the backward
//   forward       destination CSR; out [n, F] and lse [n] = m + log(l + 1e-16)
//   backward dst  destination CSR; q_i = <g_i, out_i>; per slot c = <x_i, x_j> rn_i rn_j,
//                 a = exp(beta c - lse_i), ds = a (<g_i, x_j> - q_i); writes alpha[eid] = a,
//                 bds[eid] = beta ds; u_i = sum bds rn_j x_j (d xn_i as a destination);
//                 the row's sum ds c, summed over rows in a fixed order in two stages
//   backward src  source-keyed CSR; row j: val = sum alpha_e g_i, w = sum bds_e rn_i x_i;
//                 t = u_j + w, dx_j = val + rn_j (t - xn_j <xn_j, t>) with xn_j formed by
//                 division: F.normalize's projection once per row, not once per edge
//
// Long rows follow mp_dna.hip: on a schedule with tasks of at least kAgnnSplitChunk
// units a unit is a task; a row cut by a task boundary leaves its partial in a slab
// (slot 2 * task: a continuation, 2 * task + 1: a head) and a fix-up combines the
// chain in task order -- a softmax merge of (m, l, acc) for the forward, which adds
// the 1e-16 only there, an addition for both backward passes.  The engine's slab and
// fix-up helpers of mp_agg.h are bound to its reducer protocol (a lane sees VEC
// features of one tile, never a group-wide dot product), so they do not fit here:
// NOTE agnn_pieces and agnn_chain below are copies of dna_pieces and of the chain
// lookup of k_dna_fixup (mp_dna.hip), which mirror k_agg_main / k_agg_fixup (mp_agg.h);
// a change to the walk, the slab slots or the merge order there must be mirrored here.
#include <cmath>
#include <type_traits>

#include "mp_workspace.h"

namespace mp {

constexpr int kAgnnMaxF = 1024;       // 64 lanes * 16 floats
constexpr int kAgnnSplitChunk = 64;   // task size from which the kernels run over tasks: the source backward's
                                      // slab, 4 F (N + E) / chunk floats, is (1 + N / E) / 16 of an [E, F] array
constexpr int64_t kAgnnSumRows = 4096;  // rows per stage-1 block of the d beta sum

struct AgnnP {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const int32_t* wave_row;  // NULL: one unit per row
  const int32_t* wave_slot;
  int64_t n_units;
  int32_t F, glog;
  const float* x;
  int64_t ldx;
  const float* rn;
  float* slab;
  int64_t sf;  // floats of one slab slot
};

__device__ __forceinline__ bool agnn_unit(const AgnnP& p, int64_t* unit, int* fl, int* g) {
  const int lane = lane_id();
  *g = 1 << p.glog;
  *fl = lane & (*g - 1);
  *unit = ((((int64_t)blockIdx.x << 2) + (threadIdx.x >> 6)) << (6 - p.glog)) + (lane >> p.glog);
  return *unit < p.n_units;
}

// body(row, first slot, end slot, slab slot or -1 = the row ends here: write it) for every piece of a
// row that unit `u` walks, in slot order (copy of dna_pieces, see the head of this file)
template <class Body>
__device__ __forceinline__ void agnn_pieces(const AgnnP& p, int64_t u, Body&& body) {
  if (!p.wave_row) {
    body(u, p.rowptr[u], p.rowptr[u + 1], (int64_t)-1);
    return;
  }
  const int r_first = p.wave_row[u], r_last = p.wave_row[u + 1];
  const int e_begin = p.wave_slot[u], e_end = p.wave_slot[u + 1];
  const int ce = p.rowptr[r_first];  // rowptr[n_rows] = n_edges when the task owns no row
  if (e_begin < ce) body((int64_t)r_first - 1, e_begin, ce < e_end ? ce : e_end, 2 * u);
  for (int r = r_first; r < r_last; ++r) {
    const int rs = p.rowptr[r], re = p.rowptr[r + 1];
    if (re <= e_end) body((int64_t)r, rs, re, (int64_t)-1);
    else body((int64_t)r, rs, e_end, 2 * u + 1);
  }
}

// a lane's NV elements of row p; the load is issued by every lane (an element past F reads element 0)
template <int W, int NV>
__device__ __forceinline__ void agnn_load(const float* __restrict__ p, int fl, int g, int F, float* v) {
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (fl + u * g) * W;
    const bool in = c < F;
    if constexpr (W == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + (in ? c : 0));
      v[4 * u] = in ? t.x : 0.f;
      v[4 * u + 1] = in ? t.y : 0.f;
      v[4 * u + 2] = in ? t.z : 0.f;
      v[4 * u + 3] = in ? t.w : 0.f;
    } else {
      const float t = p[in ? c : 0];
      v[u] = in ? t : 0.f;
    }
  }
}

template <int W, int NV>
__device__ __forceinline__ void agnn_store(float* __restrict__ p, int fl, int g, int F, const float* v) {
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (fl + u * g) * W;
    if (c < F) {
      if constexpr (W == 4) {
        *reinterpret_cast<f32x4*>(p + c) = f32x4{v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]};
      } else {
        p[c] = v[u];
      }
    }
  }
}

template <int N>
__device__ __forceinline__ float agnn_dot(const float* a, const float* b, int g) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) s = __fadd_rn(s, __fmul_rn(a[k], b[k]));
  return group_sum(s, g);
}

// the cosine of one slot, the same expression in the forward and the backward
__device__ __forceinline__ float agnn_cos(float dot, float ri, float rj) { return __fmul_rn(__fmul_rn(dot, ri), rj); }

template <int N>
constexpr int kAgnnU = N <= 4 ? 8 : 4;  // gathered rows in flight per group: at most 64 floats per lane

// the columns of slots [s, s + U), clamped to the piece's last slot
template <int U>
__device__ __forceinline__ void agnn_cols(const int32_t* __restrict__ a, int s, int e, int32_t* c) {
#pragma unroll
  for (int u = 0; u < U; ++u) c[u] = a[s + u < e ? s + u : e - 1];
}

// ---------------------------------------------------------------------------
// row norms
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_agnn_rnorm(const float* __restrict__ x, int64_t ldx, int64_t n, int32_t F,
                                                    int32_t glog, float* __restrict__ rn) {
  const int lane = lane_id();
  const int g = 1 << glog;
  const int fl = lane & (g - 1);
  const int64_t r = ((((int64_t)blockIdx.x << 2) + (threadIdx.x >> 6)) << (6 - glog)) + (lane >> glog);
  if (r >= n) return;
  const float* row = x + r * ldx;
  float ss = 0.f;
  for (int c = fl; c < F; c += g) ss = __fadd_rn(ss, __fmul_rn(row[c], row[c]));
  ss = group_sum(ss, g);
  if (fl == 0) rn[r] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int W, int NV>
__global__ __launch_bounds__(256) void k_agnn_fwd(AgnnP p, const float* __restrict__ beta_p, float* __restrict__ out,
                                                  int64_t ldo, float* __restrict__ lse) {
  constexpr int N = W * NV;
  constexpr int U = kAgnnU<N>;
  int fl, g;
  int64_t unit;
  if (!agnn_unit(p, &unit, &fl, &g)) return;
  const float beta = *beta_p;
  agnn_pieces(p, unit, [&](int64_t r, int b, int e, int64_t slot) {
    float xi[N], acc[N];
    agnn_load<W, NV>(p.x + r * p.ldx, fl, g, p.F, xi);
    const float ri = p.rn[r];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    float m = -INFINITY, l = 0.f;
    int32_t cj[U];
    if (b < e) agnn_cols<U>(p.col, b, e, cj);
    for (int s = b; s < e; s += U) {
      const int n = e - s < U ? e - s : U;
      float xv[U][N], rj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        agnn_load<W, NV>(p.x + (int64_t)cj[u] * p.ldx, fl, g, p.F, xv[u]);
        rj[u] = p.rn[cj[u]];
      }
      if (s + U < e) agnn_cols<U>(p.col, s + U, e, cj);
      float sc[U], bm = -INFINITY;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sc[u] = __fmul_rn(beta, agnn_cos(agnn_dot<N>(xi, xv[u], g), ri, rj[u]));
        if (u < n) bm = fmaxf(bm, sc[u]);
      }
      // one rescale per batch, to the batch's maximum
      const float mn = fmaxf(m, bm);
      const float cf = expf(m - mn);
      l = __fmul_rn(l, cf);
#pragma unroll
      for (int k = 0; k < N; ++k) acc[k] = __fmul_rn(acc[k], cf);
      m = mn;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < n) {
          const float ex = expf(sc[u] - m);
          l = __fadd_rn(l, ex);
#pragma unroll
          for (int k = 0; k < N; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(ex, xv[u][k]));
        }
      }
    }
    if (slot < 0) {
      const float den = __fadd_rn(l, 1e-16f);
#pragma unroll
      for (int k = 0; k < N; ++k) acc[k] = acc[k] / den;
      agnn_store<W, NV>(out + r * ldo, fl, g, p.F, acc);
      if (fl == 0) lse[r] = m + logf(den);
    } else {
      float* dst = p.slab + slot * p.sf;
      agnn_store<W, NV>(dst, fl, g, p.F, acc);
      if (fl == 0) {
        dst[p.sf - 4] = m;
        dst[p.sf - 3] = l;
      }
    }
  });
}

// ---------------------------------------------------------------------------
// backward over the destination CSR
// ---------------------------------------------------------------------------
template <int W, int NV>
__global__ __launch_bounds__(256) void k_agnn_bwd_dst(AgnnP p, const float* __restrict__ beta_p,
                                                      const float* __restrict__ out, int64_t ldo,
                                                      const float* __restrict__ lse, const float* __restrict__ G,
                                                      int64_t ldg, float* __restrict__ alpha, float* __restrict__ bds,
                                                      float* __restrict__ Uo, int64_t ldu, float* __restrict__ drow) {
  constexpr int N = W * NV;
  constexpr int U = kAgnnU<N>;
  int fl, g;
  int64_t unit;
  if (!agnn_unit(p, &unit, &fl, &g)) return;
  const float beta = *beta_p;
  agnn_pieces(p, unit, [&](int64_t r, int b, int e, int64_t slot) {
    float xi[N], gi[N], ua[N];
    agnn_load<W, NV>(p.x + r * p.ldx, fl, g, p.F, xi);
    agnn_load<W, NV>(G + r * ldg, fl, g, p.F, gi);
    float q;
    {
      float oi[N];
      agnn_load<W, NV>(out + r * ldo, fl, g, p.F, oi);
      q = agnn_dot<N>(gi, oi, g);
    }
    const float ri = p.rn[r];
    const float L = lse[r];
#pragma unroll
    for (int k = 0; k < N; ++k) ua[k] = 0.f;
    float db = 0.f;
    int32_t cj[U], ce[U];
    if (b < e) {
      agnn_cols<U>(p.col, b, e, cj);
      agnn_cols<U>(p.eid, b, e, ce);
    }
    for (int s = b; s < e; s += U) {
      const int n = e - s < U ? e - s : U;
      float xv[U][N], rj[U];
      int32_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        agnn_load<W, NV>(p.x + (int64_t)cj[u] * p.ldx, fl, g, p.F, xv[u]);
        rj[u] = p.rn[cj[u]];
        id[u] = ce[u];
      }
      if (s + U < e) {
        agnn_cols<U>(p.col, s + U, e, cj);
        agnn_cols<U>(p.eid, s + U, e, ce);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < n) {
          const float c = agnn_cos(agnn_dot<N>(xi, xv[u], g), ri, rj[u]);
          const float a = expf(__fmul_rn(beta, c) - L);
          const float ds = __fmul_rn(a, agnn_dot<N>(gi, xv[u], g) - q);
          const float bd = __fmul_rn(beta, ds);
          if (fl == 0) {
            alpha[id[u]] = a;
            bds[id[u]] = bd;
          }
          const float wj = __fmul_rn(bd, rj[u]);
#pragma unroll
          for (int k = 0; k < N; ++k) ua[k] = __fadd_rn(ua[k], __fmul_rn(wj, xv[u][k]));
          db = __fadd_rn(db, __fmul_rn(ds, c));
        }
      }
    }
    if (slot < 0) {
      agnn_store<W, NV>(Uo + r * ldu, fl, g, p.F, ua);
      if (fl == 0) drow[r] = db;
    } else {
      float* dst = p.slab + slot * p.sf;
      agnn_store<W, NV>(dst, fl, g, p.F, ua);
      if (fl == 0) dst[p.sf - 4] = db;
    }
  });
}

// ---------------------------------------------------------------------------
// backward over the source-keyed CSR
// ---------------------------------------------------------------------------
// dx = val + rn (t - xn <xn, t>), xn = x / max(|x|, 1e-12): for F = 1, xn = +-1 and the bracket is exactly 0
template <int N>
__device__ __forceinline__ void agnn_project(const float* xj, const float* t, float nrm, float rj, float dot_xn_t,
                                             float* val) {
#pragma unroll
  for (int k = 0; k < N; ++k)
    val[k] = __fadd_rn(val[k], __fmul_rn(rj, t[k] - __fmul_rn(xj[k] / nrm, dot_xn_t)));
}

template <int W, int NV>
__global__ __launch_bounds__(256) void k_agnn_bwd_src(AgnnP p, const float* __restrict__ G, int64_t ldg,
                                                      const float* __restrict__ alpha, const float* __restrict__ bds,
                                                      const float* __restrict__ Ui, int64_t ldu,
                                                      float* __restrict__ dx, int64_t lddx) {
  constexpr int N = W * NV;
  constexpr int U = kAgnnU<N> / 2;  // two gathered rows per slot
  int fl, g;
  int64_t unit;
  if (!agnn_unit(p, &unit, &fl, &g)) return;
  agnn_pieces(p, unit, [&](int64_t r, int b, int e, int64_t slot) {
    float val[N], wa[N];
#pragma unroll
    for (int k = 0; k < N; ++k) val[k] = wa[k] = 0.f;
    int32_t ci[U], ce[U];
    if (b < e) {
      agnn_cols<U>(p.col, b, e, ci);
      agnn_cols<U>(p.eid, b, e, ce);
    }
    for (int s = b; s < e; s += U) {
      const int n = e - s < U ? e - s : U;
      float gv[U][N], xv[U][N], a[U], wi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        agnn_load<W, NV>(G + (int64_t)ci[u] * ldg, fl, g, p.F, gv[u]);
        agnn_load<W, NV>(p.x + (int64_t)ci[u] * p.ldx, fl, g, p.F, xv[u]);
        a[u] = alpha[ce[u]];
        wi[u] = __fmul_rn(bds[ce[u]], p.rn[ci[u]]);
      }
      if (s + U < e) {
        agnn_cols<U>(p.col, s + U, e, ci);
        agnn_cols<U>(p.eid, s + U, e, ce);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < n) {
#pragma unroll
          for (int k = 0; k < N; ++k) {
            val[k] = __fadd_rn(val[k], __fmul_rn(a[u], gv[u][k]));
            wa[k] = __fadd_rn(wa[k], __fmul_rn(wi[u], xv[u][k]));
          }
        }
      }
    }
    if (slot < 0) {
      float xj[N], t[N], xn[N];
      agnn_load<W, NV>(p.x + r * p.ldx, fl, g, p.F, xj);
      agnn_load<W, NV>(Ui + r * ldu, fl, g, p.F, t);
      const float nrm = fmaxf(sqrtf(agnn_dot<N>(xj, xj, g)), 1e-12f);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        t[k] = __fadd_rn(t[k], wa[k]);
        xn[k] = xj[k] / nrm;
      }
      agnn_project<N>(xj, t, nrm, p.rn[r], agnn_dot<N>(xn, t, g), val);
      agnn_store<W, NV>(dx + r * lddx, fl, g, p.F, val);
    } else {
      float* dst = p.slab + slot * p.sf;
      agnn_store<W, NV>(dst, fl, g, p.F, val);
      agnn_store<W, NV>(dst + (p.sf >> 1), fl, g, p.F, wa);
    }
  });
}

// ---------------------------------------------------------------------------
// fix-ups: one block per split row, its chain of partials combined in task order
// ---------------------------------------------------------------------------
// row, owner and last task of split row i (copy of k_dna_fixup's lookup, see the head of this file); chain
// item k in [owner, last] sits in slab slot 2 * owner + 1 (the head) or 2 * k (a continuation)
__device__ __forceinline__ void agnn_chain(const int32_t* __restrict__ wave_row,
                                           const int32_t* __restrict__ split_waves, int32_t n_waves, int i, int* r,
                                           int* owner, int* last) {
  *last = split_waves[i];
  *r = wave_row[*last] - 1;
  int lo = 0, hi = n_waves;  // owner = the last task whose first owned row is <= r (wave_row[n_waves] = n_rows > r)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (wave_row[mid] <= *r) lo = mid;
    else hi = mid - 1;
  }
  *owner = lo;
}
__device__ __forceinline__ int64_t agnn_item(int owner, int k) {
  return k == owner ? 2 * (int64_t)owner + 1 : 2 * (int64_t)k;
}

// the sum of v over the block's 256 threads in a fixed order, in every thread
__device__ __forceinline__ float agnn_block_sum(float v, float* lds) {
  v = group_sum(v, 64);
  __syncthreads();  // an earlier call's reads come first
  if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return __fadd_rn(__fadd_rn(lds[0], lds[1]), __fadd_rn(lds[2], lds[3]));
}

// forward: the softmax merge of (m, l, acc) to the chain's maximum; the 1e-16 enters here, once
__global__ __launch_bounds__(256) void k_agnn_fixup_fwd(const int32_t* __restrict__ wave_row,
                                                        const int32_t* __restrict__ split_waves, int32_t n_waves,
                                                        const float* __restrict__ slab, int64_t sf, int32_t F,
                                                        float* __restrict__ out, int64_t ldo,
                                                        float* __restrict__ lse) {
  int r, owner, last;
  agnn_chain(wave_row, split_waves, n_waves, (int)blockIdx.x, &r, &owner, &last);
  float M = -INFINITY;
  for (int k = owner; k <= last; ++k) M = fmaxf(M, slab[agnn_item(owner, k) * sf + sf - 4]);
  float l = 0.f;
  for (int k = owner; k <= last; ++k) {
    const float* s = slab + agnn_item(owner, k) * sf;
    l = __fadd_rn(l, __fmul_rn(s[sf - 3], expf(s[sf - 4] - M)));
  }
  const float den = __fadd_rn(l, 1e-16f);
  for (int c = threadIdx.x; c < F; c += 256) {
    float a = 0.f;
    for (int k = owner; k <= last; ++k) {
      const float* s = slab + agnn_item(owner, k) * sf;
      a = __fadd_rn(a, __fmul_rn(s[c], expf(s[sf - 4] - M)));
    }
    out[(int64_t)r * ldo + c] = a / den;
  }
  if (threadIdx.x == 0) lse[r] = M + logf(den);
}

// destination backward: u and the row's d beta term, by addition
__global__ __launch_bounds__(256) void k_agnn_fixup_dst(const int32_t* __restrict__ wave_row,
                                                        const int32_t* __restrict__ split_waves, int32_t n_waves,
                                                        const float* __restrict__ slab, int64_t sf, int32_t F,
                                                        float* __restrict__ Uo, int64_t ldu,
                                                        float* __restrict__ drow) {
  int r, owner, last;
  agnn_chain(wave_row, split_waves, n_waves, (int)blockIdx.x, &r, &owner, &last);
  for (int c = threadIdx.x; c <= F; c += 256) {
    const int64_t at = c < F ? c : sf - 4;
    float t = 0.f;
    for (int k = owner; k <= last; ++k) t = __fadd_rn(t, slab[agnn_item(owner, k) * sf + at]);
    if (c < F) Uo[(int64_t)r * ldu + c] = t;
    else drow[r] = t;
  }
}

// source backward: val and w by addition, then the row's projection; thread t owns features t + 256 k
__global__ __launch_bounds__(256) void k_agnn_fixup_src(const int32_t* __restrict__ wave_row,
                                                        const int32_t* __restrict__ split_waves, int32_t n_waves,
                                                        const float* __restrict__ slab, int64_t sf, int32_t F,
                                                        const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ rn, const float* __restrict__ Ui,
                                                        int64_t ldu, float* __restrict__ dx, int64_t lddx) {
  constexpr int K = kAgnnMaxF / 256;
  __shared__ float lds[4];
  int r, owner, last;
  agnn_chain(wave_row, split_waves, n_waves, (int)blockIdx.x, &r, &owner, &last);
  float val[K], t[K], xj[K];
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const int c = threadIdx.x + 256 * q;
    val[q] = t[q] = xj[q] = 0.f;
    if (c < F) {
      float w = 0.f;
      for (int k = owner; k <= last; ++k) {
        const float* s = slab + agnn_item(owner, k) * sf;
        val[q] = __fadd_rn(val[q], s[c]);
        w = __fadd_rn(w, s[(sf >> 1) + c]);
      }
      t[q] = __fadd_rn(Ui[(int64_t)r * ldu + c], w);
      xj[q] = x[(int64_t)r * ldx + c];
    }
    ss = __fadd_rn(ss, __fmul_rn(xj[q], xj[q]));
  }
  const float nrm = fmaxf(sqrtf(agnn_block_sum(ss, lds)), 1e-12f);
  float pp = 0.f;
#pragma unroll
  for (int q = 0; q < K; ++q) pp = __fadd_rn(pp, __fmul_rn(xj[q] / nrm, t[q]));
  const float d = agnn_block_sum(pp, lds);
  agnn_project<K>(xj, t, nrm, rn[r], d, val);
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const int c = threadIdx.x + 256 * q;
    if (c < F) dx[(int64_t)r * lddx + c] = val[q];
  }
}

// d beta: block b adds in[b * per, (b + 1) * per) in a fixed order (stage 1 over the rows, stage 2, one block,
// over stage 1's partials: the two-stage form of mp_gmm.hip's parameter gradients)
__global__ __launch_bounds__(256) void k_agnn_sum(const float* __restrict__ in, int64_t n, int64_t per,
                                                  float* __restrict__ out) {
  __shared__ float lds[4];
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  float s = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s = __fadd_rn(s, in[i]);
  s = agnn_block_sum(s, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int agnn_shape(const char* fn, int32_t F) {
  MP_CHECK_ARG(F >= 1, "%s: F = %d < 1", fn, F);
  MP_CHECK_ARG(F <= kAgnnMaxF, "%s: F = %d above the limit F <= %d", fn, F, kAgnnMaxF);
  return MP_OK;
}

// whether the kernels run over the tasks of g's schedule (else over its rows)
static inline bool agnn_tasks(const mp_csr* g) { return g->wave_row != nullptr && g->chunk >= kAgnnSplitChunk; }

// floats of one slab slot: the forward and the destination backward keep F values and (m, l) or the d beta
// term, the source backward val | w
static inline int64_t agnn_slot_floats(int32_t F, int32_t pass) {
  const int64_t f4 = ceil_div(F, 4) * 4;
  return pass == MP_AGNN_PASS_SRC ? 2 * f4 : f4 + 4;
}

// The workspace of one call: two slab slots per task (continuation, head) when the kernels walk tasks, and for
// the destination backward the rows' d beta terms and their stage-1 sums.
struct AgnnWs : Carver {
  float* slab;
  float* drow;
  float* part;
  AgnnWs(void* ws, int64_t n_waves, int64_t n_rows, int32_t F, int32_t pass)
      : Carver(ws),
        slab(take<float>(2 * n_waves * agnn_slot_floats(F, pass))),
        drow(take<float>(pass == MP_AGNN_PASS_DST ? n_rows : 0)),
        part(take<float>(pass == MP_AGNN_PASS_DST ? ceil_div(n_rows, kAgnnSumRows) : 0)) {}
};
static inline AgnnWs agnn_ws_of(void* ws, const mp_csr* g, int32_t F, int32_t pass) {
  return AgnnWs(ws, agnn_tasks(g) && g->n_waves > 0 ? g->n_waves : 0, g->n_rows > 0 ? g->n_rows : 0, F, pass);
}

static int agnn_csr(const char* fn, const mp_csr* g) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->n_rows <= 0x7fffffff && g->n_edges <= 0x7fffffff, "%s: n_rows / n_edges above 2^31 - 1", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the AGNN passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (alpha and bds are kept in original edge order)", fn);
  MP_CHECK_ARG((int64_t)g->n_cols == g->n_rows, "%s: g->n_cols = %d is not n_rows = %lld (x serves both ends)", fn,
               (int)g->n_cols, (long long)g->n_rows);
  MP_CHECK_ARG(g->n_ids == 0 || g->n_ids >= g->n_edges, "%s: g->n_ids = %lld below n_edges", fn,
               (long long)g->n_ids);
  if (agnn_tasks(g)) {
    MP_CHECK_ARG(g->wave_slot != nullptr, "%s: g->wave_slot is NULL (a schedule with chunk = %d)", fn, g->chunk);
    MP_CHECK_ARG(g->n_waves >= 1, "%s: g->n_waves = %d < 1", fn, g->n_waves);
    MP_CHECK_ARG(g->n_split >= 0 && g->n_split <= g->n_waves, "%s: g->n_split = %d outside [0, n_waves = %d]", fn,
                 g->n_split, g->n_waves);
    MP_CHECK_ARG(g->n_split == 0 || g->split_waves != nullptr, "%s: g->split_waves is NULL with n_split = %d", fn,
                 g->n_split);
  }
  return MP_OK;
}

// one operand [n, F] under its row stride
static int agnn_rows(const char* fn, const char* name, const void* p, int64_t ld, size_t bytes, int64_t n,
                     int32_t F) {
  MP_CHECK_ARG(p != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_ARG(ld >= F, "%s: ld of %s = %lld < F = %d", fn, name, (long long)ld, F);
  MP_CHECK_EXTENT(fn, name, bytes, n <= 0 ? 0 : ((size_t)(n - 1) * ld + F) * sizeof(float));
  return MP_OK;
}

// one fp32 vector of n entries
static int agnn_vec(const char* fn, const char* name, const void* p, size_t bytes, int64_t n) {
  MP_CHECK_ARG(p != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_EXTENT(fn, name, bytes, (size_t)(n > 0 ? n : 0) * sizeof(float));
  return MP_OK;
}

static inline bool agnn_al4(const void* p, int64_t ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

// what every launch of one call shares: the lane mapping (W, NV, g) and the kernels' common arguments
struct AgnnLaunch {
  AgnnP p;
  int W, NV;
  int64_t blocks;
};
static int agnn_launch(const char* fn, const mp_csr* g, int32_t F, bool vec4, const float* x, int64_t ldx,
                       const float* rn, float* slab, int32_t pass, AgnnLaunch* l) {
  const bool tasks = agnn_tasks(g);
  l->W = (F % 4 == 0 && vec4 && agnn_al4(x, ldx)) ? 4 : 1;
  const int elems = F / l->W;
  const int gl = group_lanes(elems);
  l->NV = (int)ceil_div(elems, 64);
  if (l->W == 1 && l->NV > 1) l->NV = l->NV <= 4 ? 4 : 16;  // W = 1 is built at 1, 4 and 16 elements per lane
  int glog = 0;
  while ((1 << glog) < gl) ++glog;
  l->p = AgnnP{g->rowptr, g->col, g->eid, tasks ? g->wave_row : nullptr, tasks ? g->wave_slot : nullptr,
               tasks ? (int64_t)g->n_waves : g->n_rows, F, glog, x, ldx, rn, slab, agnn_slot_floats(F, pass)};
  l->blocks = ceil_div(l->p.n_units, (int64_t)4 << (6 - glog));
  MP_CHECK_ARG(l->blocks <= 0x7fffffff, "%s: grid too large (%lld rows or tasks)", fn, (long long)l->p.n_units);
  return MP_OK;
}

// fn(W, NV as integral constants) for the lane mapping of l
template <class Fn>
static inline void agnn_with(const AgnnLaunch& l, Fn&& fn) {
  using std::integral_constant;
  using W4 = integral_constant<int, 4>;
  using W1 = integral_constant<int, 1>;
  if (l.W == 4) {
    switch (l.NV) {
      case 1: return fn(W4{}, integral_constant<int, 1>{});
      case 2: return fn(W4{}, integral_constant<int, 2>{});
      case 3: return fn(W4{}, integral_constant<int, 3>{});
      default: return fn(W4{}, integral_constant<int, 4>{});
    }
  }
  switch (l.NV) {
    case 1: return fn(W1{}, integral_constant<int, 1>{});
    case 4: return fn(W1{}, integral_constant<int, 4>{});
    default: return fn(W1{}, integral_constant<int, 16>{});
  }
}

static int agnn_rnorm(const float* x, int64_t ldx, size_t x_bytes, int64_t n, int32_t F, float* rn, size_t rn_bytes,
                      void* stream, int64_t* launches) {
  const char* fn = "mp_agnn_rnorm_f32";
  if (int rc = agnn_shape(fn, F)) return rc;
  MP_CHECK_ARG(n >= 0 && n <= 0x7fffffff, "%s: n = %lld outside [0, 2^31)", fn, (long long)n);
  if (int rc = agnn_rows(fn, "x", x, ldx, x_bytes, n, F)) return rc;
  if (int rc = agnn_vec(fn, "rn", rn, rn_bytes, n)) return rc;
  if (n == 0) return MP_OK;
  const int gl = group_lanes(F);
  int glog = 0;
  while ((1 << glog) < gl) ++glog;
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(k_agnn_rnorm, dim3((unsigned)ceil_div(n, (int64_t)4 << (6 - glog))), dim3(256), 0,
                     as_stream(stream), x, ldx, n, F, glog, rn);
  MP_CHECK_LAUNCH();
  ++*launches;
  return MP_OK;
}

static int agnn_ws_check(const char* fn, const mp_csr* g, int32_t F, int32_t pass, void* ws, size_t ws_bytes) {
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, agnn_ws_of(nullptr, g, F, pass).total(0));
  return MP_OK;
}

static int agnn_aggregate(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes, const float* rn,
                          size_t rn_bytes, const float* beta, int32_t F, float* out, int64_t ldo, size_t out_bytes,
                          float* lse, size_t lse_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_agnn_aggregate_f32";
  if (int rc = agnn_shape(fn, F)) return rc;
  if (int rc = agnn_csr(fn, g)) return rc;
  if (int rc = agnn_rows(fn, "x", x, ldx, x_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "rn", rn, rn_bytes, g->n_rows)) return rc;
  MP_CHECK_ARG(beta != nullptr, "%s: beta is NULL (a device pointer to one float)", fn);
  if (int rc = agnn_rows(fn, "out", out, ldo, out_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "lse", lse, lse_bytes, g->n_rows)) return rc;
  if (int rc = agnn_ws_check(fn, g, F, MP_AGNN_PASS_FWD, ws, ws_bytes)) return rc;
  if (g->n_rows == 0) return MP_OK;
  AgnnWs w = agnn_ws_of(ws, g, F, MP_AGNN_PASS_FWD);
  AgnnLaunch l;
  if (int rc = agnn_launch(fn, g, F, agnn_al4(out, ldo), x, ldx, rn, w.slab, MP_AGNN_PASS_FWD, &l)) return rc;
  MP_DEVICE_GUARD(stream);
  agnn_with(l, [&](auto wc, auto nv) {
    hipLaunchKernelGGL((k_agnn_fwd<decltype(wc)::value, decltype(nv)::value>), dim3((unsigned)l.blocks), dim3(256), 0,
                       as_stream(stream), l.p, beta, out, ldo, lse);
  });
  MP_CHECK_LAUNCH();
  ++*launches;
  if (l.p.wave_row && g->n_split > 0) {
    hipLaunchKernelGGL(k_agnn_fixup_fwd, dim3((unsigned)g->n_split), dim3(256), 0, as_stream(stream), g->wave_row,
                       g->split_waves, g->n_waves, w.slab, l.p.sf, F, out, ldo, lse);
    MP_CHECK_LAUNCH();
    ++*launches;
  }
  return MP_OK;
}

static int agnn_backward_dst(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes, const float* rn,
                             size_t rn_bytes, const float* beta, int32_t F, const float* out, int64_t ldo,
                             size_t out_bytes, const float* lse, size_t lse_bytes, const float* gout, int64_t ldg,
                             size_t g_bytes, float* alpha, size_t alpha_bytes, float* bds, size_t bds_bytes, float* u,
                             int64_t ldu, size_t u_bytes, float* dbeta, void* ws, size_t ws_bytes, void* stream,
                             int64_t* launches) {
  const char* fn = "mp_agnn_backward_dst_f32";
  if (int rc = agnn_shape(fn, F)) return rc;
  if (int rc = agnn_csr(fn, g)) return rc;
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  if (int rc = agnn_rows(fn, "x", x, ldx, x_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "rn", rn, rn_bytes, g->n_rows)) return rc;
  MP_CHECK_ARG(beta != nullptr, "%s: beta is NULL (a device pointer to one float)", fn);
  if (int rc = agnn_rows(fn, "out", out, ldo, out_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "lse", lse, lse_bytes, g->n_rows)) return rc;
  if (int rc = agnn_rows(fn, "gout", gout, ldg, g_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "alpha", alpha, alpha_bytes, ids)) return rc;
  if (int rc = agnn_vec(fn, "bds", bds, bds_bytes, ids)) return rc;
  if (int rc = agnn_rows(fn, "u", u, ldu, u_bytes, g->n_rows, F)) return rc;
  MP_CHECK_ARG(dbeta != nullptr, "%s: dbeta is NULL (a device pointer to one float)", fn);
  if (int rc = agnn_ws_check(fn, g, F, MP_AGNN_PASS_DST, ws, ws_bytes)) return rc;
  if (g->n_rows == 0) return MP_OK;
  AgnnWs w = agnn_ws_of(ws, g, F, MP_AGNN_PASS_DST);
  AgnnLaunch l;
  const bool vec4 = agnn_al4(out, ldo) && agnn_al4(gout, ldg) && agnn_al4(u, ldu);
  if (int rc = agnn_launch(fn, g, F, vec4, x, ldx, rn, w.slab, MP_AGNN_PASS_DST, &l)) return rc;
  MP_DEVICE_GUARD(stream);
  agnn_with(l, [&](auto wc, auto nv) {
    hipLaunchKernelGGL((k_agnn_bwd_dst<decltype(wc)::value, decltype(nv)::value>), dim3((unsigned)l.blocks), dim3(256),
                       0, as_stream(stream), l.p, beta, out, ldo, lse, gout, ldg, alpha, bds, u, ldu, w.drow);
  });
  MP_CHECK_LAUNCH();
  ++*launches;
  if (l.p.wave_row && g->n_split > 0) {
    hipLaunchKernelGGL(k_agnn_fixup_dst, dim3((unsigned)g->n_split), dim3(256), 0, as_stream(stream), g->wave_row,
                       g->split_waves, g->n_waves, w.slab, l.p.sf, F, u, ldu, w.drow);
    MP_CHECK_LAUNCH();
    ++*launches;
  }
  const int64_t nb = ceil_div(g->n_rows, kAgnnSumRows);
  hipLaunchKernelGGL(k_agnn_sum, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), w.drow, g->n_rows, kAgnnSumRows,
                     w.part);
  MP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_agnn_sum, dim3(1), dim3(256), 0, as_stream(stream), w.part, nb, nb, dbeta);
  MP_CHECK_LAUNCH();
  *launches += 2;
  return MP_OK;
}

static int agnn_backward_src(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes, const float* rn,
                             size_t rn_bytes, int32_t F, const float* gout, int64_t ldg, size_t g_bytes,
                             const float* alpha, size_t alpha_bytes, const float* bds, size_t bds_bytes,
                             const float* u, int64_t ldu, size_t u_bytes, float* dx, int64_t lddx, size_t dx_bytes,
                             void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_agnn_backward_src_f32";
  if (int rc = agnn_shape(fn, F)) return rc;
  if (int rc = agnn_csr(fn, g)) return rc;
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  if (int rc = agnn_rows(fn, "x", x, ldx, x_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "rn", rn, rn_bytes, g->n_rows)) return rc;
  if (int rc = agnn_rows(fn, "gout", gout, ldg, g_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_vec(fn, "alpha", alpha, alpha_bytes, ids)) return rc;
  if (int rc = agnn_vec(fn, "bds", bds, bds_bytes, ids)) return rc;
  if (int rc = agnn_rows(fn, "u", u, ldu, u_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_rows(fn, "dx", dx, lddx, dx_bytes, g->n_rows, F)) return rc;
  if (int rc = agnn_ws_check(fn, g, F, MP_AGNN_PASS_SRC, ws, ws_bytes)) return rc;
  if (g->n_rows == 0) return MP_OK;
  AgnnWs w = agnn_ws_of(ws, g, F, MP_AGNN_PASS_SRC);
  AgnnLaunch l;
  const bool vec4 = agnn_al4(gout, ldg) && agnn_al4(u, ldu) && agnn_al4(dx, lddx);
  if (int rc = agnn_launch(fn, g, F, vec4, x, ldx, rn, w.slab, MP_AGNN_PASS_SRC, &l)) return rc;
  MP_DEVICE_GUARD(stream);
  agnn_with(l, [&](auto wc, auto nv) {
    hipLaunchKernelGGL((k_agnn_bwd_src<decltype(wc)::value, decltype(nv)::value>), dim3((unsigned)l.blocks), dim3(256),
                       0, as_stream(stream), l.p, gout, ldg, alpha, bds, u, ldu, dx, lddx);
  });
  MP_CHECK_LAUNCH();
  ++*launches;
  if (l.p.wave_row && g->n_split > 0) {
    hipLaunchKernelGGL(k_agnn_fixup_src, dim3((unsigned)g->n_split), dim3(256), 0, as_stream(stream), g->wave_row,
                       g->split_waves, g->n_waves, w.slab, l.p.sf, F, x, ldx, rn, u, ldu, dx, lddx);
    MP_CHECK_LAUNCH();
    ++*launches;
  }
  return MP_OK;
}

static inline int64_t agnn_result(int rc, int64_t launches) { return rc != MP_OK ? -(int64_t)rc : launches; }

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_agnn_ok(int32_t F) { return F >= 1 && F <= kAgnnMaxF ? 1 : 0; }

extern "C" int64_t mp_agnn_split_chunk(void) { return kAgnnSplitChunk; }

extern "C" size_t mp_agnn_workspace(const mp_csr* g, int32_t F, int32_t pass) {
  if (pass < MP_AGNN_PASS_FWD || pass > MP_AGNN_PASS_SRC) pass = MP_AGNN_PASS_FWD;
  if (F < 1) F = 1;
  if (g == nullptr) return AgnnWs(nullptr, 0, 0, F, pass).total(0);
  return agnn_ws_of(nullptr, g, F, pass).total(0);
}

extern "C" int64_t mp_agnn_rnorm_f32(const float* x, int64_t ldx, size_t x_bytes, int64_t n, int32_t F, float* rn,
                                     size_t rn_bytes, void* stream) {
  int64_t launches = 0;
  return agnn_result(agnn_rnorm(x, ldx, x_bytes, n, F, rn, rn_bytes, stream, &launches), launches);
}

extern "C" int64_t mp_agnn_aggregate_f32(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes,
                                         const float* rn, size_t rn_bytes, const float* beta, int32_t F, float* out,
                                         int64_t ldo, size_t out_bytes, float* lse, size_t lse_bytes, void* ws,
                                         size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = agnn_aggregate(g, x, ldx, x_bytes, rn, rn_bytes, beta, F, out, ldo, out_bytes, lse, lse_bytes, ws,
                                ws_bytes, stream, &launches);
  return agnn_result(rc, launches);
}

extern "C" int64_t mp_agnn_backward_dst_f32(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes,
                                            const float* rn, size_t rn_bytes, const float* beta, int32_t F,
                                            const float* out, int64_t ldo, size_t out_bytes, const float* lse,
                                            size_t lse_bytes, const float* gout, int64_t ldg, size_t g_bytes,
                                            float* alpha, size_t alpha_bytes, float* bds, size_t bds_bytes, float* u,
                                            int64_t ldu, size_t u_bytes, float* dbeta, void* ws, size_t ws_bytes,
                                            void* stream) {
  int64_t launches = 0;
  const int rc = agnn_backward_dst(g, x, ldx, x_bytes, rn, rn_bytes, beta, F, out, ldo, out_bytes, lse, lse_bytes,
                                   gout, ldg, g_bytes, alpha, alpha_bytes, bds, bds_bytes, u, ldu, u_bytes, dbeta, ws,
                                   ws_bytes, stream, &launches);
  return agnn_result(rc, launches);
}

extern "C" int64_t mp_agnn_backward_src_f32(const mp_csr* g, const float* x, int64_t ldx, size_t x_bytes,
                                            const float* rn, size_t rn_bytes, int32_t F, const float* gout,
                                            int64_t ldg, size_t g_bytes, const float* alpha, size_t alpha_bytes,
                                            const float* bds, size_t bds_bytes, const float* u, int64_t ldu,
                                            size_t u_bytes, float* dx, int64_t lddx, size_t dx_bytes, void* ws,
                                            size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = agnn_backward_src(g, x, ldx, x_bytes, rn, rn_bytes, F, gout, ldg, g_bytes, alpha, alpha_bytes, bds,
                                   bds_bytes, u, ldu, u_bytes, dx, lddx, dx_bytes, ws, ws_bytes, stream, &launches);
  return agnn_result(rc, launches);
}
