// The attention readout of Set2Set and GlobalAttention (gfx950), forward and
// backward: per graph g (nodes starts[g] .. starts[g+1]) a softmax of one scalar
// per node and the softmax-weighted sum of the graph's node rows,
//   e_n = x_n . q_g (query mode)  or  score[n] (score mode)
//   m_g = max e_n, den_g = sum exp(e_n - m_g), a_n = exp(e_n - m_g) / den_g
//   r_g = sum a_n x_n
// as ONE flash-style pass over x: a dot, a running (max, sum) and a rescaled
// accumulate.  Nothing of size N leaves the chip but e (one float per node).
// Upstream divides by den + 1e-16; den >= 1 for a graph with a node, so that
// sum is den bit for bit in fp32 and the kernels divide by den.
//
// Lanes run over channels.  A row is owned by gl = min(64, pow2 >= C / VEC) lanes
// (VEC = 4: 16-byte loads, when C % 4 == 0 and the pointers and strides allow it,
// else 1), 64 / gl nodes share a wave step, and a lane owns up to kRdPasses
// fragments of a row, so one block of channels is BW = 64 * VEC * kRdPasses wide.
// Wider rows are tiled over blockIdx.z: every tile forms the full dot (the same
// order in each, so e is the same bits) and accumulates its own channels.
//
// The path of a graph is rd_path(n_g, C), a function of those two alone:
//   0  one wave per graph, four graphs per workgroup; the wave's 64 / gl node
//      slots keep a state each and are merged by a butterfly (both partners of
//      a step form the same sum: fp add commutes)
//   1  one workgroup per graph; wave w takes the node steps w, w + 4, ..., and
//      the four wave states are merged through LDS in wave order
//   2  the graph is cut into chunks of rd_chunk(C) nodes, a workgroup each,
//      whose states go to the workspace; a second kernel merges them in chunk
//      order, rescaled by exp(m_chunk - m_g)
// The backward recomputes a_n from the saved e and (m, den), forms s_g = dr_g .
// r_g per wave, and walks the same three paths with plain sums for dq.
// No atomics; every merge order is fixed, so a graph's results are the same bits
// run to run and whatever else is in the batch.
#include "mp_workspace.h"

#include <math.h>

namespace mp {

constexpr int kRdPasses = 4;  // fragments of a row per lane
constexpr int kRdWaves = 4;   // waves per workgroup

// Unmeasured thresholds: a wave keeps a graph of up to 8192 row
// floats, a chunk is 16384 row floats, a graph of more than 4 chunks is split.
__host__ __device__ static inline int64_t rd_wave_limit(int32_t C) {
  const int64_t t = 8192 / (C < 64 ? 64 : C);
  return t < 8 ? 8 : t;
}
__host__ __device__ static inline int64_t rd_chunk(int32_t C) {
  const int64_t t = 16384 / (C < 64 ? 64 : C);
  return t < 32 ? 32 : t;
}
__host__ __device__ static inline int rd_path(int64_t n_g, int32_t C) {
  if (n_g <= rd_wave_limit(C)) return 0;
  return n_g <= 4 * rd_chunk(C) ? 1 : 2;
}
// chunk k of graph g (first node s) owns workspace slot s / chunk + g + k:
// distinct for distinct (g, k), and below n / chunk + n_graphs
__host__ __device__ static inline int64_t rd_slots(int64_t n, int64_t n_graphs, int64_t max_n, int32_t C) {
  return rd_path(max_n, C) == 2 ? n / rd_chunk(C) + n_graphs + 1 : 0;
}

// One array: per slot (m, den, row[C]); the backward uses row alone.
struct ReadoutWs : Carver {
  float* part;
  ReadoutWs(void* ws, int64_t n, int64_t n_graphs, int64_t max_n, int32_t C)
      : Carver(ws), part(take<float>(rd_slots(n, n_graphs, max_n, C) * ((int64_t)C + 2))) {}
};

struct RdFwd {
  const float* x;
  int64_t ldx;
  const int64_t* starts;
  int64_t G;
  const float* q;
  int64_t ldq;
  const float* score;
  float* out;
  int64_t ldo;
  float* q_out;
  float* e;
  float* stats;
  float* alpha;
  float* ws;
  int32_t C, glog, nb;
};

struct RdBwd {
  const float* dr;
  int64_t lddr;
  const float* x;
  int64_t ldx;
  const int64_t* starts;
  int64_t G;
  const float* q;
  int64_t ldq;
  const float* e;
  const float* stats;
  const float* r;
  int64_t ldr;
  float* dx;
  int64_t lddx;
  float* dq;
  int64_t lddq;
  float* dscore;
  float* ws;
  int32_t C, glog, nb;
};

// The lane's place: fl of gl lanes on a row, node slot sub of nsub, channel tile z.
struct RdLane {
  int fl, sub, gl, nsub, c0, C, z, nb;
};

template <int VEC>
__device__ __forceinline__ RdLane rd_lane(int32_t C, int32_t glog, int32_t nb) {
  RdLane L;
  const int lane = lane_id();
  L.gl = 1 << glog;
  L.nsub = 64 >> glog;
  L.fl = lane & (L.gl - 1);
  L.sub = lane >> glog;
  L.z = blockIdx.z;
  L.nb = nb;
  L.c0 = L.z * (64 * VEC * kRdPasses);
  L.C = C;
  return L;
}

template <int VEC>
__device__ __forceinline__ int rd_chan(const RdLane& L, int p) {
  return L.c0 + (p * L.gl + L.fl) * VEC;
}

template <int VEC>
__device__ __forceinline__ void rd_zero(Frag<VEC> (&f)[kRdPasses]) {
#pragma unroll
  for (int p = 0; p < kRdPasses; ++p)
#pragma unroll
    for (int v = 0; v < VEC; ++v) f[p].v[v] = 0.f;
}

// the lane's fragments of its own channel tile of one row
template <int VEC>
__device__ __forceinline__ void rd_load(const RdLane& L, const float* row, Frag<VEC> (&f)[kRdPasses]) {
#pragma unroll
  for (int p = 0; p < kRdPasses; ++p) {
    const int c = rd_chan<VEC>(L, p);
    if (c < L.C) f[p] = load_frag<VEC>(row + c);
  }
}

// The lane's part of a . b over ALL channels, tile by tile in order (the same
// order in every tile of the grid); b's own-tile fragments come from breg and
// a's are left in areg.
template <int VEC>
__device__ __forceinline__ float rd_dot(const RdLane& L, const float* a, const float* b,
                                        const Frag<VEC> (&breg)[kRdPasses], Frag<VEC> (&areg)[kRdPasses]) {
  float part = 0.f;
  for (int cb = 0; cb < L.nb; ++cb) {
    if (cb == L.z) {
#pragma unroll
      for (int p = 0; p < kRdPasses; ++p) {
        const int c = rd_chan<VEC>(L, p);
        if (c < L.C) {
          areg[p] = load_frag<VEC>(a + c);
#pragma unroll
          for (int v = 0; v < VEC; ++v) part += areg[p].v[v] * breg[p].v[v];
        }
      }
    } else {
      for (int p = 0; p < kRdPasses; ++p) {
        const int c = cb * (64 * VEC * kRdPasses) + (p * L.gl + L.fl) * VEC;
        if (c < L.C) {
          const Frag<VEC> av = load_frag<VEC>(a + c), bv = load_frag<VEC>(b + c);
#pragma unroll
          for (int v = 0; v < VEC; ++v) part += av.v[v] * bv.v[v];
        }
      }
    }
  }
  return part;
}

template <int VEC>
struct RdState {
  float m, den;
  Frag<VEC> acc[kRdPasses];
};

__device__ __forceinline__ float rd_scale(float m, float m_new) { return m == m_new ? 1.f : expf(m - m_new); }

// The forward over the nodes first + i0 + it * stride + sub (it = 0, 1, ...)
// of the cnt nodes from `first` on, then the butterfly over the node slots:
// every lane ends with the state of all of them.
template <int VEC>
__device__ __forceinline__ void rd_fwd_nodes(const RdFwd& a, const RdLane& L, const float* qrow,
                                             const Frag<VEC> (&qreg)[kRdPasses], int64_t first, int64_t cnt, int64_t i0,
                                             int64_t stride, RdState<VEC>& st) {
  st.m = -INFINITY;
  st.den = 0.f;
  rd_zero<VEC>(st.acc);
  const int64_t iters = cnt > i0 ? (cnt - i0 + stride - 1) / stride : 0;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t i = i0 + it * stride + L.sub;
    const bool live = i < cnt;
    const int64_t n = first + (live ? i : 0);
    const float* xr = a.x + n * a.ldx;
    Frag<VEC> xv[kRdPasses];
    rd_zero<VEC>(xv);
    float e;
    if (qrow) {
      e = group_sum(rd_dot<VEC>(L, xr, qrow, qreg, xv), L.gl);
    } else {
      rd_load<VEC>(L, xr, xv);
      e = a.score[n];
    }
    if (live) {
      if (L.fl == 0 && L.z == 0) a.e[n] = e;
      const float mn = fmaxf(st.m, e);
      const float sc = rd_scale(st.m, mn);
      const float p = expf(e - mn);
      st.den = st.den * sc + p;
#pragma unroll
      for (int k = 0; k < kRdPasses; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) st.acc[k].v[v] = st.acc[k].v[v] * sc + p * xv[k].v[v];
      st.m = mn;
    }
  }
  for (int d = L.gl; d < 64; d <<= 1) {
    const float mo = __shfl_xor(st.m, d);
    const float dn = __shfl_xor(st.den, d);
    const float mn = fmaxf(st.m, mo);
    const float s1 = rd_scale(st.m, mn), s2 = rd_scale(mo, mn);
    st.den = st.den * s1 + dn * s2;
#pragma unroll
    for (int k = 0; k < kRdPasses; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) st.acc[k].v[v] = st.acc[k].v[v] * s1 + __shfl_xor(st.acc[k].v[v], d) * s2;
    st.m = mn;
  }
}

// path 0 (and every empty graph): a wave per graph
template <int VEC>
__global__ __launch_bounds__(256) void k_readout_fwd_wave(RdFwd a) {
  const RdLane L = rd_lane<VEC>(a.C, a.glog, a.nb);
  const int64_t g = (int64_t)blockIdx.x * kRdWaves + uni((int)(threadIdx.x >> 6));
  if (g >= a.G) return;
  const int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (cnt > 0 && rd_path(cnt, a.C) != 0) return;
  const float* qrow = a.q ? a.q + g * a.ldq : nullptr;
  Frag<VEC> qreg[kRdPasses];
  rd_zero<VEC>(qreg);
  if (qrow) rd_load<VEC>(L, qrow, qreg);
  RdState<VEC> st;
  rd_fwd_nodes<VEC>(a, L, qrow, qreg, s, cnt, 0, L.nsub, st);
  if (L.sub == 0) {
#pragma unroll
    for (int p = 0; p < kRdPasses; ++p) {
      const int c = rd_chan<VEC>(L, p);
      if (c < a.C) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          a.out[g * a.ldo + c + v] = cnt > 0 ? st.acc[p].v[v] / st.den : 0.f;
          if (a.q_out) a.q_out[g * a.ldo + c + v] = qreg[p].v[v];
        }
      }
    }
  }
  if (L.z == 0 && lane_id() == 0) {
    a.stats[2 * g] = cnt > 0 ? st.m : 0.f;
    a.stats[2 * g + 1] = cnt > 0 ? st.den : 0.f;
  }
}

// paths 1 (SPLIT = false: blockIdx.x = graph) and 2 (SPLIT = true: blockIdx.y =
// chunk): a workgroup per graph or chunk, wave states merged through LDS
template <int VEC, bool SPLIT>
__global__ __launch_bounds__(256) void k_readout_fwd_wg(RdFwd a) {
  constexpr int BW = 64 * VEC * kRdPasses;
  __shared__ float sm[kRdWaves][BW + 2];
  const RdLane L = rd_lane<VEC>(a.C, a.glog, a.nb);
  const int wave = uni((int)(threadIdx.x >> 6));
  const int64_t g = blockIdx.x;
  int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (cnt == 0 || rd_path(cnt, a.C) != (SPLIT ? 2 : 1)) return;
  int64_t slot = 0;
  if (SPLIT) {
    const int64_t chunk = rd_chunk(a.C), b = (int64_t)blockIdx.y * chunk;
    if (b >= cnt) return;
    slot = s / chunk + g + blockIdx.y;
    s += b;
    cnt = cnt - b < chunk ? cnt - b : chunk;
  }
  const float* qrow = a.q ? a.q + g * a.ldq : nullptr;
  Frag<VEC> qreg[kRdPasses];
  rd_zero<VEC>(qreg);
  if (qrow) rd_load<VEC>(L, qrow, qreg);
  RdState<VEC> st;
  rd_fwd_nodes<VEC>(a, L, qrow, qreg, s, cnt, (int64_t)wave * L.nsub, (int64_t)kRdWaves * L.nsub, st);
  if (L.sub == 0) {
#pragma unroll
    for (int p = 0; p < kRdPasses; ++p) {
      const int c = rd_chan<VEC>(L, p);
      if (c < a.C) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) sm[wave][2 + c - L.c0 + v] = st.acc[p].v[v];
      }
    }
    if (L.fl == 0) {
      sm[wave][0] = st.m;
      sm[wave][1] = st.den;
    }
  }
  __syncthreads();
  float mg = sm[0][0];
#pragma unroll
  for (int w = 1; w < kRdWaves; ++w) mg = fmaxf(mg, sm[w][0]);
  float sc[kRdWaves], den = 0.f;
#pragma unroll
  for (int w = 0; w < kRdWaves; ++w) {
    sc[w] = rd_scale(sm[w][0], mg);
    den += sm[w][1] * sc[w];
  }
  const int width = a.C - L.c0 < BW ? a.C - L.c0 : BW;
  float* prow = SPLIT ? a.ws + slot * ((int64_t)a.C + 2) : nullptr;
  for (int cl = threadIdx.x; cl < width; cl += 256) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRdWaves; ++w) v += sm[w][2 + cl] * sc[w];
    const int c = L.c0 + cl;
    if (SPLIT) {
      prow[2 + c] = v;
    } else {
      a.out[g * a.ldo + c] = v / den;
      if (a.q_out) a.q_out[g * a.ldo + c] = qrow[c];
    }
  }
  if (L.z == 0 && threadIdx.x == 0) {
    if (SPLIT) {
      prow[0] = mg;
      prow[1] = den;
    } else {
      a.stats[2 * g] = mg;
      a.stats[2 * g + 1] = den;
    }
  }
}

// path 2, second kernel: the chunk states of a graph in chunk order.  The maximum
// is exact in any order; the scales exp(m_k - m_g) of 256 chunks at a time are
// staged in LDS, and a thread sums its channels (at most 4: bw <= 1024) and den
// over the chunks in chunk order.
__global__ __launch_bounds__(256) void k_readout_fwd_merge(RdFwd a, int32_t bw) {
  __shared__ float s_sc[256], s_den[256], s_red[kRdWaves];
  const int64_t g = blockIdx.x;
  const int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (rd_path(cnt, a.C) != 2) return;
  const int tid = threadIdx.x;
  const int64_t chunk = rd_chunk(a.C), nk = (cnt + chunk - 1) / chunk, stride = (int64_t)a.C + 2;
  const float* p0 = a.ws + (s / chunk + g) * stride;
  float mx = -INFINITY;
  for (int64_t k = tid; k < nk; k += 256) mx = fmaxf(mx, p0[k * stride]);
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if ((tid & 63) == 0) s_red[tid >> 6] = mx;
  __syncthreads();
  float mg = s_red[0];
#pragma unroll
  for (int w = 1; w < kRdWaves; ++w) mg = fmaxf(mg, s_red[w]);
  const int c0 = blockIdx.z * bw;
  const int width = a.C - c0 < bw ? a.C - c0 : bw;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, den = 0.f;
  for (int64_t k0 = 0; k0 < nk; k0 += 256) {
    __syncthreads();
    if (k0 + tid < nk) {
      const float sc = rd_scale(p0[(k0 + tid) * stride], mg);
      s_sc[tid] = sc;
      s_den[tid] = p0[(k0 + tid) * stride + 1] * sc;
    }
    __syncthreads();
    const int kn = nk - k0 < 256 ? (int)(nk - k0) : 256;
    for (int j = 0; j < kn; ++j) den += s_den[j];
    const float* pk = p0 + k0 * stride + 2 + c0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cl = tid + t * 256;
      if (cl < width) {
        float v = acc[t];
#pragma unroll 4
        for (int j = 0; j < kn; ++j) v += pk[j * stride + cl] * s_sc[j];
        acc[t] = v;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cl = tid + t * 256;
    if (cl < width) {
      const int c = c0 + cl;
      a.out[g * a.ldo + c] = acc[t] / den;
      if (a.q_out) a.q_out[g * a.ldo + c] = a.q[g * a.ldq + c];
    }
  }
  if (blockIdx.z == 0 && tid == 0) {
    a.stats[2 * g] = mg;
    a.stats[2 * g + 1] = den;
  }
}

// the optional alpha [N]: blockIdx.x = graph, blockIdx.y = 256 nodes of it
__global__ __launch_bounds__(256) void k_readout_alpha(const int64_t* __restrict__ starts, const float* __restrict__ e,
                                                       const float* __restrict__ stats, float* __restrict__ alpha) {
  const int64_t g = blockIdx.x;
  const int64_t s = starts[g], cnt = starts[g + 1] - s;
  const int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x;
  if (i >= cnt) return;
  alpha[s + i] = expf(e[s + i] - stats[2 * g]) / stats[2 * g + 1];
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// The backward over the same node lists as rd_fwd_nodes; dq's part of these
// nodes is left in acc (summed over the node slots when dq is wanted).
template <int VEC>
__device__ __forceinline__ void rd_bwd_nodes(const RdBwd& a, const RdLane& L, int64_t g, int64_t first, int64_t cnt,
                                             int64_t i0, int64_t stride, Frag<VEC> (&acc)[kRdPasses]) {
  const float* drow = a.dr + g * a.lddr;
  const float* qrow = a.q ? a.q + g * a.ldq : nullptr;
  Frag<VEC> dreg[kRdPasses], qreg[kRdPasses], tmp[kRdPasses];
  rd_zero<VEC>(dreg);
  rd_zero<VEC>(qreg);
  rd_zero<VEC>(tmp);
  rd_zero<VEC>(acc);
  rd_load<VEC>(L, drow, dreg);
  if (qrow) rd_load<VEC>(L, qrow, qreg);
  const float sg = group_sum(rd_dot<VEC>(L, a.r + g * a.ldr, drow, dreg, tmp), L.gl);
  const float m = a.stats[2 * g], den = a.stats[2 * g + 1];
  const int64_t iters = cnt > i0 ? (cnt - i0 + stride - 1) / stride : 0;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t i = i0 + it * stride + L.sub;
    const bool live = i < cnt;
    const int64_t n = first + (live ? i : 0);
    const float* xr = a.x + n * a.ldx;
    Frag<VEC> xv[kRdPasses];
    rd_zero<VEC>(xv);
    const float t = group_sum(rd_dot<VEC>(L, xr, drow, dreg, xv), L.gl);
    if (live) {
      const float al = expf(a.e[n] - m) / den;
      const float de = al * (t - sg);
      if (a.dscore && L.fl == 0 && L.z == 0) a.dscore[n] = de;
      if (a.dx) {
        float* dxr = a.dx + n * a.lddx;
#pragma unroll
        for (int p = 0; p < kRdPasses; ++p) {
          const int c = rd_chan<VEC>(L, p);
          if (c < a.C) {
            Frag<VEC> o;
#pragma unroll
            for (int v = 0; v < VEC; ++v) o.v[v] = qrow ? al * dreg[p].v[v] + de * qreg[p].v[v] : al * dreg[p].v[v];
            store_frag<VEC>(dxr + c, o);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < kRdPasses; ++p)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[p].v[v] += de * xv[p].v[v];
    }
  }
  if (a.dq) {
    for (int d = L.gl; d < 64; d <<= 1) {
#pragma unroll
      for (int p = 0; p < kRdPasses; ++p)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[p].v[v] += __shfl_xor(acc[p].v[v], d);
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void k_readout_bwd_wave(RdBwd a) {
  const RdLane L = rd_lane<VEC>(a.C, a.glog, a.nb);
  const int64_t g = (int64_t)blockIdx.x * kRdWaves + uni((int)(threadIdx.x >> 6));
  if (g >= a.G) return;
  const int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (cnt > 0 && rd_path(cnt, a.C) != 0) return;
  Frag<VEC> acc[kRdPasses];
  rd_zero<VEC>(acc);
  if (cnt > 0) rd_bwd_nodes<VEC>(a, L, g, s, cnt, 0, L.nsub, acc);
  if (a.dq && L.sub == 0) {
#pragma unroll
    for (int p = 0; p < kRdPasses; ++p) {
      const int c = rd_chan<VEC>(L, p);
      if (c < a.C) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) a.dq[g * a.lddq + c + v] = acc[p].v[v];
      }
    }
  }
}

template <int VEC, bool SPLIT>
__global__ __launch_bounds__(256) void k_readout_bwd_wg(RdBwd a) {
  constexpr int BW = 64 * VEC * kRdPasses;
  __shared__ float sm[kRdWaves][BW];
  const RdLane L = rd_lane<VEC>(a.C, a.glog, a.nb);
  const int wave = uni((int)(threadIdx.x >> 6));
  const int64_t g = blockIdx.x;
  int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (cnt == 0 || rd_path(cnt, a.C) != (SPLIT ? 2 : 1)) return;
  int64_t slot = 0;
  if (SPLIT) {
    const int64_t chunk = rd_chunk(a.C), b = (int64_t)blockIdx.y * chunk;
    if (b >= cnt) return;
    slot = s / chunk + g + blockIdx.y;
    s += b;
    cnt = cnt - b < chunk ? cnt - b : chunk;
  }
  Frag<VEC> acc[kRdPasses];
  rd_bwd_nodes<VEC>(a, L, g, s, cnt, (int64_t)wave * L.nsub, (int64_t)kRdWaves * L.nsub, acc);
  if (!a.dq) return;
  if (L.sub == 0) {
#pragma unroll
    for (int p = 0; p < kRdPasses; ++p) {
      const int c = rd_chan<VEC>(L, p);
      if (c < a.C) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) sm[wave][c - L.c0 + v] = acc[p].v[v];
      }
    }
  }
  __syncthreads();
  const int width = a.C - L.c0 < BW ? a.C - L.c0 : BW;
  for (int cl = threadIdx.x; cl < width; cl += 256) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRdWaves; ++w) v += sm[w][cl];
    const int c = L.c0 + cl;
    if (SPLIT) {
      a.ws[slot * ((int64_t)a.C + 2) + 2 + c] = v;
    } else {
      a.dq[g * a.lddq + c] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_readout_bwd_merge(RdBwd a) {
  const int64_t g = blockIdx.x;
  const int64_t s = a.starts[g], cnt = a.starts[g + 1] - s;
  if (rd_path(cnt, a.C) != 2) return;
  const int64_t chunk = rd_chunk(a.C), nk = (cnt + chunk - 1) / chunk, stride = (int64_t)a.C + 2;
  const float* p0 = a.ws + (s / chunk + g) * stride + 2;
  for (int c = blockIdx.y * 256 + threadIdx.x; c < a.C; c += gridDim.y * 256) {
    float v = 0.f;
#pragma unroll 8
    for (int64_t k = 0; k < nk; ++k) v += p0[k * stride + c];
    a.dq[g * a.lddq + c] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static inline bool rd_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// lanes per row and channel tiles for VEC-wide fragments
static void rd_geometry(int32_t C, int vec, int32_t* glog, int32_t* nb) {
  const int64_t frags = ceil_div(C, vec);
  *nb = (int32_t)ceil_div(frags, 64 * kRdPasses);
  int gl = 0;
  while ((1 << gl) < frags && gl < 6) ++gl;
  *glog = gl;
}

static int rd_common(const char* fn, int64_t n, int32_t C, const int64_t* starts, int64_t n_graphs, int64_t max_n) {
  MP_CHECK_ARG(C >= 1, "%s: C = %d < 1", fn, C);
  MP_CHECK_ARG(n >= 0, "%s: n = %lld < 0", fn, (long long)n);
  MP_CHECK_ARG(n_graphs >= 0, "%s: n_graphs = %lld < 0", fn, (long long)n_graphs);
  MP_CHECK_ARG(max_n >= 0 && max_n <= n, "%s: max_n = %lld outside [0, n = %lld]", fn, (long long)max_n, (long long)n);
  MP_CHECK_ARG(starts != nullptr, "%s: starts is NULL", fn);
  MP_CHECK_ARG(n_graphs > 0 || n == 0, "%s: n = %lld nodes in n_graphs = 0 graphs", fn, (long long)n);
  return MP_OK;
}

static inline size_t rd_rows_bytes(int64_t rows, int64_t ld, int32_t C) {
  return rows == 0 ? 0 : ((size_t)(rows - 1) * ld + C) * sizeof(float);
}

// Every grid dimension and every launch as a whole (HIP takes fewer than 2^32
// threads per launch: 2^24 workgroups of 256) is checked before the first
// launch, so a refused shape leaves its outputs unwritten.  The split launch
// holds n_graphs * chunks of the largest graph workgroups per channel tile.
static int rd_grid(const char* fn, int64_t n_graphs, int64_t max_n, int32_t C, int32_t nb, bool alpha) {
  const int64_t chunks = ceil_div(max_n, rd_chunk(C)), blocks256 = ceil_div(max_n, 256);
  MP_CHECK_ARG(n_graphs <= 0x7fffffff && nb <= 65535 && chunks <= 65535 && blocks256 <= 65535,
               "%s: grid too large (n_graphs %lld, max_n %lld, C %d)", fn, (long long)n_graphs, (long long)max_n, C);
  int64_t per_graph = 1;
  if (rd_path(max_n, C) == 2) per_graph = chunks;
  if (alpha && blocks256 > per_graph * nb) per_graph = ceil_div(blocks256, nb);
  MP_CHECK_ARG(n_graphs * per_graph * nb < ((int64_t)1 << 24),
               "%s: launch too large: n_graphs %lld x %lld workgroups for the largest graph (max_n %lld) x %d "
               "channel tiles is not below 2^24 workgroups",
               fn, (long long)n_graphs, (long long)per_graph, (long long)max_n, nb);
  return MP_OK;
}

static int readout_fwd(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* starts, int64_t n_graphs,
                       int64_t max_n, const float* q, int64_t ldq, const float* score, float* out, int64_t ldo,
                       size_t out_bytes, float* q_out, size_t q_out_bytes, float* e, size_t e_bytes, float* stats,
                       size_t stats_bytes, float* alpha, size_t alpha_bytes, void* ws, size_t ws_bytes, void* stream,
                       int64_t* launches) {
  const char* fn = "mp_attention_readout_f32";
  if (int rc = rd_common(fn, n, C, starts, n_graphs, max_n)) return rc;
  MP_CHECK_ARG((q != nullptr) != (score != nullptr), "%s: exactly one of q and score must be given (got %s)", fn,
               q ? "both" : "neither");
  MP_CHECK_ARG(ldx >= C, "%s: ldx = %lld < C = %d", fn, (long long)ldx, C);
  MP_CHECK_ARG(!q || ldq >= C, "%s: ldq = %lld < C = %d", fn, (long long)ldq, C);
  MP_CHECK_ARG(ldo >= C, "%s: ldo = %lld < C = %d", fn, (long long)ldo, C);
  MP_CHECK_ARG(!q_out || q, "%s: q_out needs q (query mode)", fn);
  MP_CHECK_ARG(x != nullptr || n == 0, "%s: x is NULL", fn);
  MP_CHECK_ARG(e != nullptr || n == 0, "%s: e is NULL", fn);
  MP_CHECK_ARG(out != nullptr || n_graphs == 0, "%s: out is NULL", fn);
  MP_CHECK_ARG(stats != nullptr || n_graphs == 0, "%s: stats is NULL", fn);
  MP_CHECK_EXTENT(fn, "out", out_bytes, rd_rows_bytes(n_graphs, ldo, C));
  if (q_out) MP_CHECK_EXTENT(fn, "q_out", q_out_bytes, rd_rows_bytes(n_graphs, ldo, C));
  MP_CHECK_EXTENT(fn, "e", e_bytes, (size_t)n * sizeof(float));
  MP_CHECK_EXTENT(fn, "stats", stats_bytes, (size_t)n_graphs * 2 * sizeof(float));
  if (alpha) MP_CHECK_EXTENT(fn, "alpha", alpha_bytes, (size_t)n * sizeof(float));
  const ReadoutWs w(ws, n, n_graphs, max_n, C);
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  if (n_graphs == 0) return MP_OK;
  const int vec = (C % 4 == 0 && ldx % 4 == 0 && rd_al16(x) && (!q || (ldq % 4 == 0 && rd_al16(q)))) ? 4 : 1;
  int32_t glog, nb;
  rd_geometry(C, vec, &glog, &nb);
  if (int rc = rd_grid(fn, n_graphs, max_n, C, nb, alpha != nullptr)) return rc;
  const RdFwd a{x, ldx, starts, n_graphs, q, ldq, score, out, ldo, q_out, e, stats, alpha, w.part, C, glog, nb};
  const int pmax = rd_path(max_n, C);
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  const dim3 gw((unsigned)ceil_div(n_graphs, kRdWaves), 1, (unsigned)nb), gg((unsigned)n_graphs, 1, (unsigned)nb);
  const dim3 gs((unsigned)n_graphs, (unsigned)ceil_div(max_n, rd_chunk(C)), (unsigned)nb);
  if (vec == 4) {
    hipLaunchKernelGGL(k_readout_fwd_wave<4>, gw, dim3(256), 0, st, a);
    if (pmax >= 1) hipLaunchKernelGGL((k_readout_fwd_wg<4, false>), gg, dim3(256), 0, st, a);
    if (pmax == 2) hipLaunchKernelGGL((k_readout_fwd_wg<4, true>), gs, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_readout_fwd_wave<1>, gw, dim3(256), 0, st, a);
    if (pmax >= 1) hipLaunchKernelGGL((k_readout_fwd_wg<1, false>), gg, dim3(256), 0, st, a);
    if (pmax == 2) hipLaunchKernelGGL((k_readout_fwd_wg<1, true>), gs, dim3(256), 0, st, a);
  }
  *launches = 1 + (pmax >= 1) + (pmax == 2);
  if (pmax == 2) {
    hipLaunchKernelGGL(k_readout_fwd_merge, gg, dim3(256), 0, st, a, (int32_t)(64 * vec * kRdPasses));
    ++*launches;
  }
  if (alpha && max_n > 0) {
    hipLaunchKernelGGL(k_readout_alpha, dim3((unsigned)n_graphs, (unsigned)ceil_div(max_n, 256)), dim3(256), 0, st,
                       starts, e, stats, alpha);
    ++*launches;
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int readout_bwd(const float* dr, int64_t lddr, const float* x, int64_t ldx, int64_t n, int32_t C,
                       const int64_t* starts, int64_t n_graphs, int64_t max_n, const float* q, int64_t ldq,
                       const float* e, const float* stats, const float* r, int64_t ldr, float* dx, int64_t lddx,
                       size_t dx_bytes, float* dq, int64_t lddq, size_t dq_bytes, float* dscore, size_t dscore_bytes,
                       void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_attention_readout_bwd_f32";
  if (int rc = rd_common(fn, n, C, starts, n_graphs, max_n)) return rc;
  MP_CHECK_ARG(!(q && dscore), "%s: dscore is the score mode's gradient, q was given", fn);
  MP_CHECK_ARG(q || !dq, "%s: dq is the query mode's gradient, q is NULL", fn);
  MP_CHECK_ARG(ldx >= C, "%s: ldx = %lld < C = %d", fn, (long long)ldx, C);
  MP_CHECK_ARG(lddr >= C, "%s: lddr = %lld < C = %d", fn, (long long)lddr, C);
  MP_CHECK_ARG(ldr >= C, "%s: ldr = %lld < C = %d", fn, (long long)ldr, C);
  MP_CHECK_ARG(!q || ldq >= C, "%s: ldq = %lld < C = %d", fn, (long long)ldq, C);
  MP_CHECK_ARG(!dx || lddx >= C, "%s: lddx = %lld < C = %d", fn, (long long)lddx, C);
  MP_CHECK_ARG(!dq || lddq >= C, "%s: lddq = %lld < C = %d", fn, (long long)lddq, C);
  MP_CHECK_ARG(x != nullptr || n == 0, "%s: x is NULL", fn);
  MP_CHECK_ARG(e != nullptr || n == 0, "%s: e is NULL", fn);
  MP_CHECK_ARG(dr != nullptr || n_graphs == 0, "%s: dr is NULL", fn);
  MP_CHECK_ARG(r != nullptr || n_graphs == 0, "%s: r is NULL", fn);
  MP_CHECK_ARG(stats != nullptr || n_graphs == 0, "%s: stats is NULL", fn);
  if (dx) MP_CHECK_EXTENT(fn, "dx", dx_bytes, rd_rows_bytes(n, lddx, C));
  if (dq) MP_CHECK_EXTENT(fn, "dq", dq_bytes, rd_rows_bytes(n_graphs, lddq, C));
  if (dscore) MP_CHECK_EXTENT(fn, "dscore", dscore_bytes, (size_t)n * sizeof(float));
  const ReadoutWs w(ws, n, n_graphs, max_n, C);
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  if (n_graphs == 0 || (!dx && !dq && !dscore)) return MP_OK;
  const bool al = C % 4 == 0 && ldx % 4 == 0 && rd_al16(x) && lddr % 4 == 0 && rd_al16(dr) && ldr % 4 == 0 &&
                  rd_al16(r) && (!q || (ldq % 4 == 0 && rd_al16(q))) && (!dx || (lddx % 4 == 0 && rd_al16(dx)));
  const int vec = al ? 4 : 1;
  int32_t glog, nb;
  rd_geometry(C, vec, &glog, &nb);
  if (int rc = rd_grid(fn, n_graphs, max_n, C, nb, false)) return rc;
  const RdBwd a{dr, lddr, x, ldx, starts, n_graphs, q, ldq, e, stats, r, ldr, dx, lddx, dq, lddq, dscore, w.part, C,
                glog, nb};
  const int pmax = rd_path(max_n, C);
  hipStream_t st = as_stream(stream);
  MP_DEVICE_GUARD(stream);
  const dim3 gw((unsigned)ceil_div(n_graphs, kRdWaves), 1, (unsigned)nb), gg((unsigned)n_graphs, 1, (unsigned)nb);
  const dim3 gs((unsigned)n_graphs, (unsigned)ceil_div(max_n, rd_chunk(C)), (unsigned)nb);
  if (vec == 4) {
    hipLaunchKernelGGL(k_readout_bwd_wave<4>, gw, dim3(256), 0, st, a);
    if (pmax >= 1) hipLaunchKernelGGL((k_readout_bwd_wg<4, false>), gg, dim3(256), 0, st, a);
    if (pmax == 2) hipLaunchKernelGGL((k_readout_bwd_wg<4, true>), gs, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_readout_bwd_wave<1>, gw, dim3(256), 0, st, a);
    if (pmax >= 1) hipLaunchKernelGGL((k_readout_bwd_wg<1, false>), gg, dim3(256), 0, st, a);
    if (pmax == 2) hipLaunchKernelGGL((k_readout_bwd_wg<1, true>), gs, dim3(256), 0, st, a);
  }
  *launches = 1 + (pmax >= 1) + (pmax == 2);
  if (pmax == 2 && dq) {
    const int64_t by = ceil_div(C, 256);
    hipLaunchKernelGGL(k_readout_bwd_merge, dim3((unsigned)n_graphs, (unsigned)(by < 64 ? by : 64)), dim3(256), 0, st,
                       a);
    ++*launches;
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_readout_path(int64_t n_g, int32_t C) {
  if (C < 1 || n_g < 0) {
    set_error("mp_readout_path: n_g = %lld, C = %d (n_g >= 0 and C >= 1)", (long long)n_g, C);
    return -(int64_t)MP_ERR_ARG;
  }
  return rd_path(n_g, C);
}

extern "C" int64_t mp_readout_chunk(int32_t C) {
  if (C < 1) {
    set_error("mp_readout_chunk: C = %d < 1", C);
    return -(int64_t)MP_ERR_ARG;
  }
  return rd_chunk(C);
}

extern "C" size_t mp_readout_workspace(int64_t n, int64_t n_graphs, int64_t max_n, int32_t C) {
  if (n < 0 || n_graphs < 0 || max_n < 0 || C < 1) return ReadoutWs{nullptr, 0, 0, 0, 1}.total(0);
  return ReadoutWs{nullptr, n, n_graphs, max_n, C}.total(0);
}

extern "C" int64_t mp_attention_readout_f32(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* starts,
                                            int64_t n_graphs, int64_t max_n, const float* q, int64_t ldq,
                                            const float* score, float* out, int64_t ldo, size_t out_bytes,
                                            float* q_out, size_t q_out_bytes, float* e, size_t e_bytes, float* stats,
                                            size_t stats_bytes, float* alpha, size_t alpha_bytes, void* ws,
                                            size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = readout_fwd(x, ldx, n, C, starts, n_graphs, max_n, q, ldq, score, out, ldo, out_bytes, q_out,
                             q_out_bytes, e, e_bytes, stats, stats_bytes, alpha, alpha_bytes, ws, ws_bytes, stream,
                             &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_attention_readout_bwd_f32(const float* dr, int64_t lddr, const float* x, int64_t ldx, int64_t n,
                                                int32_t C, const int64_t* starts, int64_t n_graphs, int64_t max_n,
                                                const float* q, int64_t ldq, const float* e, const float* stats,
                                                const float* r, int64_t ldr, float* dx, int64_t lddx, size_t dx_bytes,
                                                float* dq, int64_t lddq, size_t dq_bytes, float* dscore,
                                                size_t dscore_bytes, void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = readout_bwd(dr, lddr, x, ldx, n, C, starts, n_graphs, max_n, q, ldq, e, stats, r, ldr, dx, lddx,
                             dx_bytes, dq, lddq, dq_bytes, dscore, dscore_bytes, ws, ws_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}
