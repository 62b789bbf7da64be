// ARMAConv's recurrent step (gfx950): K parallel stacks, one fused launch per step.
//
// PyG 1.4.3 nn.conv.arma_conv [U], step t of T, per stack k:
//   pre_t[k] = A (H_t[k] W_t[k]) + x_drop V_t[k] + b_t[k],   H_{t+1}[k] = act(pre_t[k])
// with A = D^-1/2 W D^-1/2 summed at edge_index[0], H_0[k] = x, and the layer's
// output the mean of H_T over the stacks.  Upstream materialises [K, E, C]
// messages and walks the edge list K times per step.
//
// Layout.  Every node-level operand is [N, K*C] fp32, stack-minor: entry (k, c)
// of node n at n * ld + k * C + c, rows P = K*C rounded up to 4 floats wide (ld a
// multiple of 4, 16-byte aligned), the P - K*C padding columns written as zeros.
// One gathered row therefore carries all K stacks, and one edge-index walk serves
// them all.  A lane owns the 4 consecutive floats j = 4 * lane .. 4 * lane + 3 of
// the flattened (k, c) index; (k, c) = (j / C, j % C) is taken per float, so a
// stack boundary may fall inside a lane's vector (K = 3, C = 7).  C is not padded
// inside the row: at C % 4 == 0 a lane's vector already lies inside one stack and
// the transform takes its weights as one 16-byte LDS read per input channel.
//
// The step is a reducer on the merge-path engine (mp_agg.h): tasks of L = 4 .. 64
// lanes (the power of two covering P / 4), the slot window and its in-flight
// gathers (SlotWin, run_slots), the slabs of rows cut at a task boundary
// (slab_ref) and the order in which the fix-up adds a hub row's partials are the
// engine's.  The two kernels here are the engine's task walk and fix-up with one
// step in front -- the weight block staged in LDS by the whole workgroup before
// any wave leaves -- and a second argument block (a note at k_agg_main points
// here: a change to the walk there must be mirrored).
// Per slot:
//   acc += lap_e * Y_t[col_e, :]        (separately rounded multiply and add)
// and in finish(), once per complete row n -- from the main kernel or from the
// fix-up, never from a partial:
//   forward   h = act(acc + S_t[n, :])                        S_t = x_drop V_t + b_t
//             H_{t+1}[n, :] = h                               when the caller asks
//             Y_{t+1}[n, k, :] = h[k, :] W_{t+1}[k]           when a next step exists
//             out[n, :] = (1 / K) sum_k h[k, :]               on the last step, k ascending
//   backward  (transposed CSR, x = dPre_t)  dY_t[n, :] = acc
//             dPre_{t-1}[n, k, :] = (dY_t[n, k, :] W_t[k]^T) * (H_t[n, k, :] > 0)   for t >= 1
// A row without slots finishes with acc = 0: act(S_t).
//
// The per-stack C x C transform is a wave-level mat-vec, not MFMA: rows finish one
// at a time, at different times in the lane groups of one wave, so there is never
// a tile of finished rows to feed a matrix instruction without holding rows back.
// The finished row goes through a per-wave LDS row buffer (each lane group writes
// and reads its own 4 * L floats; the LDS operations of one wave execute in
// order, so no workgroup barrier is needed), the [K, C, C] weight block is staged
// in LDS once per workgroup before the task walk, and a lane reads its
// stack's h[k, c'] as broadcast reads.  The backward passes W_t[k]^T as the block,
// so both directions run the same loop.  fp32, fixed summation order, no atomics:
// two runs are bitwise equal.
#include "mp_agg.h"
#include "mp_workspace.h"

namespace mp {

constexpr int kArmaMaxWidth = 256;  // K * C: one feature tile of 64 lanes x 4 floats
constexpr int kArmaMaxC = 64;
constexpr int kArmaMaxW = 8192;     // K * C * C floats of the weight block: 32 KiB of LDS

__shared__ __attribute__((aligned(16))) float arma_w_lds[kArmaMaxW];
__shared__ __attribute__((aligned(16))) float arma_row_lds[kWavesPerBlock][256];

// What a step reads and writes beside the gathered operand (AggArgs: x = Y_t or dPre_t, w = lap).
struct ArmaArgs {
  const float* s;  // forward: S_t (skip + bias); backward: H_t, the mask source, or NULL
  int64_t lds;
  const float* w;  // [K, C, C]: W_{t+1} (forward), W_t transposed per stack (backward), or NULL
  float* h;        // forward: H_{t+1} when the caller wants it; backward: dY_t
  int64_t ldh;
  float* n;        // forward: Y_{t+1}; backward: dPre_{t-1}
  int64_t ldn;
  float* out;      // forward, last step: [n_rows, C]
  int64_t ldo;
  int32_t K, C, relu;
};

template <bool BWD>
struct ArmaRed : RedFlags {
  static constexpr bool kW = true;
  struct Part {
    float v[4];
  };
  float acc[4];
  float* buf;  // this lane group's row buffer: 4 * L floats
  int h = 0;   // unused (GAT only)

  __device__ ArmaRed(int f) {
    // f = 4 * (lane within its group): the group's buffer starts at 4 * (the group's first lane)
    buf = arma_row_lds[threadIdx.x >> 6] + (lane_id() * 4 - f);
  }
  __device__ __forceinline__ void begin() {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = 0.f;
  }
  __device__ __forceinline__ void consume(const Frag<4>& v, float wt, int, float) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(wt, v.v[k]));
  }
  __device__ __forceinline__ void save(PRef r, bool) const {
    Frag<4> o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.v[k] = acc[k];
    store_frag<4>(r.v, o);
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Frag<4> o = load_frag<4>(r.v);
    Part q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = o.v[k];
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = q.v[k];
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], q.v[k]);
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = acc[k];
    return q;
  }

  // o[i] = sum_c' buf[k, c'] * W[k][c'][c] for the lane's floats (k, c); padding floats give 0
  __device__ __forceinline__ void transform(int K, int C, int f, bool act, float* o) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = 0.f;
    if ((C & 3) == 0) {
      const int fa = act ? f : 0;  // an inactive lane reads what lane 0 reads and stores nothing
      const int k = fa / C;
      const float* hk = buf + k * C;
      const float* wk = arma_w_lds + k * C * C + (fa - k * C);
      for (int cp = 0; cp < C; ++cp) {
        const float hh = hk[cp];
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wk + cp * C);
        o[0] = __fmaf_rn(hh, w4.x, o[0]);
        o[1] = __fmaf_rn(hh, w4.y, o[1]);
        o[2] = __fmaf_rn(hh, w4.z, o[2]);
        o[3] = __fmaf_rn(hh, w4.w, o[3]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = f + i;
        if (act && j < K * C) {
          const int k = j / C;
          const float* hk = buf + k * C;
          const float* wk = arma_w_lds + k * C * C + (j - k * C);
          float t = 0.f;
          for (int cp = 0; cp < C; ++cp) t = __fmaf_rn(hk[cp], wk[cp * C], t);
          o[i] = t;
        }
      }
    }
  }

  __device__ __forceinline__ void finish(const ArmaArgs& p, int64_t row, int f, bool act) {
    const int K = p.K, C = p.C, KC = K * C;
    Frag<4> hv;
#pragma unroll
    for (int i = 0; i < 4; ++i) hv.v[i] = acc[i];
    if constexpr (!BWD) {
      if (act) {
        const Frag<4> s = load_frag<4>(p.s + row * p.lds + f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t = __fadd_rn(hv.v[i], s.v[i]);
          hv.v[i] = (p.relu && !(t > 0.f)) ? 0.f : t;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (f + i >= KC) hv.v[i] = 0.f;  // the row's padding columns are zeros whatever the operands held there
    if (act && p.h) store_out<4>(p.h + row * p.ldh + f, hv);
    if (!p.w && (BWD || !p.out)) return;
    // the finished row, through this group's LDS buffer; the wave's LDS operations run in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (act) store_frag<4>(buf + f, hv);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (p.w) {
      Frag<4> o;
      transform(K, C, f, act, o.v);
      if (!act) return;
      if constexpr (BWD) {
        if (p.s) {
          const Frag<4> m = load_frag<4>(p.s + row * p.lds + f);
#pragma unroll
          for (int i = 0; i < 4; ++i) o.v[i] = m.v[i] > 0.f ? o.v[i] : 0.f;
        }
      }
      store_out<4>(p.n + row * p.ldn + f, o);
    } else {
      // the mean over the stacks, k ascending
      const float inv = 1.f / (float)K;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = f + i;
        if (act && j < C) {
          float t = buf[j];
          for (int k = 1; k < K; ++k) t = __fadd_rn(t, buf[k * C + j]);
          p.out[row * p.ldo + j] = __fmul_rn(t, inv);
        }
      }
    }
  }
};

// the weight block, once per workgroup, before any wave leaves
__device__ __forceinline__ void arma_stage(const ArmaArgs& q) {
  if (q.w) {
    const int n = q.K * q.C * q.C;
    for (int i = (int)threadIdx.x; i < n; i += kBlock) arma_w_lds[i] = q.w[i];
  }
  __syncthreads();
}

// k_agg_main's task walk (one feature tile: P <= 4 * L) behind the staging
template <bool BWD, int L>
__global__ __launch_bounds__(kBlock) void k_arma_main(AggArgs p, ArmaArgs q) {
  arma_stage(q);
  using GR = Grp<L>;
  using Red = ArmaRed<BWD>;
  constexpr int U = kMainU<Red, 4, L>;
  const int lane = lane_id();
  const int gl = lane & (L - 1);
  const int wave = (int)blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
  const int w = GR::un(wave * GR::G + lane / L);  // this group's task
  if (w >= p.n_waves) return;
  const int f = gl * 4;
  const bool act = f < p.F;
  const uint32_t foff = (uint32_t)(act ? f : 0) * 4u;

  const int r_first = GR::un(p.wave_row[w]);
  const int r_last = GR::un(p.wave_row[w + 1]);
  const int64_t e_begin = GR::un(p.wave_slot[w]);
  const int64_t e_end = GR::un(p.wave_slot[w + 1]);

  Red red(f);
  SlotWin<true, false, L> win;
  win.init(p, e_begin, e_end, gl);

  // rowptr window: rp = rowptr[rbase + gl]
  int rbase = r_first;
  int rp = (rbase + gl <= p.n_rows) ? p.rowptr[rbase + gl] : 0;

  // continuation of the row owned by an earlier task
  {
    const int64_t ce = GR::bc(rp, 0);  // rowptr[r_first] (== n_edges when r_first == n_rows)
    if (e_begin < ce) {
      red.begin();
      run_slots<Red, 4, U, L>(red, p, win, e_begin, ce < e_end ? ce : e_end, foff, gl);
      if (act) red.save(slab_ref(p, 2 * (int64_t)w, f, red), false);
    }
  }
  // rows owned by this task
  for (int r = r_first; r < r_last; ++r) {
    if (r + 1 - rbase > L - 1) {
      rbase = r;
      rp = (rbase + gl <= p.n_rows) ? p.rowptr[rbase + gl] : 0;
    }
    const int64_t rs = GR::bc(rp, r - rbase);
    const int64_t re = GR::bc(rp, r - rbase + 1);
    red.begin();
    if (re <= e_end) {
      run_slots<Red, 4, U, L>(red, p, win, rs, re, foff, gl);
      red.finish(q, r, f, act);
    } else {
      run_slots<Red, 4, U, L>(red, p, win, rs, e_end, foff, gl);
      if (act) red.save(slab_ref(p, 2 * (int64_t)w + 1, f, red), false);
    }
  }
}

// k_agg_fixup behind the staging: one 4-wave block per split row; wave q adds its share of the
// row's chain of partials in task order, wave 0 adds the waves' sums in wave order and finishes
template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_arma_fixup(AggArgs p, ArmaArgs q) {
  arma_stage(q);
  using Red = ArmaRed<BWD>;
  constexpr int U = 4;
  __shared__ typename Red::Part lds[kWavesPerBlock - 1][64];
  __shared__ int has[kWavesPerBlock];
  const int lane = lane_id();
  const int wid = uni((int)(threadIdx.x >> 6));
  const int f = lane * 4;
  const bool act = f < p.F;
  const int fs = act ? f : 0;
  const int last = uni(p.split_waves[blockIdx.x]);
  const int r = uni(p.wave_row[last]) - 1;
  // owner = last task whose first owned row is <= r
  int lo = 0, hi = p.n_waves;  // wave_row[n_waves] = n_rows > r
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.wave_row[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  const int owner = uni(lo);
  const int n = last - owner + 1;
  const int c = (n + kWavesPerBlock - 1) / kWavesPerBlock;
  const int b0 = wid * c;
  const int b1 = min(n, b0 + c);
  Red red(f);
  auto item = [&](int k) {
    const int64_t slot = k == 0 ? 2 * (int64_t)owner + 1 : 2 * (int64_t)(owner + k);
    return slab_ref(p, slot, fs, red);
  };
  const bool mine = b0 < b1;
  if (mine) {
    red.set(Red::load(item(b0)));
    for (int k = b0 + 1; k < b1; k += U) {
      typename Red::Part t[U];
#pragma unroll
      for (int u = 0; u < U; ++u) t[u] = Red::load(item(min(k + u, b1 - 1)));
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (k + u < b1) red.merge(t[u]);
    }
  }
  if (lane == 0) has[wid] = mine ? 1 : 0;
  if (wid > 0 && mine) lds[wid - 1][lane] = red.part();
  __syncthreads();
  if (wid != 0) return;
  for (int k = 1; k < kWavesPerBlock; ++k)
    if (has[k]) red.merge(lds[k - 1][lane]);
  red.finish(q, r, f, act);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int arma_shape(const char* fn, int32_t K, int32_t C) {
  MP_CHECK_ARG(K >= 1, "%s: K = %d < 1", fn, K);
  MP_CHECK_ARG(C >= 1, "%s: C = %d < 1", fn, C);
  MP_CHECK_ARG(C <= kArmaMaxC, "%s: C = %d above the limit C <= %d", fn, C, kArmaMaxC);
  MP_CHECK_ARG((int64_t)K * C <= kArmaMaxWidth, "%s: K * C = %lld above the limit K * C <= %d", fn,
               (long long)((int64_t)K * C), kArmaMaxWidth);
  MP_CHECK_ARG((int64_t)K * C * C <= kArmaMaxW, "%s: K * C * C = %lld above the limit K * C * C <= %d", fn,
               (long long)((int64_t)K * C * C), kArmaMaxW);
  return MP_OK;
}

static inline int arma_width(int32_t K, int32_t C) { return (K * C + 3) & ~3; }

// The slab of one step: two slots per task (continuation, head) of one padded row each.
struct ArmaWs : Carver {
  float* slab;
  ArmaWs(void* ws, int64_t n_waves, int P) : Carver(ws), slab(take<float>(2 * n_waves * slab_ld_for(P))) {}
};

// one operand [n, P] under its row stride; required = false lets it be absent
static int arma_rows(const char* fn, const char* name, const void* p, int64_t ld, size_t bytes, int64_t n, int P,
                     bool required = true) {
  if (p == nullptr && !required) return MP_OK;
  MP_CHECK_ARG(p != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_ARG(ld >= P, "%s: ld of %s = %lld < %d", fn, name, (long long)ld, P);
  MP_CHECK_ARG(ld % 4 == 0 && (uintptr_t)p % 16 == 0, "%s: %s must be 16-byte aligned with ld a multiple of 4", fn,
               name);
  MP_CHECK_EXTENT(fn, name, bytes, n <= 0 ? 0 : ((size_t)(n - 1) * ld + P) * sizeof(float));
  return MP_OK;
}

static int arma_graph(const char* fn, const mp_csr* g, const float* lap, size_t lap_bytes, int P, void* ws,
                      size_t ws_bytes) {
  if (int rc = check_graph(g, fn)) return rc;
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->n_rows <= 0x7fffffff && g->n_edges <= 0x7fffffff, "%s: n_rows / n_edges above 2^31 - 1", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the step gathers by column)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  MP_CHECK_ARG(g->n_split >= 0 && g->n_split <= g->n_waves, "%s: g->n_split = %d outside [0, n_waves = %d]", fn,
               g->n_split, g->n_waves);
  MP_CHECK_ARG(lap != nullptr || g->n_edges == 0, "%s: lap is NULL", fn);
  MP_CHECK_EXTENT(fn, "lap", lap_bytes, (size_t)g->n_edges * sizeof(float));
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, ArmaWs(nullptr, g->n_waves, P).total(0));
  return MP_OK;
}

using ArmaKernel = void (*)(AggArgs, ArmaArgs);

template <bool BWD>
static int arma_run(const mp_csr* g, AggArgs& a, const ArmaArgs& q, void* ws, void* stream, int64_t* launches) {
  a.slab_v = ArmaWs(ws, g->n_waves, a.F).slab;
  a.slab_ld = slab_ld_for(a.F);
  int lanes = next_pow2(a.F / 4);
  lanes = lanes < 4 ? 4 : lanes;
  int per_block = kWavesPerBlock;
  const ArmaKernel main = with_lanes<4>(lanes, [&](auto lc) -> ArmaKernel {
    constexpr int L = decltype(lc)::value;
    per_block = kWavesPerBlock * (64 / L);
    return k_arma_main<BWD, L>;
  });
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(main, dim3((unsigned)ceil_div(a.n_waves, per_block)), dim3(kBlock), 0, as_stream(stream), a, q);
  MP_CHECK_LAUNCH();
  *launches = 1;
  if (a.n_split > 0) {
    hipLaunchKernelGGL(k_arma_fixup<BWD>, dim3((unsigned)a.n_split), dim3(kBlock), 0, as_stream(stream), a, q);
    MP_CHECK_LAUNCH();
    *launches = 2;
  }
  return MP_OK;
}

static int arma_step(const mp_csr* g, const float* lap, size_t lap_bytes, const float* y, int64_t ldy, size_t y_bytes,
                     const float* s, int64_t lds, size_t s_bytes, const float* w_next, size_t w_bytes, int32_t K,
                     int32_t C, int32_t relu, float* h_out, int64_t ldh, size_t h_bytes, float* y_next, int64_t ldn,
                     size_t n_bytes, float* out, int64_t ldo, size_t out_bytes, void* ws, size_t ws_bytes,
                     void* stream, int64_t* launches) {
  const char* fn = "mp_arma_step_f32";
  if (int rc = arma_shape(fn, K, C)) return rc;
  const int P = arma_width(K, C);
  if (int rc = arma_graph(fn, g, lap, lap_bytes, P, ws, ws_bytes)) return rc;
  MP_CHECK_ARG(relu == 0 || relu == 1, "%s: relu = %d is neither 0 nor 1", fn, relu);
  MP_CHECK_ARG((w_next != nullptr) == (y_next != nullptr), "%s: w_next and y_next come together", fn);
  MP_CHECK_ARG((y_next != nullptr) != (out != nullptr),
               "%s: exactly one of y_next (a next step exists) and out (the last step)", fn);
  if (int rc = arma_rows(fn, "y", y, ldy, y_bytes, g->n_cols, P)) return rc;
  if (int rc = arma_rows(fn, "s", s, lds, s_bytes, g->n_rows, P)) return rc;
  if (int rc = arma_rows(fn, "h_out", h_out, ldh, h_bytes, g->n_rows, P, false)) return rc;
  if (int rc = arma_rows(fn, "y_next", y_next, ldn, n_bytes, g->n_rows, P, false)) return rc;
  if (w_next) MP_CHECK_EXTENT(fn, "w_next", w_bytes, (size_t)K * C * C * sizeof(float));
  if (out) {
    MP_CHECK_ARG(ldo >= C, "%s: ld of out = %lld < C = %d", fn, (long long)ldo, C);
    MP_CHECK_EXTENT(fn, "out", out_bytes, g->n_rows <= 0 ? 0 : ((size_t)(g->n_rows - 1) * ldo + C) * sizeof(float));
  }
  if (g->n_rows == 0) return MP_OK;
  AggArgs a{};
  fill_graph(a, g);
  a.F = P;
  a.w = lap;
  a.x = y;
  a.ldx = ldy;
  const ArmaArgs q{s, lds, w_next, h_out, ldh, y_next, ldn, out, ldo, K, C, relu};
  return arma_run<false>(g, a, q, ws, stream, launches);
}

static int arma_step_bwd(const mp_csr* g, const float* lap, size_t lap_bytes, const float* dpre, int64_t ldp,
                         size_t dpre_bytes, const float* w_t, size_t w_bytes, const float* h, int64_t ldh,
                         size_t h_bytes, int32_t K, int32_t C, float* dy, int64_t ldd, size_t dy_bytes,
                         float* dpre_prev, int64_t ldq, size_t q_bytes, void* ws, size_t ws_bytes, void* stream,
                         int64_t* launches) {
  const char* fn = "mp_arma_step_bwd_f32";
  if (int rc = arma_shape(fn, K, C)) return rc;
  const int P = arma_width(K, C);
  if (int rc = arma_graph(fn, g, lap, lap_bytes, P, ws, ws_bytes)) return rc;
  MP_CHECK_ARG((w_t != nullptr) == (dpre_prev != nullptr), "%s: w_t and dpre_prev come together", fn);
  MP_CHECK_ARG(h == nullptr || w_t != nullptr, "%s: h (the mask source) needs w_t and dpre_prev", fn);
  if (int rc = arma_rows(fn, "dpre", dpre, ldp, dpre_bytes, g->n_cols, P)) return rc;
  if (int rc = arma_rows(fn, "dy", dy, ldd, dy_bytes, g->n_rows, P)) return rc;
  if (int rc = arma_rows(fn, "h", h, ldh, h_bytes, g->n_rows, P, false)) return rc;
  if (int rc = arma_rows(fn, "dpre_prev", dpre_prev, ldq, q_bytes, g->n_rows, P, false)) return rc;
  if (w_t) MP_CHECK_EXTENT(fn, "w_t", w_bytes, (size_t)K * C * C * sizeof(float));
  if (g->n_rows == 0) return MP_OK;
  AggArgs a{};
  fill_graph(a, g);
  a.F = P;
  a.w = lap;
  a.x = dpre;
  a.ldx = ldp;
  const ArmaArgs q{h, ldh, w_t, dy, ldd, dpre_prev, ldq, nullptr, 0, K, C, 0};
  return arma_run<true>(g, a, q, ws, stream, launches);
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_arma_ok(int32_t K, int32_t C) { return arma_shape("mp_arma_ok", K, C) == MP_OK ? 1 : 0; }

extern "C" int64_t mp_arma_width(int32_t K, int32_t C) {
  return arma_shape("mp_arma_width", K, C) == MP_OK ? arma_width(K, C) : -(int64_t)MP_ERR_ARG;
}

extern "C" size_t mp_arma_workspace(const mp_csr* g, int32_t K, int32_t C) {
  if (g == nullptr || g->n_waves < 1 || arma_shape("mp_arma_workspace", K, C) != MP_OK)
    return ArmaWs(nullptr, 0, 4).total(0);
  return ArmaWs(nullptr, g->n_waves, arma_width(K, C)).total(0);
}

extern "C" int64_t mp_arma_step_f32(const mp_csr* g, const float* lap, size_t lap_bytes, const float* y, int64_t ldy,
                                    size_t y_bytes, const float* s, int64_t lds, size_t s_bytes, const float* w_next,
                                    size_t w_bytes, int32_t K, int32_t C, int32_t relu, float* h_out, int64_t ldh,
                                    size_t h_bytes, float* y_next, int64_t ldn, size_t n_bytes, float* out,
                                    int64_t ldo, size_t out_bytes, void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = arma_step(g, lap, lap_bytes, y, ldy, y_bytes, s, lds, s_bytes, w_next, w_bytes, K, C, relu, h_out,
                           ldh, h_bytes, y_next, ldn, n_bytes, out, ldo, out_bytes, ws, ws_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_arma_step_bwd_f32(const mp_csr* g, const float* lap, size_t lap_bytes, const float* dpre,
                                        int64_t ldp, size_t dpre_bytes, const float* w_t, size_t w_bytes,
                                        const float* h, int64_t ldh, size_t h_bytes, int32_t K, int32_t C, float* dy,
                                        int64_t ldd, size_t dy_bytes, float* dpre_prev, int64_t ldq, size_t q_bytes,
                                        void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = arma_step_bwd(g, lap, lap_bytes, dpre, ldp, dpre_bytes, w_t, w_bytes, h, ldh, h_bytes, K, C, dy, ldd,
                               dy_bytes, dpre_prev, ldq, q_bytes, ws, ws_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}
