// GatedGraphConv's GRU cell (gfx950): both gate GEMMs and the whole gate chain in one
// f32 MFMA kernel, and the elementwise half of its backward.
//
// PyG nn.conv.GatedGraphConv (Li et al., Gated Graph Sequence Neural Networks), one
// recurrent step: m = A (h W_l), h' = GRUCell(m, h).  Sum and mean aggregation are
// linear, so W_l folds into the input weight, Wc = W_l W_ih^T [C, 3C], and with
// a = A h (the engine's aggregation) and Wh = W_hh^T [C, 3C] the step is
//   r  = sigmoid(a Wc_r + h Wh_r + b_r)          b_r = b_ir + b_hr
//   z  = sigmoid(a Wc_z + h Wh_z + b_z)          b_z = b_iz + b_hz
//   hn =         h Wh_n + b_hn
//   n  = tanh(a Wc_n + b_in + r * hn)
//   h' = (1 - z) * n + z * h
// torch.nn.GRUCell runs two [N, C] x [C, 3C] GEMMs that write and re-read two [N, 3C]
// gate arrays, then an elementwise chain; here no gate value reaches LDS or HBM
// unless the backward asks for it.
//
// Layout.  State rows are P = C rounded up to 16 floats wide (mp_gru_width).  The
// padding columns of every output are written as zeros, those of the inputs are
// masked to zero when a tile is staged, whatever they hold.
//
// Instruction and split.  v_mfma_f32_16x16x4_f32.  A workgroup owns a slice of up to
// four 16-column blocks (one wave each) and walks 64-row tiles of [a | h]
// persistently (32-row tiles at P > 64: with 64 rows the K = 256 kernels spilled); P > 64 puts a second slice on gridDim.y, which stages the same
// tiles again.  A wave keeps, for its 16 columns, four accumulators per 16 x 16
// tile -- r and z over the concatenated K = 2P of [a | h], a Wc_n and h Wh_n apart,
// because r multiplies only the latter -- so the epilogue runs on its own registers.
//
// B operand.  Six register arrays of P / 4 floats per lane ({r, z, n} x {a part, h
// part}), loaded once from the packed image mp_gru_pack_f32 builds and kept across
// tiles.  MFMA step s = 4 g + j of a part reads, in lane quarter q, the physical
// k = 16 g + 4 q + j: any assignment of k to (step, quarter) is a valid product as
// long as A and B agree, and this one makes a lane's four A values of a group
// the 16 contiguous bytes at k = 16 g + 4 q -- the LDS image is the plain row.
// Image: [block][chunk v][lane][4 floats], chunk v = array * (P / 16) + g, so a
// wave's load of one chunk is 1 KiB contiguous and a lane's is one f32x4; then
// [P][4] floats of (b_r, b_z, b_in, b_hn) per column.  Zero where k or the column
// is >= C.
//
// LDS.  Two buffers of 64 (32) rows x (2 P + 4) floats.  The A fragment is one
// ds_read_b128 per lane at row * (2 P + 4) + 16 g + 4 q: the 16 lanes of a quarter
// differ in the row alone, and the row stride is 4 mod 64 banks, so a quarter's 16
// reads cover the 64 banks once.  The next tile is loaded one or a few f32x4 per
// thread per group and written to the other buffer one group later, under the
// MFMAs; one workgroup barrier per tile.  Rows past N are clamped on load and never
// stored.
//
// fp32, fixed summation order (the k order above, bias first), no atomics: two
// calls give the same bits.
#include <math.h>

#include "mp_common.h"

namespace mp {

constexpr int kGruMaxC = 128;

static inline int gru_width(int C) { return (C + 15) & ~15; }
static inline size_t gru_pack_floats(int P) { return (size_t)6 * P * P + (size_t)4 * P; }

// ---- the weight image ------------------------------------------------------
// wc / wh: [C, 3C] under (row, column) strides in floats, so W_hh^T is passed as a
// view of W_hh.  One thread per float of the image.
__global__ __launch_bounds__(256) void k_gru_pack(const float* __restrict__ wc, int64_t wc_rs, int64_t wc_cs,
                                                  const float* __restrict__ wh, int64_t wh_rs, int64_t wh_cs,
                                                  const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                  int C, int P, float* __restrict__ pack) {
  const int nkb = P / 16;
  const int n_w = 6 * P * P;
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx < n_w) {
    const int e = idx & 3, lane = (idx >> 2) & 63;
    const int v = (idx >> 8) % (6 * nkb), cb = (idx >> 8) / (6 * nkb);
    const int arr = v / nkb, g = v % nkb;
    const int k = 16 * g + 4 * (lane >> 4) + e;
    const int n = 16 * cb + (lane & 15);
    const int gate = arr % 3;  // r, z, n
    float val = 0.f;
    if (k < C && n < C)
      val = arr < 3 ? wc[k * wc_rs + (int64_t)(gate * C + n) * wc_cs] : wh[k * wh_rs + (int64_t)(gate * C + n) * wh_cs];
    pack[idx] = val;
  } else if (idx < n_w + 4 * P) {
    const int t = idx - n_w;
    const int n = t >> 2, which = t & 3;  // b_r, b_z, b_in, b_hn
    float val = 0.f;
    if (n < C) {
      const float bi = b_ih ? b_ih[(which < 2 ? which : 2) * C + n] : 0.f;
      const float bh = b_hh ? b_hh[(which < 2 ? which : 2) * C + n] : 0.f;
      val = which < 2 ? __fadd_rn(bi, bh) : (which == 2 ? bi : bh);
    }
    pack[idx] = val;
  }
}

// ---- the forward cell -------------------------------------------------------
__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int P>
struct GruShape {
  static constexpr int kNkb = P / 16;                    // 16-wide k groups per part, and column blocks
  static constexpr int kWaves = kNkb < 4 ? kNkb : 4;     // per workgroup
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kBM = P > 64 ? 32 : 64;           // rows per tile: 32 keeps K = 256 clear of spills
  static constexpr int kSub = kBM / 16;                  // 16-row MFMA tiles of one row tile
  static constexpr int kRS = 2 * P + 4;                  // LDS row stride in floats
  static constexpr int kRowF4 = 2 * P / 4;               // f32x4 of one [a | h] row
  static constexpr int kTileF4 = kBM * kRowF4 / kThreads;     // f32x4 a thread stages per tile (8, or kNkb)
  static constexpr int kGroups = 2 * kNkb;               // k groups of one tile
  static constexpr int kPer = (kTileF4 + kGroups - 1) / kGroups;  // staged per group
  static constexpr size_t kLdsBytes = (size_t)2 * kBM * kRS * sizeof(float);
  // the kernel is budgeted for one wave per SIMD (the B operand alone is up to 192 registers):
  // a CU takes as many workgroups as it has SIMDs for their waves
  static constexpr int kPerCu = 4 / kWaves;
};

template <int P, bool GATES>
__global__ __launch_bounds__(GruShape<P>::kThreads) void k_gru_cell(
    const float* __restrict__ a, int64_t lda, const float* __restrict__ h, int64_t ldh, int64_t N, int C,
    const float* __restrict__ pack, float* __restrict__ out, int64_t ldo, float* __restrict__ gates, int64_t ldg) {
  using S = GruShape<P>;
  constexpr int NKB = S::kNkb, T = S::kThreads, RS = S::kRS, BM = S::kBM, SUB = S::kSub;
  __shared__ __attribute__((aligned(16))) float lds[2][BM * RS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int q = lane >> 4, j16 = lane & 15;
  const int cb = (int)blockIdx.y * 4 + (tid >> 6);  // this wave's column block
  const bool live = cb < NKB;                        // the second slice may hold fewer than 4 blocks
  const int col = 16 * cb + j16;
  const int64_t n_tiles = (N + BM - 1) / BM;

  // B operand: breg[arr][4 g + j], arr = {a: r, z, n; h: r, z, n}
  f32x4 breg[6][NKB];
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const f32x4* img = reinterpret_cast<const f32x4*>(pack) + (size_t)cb * (6 * NKB) * 64 + lane;
#pragma unroll
    for (int arr = 0; arr < 6; ++arr)
#pragma unroll
      for (int g = 0; g < NKB; ++g) breg[arr][g] = img[(arr * NKB + g) * 64];
    bias = *reinterpret_cast<const f32x4*>(pack + 6 * P * P + 4 * col);
  } else {
#pragma unroll
    for (int arr = 0; arr < 6; ++arr)
#pragma unroll
      for (int g = 0; g < NKB; ++g) breg[arr][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // retire the B loads before the tile loop (k_gemm_n256 explains why)
  __builtin_amdgcn_s_waitcnt(0);

  // staging: f32x4 number e = i * T + tid of the tile is (row e / kRowF4, column 4 (e % kRowF4)) of [a | h];
  // columns >= C become zeros, rows past N the last row
  f32x4 pre[S::kPer];
  auto load = [&](int64_t tile, int i0) {
#pragma unroll
    for (int u = 0; u < S::kPer; ++u) {
      const int i = i0 + u;
      if (i < S::kTileF4) {
        const int e = i * T + tid;
        const int r = e / S::kRowF4, c4 = e % S::kRowF4;
        int64_t row = tile * BM + r;
        row = row < N ? row : N - 1;
        const bool is_h = c4 >= P / 4;
        const int c = 4 * (is_h ? c4 - P / 4 : c4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c < C) v = *reinterpret_cast<const f32x4*>((is_h ? h + row * ldh : a + row * lda) + c);
        if (c + 1 >= C) v.y = 0.f;
        if (c + 2 >= C) v.z = 0.f;
        if (c + 3 >= C) v.w = 0.f;
        pre[u] = v;
      }
    }
  };
  auto stash = [&](float* buf, int i0) {
#pragma unroll
    for (int u = 0; u < S::kPer; ++u) {
      const int i = i0 + u;
      if (i < S::kTileF4) {
        const int e = i * T + tid;
        const int r = e / S::kRowF4, c4 = e % S::kRowF4;
        *reinterpret_cast<f32x4*>(buf + r * RS + 4 * c4) = pre[u];
      }
    }
  };

  int64_t tile = blockIdx.x;
  int cur = 0;
  if (tile < n_tiles) {
#pragma unroll
    for (int i0 = 0; i0 < S::kTileF4; i0 += S::kPer) {
      load(tile, i0);
      stash(lds[0], i0);
    }
  }
  __syncthreads();

  for (; tile < n_tiles; tile += gridDim.x) {
    const int64_t next = tile + gridDim.x;
    const bool more = next < n_tiles;
    const float* img = lds[cur];
    float* other = lds[cur ^ 1];
    f32x4 acc_r[SUB], acc_z[SUB], acc_n[SUB], acc_hn[SUB];
#pragma unroll
    for (int m = 0; m < SUB; ++m) {
      acc_r[m] = f32x4{bias.x, bias.x, bias.x, bias.x};
      acc_z[m] = f32x4{bias.y, bias.y, bias.y, bias.y};
      acc_n[m] = f32x4{bias.z, bias.z, bias.z, bias.z};
      acc_hn[m] = f32x4{bias.w, bias.w, bias.w, bias.w};
    }
    const float* ap = img + j16 * RS + 4 * q;
#pragma unroll
    for (int gg = 0; gg < S::kGroups; ++gg) {
      // the next tile: what group gg - 1 loaded goes to the other buffer, then this group's share is loaded
      if (more) {
        if (gg > 0) stash(other, (gg - 1) * S::kPer);
        load(next, gg * S::kPer);
      }
      const bool hp = gg >= NKB;  // the h part
      const int g = hp ? gg - NKB : gg;
      if (!live) continue;  // a wave past the last column block only stages
#pragma unroll
      for (int m = 0; m < SUB; ++m) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 16 * m * RS + 16 * gg);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc_r[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], breg[hp ? 3 : 0][g][j], acc_r[m], 0, 0, 0);
          acc_z[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], breg[hp ? 4 : 1][g][j], acc_z[m], 0, 0, 0);
          if (hp)
            acc_hn[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], breg[5][g][j], acc_hn[m], 0, 0, 0);
          else
            acc_n[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], breg[2][g][j], acc_n[m], 0, 0, 0);
        }
        // keep the unrolled loop's LDS reads where they are written (hoisted, they cost hundreds of registers)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) stash(other, (S::kGroups - 1) * S::kPer);

    // C/D map of the 16x16 f32 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
    if (live) {
      const bool pad = col >= C;
#pragma unroll
      for (int m = 0; m < SUB; ++m) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int rl = 16 * m + 4 * q + r4;
          const int64_t row = tile * BM + rl;
          if (row < N) {
            const float hv = img[rl * RS + P + col];
            const float r = gru_sigmoid(acc_r[m][r4]);
            const float z = gru_sigmoid(acc_z[m][r4]);
            const float hn = acc_hn[m][r4];
            const float n = tanhf(__fmaf_rn(r, hn, acc_n[m][r4]));
            const float o = __fmaf_rn(z, hv, __fmul_rn(1.f - z, n));
            out[row * ldo + col] = pad ? 0.f : o;
            if constexpr (GATES) {
              float* gp = gates + row * ldg + col;
              gp[0] = pad ? 0.f : n;
              gp[P] = pad ? 0.f : r;
              gp[2 * P] = pad ? 0.f : z;
              gp[3 * P] = pad ? 0.f : hn;
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// ---- the backward cell: one elementwise pass ---------------------------------
// dG = [dn_pre | dr_pre | dz_pre | dhn_pre] and dh_dir = dh' * z, one f32x4 of one row per thread
__global__ __launch_bounds__(256) void k_gru_cell_bwd(const float* __restrict__ dh, int64_t ldd,
                                                      const float* __restrict__ h, int64_t ldh,
                                                      const float* __restrict__ gates, int64_t ldg, int64_t N, int C,
                                                      int P, float* __restrict__ dG, int64_t ldq,
                                                      float* __restrict__ dir, int64_t ldr) {
  const int p4 = P / 4;
  const int64_t total = N * p4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / p4;
    const int c = 4 * (int)(i % p4);
    f32x4 o_n = {0.f, 0.f, 0.f, 0.f}, o_r = o_n, o_z = o_n, o_hn = o_n, o_d = o_n;
    if (c < C) {
      const float* gp = gates + row * ldg + c;
      const f32x4 g = *reinterpret_cast<const f32x4*>(dh + row * ldd + c);
      const f32x4 hv = *reinterpret_cast<const f32x4*>(h + row * ldh + c);
      const f32x4 n = *reinterpret_cast<const f32x4*>(gp);
      const f32x4 r = *reinterpret_cast<const f32x4*>(gp + P);
      const f32x4 z = *reinterpret_cast<const f32x4*>(gp + 2 * P);
      const f32x4 hn = *reinterpret_cast<const f32x4*>(gp + 3 * P);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c + k < C) {
          const float dn = g[k] * (1.f - z[k]) * (1.f - n[k] * n[k]);
          o_n[k] = dn;
          o_r[k] = dn * hn[k] * (r[k] * (1.f - r[k]));
          o_z[k] = g[k] * (hv[k] - n[k]) * (z[k] * (1.f - z[k]));
          o_hn[k] = dn * r[k];
          o_d[k] = g[k] * z[k];
        }
      }
    }
    float* qp = dG + row * ldq + c;
    *reinterpret_cast<f32x4*>(qp) = o_n;
    *reinterpret_cast<f32x4*>(qp + P) = o_r;
    *reinterpret_cast<f32x4*>(qp + 2 * P) = o_z;
    *reinterpret_cast<f32x4*>(qp + 3 * P) = o_hn;
    *reinterpret_cast<f32x4*>(dir + row * ldr + c) = o_d;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int gru_shape(const char* fn, int32_t C) {
  MP_CHECK_ARG(C >= 1, "%s: C = %d < 1", fn, C);
  MP_CHECK_ARG(C <= kGruMaxC, "%s: C = %d above the limit C <= %d", fn, C, kGruMaxC);
  return MP_OK;
}

// one operand [n, width] under its row stride; required = false lets it be absent
static int gru_rows(const char* fn, const char* name, const void* p, int64_t ld, size_t bytes, int64_t n, int width,
                    bool required = true) {
  if (p == nullptr && !required) return MP_OK;
  MP_CHECK_ARG(p != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_ARG(ld >= width, "%s: ld of %s = %lld < %d", fn, name, (long long)ld, width);
  MP_CHECK_ARG(ld % 4 == 0 && (uintptr_t)p % 16 == 0, "%s: %s must be 16-byte aligned with ld a multiple of 4", fn,
               name);
  MP_CHECK_EXTENT(fn, name, bytes, n <= 0 ? 0 : ((size_t)(n - 1) * ld + width) * sizeof(float));
  return MP_OK;
}

// a [C, 3C] matrix under (row, column) strides
static int gru_matrix(const char* fn, const char* name, const float* w, int64_t rs, int64_t cs, size_t bytes, int C) {
  MP_CHECK_ARG(w != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_ARG(rs >= 1 && cs >= 1, "%s: strides of %s must be >= 1 (got %lld, %lld)", fn, name, (long long)rs,
               (long long)cs);
  MP_CHECK_EXTENT(fn, name, bytes, ((size_t)(C - 1) * rs + (size_t)(3 * C - 1) * cs + 1) * sizeof(float));
  return MP_OK;
}

static int gru_pack(const float* wc, int64_t wc_rs, int64_t wc_cs, size_t wc_bytes, const float* wh, int64_t wh_rs,
                    int64_t wh_cs, size_t wh_bytes, const float* b_ih, size_t bi_bytes, const float* b_hh,
                    size_t bh_bytes, int32_t C, float* pack, size_t pack_bytes, void* stream) {
  const char* fn = "mp_gru_pack_f32";
  if (int rc = gru_shape(fn, C)) return rc;
  const int P = gru_width(C);
  if (int rc = gru_matrix(fn, "wc", wc, wc_rs, wc_cs, wc_bytes, C)) return rc;
  if (int rc = gru_matrix(fn, "wh", wh, wh_rs, wh_cs, wh_bytes, C)) return rc;
  if (b_ih) MP_CHECK_EXTENT(fn, "b_ih", bi_bytes, (size_t)3 * C * sizeof(float));
  if (b_hh) MP_CHECK_EXTENT(fn, "b_hh", bh_bytes, (size_t)3 * C * sizeof(float));
  MP_CHECK_ARG(pack != nullptr && (uintptr_t)pack % 16 == 0, "%s: pack is NULL or not 16-byte aligned", fn);
  MP_CHECK_EXTENT(fn, "pack", pack_bytes, gru_pack_floats(P) * sizeof(float));
  MP_DEVICE_GUARD(stream);
  const unsigned grid = (unsigned)ceil_div((int64_t)gru_pack_floats(P), 256);
  k_gru_pack<<<grid, 256, 0, as_stream(stream)>>>(wc, wc_rs, wc_cs, wh, wh_rs, wh_cs, b_ih, b_hh, C, P, pack);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int gru_cus() {
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    n_cu = n > 0 ? n : 256;
  }
  return n_cu;
}

template <int P>
static void gru_launch(const float* a, int64_t lda, const float* h, int64_t ldh, int64_t N, int C, const float* pack,
                       float* out, int64_t ldo, float* gates, int64_t ldg, void* stream) {
  using S = GruShape<P>;
  const int64_t n_tiles = ceil_div(N, S::kBM);
  static_assert(S::kPerCu * S::kLdsBytes <= 160 * 1024, "the CU's LDS holds kPerCu workgroups");
  const int64_t cap = (int64_t)gru_cus() * S::kPerCu;
  const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap), S::kNkb > 4 ? 2 : 1);
  if (gates)
    k_gru_cell<P, true><<<grid, S::kThreads, 0, as_stream(stream)>>>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg);
  else
    k_gru_cell<P, false><<<grid, S::kThreads, 0, as_stream(stream)>>>(a, lda, h, ldh, N, C, pack, out, ldo, nullptr,
                                                                      0);
}

static int gru_cell(const float* a, int64_t lda, size_t a_bytes, const float* h, int64_t ldh, size_t h_bytes,
                    int64_t N, int32_t C, const float* pack, size_t pack_bytes, float* out, int64_t ldo,
                    size_t out_bytes, float* gates, int64_t ldg, size_t g_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_gru_cell_f32";
  if (int rc = gru_shape(fn, C)) return rc;
  const int P = gru_width(C);
  MP_CHECK_ARG(N >= 0, "%s: N = %lld < 0", fn, (long long)N);
  if (int rc = gru_rows(fn, "a", a, lda, a_bytes, N, P)) return rc;
  if (int rc = gru_rows(fn, "h", h, ldh, h_bytes, N, P)) return rc;
  if (int rc = gru_rows(fn, "out", out, ldo, out_bytes, N, P)) return rc;
  if (int rc = gru_rows(fn, "gates", gates, ldg, g_bytes, N, 4 * P, false)) return rc;
  MP_CHECK_ARG(pack != nullptr && (uintptr_t)pack % 16 == 0, "%s: pack is NULL or not 16-byte aligned", fn);
  MP_CHECK_EXTENT(fn, "pack", pack_bytes, gru_pack_floats(P) * sizeof(float));
  MP_CHECK_ARG(out != a && out != h, "%s: out must not alias a or h (tiles are re-read by the second slice)", fn);
  if (N == 0) return MP_OK;
  MP_DEVICE_GUARD(stream);
  switch (P / 16) {
    case 1: gru_launch<16>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 2: gru_launch<32>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 3: gru_launch<48>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 4: gru_launch<64>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 5: gru_launch<80>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 6: gru_launch<96>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    case 7: gru_launch<112>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
    default: gru_launch<128>(a, lda, h, ldh, N, C, pack, out, ldo, gates, ldg, stream); break;
  }
  MP_CHECK_LAUNCH();
  *launches = 1;
  return MP_OK;
}

static int gru_cell_bwd(const float* dh, int64_t ldd, size_t dh_bytes, const float* h, int64_t ldh, size_t h_bytes,
                        const float* gates, int64_t ldg, size_t g_bytes, int64_t N, int32_t C, float* dG, int64_t ldq,
                        size_t q_bytes, float* dir, int64_t ldr, size_t dir_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_gru_cell_bwd_f32";
  if (int rc = gru_shape(fn, C)) return rc;
  const int P = gru_width(C);
  MP_CHECK_ARG(N >= 0, "%s: N = %lld < 0", fn, (long long)N);
  if (int rc = gru_rows(fn, "dh", dh, ldd, dh_bytes, N, P)) return rc;
  if (int rc = gru_rows(fn, "h", h, ldh, h_bytes, N, P)) return rc;
  if (int rc = gru_rows(fn, "gates", gates, ldg, g_bytes, N, 4 * P)) return rc;
  if (int rc = gru_rows(fn, "dG", dG, ldq, q_bytes, N, 4 * P)) return rc;
  if (int rc = gru_rows(fn, "dh_dir", dir, ldr, dir_bytes, N, P)) return rc;
  if (N == 0) return MP_OK;
  MP_DEVICE_GUARD(stream);
  const int64_t blocks = ceil_div(N * (P / 4), 256);
  const int64_t cap = (int64_t)gru_cus() * 16;
  k_gru_cell_bwd<<<(unsigned)(blocks < cap ? blocks : cap), 256, 0, as_stream(stream)>>>(dh, ldd, h, ldh, gates, ldg, N,
                                                                                         C, P, dG, ldq, dir, ldr);
  MP_CHECK_LAUNCH();
  *launches = 1;
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_gru_ok(int32_t C) { return C >= 1 && C <= kGruMaxC ? 1 : 0; }

extern "C" int64_t mp_gru_width(int32_t C) {
  return gru_shape("mp_gru_width", C) == MP_OK ? gru_width(C) : -(int64_t)MP_ERR_ARG;
}

extern "C" size_t mp_gru_pack_bytes(int32_t C) {
  return C >= 1 && C <= kGruMaxC ? gru_pack_floats(gru_width(C)) * sizeof(float) : 0;
}

extern "C" int64_t mp_gru_pack_f32(const float* wc, int64_t wc_rs, int64_t wc_cs, size_t wc_bytes, const float* wh,
                                   int64_t wh_rs, int64_t wh_cs, size_t wh_bytes, const float* b_ih, size_t bi_bytes,
                                   const float* b_hh, size_t bh_bytes, int32_t C, float* pack, size_t pack_bytes,
                                   void* stream) {
  const int rc = gru_pack(wc, wc_rs, wc_cs, wc_bytes, wh, wh_rs, wh_cs, wh_bytes, b_ih, bi_bytes, b_hh, bh_bytes, C,
                          pack, pack_bytes, stream);
  return rc != MP_OK ? -(int64_t)rc : 1;
}

extern "C" int64_t mp_gru_cell_f32(const float* a, int64_t lda, size_t a_bytes, const float* h, int64_t ldh,
                                   size_t h_bytes, int64_t N, int32_t C, const float* pack, size_t pack_bytes,
                                   float* out, int64_t ldo, size_t out_bytes, float* gates, int64_t ldg,
                                   size_t g_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = gru_cell(a, lda, a_bytes, h, ldh, h_bytes, N, C, pack, pack_bytes, out, ldo, out_bytes, gates, ldg,
                          g_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}

extern "C" int64_t mp_gru_cell_bwd_f32(const float* dh, int64_t ldd, size_t dh_bytes, const float* h, int64_t ldh,
                                       size_t h_bytes, const float* gates, int64_t ldg, size_t g_bytes, int64_t N,
                                       int32_t C, float* dG, int64_t ldq, size_t q_bytes, float* dh_dir, int64_t ldr,
                                       size_t dir_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = gru_cell_bwd(dh, ldd, dh_bytes, h, ldh, h_bytes, gates, ldg, g_bytes, N, C, dG, ldq, q_bytes, dh_dir,
                              ldr, dir_bytes, stream, &launches);
  return rc != MP_OK ? -(int64_t)rc : launches;
}
