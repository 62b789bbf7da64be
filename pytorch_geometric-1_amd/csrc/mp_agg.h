// The merge-path aggregation engine (gfx950, MI355X), shared by the units that
// run a reducer through it: mp_aggregate.hip (sum / mean / max / min, per-head
// sums, two-pass GAT statistics), mp_gat_fwd.hip, mp_gat_bwd.hip, mp_gat_wide.hip.
//
// Fused gather -> message -> segment-reduce.  It replaces, for one
// MessagePassing.propagate() [U1]:
//   x_j = x.index_select(0, edge_index[j])             (ATen index_select, [E',F] in HBM)
//   msg = norm.view(-1,1) * x_j   (GCNConv.message)    (elementwise, [E',F] in HBM)
//   out = torch_scatter.scatter_{sum,mean,max,min}(msg, edge_index[i], 0, dim_size=N)
//   out = out + bias              (GCNConv.update)
// with one pass that reads each x_j row once and writes each output row once.
//
// Mapping to CDNA4:
//   * one wave (64 lanes) = one merge-path task: `chunk` work units where a unit
//     is either "gather one CSR slot" or "finish one row" (mp_csr.hip).  Every
//     wave therefore does the same amount of work whatever the in-degree
//     distribution (RMAT hubs have ~1e4-1e5 in-edges, most rows < 10).
//   * a lane owns VEC consecutive features (VEC=4: one dwordx4, a 256-feature
//     row is one 1 KiB coalesced wave load); gridDim.y tiles wider rows.
//   * the wave walks its slots in CSR order; col/weight/eid for 64 slots are
//     loaded once per 64 slots (one coalesced dword per lane, next window
//     prefetched) and broadcast with v_readlane -> the x-row address is a
//     scalar base + lane offset.  U x-row loads are in flight per wave.
//   * accumulation stays in VGPRs; a row is stored once (no atomics).  A row
//     whose slots cross a task boundary leaves partials in a slab; a small
//     fix-up kernel combines them in task order (deterministic).
//
// ---------------------------------------------------------------------------
// The reducer protocol.  k_agg_main<Red, VEC, U, L> and k_agg_fixup<Red, VEC>
// know a reducer only through what is listed here; a reducer derives from
// RedFlags (every flag false) and shadows the flags it sets.
//
// Flags (static constexpr bool), and what the engine does when one is set:
//   kW          the slot window loads w[slot]; consume() gets it (otherwise 1).
//   kEid        the slot window loads eid[slot]; consume() gets it (otherwise
//               0), consume_gatb() gets it as the slot's index into de, and it
//               is the dropout key when there is no drop_ids array.
//   kHW         consume() gets the per-head weight w[slot * H + red.h] instead.
//   kGat        a slot goes to consume_gat(p, v, a_src, keep_bits); a_src is
//               a_src[col * H + red.h], for 64-lane tasks staged per window in
//               LDS (kGatWin), or, with
//   kOwnAs      red.own_as(v), taken from the gathered row itself.
//   kNodeScores after a batch's loads are issued the engine calls
//               red.node_scores(p) while red.need_ad is set, and
//               red.flush_scores(p) before it saves an owned row's partial.
//   kGatB       a slot's pack[col * H + red.h] is gathered with its row and it
//               goes to consume_gatb(p, v, red.dot(v), pack, eid, keep_bits);
//               the fix-up calls red.row_terms(p, row) before finish(); 64-lane
//               tasks keep kU_Vec4 rows in flight whatever VEC.
//   kGatWide    the pack is gathered likewise and the slot goes to
//               consume_gatw(p, v, pack, keep_bits).
//   kDrop       the slot window hashes each slot's dropout keep bits (drop_bits
//               of drop_ids[slot], else of eid[slot] under kEid, else of the slot);
//               the consume_gat* calls get them, otherwise they get 0.
//   kStat       save() is told which lane writes the per-head statistics: the
//               one holding a head's first feature (f % C == 0; C must be set).
//   kTrain      64-lane VEC = 4 tasks keep Red::kUTrain rows in flight, not kU_Vec4.
//
// Members the engine uses (p: the launch's AggArgs; f: the lane's first
// feature; act: f < F -- an inactive lane runs everything but touches no memory):
//   Red(p, f, act)                  once per task (main) or block (fix-up)
//   int h                           the lane's head; indexes the per-head slabs and gathers
//   begin(p, row, owned, f, act)    before a row's first slot in this task; owned is
//                                   false for the continuation of an earlier task's row
//   consume(v, w, eid, 0.f) / consume_gat / consume_gatb / consume_gatw
//                                   once per slot, in CSR order
//   finish(p, row, n_slots, f, act, with_bias = true)
//                                   the row is complete: write it.  The fix-up calls it
//                                   on a reducer that never saw begin().
//   save(PRef, stat_writer)         the row continues in another task: store the state
//   struct Part; static load(PRef) -> Part; set(Part); merge(Part); part() -> Part
//                                   the fix-up rebuilds a split row from its partials
//                                   in task order: set() the first, merge() the rest.
//
// Part is the reducer's state as a trivially copyable value (it crosses the
// fix-up's LDS); save() writes, and load() reads, exactly that state through a
// PRef: v (VEC values at the lane's features), a (VEC arg ids), st (two floats
// per head), v2 / s2 (a second accumulator and its per-head sum).  A part the
// reducer does not use may be null: the launch carves only the slabs it needs.
// ---------------------------------------------------------------------------
#pragma once

#include <cmath>
#include <type_traits>

#include "mp_common.h"

// Kernel-shape constants the engine reads.  Every value below was chosen by an
// in-process A/B with bitwise-equal outputs; dispatch-level
// choices that tests and A/B runs switch at run time go through mp_tune.
namespace mp {
constexpr int kU_Vec4 = 8;      // x-row loads in flight per task (VEC=4, 64-lane tasks: GAT)
constexpr int kU_Vec2 = 16;     // x-row loads in flight per task (VEC=2: the flat kernel, 128-feature tiles)
constexpr int kU_Vec1 = 16;     // x-row loads in flight per task (VEC=1)
constexpr int kU_Narrow = 12;   // x-row loads in flight per task (VEC=4, tasks of < 64 lanes)
constexpr int kWideLanes = 32;  // lanes per task of k_agg_main for rows of >= 256 features (32 beats 64 by ~9%)
constexpr int kGatLanes = 64;   // lanes per GAT task for H*C >= 256
constexpr bool kNtOut = true;   // non-temporal output-row stores (A/B: -0.4%)
constexpr bool kNtIdx = true;   // non-temporal col/weight/eid stream loads (A/B: -0.3%)
constexpr bool kXcdTiles = true;  // feature tile = (block % 8) % tiles when tiles divide 8: each XCD's L2
                                  // holds one tile (A/B: -1.5%)

struct RedFlags {
  static constexpr bool kW = false;
  static constexpr bool kEid = false;
  static constexpr bool kHW = false;
  static constexpr bool kGat = false;
  static constexpr bool kOwnAs = false;
  static constexpr bool kNodeScores = false;
  static constexpr bool kGatB = false;
  static constexpr bool kGatWide = false;
  static constexpr bool kDrop = false;
  static constexpr bool kStat = false;
  static constexpr bool kTrain = false;
  static constexpr int kUTrain = kU_Vec4;  // read under kTrain only
};

template <int VEC>
__device__ __forceinline__ void store_out(float* p, const Frag<VEC>& f) {
  if constexpr (kNtOut) store_frag_nt<VEC>(p, f);
  else store_frag<VEC>(p, f);
}

template <class T>
__device__ __forceinline__ T ld_stream(const T* p) {
  if constexpr (kNtIdx) return __builtin_nontemporal_load(p);
  else return *p;
}

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;

struct AggArgs {
  // graph + schedule
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const int32_t* wave_row;
  const int32_t* wave_slot;
  const int32_t* split_waves;
  int64_t n_rows;
  int64_t n_edges;
  int64_t n_ids;     // edge-id space (empty max/min rows report this arg)
  int32_t chunk;
  int32_t n_waves;
  int32_t n_split;
  int32_t F;
  int32_t n_cols;
  uint32_t x_bytes;  // extent of x for the scalar-batch buffer path (0: not used)
  int32_t seq_tiles; // flat kernel: feature tiles one after another on all XCDs (no XCD-affine map)
  // features
  const float* w;
  const float* x;
  int64_t ldx;
  int32_t flags;
  const float* bias;
  float* out;
  int64_t ldo;
  int64_t* arg_out;
  // partial slabs: slot index s = 2*task + kind (kind 0 = continuation, 1 = head)
  float* slab_v;
  int32_t* slab_a;
  int64_t slab_ld;
  // GAT
  const float* a_src;
  const float* a_dst;
  float* a_src_out;   // GAT forward with in-kernel node scores (kNodeScores): written per owned row
  float* a_dst_out;
  int32_t H;
  int32_t C;
  float slope;
  float* row_stats;
  float* slab_s;
  const int32_t* slot_row;  // two-pass GAT: row owning each CSR slot
  // GAT backward (transposed CSR: rows = source nodes j, col = destination i)
  const float* y;     // xw, the row's own features (d alpha = <g_i, xw_j>)
  int64_t ldy;
  const f32x4* pack;  // [n_cols, H]  (a_dst, m, 1/den, rs) of the destination, rs = <g_i, agg_i>_h
  float* de;          // [n_edges, H] d score per slot (this CSR's slot order)
  float* ga;          // [n_rows, H]  d a_src = row sums of d score
  const float* ga_dst_in;  // [n_rows, H] d a_dst of each row (node-wise, training forward): the
                           // row's d xw also takes d a_dst (x) att_dst at its finish
  const float* att;   // [H, 2C]      (att_dst | att_src)
  // GAT training forward (kTrain): out2[r, f] = sum_k alpha leaky' xw (ld F),
  // row_s2[r, h] = sum_k alpha leaky', and their partial slabs
  float* out2;
  float* row_s2;
  float* agg_nb;  // pre-bias output (ld F), when the output carries the bias
  float* slab_v2;
  float* slab_s2;
  // GAT attention dropout (training: F.dropout on alpha, see drop_bits)
  uint64_t drop_seed;
  uint32_t drop_thr;
  float drop_scale;
  const int32_t* drop_ids;  // (ABI 7) the key of each slot of this CSR (an edge id), or NULL: the dst slot
  // tile-major operands (mp_aggregate_tiles_f32; 0 = row-major): feature f of
  // row r at x[(f / x_tw) * x_ts + r * x_tw + f % x_tw], likewise out with o_tw
  // / o_ts.  Widths are multiples of 64, so a flat-kernel block's 64-feature
  // tile lies inside one operand tile.
  int32_t x_tw;
  int32_t o_tw;
  int64_t x_ts;
  int64_t o_ts;
  // per-row bias flags (mp_aggregate_tiles_f32; NULL = every row): the bias is
  // added to row r only where bias_rows[r] != 0
  const int32_t* bias_rows;
};

// This block's view of tile-major operands: x_tile / ldx_tile / fx0 address
// feature f of row r at x_tile[r * ldx_tile + f - fx0]; out is rebased in place
// so that out + r * ldo + f addresses it (fb: the block's first feature).
__device__ __forceinline__ void tile_view(AggArgs& p, int fb, const float*& x_tile, int64_t& ldx_tile, int& fx0) {
  x_tile = p.x;
  ldx_tile = p.ldx;
  fx0 = 0;
  if (p.x_tw) {
    const int t = fb / p.x_tw;
    x_tile = p.x + (int64_t)t * p.x_ts;
    ldx_tile = p.x_tw;
    fx0 = t * p.x_tw;
  }
  if (p.o_tw) {
    const int t = fb / p.o_tw;
    p.out += (int64_t)t * (p.o_ts - p.o_tw);
    p.ldo = p.o_tw;
  }
}

// ---------------------------------------------------------------------------
// GAT attention dropout (GATConv training: `F.dropout(alpha, p)` after the
// softmax [U6]).  The keep bit of (k, h) -- k the edge's key, h the head -- is
// a counter-based hash of (seed, k * H + h) compared with p * 2^32, so the
// forward and the transposed backward evaluate the same mask without storing
// it; a kept alpha is scaled by 1 / (1 - p).  The key (ABI 7) comes from a
// per-slot array of each pass's CSR (drop_ids): the layer's edge id on one
// GPU, the GLOBAL edge id on a shard -- so a sharded layer draws the
// single-GPU mask; without the array it is the edge's destination-CSR slot.
// oracle/pyg_ref.py restates the hash.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t drop_mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t drop_hash(uint64_t seed, uint64_t idx) {
  const uint32_t a = drop_mix32((uint32_t)idx ^ (uint32_t)seed);
  return drop_mix32(a + 0x9E3779B9u * ((uint32_t)(idx >> 32) ^ (uint32_t)(seed >> 32)) + 0x632BE5ABu);
}
// keep bits of slot s, bit h for head h (H <= 32)
__device__ __forceinline__ uint32_t drop_bits(const AggArgs& p, int64_t s) {
  const uint64_t base = (uint64_t)s * (uint64_t)p.H;
  uint32_t b = 0;
  for (int h = 0; h < p.H; ++h) b |= (uint32_t)(drop_hash(p.drop_seed, base + (uint64_t)h) >= p.drop_thr) << h;
  return b;
}
__device__ __forceinline__ float drop_factor(const AggArgs& p, uint32_t bits, int h) {
  return ((bits >> h) & 1u) ? p.drop_scale : 0.f;
}

// ---------------------------------------------------------------------------
// Reducers: per-lane state for VEC features of one (partial) row.
//
// A partial (the state of a row cut at a task boundary) lives in a slab slot
// in HBM between the main kernel and the fix-up, and in LDS between the
// waves of one fix-up block.  PRef points at one lane's share of a partial:
//   v  : VEC values,  a : VEC arg ids (max/min),  st : (m, s) pair (GAT).
// Red::Part is the same state in registers, so a chain of partials can be
// loaded U at a time (U loads in flight) and merged in order.
// ---------------------------------------------------------------------------

struct PRef {
  float* v;
  int32_t* a;
  float* st;
  float* v2;  // GAT training forward: second accumulator, and its per-head sum
  float* s2;
};

// this lane's share of slab slot s (2*task + kind)
template <class Red>
__device__ __forceinline__ PRef slab_ref(const AggArgs& p, int64_t s, int f, const Red& red) {
  PRef r;
  r.v = p.slab_v + s * p.slab_ld + f;
  r.a = p.slab_a ? p.slab_a + s * p.slab_ld + f : nullptr;
  r.st = p.slab_s ? p.slab_s + (s * p.H + red.h) * 2 : nullptr;
  r.v2 = p.slab_v2 ? p.slab_v2 + s * p.slab_ld + f : nullptr;
  r.s2 = p.slab_s2 ? p.slab_s2 + s * p.H + red.h : nullptr;
  return r;
}

// ---------------------------------------------------------------------------
// Lane groups.  A wave runs G = 64/L independent merge-path tasks, one per
// group of L lanes (L = 64: one task per wave, every per-task value is
// wave-uniform and lives in SGPRs).  A group covers L*VEC features of a row;
// gridDim.y walks the feature tiles, which the dispatcher runs roughly one
// after another, so the gathered working set of a pass is L*VEC*4 bytes per
// row -- narrow tiles keep more hub rows resident in L2.
// ---------------------------------------------------------------------------
template <int L>
struct Grp {
  static constexpr int G = 64 / L;
  static __device__ __forceinline__ int bc(int v, int idx) {
    if constexpr (L == 64) return readlane(v, idx);
    else return __shfl(v, idx, L);
  }
  static __device__ __forceinline__ float bc(float v, int idx) {
    if constexpr (L == 64) return readlane(v, idx);
    else return __shfl(v, idx, L);
  }
  static __device__ __forceinline__ int un(int v) {
    if constexpr (L == 64) return uni(v);
    else return v;
  }
};

// ---------------------------------------------------------------------------
// Per-group slot window: col / weight / eid of L consecutive CSR slots held one
// per lane, the next L prefetched.  DR: the lane's slot's dropout keep bits,
// computed when its window becomes current (key: the eid channel when EID --
// the transposed backward's dst slot -- else the slot itself).
// ---------------------------------------------------------------------------
template <bool W, bool EID, int L, bool GW = false, bool DR = false>
struct SlotWin {
  int64_t base, limit;
  int col, col_n, eid, eid_n;
  int did = 0, did_n = 0;  // DR with drop_ids: the dropout key of each slot of the window
  float w, w_n;
  uint32_t dr = 0;
  // GAT (GW, 64-lane tasks, H a power of two <= 8): a_src rows of the current
  // window staged in the wave's LDS (one load per lane per window instead of
  // one gather per slot); the column window runs two windows ahead so the
  // next window's a_src loads are issued a window before they are needed.
  int col_nn;
  float asn[8];
  float* lds;
  bool gw;

  __device__ __forceinline__ void fetch(const AggArgs& p, int64_t b, int gl, int& c, float& wt, int& e) {
    int64_t k = b + gl;
    bool ok = k < limit;
    c = ok ? (p.col ? ld_stream(p.col + k) : (int)k) : 0;  // col == nullptr: identity (rows in slot order)
    if (W) wt = ok ? ld_stream(p.w + k) : 0.f;
    if (EID) e = ok ? ld_stream(p.eid + k) : 0;
  }
  // the dropout keys of a window's slots (drop_ids; loaded a window ahead, with its columns)
  __device__ __forceinline__ void fetch_did(const AggArgs& p, int64_t b, int gl, int& d) {
    if constexpr (DR) {
      const int64_t k = b + gl;
      d = (p.drop_ids && k < limit) ? ld_stream(p.drop_ids + k) : 0;
    }
  }
  __device__ __forceinline__ int64_t drop_key(const AggArgs& p, int gl) const {
    return p.drop_ids ? (int64_t)did : (EID ? (int64_t)eid : base + gl);
  }
  __device__ __forceinline__ void load_as(const AggArgs& p, int c) {
    const float* r = p.a_src + (int64_t)c * p.H;
    if (p.H == 8) {
      f32x4 a = *reinterpret_cast<const f32x4*>(r);
      f32x4 b = *reinterpret_cast<const f32x4*>(r + 4);
      asn[0] = a.x; asn[1] = a.y; asn[2] = a.z; asn[3] = a.w;
      asn[4] = b.x; asn[5] = b.y; asn[6] = b.z; asn[7] = b.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) asn[k] = k < p.H ? r[k] : 0.f;
    }
  }
  __device__ __forceinline__ void store_as(const AggArgs& p, int gl) {
    __builtin_amdgcn_wave_barrier();  // earlier reads of the previous window come first
    if (p.H == 8) {
      f32x4 a = {asn[0], asn[1], asn[2], asn[3]};
      f32x4 b = {asn[4], asn[5], asn[6], asn[7]};
      *reinterpret_cast<f32x4*>(lds + gl * 8) = a;
      *reinterpret_cast<f32x4*>(lds + gl * 8 + 4) = b;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < p.H) lds[gl * p.H + k] = asn[k];
    }
    __builtin_amdgcn_wave_barrier();  // LDS ops of one wave run in order: later reads see the stores
  }
  __device__ __forceinline__ void init(const AggArgs& p, int64_t b, int64_t lim, int gl, float* wave_lds = nullptr) {
    base = b;
    limit = lim;
    fetch(p, base, gl, col, w, eid);
    fetch(p, base + L, gl, col_n, w_n, eid_n);
    fetch_did(p, base, gl, did);
    fetch_did(p, base + L, gl, did_n);
    if constexpr (DR) dr = drop_bits(p, drop_key(p, gl));
    if constexpr (GW) {
      lds = wave_lds;
      gw = p.H <= 8 && (p.H & (p.H - 1)) == 0;
      if (gw) {
        float dw;
        int de;
        fetch(p, base + 2 * L, gl, col_nn, dw, de);
        load_as(p, col);
        store_as(p, gl);
        load_as(p, col_n);
      }
    }
  }
  __device__ __forceinline__ void ensure(const AggArgs& p, int64_t e, int gl) {
    if (e >= base + L) {  // slots are consumed in order, never skipping a window
      base += L;
      col = col_n;
      w = w_n;
      eid = eid_n;
      did = did_n;
      if constexpr (DR) dr = drop_bits(p, drop_key(p, gl));  // eid_n / did_n were loaded a window ago
      fetch_did(p, base + L, gl, did_n);
      if constexpr (GW) {
        if (gw) {
          col_n = col_nn;
          float dw;
          int de;
          fetch(p, base + 2 * L, gl, col_nn, dw, de);
          store_as(p, gl);      // asn holds the a_src rows of the new current window
          load_as(p, col_n);
          return;
        }
      }
      fetch(p, base + L, gl, col_n, w_n, eid_n);
    }
  }
  __device__ __forceinline__ float a_src_of(const AggArgs& p, int slot_in_win, int c, int h) const {
    if constexpr (GW) {
      if (gw) return lds[slot_in_win * p.H + h];
    }
    return p.a_src[(int64_t)c * p.H + h];
  }
};

// GAT forward: a_src of each 64-slot window staged in LDS (see SlotWin; 8.85 -> 8.66 ms, bitwise the same)
template <class Red, int L>
constexpr bool kGatWin = Red::kGat && !Red::kOwnAs && L == 64;

// Process CSR slots [s, t) of the current (partial) row.
// All U row loads are issued unconditionally (indices past the segment are
// clamped to its last slot, inactive lanes read feature 0) so no load sits
// under an exec mask; only the group-uniform consume loop is bounded by n.
// For L = 64 the row address is a uniform base (SGPR pair) + one shared
// 32-bit lane offset, so U rows cost U*VEC data VGPRs only.
template <class Red, int VEC, int U, int L>
__device__ __forceinline__ void run_slots(Red& red, const AggArgs& p,
                                          SlotWin<Red::kW, Red::kEid, L, kGatWin<Red, L>, Red::kDrop>& win,
                                          int64_t s, int64_t t, uint32_t foff, int gl) {
  using GR = Grp<L>;
  const char* xb = reinterpret_cast<const char*>(p.x);
  const int64_t ldxb = p.ldx * 4;
  int64_t e = s;
  while (e < t) {
    win.ensure(p, e, gl);
    const int off = (int)(e - win.base);
    int64_t rem = t - e;
    int n = L - off;
    if (rem < n) n = (int)rem;
    if (n > U) n = U;
    n = GR::un(n);
    Frag<VEC> v[U];
    float as[U];
    [[maybe_unused]] float hw[U];
    [[maybe_unused]] f32x4 pk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int uu = u < n ? u : n - 1;
      if constexpr (Red::kHW) hw[u] = p.w[(e + uu) * p.H + red.h];
      const int c = GR::bc(win.col, off + uu);
      v[u] = load_frag<VEC>(reinterpret_cast<const float*>(xb + (int64_t)c * ldxb + foff));
      if constexpr (Red::kGat && !Red::kOwnAs) as[u] = win.a_src_of(p, off + uu, c, red.h);
      if constexpr (Red::kGatB || Red::kGatWide) pk[u] = p.pack[(int64_t)c * p.H + red.h];
    }
    if constexpr (Red::kGatB) {
#pragma unroll
      for (int u = 0; u < U; ++u) as[u] = red.dot(v[u]);
    }
    if constexpr (Red::kNodeScores) {
      // the row's own scores, once, after this batch's loads are in flight
      if (red.need_ad) red.node_scores(p);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < n) {
        [[maybe_unused]] uint32_t db = 0;
        if constexpr (Red::kDrop) db = (uint32_t)GR::bc((int)win.dr, off + u);
        if constexpr (Red::kGat) {
          // own_as next to its consume: slot u waits only for its own row
          if constexpr (Red::kOwnAs) red.consume_gat(p, v[u], red.own_as(v[u]), db);
          else red.consume_gat(p, v[u], as[u], db);
        } else if constexpr (Red::kGatWide) {
          red.consume_gatw(p, v[u], pk[u], db);
        } else if constexpr (Red::kGatB) {
          red.consume_gatb(p, v[u], as[u], pk[u], GR::bc(win.eid, off + u), db);
        } else {
          const float wt = Red::kHW ? hw[u] : (Red::kW ? GR::bc(win.w, off + u) : 1.f);
          const int ei = Red::kEid ? GR::bc(win.eid, off + u) : 0;
          red.consume(v[u], wt, ei, 0.f);
        }
      }
    }
    e += n;
  }
}

template <class Red, int VEC, int U, int L>
__global__ __launch_bounds__(kBlock) void k_agg_main(AggArgs p) {
  using GR = Grp<L>;
  const int lane = lane_id();
  const int gl = lane & (L - 1);
  int bx = (int)blockIdx.x, tile = (int)blockIdx.y;
  if constexpr (kXcdTiles) {
    // blocks b and b+8 share an XCD (dispatch is round-robin over the 8 XCDs;
    // speed only): give every XCD one feature tile so its L2 holds only that
    // tile of the hot rows.  tiles = gridDim.y divides 8 (checked on the host).
    const int T = (int)gridDim.y;
    if (8 % T == 0) {  // the host pads the grid to a multiple of 8/T blocks per tile
      const int b = (int)(blockIdx.y * gridDim.x + blockIdx.x);
      const int xcd = b & 7;
      tile = xcd % T;
      bx = (b >> 3) * (8 / T) + xcd / T;
    }
  }
  const int wave = bx * kWavesPerBlock + (int)(threadIdx.x >> 6);
  const int w = GR::un(wave * GR::G + lane / L);  // this group's task
  if (w >= p.n_waves) return;
  const int f = tile * L * VEC + gl * VEC;
  const bool act = f < p.F;
  const uint32_t foff = (uint32_t)(act ? f : 0) * 4u;

  const int r_first = GR::un(p.wave_row[w]);
  const int r_last = GR::un(p.wave_row[w + 1]);
  const int64_t e_begin = GR::un(p.wave_slot[w]);
  const int64_t e_end = GR::un(p.wave_slot[w + 1]);

  Red red(p, f, act);
  SlotWin<Red::kW, Red::kEid, L, kGatWin<Red, L>, Red::kDrop> win;
  [[maybe_unused]] float* wave_lds = nullptr;
  if constexpr (kGatWin<Red, L>) {
    __shared__ float gat_as[kWavesPerBlock][64 * 8];
    wave_lds = gat_as[threadIdx.x >> 6];
  }
  win.init(p, e_begin, e_end, gl, wave_lds);

  // rowptr window: rp = rowptr[rbase + gl]
  int rbase = r_first;
  int rp = (rbase + gl <= p.n_rows) ? p.rowptr[rbase + gl] : 0;

  // continuation of the row owned by an earlier task
  {
    const int64_t ce = GR::bc(rp, 0);  // rowptr[r_first] (== n_edges when r_first == n_rows)
    if (e_begin < ce) {
      red.begin(p, r_first - 1, false, f, act);
      run_slots<Red, VEC, U, L>(red, p, win, e_begin, ce < e_end ? ce : e_end, foff, gl);
      if (act) red.save(slab_ref(p, 2 * (int64_t)w, f, red), Red::kStat && (f % p.C == 0));
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
    red.begin(p, r, true, f, act);
    if (re <= e_end) {
      run_slots<Red, VEC, U, L>(red, p, win, rs, re, foff, gl);
      red.finish(p, r, re - rs, f, act);
    } else {
      run_slots<Red, VEC, U, L>(red, p, win, rs, e_end, foff, gl);
      if constexpr (Red::kNodeScores) red.flush_scores(p);
      if (act) red.save(slab_ref(p, 2 * (int64_t)w + 1, f, red), Red::kStat && (f % p.C == 0));
    }
  }
}

// One 4-wave block per split row.  The row's partials form a chain in task
// order: item 0 = head slab of the owning task, item k = continuation slab of
// task owner+k.  Wave q reduces items [q*c, (q+1)*c) in order (U loads in
// flight), waves 1..3 hand their result to wave 0 through LDS, wave 0 merges
// them in wave order and finishes the row: a fixed order, so deterministic.
template <class Red, int VEC>
__global__ __launch_bounds__(kBlock) void k_agg_fixup(AggArgs p) {
  constexpr int U = 4;
  __shared__ typename Red::Part lds[kWavesPerBlock - 1][64];
  __shared__ int has[kWavesPerBlock];
  const int lane = lane_id();
  const int wid = uni((int)(threadIdx.x >> 6));
  const int i = (int)blockIdx.x;
  const int f = (int)blockIdx.y * 64 * VEC + lane * VEC;
  const bool act = f < p.F;
  const int fs = act ? f : 0;
  if (p.o_tw) {  // tile-major out (the host runs this fix-up 64 features wide then)
    const float* xt;
    int64_t ldt;
    int fx0;
    tile_view(p, (int)blockIdx.y * 64 * VEC, xt, ldt, fx0);
  }
  const int last = uni(p.split_waves[i]);
  const int r = uni(p.wave_row[last]) - 1;
  const int64_t rs = uni(p.rowptr[r]);
  const int64_t re = uni(p.rowptr[r + 1]);
  // owner = last task whose first owned row is <= r
  int lo = 0, hi = p.n_waves;  // wave_row[n_waves] = n_rows > r
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (p.wave_row[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  const int owner = uni(lo);
  const int L = last - owner + 1;
  const int c = (L + kWavesPerBlock - 1) / kWavesPerBlock;
  const int b0 = wid * c;
  const int b1 = min(L, b0 + c);
  Red red(p, f, act);
  auto item = [&](int k) {
    int64_t slot = k == 0 ? 2 * (int64_t)owner + 1 : 2 * (int64_t)(owner + k);
    return slab_ref(p, slot, fs, red);
  };
  const bool mine = b0 < b1;
  if (mine) {
    red.set(Red::load(item(b0)));
    for (int k = b0 + 1; k < b1; k += U) {
      typename Red::Part q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = Red::load(item(min(k + u, b1 - 1)));
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (k + u < b1) red.merge(q[u]);
    }
  }
  if (lane == 0) has[wid] = mine ? 1 : 0;
  if (wid > 0 && mine) lds[wid - 1][lane] = red.part();
  __syncthreads();
  if (wid != 0) return;
  for (int q = 1; q < kWavesPerBlock; ++q)
    if (has[q]) red.merge(lds[q - 1][lane]);
  if constexpr (Red::kGatB) red.row_terms(p, r);
  red.finish(p, r, re - rs, f, act, p.bias_rows == nullptr || p.bias_rows[r] != 0);
}

// ---------------------------------------------------------------------------
// host side.  Choosing and launching are separate: a unit names the kernels of
// one aggregation as a value (AggLaunch: the main kernel, its grid, the
// fix-up), and run() is the only function that launches one.  AggArgs holds
// what the kernels read and nothing else.
// ---------------------------------------------------------------------------

struct Shape {
  int vec, lanes;
};

static inline int next_pow2(int v) {
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}

// VEC = widest aligned per-lane vector; L = lanes per task: enough to cover
// the row (small F packs several tasks per wave), at most 64.
static inline Shape pick_shape(int F, int64_t ldx, const void* x, int64_t ldo, const void* out) {
  auto aligned = [](const void* ptr, int64_t ld, int v) {
    return ((uintptr_t)ptr % (4 * v) == 0) && (ld % v == 0);
  };
  int vec = 1;
  if (F % 4 == 0 && aligned(x, ldx, 4) && aligned(out, ldo, 4)) vec = 4;
  else if (F % 2 == 0 && F > 64 && aligned(x, ldx, 2) && aligned(out, ldo, 2)) vec = 2;
  int lanes = 64;
  if (vec == 4) {
    int need = next_pow2((F + 3) / 4);
    lanes = need < 4 ? 4 : (need > 64 ? 64 : need);
    if (F >= 256) lanes = kWideLanes;
  }
  return {vec, lanes};
}

// MP_TUNE_GAT_BWD_VEC of the one mp_tune table (mp_aggregate.hip)
int64_t tuned_gat_bwd_vec();

// x-row loads in flight per task of k_agg_main<Red, VEC, ., L>
template <class Red, int VEC, int L>
constexpr int kMainU =
    // the GAT backward holds a 16-B destination pack per slot in flight: U = 8 at every width
    (Red::kGatB && L == 64) ? kU_Vec4
    : VEC == 4 ? (L == 64 ? (Red::kTrain ? Red::kUTrain : kU_Vec4) : kU_Narrow)
               : (VEC == 2 ? kU_Vec2 : (L < kU_Vec1 ? L : kU_Vec1));  // VEC=1 groups < 16 lanes: GAT stats

// grid of a main-stage kernel with L-lane tasks and VEC features per lane
template <int VEC, int L>
static inline dim3 main_grid(const AggArgs& a) {
  const int ftiles = (int)ceil_div(a.F, L * VEC);
  int64_t nb = ceil_div(a.n_waves, kWavesPerBlock * (64 / L));
  if (kXcdTiles && 8 % ftiles == 0) nb = ceil_div(nb, 8 / ftiles) * (8 / ftiles);
  return dim3((unsigned)nb, (unsigned)ftiles);
}

// One aggregation's kernels, chosen on the host; nothing in it crosses to the device.
using AggKernel = void (*)(AggArgs);
struct AggLaunch {
  AggKernel main;
  dim3 main_grid;
  AggKernel fixup;       // combines the split rows' partials, after main
  unsigned fixup_tiles;  // grid.y of the fix-up; grid.x is a.n_split
};

// main and its grid, with the fix-up of reducer FixRed at FVEC features per lane
template <class FixRed, int FVEC>
static inline AggLaunch with_fixup(AggKernel main, dim3 grid, const AggArgs& a) {
  return {main, grid, k_agg_fixup<FixRed, FVEC>, (unsigned)ceil_div(a.F, 64 * FVEC)};
}

// k_agg_main with L-lane tasks, and the fix-up of its split rows
template <class Red, int VEC, int L>
static inline AggLaunch engine_launch(const AggArgs& a) {
  return with_fixup<Red, VEC>(k_agg_main<Red, VEC, kMainU<Red, VEC, L>, L>, main_grid<VEC, L>(a), a);
}

// The only place that launches: the stages asked for, the fix-up only when rows are split.
static inline int run(const AggLaunch& l, const AggArgs& a, int stages, hipStream_t s) {
  if (stages & MP_STAGE_MAIN) {
    hipLaunchKernelGGL(l.main, l.main_grid, dim3(kBlock), 0, s, a);
    MP_CHECK_LAUNCH();
  }
  if ((stages & MP_STAGE_FIXUP) && a.n_split > 0) {
    hipLaunchKernelGGL(l.fixup, dim3((unsigned)a.n_split, l.fixup_tiles), dim3(kBlock), 0, s, a);
    MP_CHECK_LAUNCH();
  }
  return MP_OK;
}

// fn(std::integral_constant<int, L>) for the task width `lanes` (VEC = 4: 4 .. 64, else 64)
template <int VEC, class Fn>
static inline auto with_lanes(int lanes, Fn&& fn) {
  if constexpr (VEC == 4) {
    switch (lanes) {
      case 4: return fn(std::integral_constant<int, 4>{});
      case 8: return fn(std::integral_constant<int, 8>{});
      case 16: return fn(std::integral_constant<int, 16>{});
      case 32: return fn(std::integral_constant<int, 32>{});
      default: break;
    }
  }
  return fn(std::integral_constant<int, 64>{});
}

// the engine's launch at the task width `lanes`, and that launch run
template <class Red, int VEC>
static inline AggLaunch engine_launch_at(int lanes, const AggArgs& a) {
  return with_lanes<VEC>(lanes, [&](auto l) { return engine_launch<Red, VEC, decltype(l)::value>(a); });
}
template <class Red, int VEC>
static inline int launch(const AggArgs& a, int stages, hipStream_t s, int lanes = 64) {
  return run(engine_launch_at<Red, VEC>(lanes, a), a, stages, s);
}

static inline int64_t slab_ld_for(int F) { return ceil_div(F, 256) * 256; }

// The partial slabs of one launch, carved from the caller's workspace in this
// order: v | a (max/min arg ids) or s (per-head statistics) | 256 spare bytes |
// v2 | s2 (the second accumulator and its per-head sum).  The *_slab_bytes
// entry points return `total`; the launches place their slabs at the offsets.
enum : unsigned { kSlabArg = 1, kSlabStat = 2, kSlabV2 = 4, kSlabS2 = 8 };
struct SlabLayout {
  size_t a, s, v2, s2, total;
};
static inline SlabLayout slab_layout(int32_t n_waves, int F, int H, unsigned parts) {
  const size_t slots = 2 * (size_t)n_waves;
  const size_t v = align_up(slots * (size_t)slab_ld_for(F) * 4, 256);
  SlabLayout l;
  size_t o = v;
  l.a = o;
  if (parts & kSlabArg) o += v;
  l.s = o;
  if (parts & kSlabStat) o += align_up(slots * (size_t)H * 2 * 4, 256);
  o += 256;
  l.v2 = o;
  if (parts & kSlabV2) o += v;
  l.s2 = o;
  if (parts & kSlabS2) o += align_up(slots * (size_t)H * 4, 256);
  l.total = o;
  return l;
}
// a.slab_ld and the slab pointers of the wanted parts (a.F, a.H and a.n_waves set)
static inline void carve_slabs(AggArgs& a, void* slab, unsigned parts) {
  const SlabLayout l = slab_layout(a.n_waves, a.F, a.H, parts);
  char* b = (char*)slab;
  a.slab_ld = slab_ld_for(a.F);
  a.slab_v = (float*)b;
  if (parts & kSlabArg) a.slab_a = (int32_t*)(b + l.a);
  if (parts & kSlabStat) a.slab_s = (float*)(b + l.s);
  if (parts & kSlabV2) a.slab_v2 = (float*)(b + l.v2);
  if (parts & kSlabS2) a.slab_s2 = (float*)(b + l.s2);
}

static inline int check_graph(const mp_csr* g, const char* who) {
  MP_CHECK_ARG(g != nullptr, "%s: null graph", who);
  MP_CHECK_ARG(g->rowptr && g->wave_row && g->wave_slot && (g->n_split == 0 || g->split_waves),
               "%s: graph has null arrays", who);
  MP_CHECK_ARG(g->n_edges == 0 || g->eid, "%s: graph has null eid", who);
  MP_CHECK_ARG(g->n_ids == 0 || (g->n_ids >= g->n_edges && g->n_ids <= INT32_MAX),
               "%s: n_ids must be 0 or in [n_edges, 2^31)", who);
  MP_CHECK_ARG(g->chunk >= 16 && g->chunk % 8 == 0 && g->n_waves >= 1, "%s: bad schedule", who);
  MP_CHECK_ARG(g->col == nullptr || g->n_edges == 0 || g->n_cols > 0,
               "%s: n_cols must be the row count of the gathered x (got %d with a column array)", who,
               (int)g->n_cols);
  return MP_OK;
}

static inline void fill_graph(AggArgs& a, const mp_csr* g) {
  a.rowptr = g->rowptr;
  a.col = g->col;
  a.eid = g->eid;
  a.wave_row = g->wave_row;
  a.wave_slot = g->wave_slot;
  a.split_waves = g->split_waves;
  a.n_rows = g->n_rows;
  a.n_edges = g->n_edges;
  a.n_ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  a.chunk = g->chunk;
  a.n_waves = g->n_waves;
  a.n_split = g->n_split;
  a.n_cols = g->n_cols;
}

// keep threshold p * 2^32 and scale 1 / (1 - p) (in double, then rounded: F.dropout's scale)
static inline void set_drop(AggArgs& a, uint64_t seed, float p_drop, const int32_t* drop_ids = nullptr) {
  const double t = std::floor((double)p_drop * 4294967296.0);
  a.drop_seed = seed;
  a.drop_ids = drop_ids;
  a.drop_thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  a.drop_scale = (float)(1.0 / (1.0 - (double)p_drop));
}

static inline int drop_check(float p_drop, int32_t H, const char* who) {
  MP_CHECK_ARG(p_drop > 0.f && p_drop < 1.f, "%s: dropout p must be in (0, 1) (got %g)", who, (double)p_drop);
  MP_CHECK_ARG(H >= 1 && H <= 32, "%s: attention dropout needs H <= 32 (got %d)", who, H);
  return MP_OK;
}

}  // namespace mp
