// Sparse x sparse product C = A B over row CSRs, per-row accumulators in LDS (gfx950).
//
// torch_sparse.spspmm's job (cusparse csrgemm upstream): the coalesced product, distinct
// (row, col) pairs in row-major order, fp32 values, an entry whose products cancel KEPT
// (the structure is symbolic).  A [m, k] and B [k, n] arrive as the stable row CSRs of
// mp_csr_build (rowptr, col, eid: a row's slots stay in input order; values are read in
// place through eid).  Unsorted inputs and duplicate entries are fine: a duplicate is one
// more product on the same output column.
//
// Two passes over the same binned rows, one kernel template:
//   count  ub_i = sum over A_i's slots of nnz(B_k), by a wave per row; rows are appended
//          to one of three lists by ub (an empty row goes nowhere and costs nothing); each
//          listed row's distinct columns are counted into rowptr_c[i + 1]; an inclusive
//          scan makes rowptr_c, and stats = { nnz(C), rows per bin } is the caller's one
//          host read, which sizes the output.
//   fill   the same walk with values; each row's columns come out sorted into
//          [rowptr_c[i], rowptr_c[i + 1]).
//
// Bins (mp_spgemm_bin_cap answers every limit):
//   wave       ub <= 256: one wave (a 64-thread workgroup) per row, a hash table of at
//              most 512 slots (keys, values, tags: 6 KB, so many rows per CU).
//   workgroup  ub <= 4096: 512 threads per row, one table of at most 8192 slots (96 KB of
//              the CU's 160 KB).
//   window     above: 1024 threads per row pass over column windows of 16384 columns with
//              a dense accumulator, its tags (64 KB each) and a presence bitmap (2 KB);
//              every pass re-walks the row's products and keeps those in the window.  No
//              hash table in global memory, nothing of size sum(ub).
// A table is the power of two >= 2 ub (at least 64) slots, the hash is col mod slots with
// linear probing, so a load of at most 1/2.  Only the used part is cleared and sorted.
//
// The walk.  A row's products are numbered in A-slot order, B-slot order within: BLOCK
// A slots at a time are loaded (one per thread: B_k's first slot, its length, A's value),
// their lengths scanned in LDS, and the products of the chunk taken BLOCK at a time;
// thread t of a batch finds its A slot by bisecting the scanned lengths.  So every lane
// of every batch is busy whatever the lengths of the B rows.
//
// Determinism.  Keys are claimed by integer compare-and-swap; where a key lands in the
// table depends on the race, the sorted output does not.  No float atomic exists: after a
// batch's threads know their slots, each pending thread puts its thread id into the
// slot's tag by an integer atomicMin; after a barrier the thread that reads its own id
// adds its product (a plain LDS read-add-write with __fadd_rn) and resets the tag; the
// rest go round again.  Products on one column are therefore added in thread order within
// a batch and in batch order across batches: ascending product number, which for
// coalesced inputs is ascending A-slot order.  Batches without a shared column, the usual
// case, take one round.  The dense windows use the same tags.
//
// Columns are sorted in LDS: a bitonic sort of the table's used slots (empty keys last)
// for the hash bins, the bitmap's bit order for the windows.  With MP_SPGEMM_DROP_DIAG a
// product on column == row is skipped by both passes (GraphUNet's augment_adj).  An index
// outside its range (csr_build counts those for the caller) contributes nothing.
#include <rocprim/device/device_scan.hpp>

#include "mp_workspace.h"

namespace mp {

constexpr int kSpWaveCap = 256, kSpWaveSlots = 512, kSpWaveBlock = 64;
constexpr int kSpWgCap = 4096, kSpWgSlots = 8192, kSpWgBlock = 512;
constexpr int kSpWindow = 16384, kSpWinBlock = 1024;
constexpr int kSpEmpty = 0x7fffffff;  // an empty key and an idle tag: above every column and thread id

struct SpP {
  const int32_t *rowptr_a, *col_a, *eid_a;
  const float* val_a;
  const int32_t *rowptr_b, *col_b, *eid_b;
  const float* val_b;
  int32_t m, k, n, drop;
  int64_t* rowptr_c;
  const int32_t* list;     // this bin's rows
  const int32_t* n_list;   // their number, on the device
  const int32_t* ub;       // per row, clamped to int32
  int64_t* out_row;
  int64_t* out_col;
  float* out_val;
  int64_t nnz_c;  // the extent of the three: nothing is written past it
};

template <int BLOCK, int SLOTS, bool DENSE, bool FILL, class P>
struct SpLds {
  P end[BLOCK];        // the chunk's scanned B-row lengths
  P wsum[16];
  int32_t isum[16];
  int32_t bs[BLOCK];   // B_k's first slot
  float av[BLOCK];     // A's value
  int32_t keys[DENSE ? SLOTS / 32 : SLOTS];  // hash keys, or the window's presence words
  float vals[FILL ? SLOTS : 1];
  int32_t tag[FILL ? SLOTS : 1];
  int32_t count;
};

// inclusive scan of v over the block's threads; sums: one entry per wave, free to overwrite
template <int BLOCK, class T>
__device__ __forceinline__ T sp_block_scan(T v, T* sums) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  if constexpr (BLOCK > 64) {
    const int wave = threadIdx.x >> 6;
    if (lane == 63) sums[wave] = v;
    __syncthreads();
    T add = 0;
    for (int w = 0; w < wave; ++w) add += sums[w];
    v += add;
  }
  return v;
}

// One pass over the products of A's slots [as, ae): those on a column the table takes (every column,
// or window [w0, w0 + SLOTS)) are inserted and, for FILL, added in product order.
template <int BLOCK, int SLOTS, bool DENSE, bool FILL, class P>
__device__ __forceinline__ void sp_walk(const SpP& p, SpLds<BLOCK, SLOTS, DENSE, FILL, P>& s, int row, int as, int ae,
                                        int mask, int w0) {
  const int tid = threadIdx.x;
  for (int c0 = as; c0 < ae; c0 += BLOCK) {
    __syncthreads();  // the chunk before is read out
    const int j = c0 + tid;
    int bs = 0, len = 0;
    float av = 0.f;
    if (j < ae) {
      const int kk = p.col_a[j];
      if ((unsigned)kk < (unsigned)p.k) {
        bs = p.rowptr_b[kk];
        len = p.rowptr_b[kk + 1] - bs;
      }
      if constexpr (FILL) av = p.val_a[p.eid_a[j]];
    }
    s.bs[tid] = bs;
    s.av[tid] = av;
    s.end[tid] = sp_block_scan<BLOCK, P>((P)len, s.wsum);
    __syncthreads();
    const P tot = s.end[BLOCK - 1];
    for (P p0 = 0; p0 < tot; p0 += BLOCK) {
      const P pp = p0 + tid;
      int h = -1;
      float v = 0.f;
      if (pp < tot) {
        int lo = 0, hi = BLOCK - 1;  // the first slot whose scanned end lies above pp
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s.end[mid] > pp) hi = mid;
          else lo = mid + 1;
        }
        const int slot = s.bs[lo] + (int)(pp - (lo ? s.end[lo - 1] : (P)0));
        const int col = p.col_b[slot];
        if ((unsigned)col < (unsigned)p.n && !(p.drop && col == row)) {
          if constexpr (DENSE) {
            if (col >= w0 && col - w0 < SLOTS) {
              h = col - w0;
              atomicOr((unsigned*)&s.keys[h >> 5], 1u << (h & 31));
            }
          } else {
            h = col & mask;
            for (;;) {
              const int old = atomicCAS(&s.keys[h], kSpEmpty, col);
              if (old == kSpEmpty) atomicAdd(&s.count, 1);
              if (old == kSpEmpty || old == col) break;
              h = (h + 1) & mask;
            }
          }
          if constexpr (FILL) {
            if (h >= 0) v = __fmul_rn(s.av[lo], p.val_b[p.eid_b[slot]]);
          }
        }
      }
      if constexpr (FILL) {
        bool pend = h >= 0;
        while (__syncthreads_or(pend)) {  // also: the tags reset by the round before are seen
          if (pend) atomicMin(&s.tag[h], tid);
          __syncthreads();
          if (pend && s.tag[h] == tid) {
            s.vals[h] = __fadd_rn(s.vals[h], v);
            s.tag[h] = kSpEmpty;
            pend = false;
          }
        }
      }
    }
  }
}

template <int BLOCK, int SLOTS, bool DENSE, bool FILL, class P>
__global__ __launch_bounds__(BLOCK) void k_spgemm_rows(SpP p) {
  static_assert(!DENSE || SLOTS / 32 <= BLOCK, "one presence word per thread");
  __shared__ SpLds<BLOCK, SLOTS, DENSE, FILL, P> s;
  const int tid = threadIdx.x;
  const int n_list = *p.n_list;
  for (int li = blockIdx.x; li < n_list; li += gridDim.x) {
    const int row = p.list[li];
    const int as = p.rowptr_a[row], ae = p.rowptr_a[row + 1];
    const int64_t obase = FILL ? p.rowptr_c[row] : 0;
    __syncthreads();  // the row before is written out
    if constexpr (DENSE) {
      for (int i = tid; i < SLOTS; i += BLOCK) {
        if (i < SLOTS / 32) s.keys[i] = 0;
        if constexpr (FILL) {
          s.vals[i] = 0.f;
          s.tag[i] = kSpEmpty;
        }
      }
      int64_t run = 0;  // the row's entries in the windows before
      for (int w0 = 0; w0 < p.n; w0 += SLOTS) {
        sp_walk<BLOCK, SLOTS, DENSE, FILL, P>(p, s, row, as, ae, 0, w0);
        __syncthreads();
        unsigned word = tid < SLOTS / 32 ? (unsigned)s.keys[tid] : 0u;
        const int pc = __popc(word);
        int at = sp_block_scan<BLOCK, int32_t>(pc, s.isum);
        if (tid == BLOCK - 1) s.count = at;
        at -= pc;
        if constexpr (FILL) {
          while (word) {  // ascending bits: ascending columns
            const int b = __ffs(word) - 1;
            word &= word - 1;
            const int idx = tid * 32 + b;
            const int64_t o = obase + run + at++;
            if (o < p.nnz_c) {
              p.out_row[o] = row;
              p.out_col[o] = (int64_t)w0 + idx;
              p.out_val[o] = s.vals[idx];
            }
            s.vals[idx] = 0.f;
          }
        }
        if (tid < SLOTS / 32) s.keys[tid] = 0;
        __syncthreads();
        run += s.count;
      }
      if (!FILL && tid == 0) p.rowptr_c[row + 1] = run;
    } else {
      int T = 64;
      while (T < 2 * p.ub[row]) T <<= 1;  // ub <= the bin's cap = SLOTS / 2
      for (int i = tid; i < T; i += BLOCK) {
        s.keys[i] = kSpEmpty;
        if constexpr (FILL) {
          s.vals[i] = 0.f;
          s.tag[i] = kSpEmpty;
        }
      }
      if (tid == 0) s.count = 0;
      sp_walk<BLOCK, SLOTS, DENSE, FILL, P>(p, s, row, as, ae, T - 1, 0);
      __syncthreads();
      if constexpr (FILL) {
        for (int k2 = 2; k2 <= T; k2 <<= 1) {
          for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < T; i += BLOCK) {
              const int x = i ^ j;
              if (x > i) {
                const int a = s.keys[i], b = s.keys[x];
                if ((a > b) == ((i & k2) == 0)) {
                  s.keys[i] = b;
                  s.keys[x] = a;
                  const float t = s.vals[i];
                  s.vals[i] = s.vals[x];
                  s.vals[x] = t;
                }
              }
            }
            __syncthreads();
          }
        }
        const int64_t left = p.nnz_c - obase;
        const int cnt = s.count < left ? s.count : (int)(left > 0 ? left : 0);
        for (int i = tid; i < cnt; i += BLOCK) {
          p.out_row[obase + i] = row;
          p.out_col[obase + i] = s.keys[i];
          p.out_val[obase + i] = s.vals[i];
        }
      } else if (tid == 0) {
        p.rowptr_c[row + 1] = s.count;
      }
    }
  }
}

// counters[0..2] = rows per bin
__global__ void k_spgemm_zero(int32_t* counters, int64_t* rowptr_c) {
  if (threadIdx.x < 4) counters[threadIdx.x] = 0;
  if (threadIdx.x == 0) rowptr_c[0] = 0;
}

// a wave per row: ub, the row's bin and list slot; an empty row's count
__global__ __launch_bounds__(256) void k_spgemm_ub(const int32_t* __restrict__ rowptr_a,
                                                   const int32_t* __restrict__ col_a,
                                                   const int32_t* __restrict__ rowptr_b, int32_t m, int32_t k,
                                                   int32_t* __restrict__ ub, int32_t* __restrict__ lists,
                                                   int32_t* __restrict__ counters, int64_t* __restrict__ rowptr_c) {
  const int64_t row = ((int64_t)blockIdx.x << 2) + (threadIdx.x >> 6);
  if (row >= m) return;
  long long t = 0;
  for (int j = rowptr_a[row] + lane_id(), e = rowptr_a[row + 1]; j < e; j += 64) {
    const int kk = col_a[j];
    if ((unsigned)kk < (unsigned)k) t += rowptr_b[kk + 1] - rowptr_b[kk];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
  if (lane_id() != 0) return;
  ub[row] = t > 0x7fffffffLL ? 0x7fffffff : (int32_t)t;
  if (t == 0) {
    rowptr_c[row + 1] = 0;
    return;
  }
  const int bin = t <= kSpWaveCap ? 0 : t <= kSpWgCap ? 1 : 2;
  lists[(int64_t)bin * m + atomicAdd(&counters[bin], 1)] = (int32_t)row;  // the order within a list decides nothing
}

__global__ void k_spgemm_stats(const int64_t* __restrict__ rowptr_c, int32_t m, const int32_t* __restrict__ counters,
                               int64_t* __restrict__ stats) {
  if (threadIdx.x == 0) stats[0] = rowptr_c[m];
  else if (threadIdx.x < 4) stats[threadIdx.x] = counters[threadIdx.x - 1];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The workspace of one product, filled by the count pass and read by the fill pass: every row's ub,
// the three bins' row lists and their lengths; the scan's temp follows.
struct SpgemmWs : Carver {
  int32_t* ub;
  int32_t* lists;
  int32_t* counters;
  SpgemmWs(void* ws, int64_t m) : Carver(ws), ub(take<int32_t>(m)), lists(take<int32_t>(3 * m)), counters(take<int32_t>(4)) {}
};

static hipError_t sp_scan_bytes(int64_t m, size_t* bytes) {
  return rocprim::inclusive_scan((void*)nullptr, *bytes, (int64_t*)nullptr, (int64_t*)nullptr, (size_t)(m > 0 ? m : 1),
                                 rocprim::plus<int64_t>(), (hipStream_t)0, false);
}

static int sp_array(const char* fn, const char* name, const void* ptr, size_t bytes, int64_t count, size_t elem) {
  MP_CHECK_ARG(ptr != nullptr || count == 0, "%s: %s is NULL", fn, name);
  MP_CHECK_EXTENT(fn, name, bytes, (size_t)count * elem);
  return MP_OK;
}

struct SpShape {
  int64_t m, k, n, nnz_a, nnz_b;
};

static int sp_shape(const char* fn, const SpShape& s, int32_t flags) {
  const int64_t v[5] = {s.m, s.k, s.n, s.nnz_a, s.nnz_b};
  const char* names[5] = {"m", "k", "n", "nnz_a", "nnz_b"};
  for (int i = 0; i < 5; ++i) {
    MP_CHECK_ARG(v[i] >= 0, "%s: %s = %lld < 0", fn, names[i], (long long)v[i]);
    MP_CHECK_ARG(v[i] < 0x7fffffffLL, "%s: %s = %lld above the int32 limit 2^31 - 2", fn, names[i], (long long)v[i]);
  }
  MP_CHECK_ARG((flags & ~MP_SPGEMM_DROP_DIAG) == 0, "%s: unknown flags %d", fn, flags);
  return MP_OK;
}

static int sp_csrs(const char* fn, const SpShape& s, const int32_t* rowptr_a, size_t rowptr_a_bytes, const int32_t* col_a,
                   size_t col_a_bytes, const int32_t* rowptr_b, size_t rowptr_b_bytes, const int32_t* col_b,
                   size_t col_b_bytes) {
  MP_CHECK_ARG(rowptr_a != nullptr, "%s: rowptr_a is NULL", fn);
  MP_CHECK_EXTENT(fn, "rowptr_a", rowptr_a_bytes, (size_t)(s.m + 1) * 4);
  if (int rc = sp_array(fn, "col_a", col_a, col_a_bytes, s.nnz_a, 4)) return rc;
  MP_CHECK_ARG(rowptr_b != nullptr, "%s: rowptr_b is NULL", fn);
  MP_CHECK_EXTENT(fn, "rowptr_b", rowptr_b_bytes, (size_t)(s.k + 1) * 4);
  return sp_array(fn, "col_b", col_b, col_b_bytes, s.nnz_b, 4);
}

static int sp_ws(const char* fn, int64_t m, void* ws, size_t ws_bytes, size_t* scan_bytes, hipError_t* query) {
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  *query = sp_scan_bytes(m, scan_bytes);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, SpgemmWs(nullptr, m).total(*scan_bytes));
  return MP_OK;
}

static inline unsigned sp_grid(int64_t m, int64_t cap) { return (unsigned)(m < cap ? m : cap); }

// the three bins' launches of one pass
template <bool FILL>
static int sp_launch_bins(SpP p, const SpgemmWs& w, void* stream, int64_t* launches) {
  hipStream_t st = as_stream(stream);
  const int64_t m = p.m;
  p.list = w.lists;
  p.n_list = w.counters;
  hipLaunchKernelGGL((k_spgemm_rows<kSpWaveBlock, kSpWaveSlots, false, FILL, int32_t>), dim3(sp_grid(m, 1 << 16)),
                     dim3(kSpWaveBlock), 0, st, p);
  MP_CHECK_LAUNCH();
  p.list = w.lists + m;
  p.n_list = w.counters + 1;
  hipLaunchKernelGGL((k_spgemm_rows<kSpWgBlock, kSpWgSlots, false, FILL, int32_t>), dim3(sp_grid(m, 2048)),
                     dim3(kSpWgBlock), 0, st, p);
  MP_CHECK_LAUNCH();
  p.list = w.lists + 2 * m;
  p.n_list = w.counters + 2;
  hipLaunchKernelGGL((k_spgemm_rows<kSpWinBlock, kSpWindow, true, FILL, int64_t>), dim3(sp_grid(m, 1024)),
                     dim3(kSpWinBlock), 0, st, p);
  MP_CHECK_LAUNCH();
  *launches += 3;
  return MP_OK;
}

static int spgemm_count(const int32_t* rowptr_a, size_t rowptr_a_bytes, const int32_t* col_a, size_t col_a_bytes,
                        const int32_t* rowptr_b, size_t rowptr_b_bytes, const int32_t* col_b, size_t col_b_bytes,
                        const SpShape& s, int32_t flags, int64_t* rowptr_c, size_t rowptr_c_bytes, int64_t* stats,
                        size_t stats_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_spgemm_count";
  if (int rc = sp_shape(fn, s, flags)) return rc;
  if (int rc = sp_csrs(fn, s, rowptr_a, rowptr_a_bytes, col_a, col_a_bytes, rowptr_b, rowptr_b_bytes, col_b,
                       col_b_bytes))
    return rc;
  MP_CHECK_ARG(rowptr_c != nullptr, "%s: rowptr_c is NULL", fn);
  MP_CHECK_EXTENT(fn, "rowptr_c", rowptr_c_bytes, (size_t)(s.m + 1) * 8);
  MP_CHECK_ARG(stats != nullptr, "%s: stats is NULL", fn);
  MP_CHECK_EXTENT(fn, "stats", stats_bytes, 4 * 8);
  size_t scan_bytes = 0;
  hipError_t query;
  if (int rc = sp_ws(fn, s.m, ws, ws_bytes, &scan_bytes, &query)) return rc;
  MP_CHECK_HIP(query);
  SpgemmWs w(ws, s.m);
  MP_DEVICE_GUARD(stream);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_spgemm_zero, dim3(1), dim3(64), 0, st, w.counters, rowptr_c);
  MP_CHECK_LAUNCH();
  ++*launches;
  if (s.m > 0) {
    hipLaunchKernelGGL(k_spgemm_ub, dim3((unsigned)ceil_div(s.m, 4)), dim3(256), 0, st, rowptr_a, col_a, rowptr_b,
                       (int32_t)s.m, (int32_t)s.k, w.ub, w.lists, w.counters, rowptr_c);
    MP_CHECK_LAUNCH();
    ++*launches;
    SpP p{rowptr_a, col_a, nullptr, nullptr, rowptr_b, col_b, nullptr, nullptr, (int32_t)s.m, (int32_t)s.k,
          (int32_t)s.n, flags & MP_SPGEMM_DROP_DIAG, rowptr_c, nullptr, nullptr, w.ub, nullptr, nullptr, nullptr, 0};
    if (int rc = sp_launch_bins<false>(p, w, stream, launches)) return rc;
    MP_CHECK_HIP(rocprim::inclusive_scan(w.rest(), scan_bytes, rowptr_c + 1, rowptr_c + 1, (size_t)s.m,
                                         rocprim::plus<int64_t>(), st, false));
    ++*launches;
  }
  hipLaunchKernelGGL(k_spgemm_stats, dim3(1), dim3(64), 0, st, rowptr_c, (int32_t)s.m, w.counters, stats);
  MP_CHECK_LAUNCH();
  ++*launches;
  return MP_OK;
}

static int spgemm_fill(const int32_t* rowptr_a, size_t rowptr_a_bytes, const int32_t* col_a, size_t col_a_bytes,
                       const int32_t* eid_a, size_t eid_a_bytes, const float* val_a, size_t val_a_bytes,
                       const int32_t* rowptr_b, size_t rowptr_b_bytes, const int32_t* col_b, size_t col_b_bytes,
                       const int32_t* eid_b, size_t eid_b_bytes, const float* val_b, size_t val_b_bytes,
                       const SpShape& s, int32_t flags, const int64_t* rowptr_c, size_t rowptr_c_bytes, int64_t nnz_c,
                       int64_t* out_row, size_t out_row_bytes, int64_t* out_col, size_t out_col_bytes, float* out_val,
                       size_t out_val_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_spgemm_fill_f32";
  if (int rc = sp_shape(fn, s, flags)) return rc;
  if (int rc = sp_csrs(fn, s, rowptr_a, rowptr_a_bytes, col_a, col_a_bytes, rowptr_b, rowptr_b_bytes, col_b,
                       col_b_bytes))
    return rc;
  if (int rc = sp_array(fn, "eid_a", eid_a, eid_a_bytes, s.nnz_a, 4)) return rc;
  if (int rc = sp_array(fn, "val_a", val_a, val_a_bytes, s.nnz_a, 4)) return rc;
  if (int rc = sp_array(fn, "eid_b", eid_b, eid_b_bytes, s.nnz_b, 4)) return rc;
  if (int rc = sp_array(fn, "val_b", val_b, val_b_bytes, s.nnz_b, 4)) return rc;
  MP_CHECK_ARG(rowptr_c != nullptr, "%s: rowptr_c is NULL", fn);
  MP_CHECK_EXTENT(fn, "rowptr_c", rowptr_c_bytes, (size_t)(s.m + 1) * 8);
  MP_CHECK_ARG(nnz_c >= 0, "%s: nnz_c = %lld < 0", fn, (long long)nnz_c);
  MP_CHECK_ARG(nnz_c < 0x7fffffffLL, "%s: nnz_c = %lld above the int32 limit 2^31 - 2", fn, (long long)nnz_c);
  if (int rc = sp_array(fn, "out_row", out_row, out_row_bytes, nnz_c, 8)) return rc;
  if (int rc = sp_array(fn, "out_col", out_col, out_col_bytes, nnz_c, 8)) return rc;
  if (int rc = sp_array(fn, "out_val", out_val, out_val_bytes, nnz_c, 4)) return rc;
  size_t scan_bytes = 0;
  hipError_t query;
  if (int rc = sp_ws(fn, s.m, ws, ws_bytes, &scan_bytes, &query)) return rc;
  if (s.m == 0 || nnz_c == 0) return MP_OK;
  SpgemmWs w(ws, s.m);
  MP_DEVICE_GUARD(stream);
  SpP p{rowptr_a, col_a, eid_a, val_a, rowptr_b, col_b, eid_b, val_b, (int32_t)s.m, (int32_t)s.k, (int32_t)s.n,
        flags & MP_SPGEMM_DROP_DIAG, const_cast<int64_t*>(rowptr_c), nullptr, nullptr, w.ub, out_row, out_col,
        out_val, nnz_c};
  return sp_launch_bins<true>(p, w, stream, launches);
}

static inline int64_t sp_result(int rc, int64_t launches) { return rc != MP_OK ? -(int64_t)rc : launches; }

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_spgemm_bin_cap(int32_t which) {
  switch (which) {
    case MP_SPGEMM_CAP_WAVE: return kSpWaveCap;
    case MP_SPGEMM_CAP_WG: return kSpWgCap;
    case MP_SPGEMM_WINDOW: return kSpWindow;
    case MP_SPGEMM_SLOTS_WAVE: return kSpWaveSlots;
    case MP_SPGEMM_SLOTS_WG: return kSpWgSlots;
  }
  set_error("mp_spgemm_bin_cap: which = %d outside [0, 4]", which);
  return -(int64_t)MP_ERR_ARG;
}

extern "C" size_t mp_spgemm_workspace(int64_t m) {
  if (m < 0) m = 0;
  size_t scan_bytes = 0;
  (void)sp_scan_bytes(m, &scan_bytes);
  return SpgemmWs(nullptr, m).total(scan_bytes);
}

extern "C" int64_t mp_spgemm_count(const int32_t* rowptr_a, size_t rowptr_a_bytes, const int32_t* col_a,
                                   size_t col_a_bytes, const int32_t* rowptr_b, size_t rowptr_b_bytes,
                                   const int32_t* col_b, size_t col_b_bytes, int64_t m, int64_t k, int64_t n,
                                   int64_t nnz_a, int64_t nnz_b, int32_t flags, int64_t* rowptr_c,
                                   size_t rowptr_c_bytes, int64_t* stats, size_t stats_bytes, void* ws,
                                   size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = spgemm_count(rowptr_a, rowptr_a_bytes, col_a, col_a_bytes, rowptr_b, rowptr_b_bytes, col_b,
                              col_b_bytes, SpShape{m, k, n, nnz_a, nnz_b}, flags, rowptr_c, rowptr_c_bytes, stats,
                              stats_bytes, ws, ws_bytes, stream, &launches);
  return sp_result(rc, launches);
}

extern "C" int64_t mp_spgemm_fill_f32(const int32_t* rowptr_a, size_t rowptr_a_bytes, const int32_t* col_a,
                                      size_t col_a_bytes, const int32_t* eid_a, size_t eid_a_bytes, const float* val_a,
                                      size_t val_a_bytes, const int32_t* rowptr_b, size_t rowptr_b_bytes,
                                      const int32_t* col_b, size_t col_b_bytes, const int32_t* eid_b,
                                      size_t eid_b_bytes, const float* val_b, size_t val_b_bytes, int64_t m, int64_t k,
                                      int64_t n, int64_t nnz_a, int64_t nnz_b, int32_t flags, const int64_t* rowptr_c,
                                      size_t rowptr_c_bytes, int64_t nnz_c, int64_t* out_row, size_t out_row_bytes,
                                      int64_t* out_col, size_t out_col_bytes, float* out_val, size_t out_val_bytes,
                                      void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = spgemm_fill(rowptr_a, rowptr_a_bytes, col_a, col_a_bytes, eid_a, eid_a_bytes, val_a, val_a_bytes,
                             rowptr_b, rowptr_b_bytes, col_b, col_b_bytes, eid_b, eid_b_bytes, val_b, val_b_bytes,
                             SpShape{m, k, n, nnz_a, nnz_b}, flags, rowptr_c, rowptr_c_bytes, nnz_c, out_row,
                             out_row_bytes, out_col, out_col_bytes, out_val, out_val_bytes, ws, ws_bytes, stream,
                             &launches);
  return sp_result(rc, launches);
}
