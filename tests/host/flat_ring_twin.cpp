// Host twin of the rolling gather window of k_agg_flat's scalar-batch path
// (csrc/mp_flat_ring.h; the loop in csrc/mp_aggregate.hip).  It walks tasks the
// way a wave does -- prologue, batches, refills, look-ahead loads -- with the
// kernel's own index functions, over col / w arrays of exactly n_edges
// elements on the heap, so AddressSanitizer sees any look-ahead that leaves
// them, and checks for every slot that the ring entry consumed holds that
// slot's column and that the weight beside it is that slot's.
//
//   flat_ring_twin U n_edges b0 b1 ... bT     tasks [b0,b1) [b1,b2) ... (b0 >= 0, bT <= n_edges)
//
// Built and run by tests/test_flat_ring_host.py with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mp_flat_ring.h"

namespace {

struct Arrays {
  int64_t n;
  int32_t* col;  // col[k] = 7 * k + 1: a value that names its slot
  float* w;      // w[k] = k
};

int g_fail = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      fprintf(stderr, __VA_ARGS__);   \
      fputc('\n', stderr);            \
      ++g_fail;                       \
    }                                 \
  } while (0)

// scalar_batch of the kernel: slots [e, e + U) of an array of n, clamped to its last element
template <class T>
void scalar_batch(const T* a, int64_t n, int64_t e, int U, T* v) {
  CHECK(e >= 0 && e < n, "scalar_batch starts at %lld of %lld", (long long)e, (long long)n);
  if (e + U <= n) {
    for (int u = 0; u < U; ++u) v[u] = a[e + u];
  } else {
    for (int u = 0; u < U; ++u) v[u] = a[mp::batch_slot(e, u, n)];
  }
}

struct Stats {
  int64_t consumed = 0, issued = 0, wasted = 0;
  int min_flight = 1 << 30;  // least gathers in flight behind a refill
};

// One task, as the kernel's loop runs it.  A ring entry records the column it
// was issued with; consuming entry u at slot k checks it against col[k].
void run_task(const Arrays& A, int U, int64_t e_begin, int64_t e_end, Stats& st) {
  std::vector<int32_t> c_nxt(U), ring(U, -1);
  std::vector<float> w_cur(U);
  if (e_begin >= e_end) return;
  int64_t e = e_begin, next = e_begin;
  int flight = 0;
  auto issue = [&](int u, int64_t slot) {
    ring[u] = c_nxt[u];
    ++flight;
    ++st.issued;
    if (slot >= e_end) ++st.wasted;  // issued past the task's end: loaded, never consumed
    else CHECK(ring[u] == A.col[slot], "gather for slot %lld carries column %d", (long long)slot, ring[u]);
  };
  auto consume = [&](int u, int64_t k) {
    CHECK(k == next && k < e_end, "slot %lld consumed, %lld expected", (long long)k, (long long)next);
    ++next;
    CHECK(ring[u] == A.col[k], "slot %lld: ring entry %d holds column %d, not %d", (long long)k, u, ring[u], A.col[k]);
    CHECK(w_cur[u] == A.w[k], "slot %lld: weight %g, not %g", (long long)k, w_cur[u], A.w[k]);
    --flight;
    ++st.consumed;
  };
  scalar_batch(A.col, A.n, e, U, c_nxt.data());
  for (int u = 0; u < U; ++u) issue(u, e + u);
  if (mp::ring_refills(e, e_end, U)) scalar_batch(A.col, A.n, e + U, U, c_nxt.data());
  scalar_batch(A.w, A.n, e, U, w_cur.data());
  for (; mp::ring_refills(e, e_end, U); e += U) {
    for (int u = 0; u < U; ++u) {
      consume(u, e + u);
      issue(u, e + U + u);
      if (flight < st.min_flight) st.min_flight = flight;
    }
    if (mp::ring_loads_cols(e, e_end, U)) scalar_batch(A.col, A.n, e + 2 * (int64_t)U, U, c_nxt.data());
    scalar_batch(A.w, A.n, e + U, U, w_cur.data());
  }
  CHECK(e < e_end && e_end - e <= U, "last batch at %lld of a task ending at %lld", (long long)e, (long long)e_end);
  const int n = mp::ring_last(e, e_end);
  for (int u = 0; u < U; ++u)
    if (u < n) consume(u, e + u);
  CHECK(next == e_end, "task [%lld, %lld) stopped at %lld", (long long)e_begin, (long long)e_end, (long long)next);
  CHECK(flight == U - n, "%d gathers left in flight behind a last batch of %d", flight, n);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s U n_edges b0 b1 ... bT\n", argv[0]);
    return 2;
  }
  const int U = atoi(argv[1]);
  Arrays A;
  A.n = atoll(argv[2]);
  if (U < 1 || A.n < 1) return 2;
  A.col = (int32_t*)malloc(sizeof(int32_t) * (size_t)A.n);
  A.w = (float*)malloc(sizeof(float) * (size_t)A.n);
  for (int64_t k = 0; k < A.n; ++k) {
    A.col[k] = (int32_t)(7 * k + 1);
    A.w[k] = (float)k;
  }
  Stats st;
  int64_t slots = 0;
  for (int i = 3; i + 1 < argc; ++i) {
    const int64_t b = atoll(argv[i]), t = atoll(argv[i + 1]);
    if (b < 0 || t < b || t > A.n) return 2;
    run_task(A, U, b, t, st);
    slots += t - b;
  }
  CHECK(st.consumed == slots, "%lld slots consumed of %lld", (long long)st.consumed, (long long)slots);
  CHECK(st.issued == st.consumed + st.wasted, "%lld gathers issued for %lld slots (+ %lld past short tasks)",
        (long long)st.issued, (long long)st.consumed, (long long)st.wasted);
  CHECK(st.min_flight >= U, "the ring fell to %d of %d in flight before a task's last batch", st.min_flight, U);
  free(A.col);
  free(A.w);
  if (g_fail) return 1;
  printf("ok U=%d tasks=%d slots=%lld issued=%lld\n", U, argc - 4, (long long)slots, (long long)st.issued);
  return 0;
}
