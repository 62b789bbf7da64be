/*
 * abi_reject_glob.c -- argument / extent rejection harness for the attention
 * readout entry points of include/mi355_mp.h (mp_readout_path,
 * mp_readout_chunk, mp_readout_workspace, mp_attention_readout_f32,
 * mp_attention_readout_bwd_f32).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_glob`) and run as a plain program
 * on a machine with no GPU by tests/test_glob_host.py.  Every case calls one
 * entry point with one bad argument and expects -MP_ERR_ARG and an error text
 * naming the problem -- no launch, no device access, no host memory error (ASAN
 * aborts the run on one).  ACCEPT cases pass every check (the call then fails at
 * its first HIP call, -MP_ERR_HIP, as there is no GPU): the boundary is the
 * documented one, not a looser one.
 * Output: one line per case, then "abi_reject_glob: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)
#define DEVL ((int64_t*)DEV)

static void expect(int line, const char* what, int64_t rc, int want_arg, const char* needle) {
  ++n_cases;
  const char* err = mp_last_error();
  int ok;
  if (want_arg) {
    ok = rc == -MP_ERR_ARG && (!needle || (err && strstr(err, needle)));
  } else {
    ok = rc != -MP_ERR_ARG;
  }
  printf("%s line %d: %s -> rc %lld (%s)\n", ok ? "ok  " : "FAIL", line, what, (long long)rc, err ? err : "");
  if (!ok) ++n_fail;
}

#define REJECT(needle, call) expect(__LINE__, #call, (call), 1, needle)
#define ACCEPT(call) expect(__LINE__, #call, (call), 0, NULL)

int main(void) {
  enum { N = 5000, G = 7, C = 33, MAXN = 3000, LD = 40 };
  const size_t WS = mp_readout_workspace(N, G, MAXN, C);
  const size_t OUTB = ((size_t)(G - 1) * LD + C) * 4, EB = (size_t)N * 4, SB = (size_t)G * 8;
  const size_t DXB = ((size_t)(N - 1) * LD + C) * 4;

  /* the path query: every path, the argument check */
  ++n_cases;
  if (!(mp_readout_path(0, 64) == 0 && mp_readout_path(1, 64) == 0 && mp_readout_path(1 << 20, 64) == 2 &&
        mp_readout_path(1 << 20, 1) == 2 && mp_readout_path(5, 0) == -MP_ERR_ARG &&
        mp_readout_path(5, -3) == -MP_ERR_ARG && mp_readout_path(-1, 4) == -MP_ERR_ARG &&
        mp_readout_chunk(0) == -MP_ERR_ARG && mp_readout_chunk(64) >= 1 &&
        mp_readout_path(4 * mp_readout_chunk(64), 64) == 1 && mp_readout_path(4 * mp_readout_chunk(64) + 1, 64) == 2)) {
    printf("FAIL mp_readout_path / mp_readout_chunk\n");
    ++n_fail;
  } else {
    printf("ok   mp_readout_path / mp_readout_chunk\n");
  }
  /* the workspace: a split graph needs its chunk slots, an unsplit batch only the spare step */
  ++n_cases;
  if (!(WS >= ((size_t)N / mp_readout_chunk(C) + G) * (C + 2) * 4 && mp_readout_workspace(N, G, 8, C) <= 1024 &&
        mp_readout_workspace(0, 0, 0, C) >= 256)) {
    printf("FAIL mp_readout_workspace\n");
    ++n_fail;
  } else {
    printf("ok   mp_readout_workspace\n");
  }

#define FWD(x, ldx, n, c, st, g, mx, q, ldq, sc, out, ldo, ob, qo, qob, e, eb, sts, sb, al, ab, ws, wsb) \
  mp_attention_readout_f32(x, ldx, n, c, st, g, mx, q, ldq, sc, out, ldo, ob, qo, qob, e, eb, sts, sb, al, ab, ws, wsb, NULL)

  /* forward, query mode */
  REJECT("x is NULL", FWD(NULL, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("starts is NULL", FWD(DEVF, LD, N, C, NULL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("out is NULL", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, NULL, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("e is NULL", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, NULL, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("stats is NULL", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, NULL, SB, NULL, 0, DEV, WS));
  REJECT("ws is NULL", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, NULL, WS));
  REJECT("C = 0", FWD(DEVF, LD, N, 0, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("ldx", FWD(DEVF, C - 1, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("ldq", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, C - 1, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("ldo", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, C - 1, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("n = -1", FWD(DEVF, LD, -1, C, DEVL, G, 0, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("n_graphs = -1", FWD(DEVF, LD, N, C, DEVL, -1, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("max_n", FWD(DEVF, LD, N, C, DEVL, G, -1, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("max_n", FWD(DEVF, LD, N, C, DEVL, G, N + 1, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("n_graphs = 0", FWD(DEVF, LD, N, C, DEVL, 0, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("both", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("neither", FWD(DEVF, LD, N, C, DEVL, G, MAXN, NULL, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("q_out needs q", FWD(DEVF, LD, N, C, DEVL, G, MAXN, NULL, 0, DEVF, DEVF, LD, OUTB, DEVF, OUTB, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("out holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB - 1, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("q_out holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, DEVF, OUTB - 1, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("e holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB - 1, DEVF, SB, NULL, 0, DEV, WS));
  REJECT("stats holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB - 1, NULL, 0, DEV, WS));
  REJECT("alpha holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, DEVF, EB - 1, DEV, WS));
  REJECT("ws holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS - 1));
  REJECT("ws holds", FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, 0));
  ACCEPT(FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  ACCEPT(FWD(DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, LD, OUTB, DEVF, OUTB, DEVF, EB, DEVF, SB, DEVF, EB, DEV, WS));
  ACCEPT(FWD(DEVF, C, N, C, DEVL, G, MAXN, NULL, 0, DEVF, DEVF, C, ((size_t)(G - 1) * C + C) * 4, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV, WS));
  ACCEPT(FWD(DEVF, 1, N, 1, DEVL, G, N, NULL, 0, DEVF, DEVF, 1, (size_t)G * 4, NULL, 0, DEVF, EB, DEVF, SB, NULL, 0, DEV,
             mp_readout_workspace(N, G, N, 1)));
  /* no graphs and no nodes: nothing to do, accepted with empty arrays */
  ACCEPT(FWD(NULL, C, 0, C, DEVL, 0, 0, DEVF, C, NULL, NULL, C, 0, NULL, 0, NULL, 0, NULL, 0, NULL, 0, DEV,
             mp_readout_workspace(0, 0, 0, C)));
  /* graphs without nodes */
  ACCEPT(FWD(NULL, C, 0, C, DEVL, G, 0, DEVF, C, NULL, DEVF, C, (size_t)G * C * 4, NULL, 0, NULL, 0, DEVF, SB, NULL, 0, DEV,
             mp_readout_workspace(0, G, 0, C)));

#define BWD(dr, lddr, x, ldx, n, c, st, g, mx, q, ldq, e, sts, r, ldr, dx, lddx, dxb, dq, lddq, dqb, ds, dsb, ws, wsb) \
  mp_attention_readout_bwd_f32(dr, lddr, x, ldx, n, c, st, g, mx, q, ldq, e, sts, r, ldr, dx, lddx, dxb, dq, lddq, dqb, ds, dsb, ws, wsb, NULL)

  /* backward */
  REJECT("dr is NULL", BWD(NULL, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("x is NULL", BWD(DEVF, LD, NULL, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("starts is NULL", BWD(DEVF, LD, DEVF, LD, N, C, NULL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("e is NULL", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, NULL, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("stats is NULL", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, NULL, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("r is NULL", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, NULL, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("ws is NULL", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, NULL, WS));
  REJECT("C = 0", BWD(DEVF, LD, DEVF, LD, N, 0, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("lddr", BWD(DEVF, C - 1, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("ldx", BWD(DEVF, LD, DEVF, C - 1, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("ldq", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, C - 1, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("ldr", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, C - 1, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("lddx", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, C - 1, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("lddq", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, C - 1, OUTB, NULL, 0, DEV, WS));
  REJECT("n = -5", BWD(DEVF, LD, DEVF, LD, -5, C, DEVL, G, 0, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("dscore is the score mode", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, NULL, LD, 0, DEVF, EB, DEV, WS));
  REJECT("dq is the query mode", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, NULL, 0, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("dx holds", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB - 1, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  REJECT("dq holds", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB - 1, NULL, 0, DEV, WS));
  REJECT("dscore holds", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, NULL, 0, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, NULL, 0, 0, DEVF, EB - 1, DEV, WS));
  REJECT("ws holds", BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS - 1));
  ACCEPT(BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, DEVF, LD, OUTB, NULL, 0, DEV, WS));
  ACCEPT(BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, NULL, 0, DEVF, DEVF, DEVF, LD, DEVF, LD, DXB, NULL, 0, 0, DEVF, EB, DEV, WS));
  ACCEPT(BWD(DEVF, C, DEVF, C, N, C, DEVL, G, MAXN, DEVF, C, DEVF, DEVF, DEVF, C, NULL, 0, 0, DEVF, C, (size_t)G * C * 4, NULL, 0, DEV, WS));
  /* no gradient wanted: nothing to do */
  ACCEPT(BWD(DEVF, LD, DEVF, LD, N, C, DEVL, G, MAXN, DEVF, LD, DEVF, DEVF, DEVF, LD, NULL, 0, 0, NULL, 0, 0, NULL, 0, DEV, WS));

  /* a launch of 2^24 workgroups or more is refused by name before anything runs: 2^17 graphs beside one of
   * 2^20 nodes is 2^17 * 4096 chunk workgroups; 2^11 graphs beside it (2^23) pass */
  {
    const int64_t NB = (int64_t)1 << 21, MB = (int64_t)1 << 20, GB = (int64_t)1 << 17, GS = (int64_t)1 << 11;
    REJECT("launch too large", FWD(DEVF, 64, NB, 64, DEVL, GB, MB, DEVF, 64, NULL, DEVF, 64, (size_t)GB * 256, NULL, 0, DEVF, (size_t)NB * 4,
                                   DEVF, (size_t)GB * 8, NULL, 0, DEV, mp_readout_workspace(NB, GB, MB, 64)));
    ACCEPT(FWD(DEVF, 64, NB, 64, DEVL, GS, MB, DEVF, 64, NULL, DEVF, 64, (size_t)GS * 256, NULL, 0, DEVF, (size_t)NB * 4, DEVF,
               (size_t)GS * 8, NULL, 0, DEV, mp_readout_workspace(NB, GS, MB, 64)));
    REJECT("launch too large", BWD(DEVF, 64, DEVF, 64, NB, 64, DEVL, GB, MB, DEVF, 64, DEVF, DEVF, DEVF, 64, DEVF, 64, (size_t)NB * 256,
                                   DEVF, 64, (size_t)GB * 256, NULL, 0, DEV, mp_readout_workspace(NB, GB, MB, 64)));
  }

  printf("abi_reject_glob: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
