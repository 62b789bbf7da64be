// Index arithmetic of k_agg_flat's rolling gather window (the scalar-batch
// path): which batches refill the ring, how far ahead the scalar column /
// weight batches are loaded, and the clamp of a batch that reaches the end of
// its array.  Plain integer functions, compiled into the kernel and into the
// host twin tests/host/flat_ring_twin.cpp, which replays whole schedules
// through them under AddressSanitizer.
//
// A task's slots [e_begin, e_end) go through a ring of U gathers in batches
// that start at e_begin + k*U.  On entry to the batch at e, ring entry u holds
// slot e + u.  Every batch but the task's last consumes all U entries and
// refills each, as soon as it is consumed, with slot e + U + u, from the
// columns of the batch at e + U; behind the last refill it loads the columns
// of the batch at e + 2U (if the task has one) and the weights of the batch at
// e + U.  The last batch consumes its 1 .. U slots and issues nothing.  The
// refills of the last-but-one batch that fall past e_end are issued with the
// columns scalar_batch clamped for them, and never consumed.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MP_RING_HD __host__ __device__ __forceinline__
#else
#define MP_RING_HD inline
#endif

namespace mp {

// Element u of the scalar batch at slot e of an array of n (n >= 1): slots past
// the end of the array read its last element (loaded, never consumed).
MP_RING_HD int64_t batch_slot(int64_t e, int u, int64_t n) { return e + u < n ? e + u : n - 1; }

// the batch at e is not the task's last: it refills the ring and loads the weights of the batch at e + U
MP_RING_HD bool ring_refills(int64_t e, int64_t e_end, int U) { return e + U < e_end; }

// the task has a batch at e + 2U: the batch at e loads its columns
MP_RING_HD bool ring_loads_cols(int64_t e, int64_t e_end, int U) { return e + 2 * (int64_t)U < e_end; }

// slots of the task's last batch, at e: 1 .. U
MP_RING_HD int ring_last(int64_t e, int64_t e_end) { return (int)(e_end - e); }

}  // namespace mp
