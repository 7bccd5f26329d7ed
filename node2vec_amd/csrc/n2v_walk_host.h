// n2v_walk_host.h -- the host side the walk files share: the arguments of a walk and of a partitioned step as
// the dispatchers (n2v_capi.hip) build them, the per-(p, q) constants of the unit-weight kernels, and the one
// declaration of every launcher that is called from another file than its kernel's.  C++ linkage throughout: a
// prototype that differs from its definition does not link, and none of these names is exported beside the C
// ABI of include/n2v_hip.h.
#pragma once
#include "n2v_common.h"

namespace n2v {

// n2v_walk / n2v_walk_ws, checked: a graph with rowptr and col, at least one walker, every buffer present
struct WalkArgs {
  const n2v_graph *g;
  const int32_t *start_ids;
  int64_t n_start;
  int32_t num_walks, walk_length;
  double p, q;
  uint64_t seed;
  int32_t *walks_out;
  uint8_t *valid_out;
  uint32_t *status;
  hipStream_t stream;
  int64_t total() const { return n_start * (int64_t)num_walks; }
};

// n2v_partition_step, checked: k > 0 walkers, status[1] zeroed on the stream
struct StepArgs {
  const int64_t *rowptr;
  const int32_t *col;
  const float *w;
  const double *w64;
  int64_t lo, n_local;
  const int64_t *head;
  int32_t head_cols;
  const int64_t *src_ptr;
  const int32_t *src_ids;
  int32_t src_kind;
  int64_t k;
  double p, q;
  uint64_t seed;
  int32_t *next_out;
  int64_t *edge_out;
  uint32_t *status;
  hipStream_t stream;
};

struct UnitConsts {
  double bR, bM, bO;     // 1/p, 1, 1/q
  int64_t TR, TM, TO;    // the same times 2^20 (exact integers; dyadic kernel only)
  int64_t gR, gM, gO;    // TR, TM, TO divided by their greatest common divisor
  double fR, fM, fO;     // the same as fp64 (exact): the closed forms compute in doubles
  int dyadic;            // 1/p, 1/q are multiples of 2^-20: TR .. fO are valid
};
// the constants of (p, q); false = the pair is outside the unit-weight kernels' range (n2v_walk_unit.hip)
bool unit_consts(double p, double q, UnitConsts &K);

// One launcher per kernel, beside the kernel: it chooses its template instance and its grid, nothing else.
// Each returns N2V_OK or N2V_ELAUNCH.  The kernels that take walkers from status[1] find it zeroed.
int launch_walk_uniform(const WalkArgs &a, int form);                     // n2v_walk_uniform.hip
int launch_walk_wedge_slots(const WalkArgs &a, const UnitConsts &K);      // n2v_walk_wedge.hip
int launch_walk_wedge(const WalkArgs &a, const UnitConsts &K);            // n2v_walk_wedge.hip
int launch_walk_unit_lanes(const WalkArgs &a, const UnitConsts &K);       // n2v_walk_unit.hip
int launch_walk_unit_wave(const WalkArgs &a, const UnitConsts &K);        // n2v_walk_unit.hip
int launch_walk_fast(const WalkArgs &a);                                  // n2v_walk_fast.hip
int launch_walk_exact(const WalkArgs &a);                                 // n2v_walk.hip
int launch_step_wedge(const StepArgs &a, const UnitConsts &K);            // n2v_walk_wedge.hip
int launch_step_unit(const StepArgs &a, const UnitConsts &K);             // n2v_walk_unit.hip
int launch_step_generic(const StepArgs &a);                               // n2v_walk.hip
// n2v_edge_row_sums_build (n2v_walk_unit.hip) -> n2v_walk_wedge.hip
int launch_edge_row_sums(const n2v_graph *g, const UnitConsts &K, double q, const int64_t *edges, int64_t k,
                         double *sums_out, hipStream_t stream);
// the long rows of n2v_walk_weighted_step (n2v_walk_wlanes.hip) -> n2v_walk.hip
int launch_weighted_step_wave(const n2v_graph *g, const int32_t *start_ids, int32_t num_walks, const int64_t *order,
                              int64_t n_rows, int32_t min_n, int32_t step, int32_t walk_length, double p, double q,
                              uint64_t seed, int64_t *edge_state, int32_t *walks, uint8_t *valid, uint32_t *status,
                              hipStream_t stream);

inline int launch_status(hipError_t e) { return e == hipSuccess ? N2V_OK : N2V_ELAUNCH; }

}  // namespace n2v
