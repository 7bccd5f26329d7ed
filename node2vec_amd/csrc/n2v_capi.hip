// n2v_capi.hip -- argument checking and dispatch for the C ABI of include/n2v_hip.h: which kernel walks
// (n2v_walk, n2v_walk_ws) and which kernel steps the walkers of one part (n2v_partition_step).
#include "n2v_walk_host.h"

namespace n2v {

// status[1] is the walker counter of the kernels that deal walkers out: started at zero on the same stream
static bool zero_walker_counter(uint32_t *status, hipStream_t stream) {
  return hipMemsetAsync(status + 1, 0, sizeof(uint32_t), stream) == hipSuccess;
}

// Which kernel walks.  The first row that applies, top to bottom; "unit" = every weight 1.0 (w == w64 == NULL),
// "few" = fewer than 0xffffff00 walkers, "biased" = not p == q == 1, K = unit_consts(p, q).
//
//   mode   graph, (p, q)                                          kernel (launcher)
//   -----  -----------------------------------------------------  ---------------------------------------------
//   exact  unit, p == q == 1, few                                 walk_uniform_kernel, two gathers per step or
//                                                                 one: the table by rank_hops (rank_emit 2: the
//                                                                 pairs) > hops8 > hops > rowptr + col; its
//                                                                 fields are checked before anything is put on
//                                                                 the stream                    (launch_walk_uniform)
//   exact  unit, (p, q) in the unit kernels' range:
//            biased, few, hops + wedge_off + wedge_pos, not
//            N2V_DIAG_NO_TABLES_KERNEL: every per-edge table is
//            at hand, no step needs the wave
//              wedge_slots, not N2V_DIAG_NO_SLOTS_KERNEL,         walk_exact_wedge_slots_kernel: the list of a
//              wedge_wide 0, or a mixed table (>= 2) whose        step arrives with its hop entry
//              slots are N2V_SLOTS_FOLDED                                                   (launch_walk_wedge_slots)
//              otherwise (N2V_HOPS_INLINE_RPOS: N2V_EINVAL,       walk_exact_wedge_kernel
//              that hop table is the slots kernel's alone)                                        (launch_walk_wedge)
//            (hops with N2V_HOPS_INLINE_RPOS and biased: N2V_EINVAL from here on)
//            dyadic, few, 1/q <= 1 and 1/p >= 1/q (or p == q      walk_exact_unit_lanes_kernel: a lane per
//            == 1), and edge_classes or hops (p == q == 1 needs   walker, the wave as fallback
//            neither)                                                                        (launch_walk_unit_lanes)
//            otherwise                                            walk_exact_unit_kernel: a wave per walker
//                                                                                             (launch_walk_unit_wave)
//   exact  p == q == 1 with the K1 slots                          walk_fast_kernel             (launch_walk_fast)
//   exact  anything else                                          walk_exact_kernel           (launch_walk_exact)
//   fast   unit, or weighted with the K1 slots (else N2V_EINVAL)  walk_fast_kernel             (launch_walk_fast)
//
// Unit weights, p == q == 1: the table of every step is uniform and the draw is `pick` itself (n2v_walk_uniform.hip).
// Other weights at p == q == 1 (the reference's defaults, constants.py:22,26): w/p == w/q == w exactly, so the table
// generate_edge_alias_tables builds at (s, v) IS generate_alias_tables(row v) -- the K1 slots when the caller has
// them.  One 16-byte gather per step instead of a rebuild, same bits (the unbiased draw of the fast kernel is the
// exact draw).
// Unit weights, biased: every dyadic (p, q) has its pairing in closed form (n2v_unit_core.h): "other" alone on its
// stack -- the only underfull class (1/q <= 1, 1/p >= 1/q) or the only overfull one (1/q >= 1, 1/p <= 1/q; with
// p == q the return slot is an "other" slot) --, or sharing it with the return run (q > 1 with p > q; q < 1 with
// p < q).  Values that are not dyadic: the same kernels add the row up in the reference's order and replay every
// pairing run by run.
// Lanes or wave, when a table is missing: the lanes kernel wants the "other" class -- nearly every slot of a row --
// to be the underfull one; then ~80 % of the steps leave through the per-lane exits.  For the other arrangements
// (q < 1, or p > q) the usual `pick` is an overfull slot, every step needs the pairing, and one wave per walker is
// the better shape (measured: cfg 2, p = 4, q = 0.25: 344 against 241 M steps/s; p = 2, q = 1: 938 against 711).
static int dispatch_walk(const WalkArgs &a, int32_t mode) {
  const n2v_graph *g = a.g;
  const bool unit = !g->w && !g->w64, biased = !(a.p == 1.0 && a.q == 1.0);
  const bool few = a.total() < 0xffffff00ll;
  if (mode == N2V_WALK_FAST) {
    if (!unit && !g->slots) return N2V_EINVAL;
    return launch_walk_fast(a);
  }
  if (mode != N2V_WALK_EXACT) return N2V_EINVAL;
  if (unit && !biased && few) {
    // rank_emit says what rank_hops points at: 0 / 1 the 4-byte ranks (vertex ids / ranks out), 2 the 8-byte pairs
    const int form = g->rank_hops ? (g->rank_emit == 2 ? 4 : 3) : g->hops8 ? 2 : (g->hops ? 1 : 0);
    if (form >= 3) {
      const int P = g->rank_classes;
      if (P < 2 || P > 8192 || (P & (P - 1)) || !g->rank_of || !g->rank_class_first || !g->rank_class_off ||
          g->n_edges >= (1ll << 32) ||
          g->rank_head_n < 0 || g->rank_head_n > (1 << 22) || (g->rank_head_n > 0 && !g->rank_head) ||
          (g->rank_emit == 0 && !g->rank_vertex) || g->rank_emit < 0 || g->rank_emit > 2)
        return N2V_EINVAL;
    }
    if (form == 2 && (g->hop8_col_bits < 1 || g->hop8_row_bits < 1 ||
                      g->hop8_col_bits + g->hop8_row_bits > 62 || g->hop8_align_shift < 0 ||
                      g->hop8_align_shift > 6 || (g->hop8_align_shift > 0 && !g->hop8_rowptr)))
      return N2V_EINVAL;
    if (!zero_walker_counter(a.status, a.stream)) return N2V_ELAUNCH;
    return launch_walk_uniform(a, form);
  }
  UnitConsts K;
  if (unit && unit_consts(a.p, a.q, K)) {
    if (!zero_walker_counter(a.status, a.stream)) return N2V_ELAUNCH;
    if (biased && !(g->reserved & N2V_DIAG_NO_TABLES_KERNEL) && g->hops && g->wedge_off && g->wedge_pos && few) {
      if (g->wedge_wide < 0 || g->wedge_wide > 65536) return N2V_EINVAL;
      if (g->wedge_slots && g->wedge_wide != 1 && !(g->reserved & N2V_DIAG_NO_SLOTS_KERNEL) &&
          (g->wedge_wide == 0 || (g->reserved2 & N2V_SLOTS_FOLDED)))
        return launch_walk_wedge_slots(a, K);
      if (g->reserved2 & N2V_HOPS_INLINE_RPOS) return N2V_EINVAL;
      return launch_walk_wedge(a, K);
    }
    if (g->hops && (g->reserved2 & N2V_HOPS_INLINE_RPOS) && biased) return N2V_EINVAL;
    const bool lanes_regime = !biased || (K.bO <= 1.0 && K.bR >= K.bO);
    if (K.dyadic && lanes_regime && few && (g->edge_classes || g->hops || !biased))
      return launch_walk_unit_lanes(a, K);
    return launch_walk_unit_wave(a, K);
  }
  if (!biased && g->slots) return launch_walk_fast(a);
  if (!zero_walker_counter(a.status, a.stream)) return N2V_ELAUNCH;
  return launch_walk_exact(a);
}

// Which kernel steps the walkers of one part (n2v_partition_step, checked; status[1] zeroed).  The first row that
// applies:
//
//   part, (p, q), src_kind                                        kernel (launcher)
//   ------------------------------------------------------------  ------------------------------------------------
//   unit weights, (p, q) in the unit kernels' range:
//     N2V_SRC_WEDGES / _AT: the wedge list of the edge walked     partition_step_wedge_kernel: one LANE per
//     last travelled with the walker (biased: head_cols >= 5,     walker, the closed forms of the wedge kernel
//     src_ptr and src_ids, else N2V_EINVAL)                                                       (launch_step_wedge)
//     N2V_SRC_ROWS: the row of the previous vertex travelled      partition_step_unit_kernel: one wave per walker
//                                                                                                  (launch_step_unit)
//   N2V_SRC_ROWS, any weights                                     partition_step_kernel: one wave per walker
//                                                                                               (launch_step_generic)
//   otherwise                                                     N2V_EINVAL
static int dispatch_step(const StepArgs &a) {
  UnitConsts K;
  if (!a.w && !a.w64 && unit_consts(a.p, a.q, K)) {
    if (a.src_kind == N2V_SRC_ROWS) return launch_step_unit(a, K);
    // p == q == 1: the header's first four words do
    if (!(a.p == 1.0 && a.q == 1.0) && (a.head_cols < 5 || !a.src_ptr || !a.src_ids)) return N2V_EINVAL;
    return launch_step_wedge(a, K);
  }
  if (a.src_kind != N2V_SRC_ROWS) return N2V_EINVAL;  // (p, q) outside the unit kernels' range
  return launch_step_generic(a);
}

}  // namespace n2v

extern "C" {

int n2v_abi_version(void) { return N2V_ABI_VERSION; }

const char *n2v_status_string(int code) {
  switch (code) {
    case N2V_OK: return "ok";
    case N2V_EINVAL: return "invalid argument";
    case N2V_ELAUNCH: return "HIP launch/runtime error";
    case N2V_ENOGPU: return "no HIP device";
    default: return "unknown status";
  }
}

int n2v_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// no walk kernel takes a workspace (include/n2v_hip.h): none is asked for, and n2v_walk_ws ignores what it is lent
int64_t n2v_walk_workspace_bytes(const n2v_graph *, int64_t, int32_t, int32_t, double, double, int32_t) {
  return 0;
}

int n2v_walk(const n2v_graph *g, const int32_t *start_ids, int64_t n_start, int32_t num_walks,
             int32_t walk_length, double return_param, double inout_param, uint64_t seed,
             int32_t mode, int32_t *walks_out, uint8_t *valid_out, uint32_t *status,
             void *stream) {
  return n2v_walk_ws(g, start_ids, n_start, num_walks, walk_length, return_param, inout_param, seed,
                     mode, walks_out, valid_out, status, nullptr, 0, stream);
}

int n2v_walk_ws(const n2v_graph *g, const int32_t *start_ids, int64_t n_start, int32_t num_walks,
                int32_t walk_length, double return_param, double inout_param, uint64_t seed,
                int32_t mode, int32_t *walks_out, uint8_t *valid_out, uint32_t *status,
                void *, int64_t, void *stream) {
  if (!g || !g->rowptr || !g->col || n_start < 0 || num_walks < 0 || walk_length < 0)
    return N2V_EINVAL;
  // buffers are only required when there is at least one walker
  const bool any = n_start > 0 && num_walks > 0;
  if (any && (!start_ids || !walks_out || !valid_out || !status)) return N2V_EINVAL;
  // generate_edge_alias_tables raises ValueError on p == 0 or q == 0 (randomwalk.py:214-217)
  if (return_param == 0.0 || inout_param == 0.0) return N2V_EINVAL;
  if (!any) return (mode == N2V_WALK_EXACT || mode == N2V_WALK_FAST) ? N2V_OK : N2V_EINVAL;
  if (g->w && g->w64) return N2V_EINVAL;  // one storage form at most
  return n2v::dispatch_walk({g, start_ids, n_start, num_walks, walk_length, return_param, inout_param, seed,
                             walks_out, valid_out, status, (hipStream_t)stream},
                            mode);
}

int n2v_partition_step(const int64_t *rowptr, const int32_t *col, const float *w, const double *w64, int64_t lo,
                       int64_t n_local, const int64_t *head, int32_t head_cols, const int64_t *src_ptr,
                       const int32_t *src_ids, int32_t src_kind, int64_t k, double p, double q, uint64_t seed,
                       int32_t *next_out, int64_t *edge_out, uint32_t *status, void *stream) {
  if (k < 0 || n_local < 0 || k >= 0xfffffff0ll || (w && w64)) return N2V_EINVAL;
  if (p == 0.0 || q == 0.0) return N2V_EINVAL;  // randomwalk.py:209-212 (ValueError upstream)
  if (src_kind != N2V_SRC_ROWS && src_kind != N2V_SRC_WEDGES && src_kind != N2V_SRC_WEDGES_AT)
    return N2V_EINVAL;
  if (head_cols < 4) return N2V_EINVAL;  // (wedge lists with p or q != 1: 5, checked by the dispatch)
  if (src_kind != N2V_SRC_ROWS && (w || w64)) return N2V_EINVAL;  // unit-weight parts only
  if (k == 0) return N2V_OK;
  if (!rowptr || !head || !next_out || !status) return N2V_EINVAL;  // (col: NULL for a part without edges)
  if (q != 1.0 && !src_ptr) return N2V_EINVAL;
  if (!n2v::zero_walker_counter(status, (hipStream_t)stream)) return N2V_ELAUNCH;
  return n2v::dispatch_step({rowptr, col, w, w64, lo, n_local, head, head_cols, src_ptr, src_ids, src_kind, k, p, q,
                             seed, next_out, edge_out, status, (hipStream_t)stream});
}
}
