// n2v_dense_host.h -- the host-side scaffolding the dense tasks over the trained vectors share (n2v_knn.hip,
// n2v_pairs.hip, n2v_kmeans.hip, n2v_logreg.hip): the bounds on X[n, dim], the 16-byte-access predicate, the slab
// rule, the workspace carver and the dispatch of runtime values to template arguments.  Nothing here runs inside a
// hot kernel (their shared arithmetic is n2v_score_tile.h).
#pragma once

#include <type_traits>

#include "n2v_common.h"

namespace {

__host__ __device__ inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// the bounds every dense task puts on its matrix
inline bool matrix_ok(int64_t n, int32_t dim) { return dim >= 1 && dim <= 1024 && n >= 0 && n < ((int64_t)1 << 31); }

// rows may be read (and written) in 16-byte pieces: VEC of the kernels
template <typename... P>
inline bool vec_ok(int32_t dim, const P *...base) {
  return dim % 4 == 0 && ((... | (uintptr_t)base) & 15) == 0;
}

inline bool workspace_ok(const void *ws, int64_t ws_bytes, int64_t need) {
  return ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need;
}

// A workspace is cut up by ONE sequence of take() calls that the size query and the launcher both run, so the sum
// and the pointers cannot disagree: take returns the current position and advances by round_up(bytes, 256).  From a
// null base nothing is dereferenced and `used` at the end is the size.
struct Carver {
  uintptr_t base;
  int64_t used = 0;
  explicit Carver(void *ws) : base((uintptr_t)ws) {}
  template <typename T>
  T *take(int64_t bytes) {
    T *p = reinterpret_cast<T *>(base + (uintptr_t)used);
    used += round_up(bytes, 256);
    return p;
  }
};

// The slab rule of the kernels that sum per slab of rows and fold the slabs afterwards: a block owns a slab, a slab
// is a multiple of the 64 rows of a block step, and the slabs' partial sums stay under a cap.
constexpr int kSlabStepRows = 64;                  // rows per block step: 16 per wave, 4 waves
constexpr int kMaxSlabs = 2048;                    // blocks of the launch (8 per CU)
constexpr int64_t kPartialsCap = 512ll << 20;      // bytes of slab partials at most

struct SlabPlan {
  int64_t slab_rows;
  int32_t n_slabs;
};

inline SlabPlan slab_plan(int64_t n, int64_t per_slab_bytes) {
  int64_t most = kPartialsCap / per_slab_bytes;  // >= 127: a slab's partials are at most 4 MiB + 12 KiB
  if (most > kMaxSlabs) most = kMaxSlabs;
  const int64_t share = (n + most - 1) / most;
  SlabPlan p;
  p.slab_rows = round_up(share < 1 ? 1 : share, kSlabStepRows);
  p.n_slabs = (int32_t)((n + p.slab_rows - 1) / p.slab_rows);
  return p;
}

// f(std::true_type) or f(std::false_type): a runtime bool becomes a template argument in one place
template <typename F>
inline void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// f(G, VEC) for the kernels built on score_tile: G = 1 group of 16 columns per tile for up to 16 columns, 4 beyond
// (the bits do not depend on the tile)
template <typename F>
inline void with_tile(int32_t cols, bool vec, F &&f) {
  with_bool(cols <= 16, [&](auto one) {
    with_bool(vec, [&](auto v) { f(std::integral_constant<int, decltype(one)::value ? 1 : 4>{}, v); });
  });
}

}  // namespace
