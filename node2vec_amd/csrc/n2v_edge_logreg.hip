// n2v_edge_logreg.hip -- the link-prediction classifier of the node2vec paper (section 4.4): binary logistic
// regression on the edge feature f = op(x_a, x_b) of a list of vertex pairs, without the [n_pairs, dim] feature
// matrix.  One launch gathers the two rows of every pair, forms the feature in registers, scores it against one
// weight vector and adds the pair's loss and gradient to its slab's partial sums; a finishing kernel folds the slabs
// in fp64.  Read-only on X; no float atomics; every result is a function of (X, a, b, y, w, b0, op) alone
// (DESIGN.md "Link-prediction classifier"; tests/cpu_edge_logreg/n2v_edge_logreg_cpu.c restates it).
//
// Per pair i, in fp32:
//   f[d] = feature(op, x_a[d], x_b[d])                     (n2v_pair_load.h: the bits n2v_pair_features writes)
//   z    = dot(w, f) + b0, dot in the fixed order of n2v_pairs.hip with w in the place of x_a and f in that of x_b:
//          G = 16 for dim <= 128, 32 for dim <= 256, 64 beyond; lane l of the G: s_l = +0; for c = l, l + G, ..
//          while 4 c < dim, j = 0 .. 3 while 4 c + j < dim: s_l = fmaf(w[4 c + j], f[4 c + j], s_l); then for
//          off = 1, 2, 4, .. < G: s_l = s_l + s_(l xor off); dot = s_0; then the one add of b0.
//   res, l = logistic_point(z, y[i] != 0)                  (n2v_logistic.h, as in n2v_logreg.hip)
//   A pair with an index outside [0, n) is never dereferenced: its rows read as 0 and its z is NaN, so res, l and
//   every sum it enters are NaN (fmaf(NaN, +0, acc)).
//
// The order of summation.  It depends on n_pairs, dim and op alone.  With S = slab_pairs(n_pairs, dim) (the slab rule
// of n2v_dense_host.h at the bytes of one class: a multiple of 64) and P = 64 / G:
//   slab s holds the pairs [s S, min((s + 1) S, n_pairs)); group t of the slab its pairs [64 t, 64 t + 64); pair q of
//   a group (q = 0 .. 63) belongs to chain (v, g) = (t mod 4, q mod P) of the slab.
//   chain (v, g), element d:  acc = +0; over the chain's pairs, t ascending and within a group q ascending:
//                             acc = fmaf(res, f[d], acc).
//                   likewise  cb = +0; cb = cb + res   and   cl = 0.0; cl = cl + (double)l   over the same pairs.
//   The places that pad the last group of a slab to 64 pairs belong to no chain: they add nothing, so a chain
//   without pairs stays +0 and a chain that has underflowed to -0 stays -0 until it meets another chain.
//   lane groups: for off = 1, 2, .. < P, for every g at once: chain (v, g) = chain (v, g) + chain (v, g xor off)
//                (acc and cb in fp32, cl in fp64); wave v's sum is chain (v, 0).
//   waves:       GW[s][d] = ((wave 0 + wave 1) + wave 2) + wave 3 in fp32, likewise Gb[s]; L[s] the same in fp64.  A
//                wave without pairs contributes +0, so GW[s][d] is -0 only where all 4 P chains are -0.
//   slabs:       gw[d] = 0.0 + (double)GW[0][d] + (double)GW[1][d] + .., likewise gb; loss = 0.0 + L[0] + L[1] + ..
//                (so gw, gb and loss are never -0).
// gw(a, b) == gw(b, a) bit for bit: the four operators commute bitwise and nothing else sees the sides.
//
// Shape: the layout of pair_features_kernel.  A wave owns 64 consecutive pairs at a time, P of them side by side per
// step, 16-byte loads, eight of them per lane in flight before the first is used.  A lane keeps its 4 K <= 16
// elements of w and its 4 K accumulators in registers across the slab; every lane of a group computes the group's
// res and l (the gather is the cost).  A block of four waves owns a slab; the slab's partials are written once.
// dim % 4 != 0 or a pointer that is not 16-byte aligned goes element by element through the same guards (VEC = false).
#include <math.h>

#include "n2v_logistic.h"
#include "n2v_pair_load.h"

namespace {

constexpr int kMaxDim = 1024;

// the slabs, and the workspace `ws` laid out (ws null: only `bytes` means anything): the slabs' partial GW, Gb and L
struct Plan {
  SlabPlan slabs;
  int64_t bytes;
  float *GW, *Gb;
  double *L;
};

Plan plan_of(int64_t n_pairs, int32_t dim, void *ws) {
  Plan p{};
  p.slabs = slab_plan(n_pairs, 4 * (int64_t)(dim + 3));  // GW and Gb in fp32, L in fp64
  const int64_t s = p.slabs.n_slabs;
  Carver carve(ws);
  p.GW = carve.take<float>(s * dim * 4);
  p.Gb = carve.take<float>(s * 4);
  p.L = carve.take<double>(s * 8);
  p.bytes = carve.used;
  return p;
}

// this lane's elements of the features of one pair
template <int K>
__device__ __forceinline__ void features_of(int32_t op, const f32x4 (&va)[K], const f32x4 (&vb)[K], f32x4 (&f)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) f[k][j] = feature(op, va[k][j], vb[k][j]);
}

// dot(w, f) over the lane group: every lane of the group returns the same bits
template <int G, int K>
__device__ __forceinline__ float group_dot(const f32x4 (&wv)[K], const f32x4 (&f)[K], int32_t dim, int l) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = l + k * G;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * c + j < dim) s = __fmaf_rn(wv[k][j], f[k][j], s);
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) s += __shfl_xor(s, off, 64);
  return s;
}

template <int G, int K, bool VEC>
__global__ __launch_bounds__(256) void edge_scores_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                          const int64_t *__restrict__ a,
                                                          const int64_t *__restrict__ b, int64_t n_pairs, int32_t op,
                                                          const float *__restrict__ w, const float *__restrict__ b0,
                                                          float *__restrict__ out) {
  constexpr int GP = 64 / G, U = Unroll<K>::U;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kWavePairs;
  if (p0 >= n_pairs) return;
  const int cnt = n_pairs - p0 < kWavePairs ? (int)(n_pairs - p0) : kWavePairs;
  int32_t ra, rb;
  load_pair(a, b, p0, cnt, n, lane, ra, rb);
  const int l = lane % G;
  f32x4 wv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wv[k] = load_chunk<VEC>(w, l + k * G, dim, true);
  const float bias = b0[0];
  float res = 0.f;
  for (int base = 0; base < cnt; base += GP * U) {
    f32x4 va[U][K], vb[U][K];
    bool live[U];
    load_step<G, K, VEC>(X, dim, ra, rb, base, lane, va, vb, live);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f32x4 f[K];
      features_of<K>(op, va[u], vb[u], f);
      const float s = group_dot<G, K>(wv, f, dim, l);
      // the GP dots of this step go to the lanes that own those pairs
      const int d = lane - (base + u * GP);
      const float t = __shfl(s, (d & (GP - 1)) * G, 64);
      if (d >= 0 && d < GP) res = t;
    }
  }
  if (lane < cnt) out[p0 + lane] = ra < 0 ? NAN : res + bias;
}

// Block s owns slab s; wave v its groups v, v + 4, ..  (the file header's chains).
template <int G, int K, bool VEC>
__global__ __launch_bounds__(256) void edge_loss_grad_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                             const int64_t *__restrict__ a,
                                                             const int64_t *__restrict__ b,
                                                             const uint8_t *__restrict__ y, int64_t n_pairs,
                                                             int32_t op, const float *__restrict__ w,
                                                             const float *__restrict__ b0, int64_t slab_pairs,
                                                             float *__restrict__ GW, float *__restrict__ Gb,
                                                             double *__restrict__ L) {
  constexpr int GP = 64 / G, U = Unroll<K>::U;
  __shared__ float sw[4][kMaxDim];
  __shared__ float sb[4];
  __shared__ double sl[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane / G, l = lane % G;
  const int64_t lo = (int64_t)blockIdx.x * slab_pairs;
  const int64_t hi = lo + slab_pairs < n_pairs ? lo + slab_pairs : n_pairs;
  f32x4 wv[K], ga[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wv[k] = load_chunk<VEC>(w, l + k * G, dim, true);
    ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float bias = b0[0];
  float cb = 0.f;
  double cl = 0.0;

  for (int64_t p0 = lo + (int64_t)wave * kWavePairs; p0 < hi; p0 += kBlockPairs) {
    const int cnt = hi - p0 < kWavePairs ? (int)(hi - p0) : kWavePairs;
    int32_t ra, rb;
    load_pair(a, b, p0, cnt, n, lane, ra, rb);
    const uint32_t yl = lane < cnt ? (y[p0 + lane] != 0 ? 1u : 0u) : 0u;
    for (int base = 0; base < cnt; base += GP * U) {
      f32x4 va[U][K], vb[U][K];
      bool live[U];
      load_step<G, K, VEC>(X, dim, ra, rb, base, lane, va, vb, live);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = base + u * GP + g;  // < 64
        f32x4 f[K];
        features_of<K>(op, va[u], vb[u], f);
        const float s = group_dot<G, K>(wv, f, dim, l);
        const float z = live[u] ? s + bias : NAN;
        const uint32_t yq = (uint32_t)__shfl((int)yl, q, 64);
        float res, ls;
        logistic_point(z, yq, res, ls);
        if (q < cnt) {  // a place that pads the group belongs to no chain
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) ga[k][j] = __fmaf_rn(res, f[k][j], ga[k][j]);
          cb = cb + res;
          cl = cl + (double)ls;
        }
      }
    }
  }
  // the lane groups of the wave
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) ga[k][j] = ga[k][j] + __shfl_xor(ga[k][j], off, 64);
    cb = cb + __shfl_xor(cb, off, 64);
    cl = cl + __shfl_xor(cl, off, 64);
  }
  if (lane < G) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = 4 * (l + k * G) + j;
        if (d < dim) sw[wave][d] = ga[k][j];
      }
  }
  if (lane == 0) sb[wave] = cb, sl[wave] = cl;
  __syncthreads();
  // the waves of the block, ascending; the slab's partials are written once
  for (int d = tid; d < dim; d += 256) {
    float p = sw[0][d] + sw[1][d];
    p = p + sw[2][d];
    p = p + sw[3][d];
    GW[(int64_t)blockIdx.x * dim + d] = p;
  }
  if (tid == 0) {
    float p = sb[0] + sb[1];
    p = p + sb[2];
    p = p + sb[3];
    Gb[blockIdx.x] = p;
    double q = sl[0] + sl[1];
    q = q + sl[2];
    q = q + sl[3];
    L[blockIdx.x] = q;
  }
}

// the slab partials folded in ascending slab order in fp64: a thread per element of gw, then gb and the loss
__global__ __launch_bounds__(256) void edge_fold_kernel(const float *__restrict__ GW, const float *__restrict__ Gb,
                                                        const double *__restrict__ L, int32_t n_slabs, int32_t dim,
                                                        double *__restrict__ gw, double *__restrict__ gb,
                                                        double *__restrict__ loss) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (i < dim) {
    for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + (double)GW[(int64_t)sl * dim + i];
    gw[i] = s;
  } else if (i == dim) {
    for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + (double)Gb[sl];
    gb[0] = s;
  } else if (i == dim + 1) {
    for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + L[sl];
    loss[0] = s;
  }
}

bool pairs_ok(int64_t n_pairs, int32_t dim) {
  return dim >= 1 && dim <= kMaxDim && n_pairs >= 0 && n_pairs < ((int64_t)1 << 31);
}

bool op_ok(int32_t op) {
  return op == N2V_PAIR_AVERAGE || op == N2V_PAIR_HADAMARD || op == N2V_PAIR_L1 || op == N2V_PAIR_L2;
}

}  // namespace

extern "C" {

int64_t n2v_edge_logreg_slab_pairs(int64_t n_pairs, int32_t dim) {
  if (!pairs_ok(n_pairs, dim)) return -1;
  return plan_of(n_pairs, dim, nullptr).slabs.slab_rows;
}

int64_t n2v_edge_logreg_workspace_bytes(int64_t n_pairs, int32_t dim) {
  if (!pairs_ok(n_pairs, dim)) return -1;
  return n_pairs == 0 ? 0 : plan_of(n_pairs, dim, nullptr).bytes;
}

int n2v_edge_logreg_scores(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                           int64_t n_pairs, int32_t op, const float *w, const float *b0, float *z_out,
                           void *stream) {
  if (!matrix_ok(n, dim) || !pairs_ok(n_pairs, dim)) return N2V_EINVAL;
  if (!op_ok(op)) return N2V_EINVAL;
  if (n_pairs == 0) return N2V_OK;
  if (!X || !a || !b || !w || !b0 || !z_out) return N2V_EINVAL;
  const unsigned blocks = (unsigned)((n_pairs + kBlockPairs - 1) / kBlockPairs);
  with_shape(dim, vec_ok(dim, X, w), [&](auto G, auto K, auto VEC) {
    hipLaunchKernelGGL((edge_scores_kernel<G, K, VEC>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, X, n, dim,
                       a, b, n_pairs, op, w, b0, z_out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_edge_logreg_loss_grad(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                              const uint8_t *y, int64_t n_pairs, int32_t op, const float *w, const float *b0,
                              double *loss_out, double *grad_w_out, double *grad_b_out, void *workspace,
                              int64_t workspace_bytes, void *stream) {
  if (!matrix_ok(n, dim) || !pairs_ok(n_pairs, dim)) return N2V_EINVAL;
  if (!op_ok(op)) return N2V_EINVAL;
  if (n_pairs == 0) return N2V_OK;
  if (!X || !a || !b || !y || !w || !b0 || !loss_out || !grad_w_out || !grad_b_out) return N2V_EINVAL;
  const Plan p = plan_of(n_pairs, dim, workspace);
  if (!workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  with_shape(dim, vec_ok(dim, X, w), [&](auto G, auto K, auto VEC) {
    hipLaunchKernelGGL((edge_loss_grad_kernel<G, K, VEC>), dim3((unsigned)p.slabs.n_slabs), dim3(256), 0, st, X, n,
                       dim, a, b, y, n_pairs, op, w, b0, p.slabs.slab_rows, p.GW, p.Gb, p.L);
  });
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(edge_fold_kernel, dim3((unsigned)((dim + 2 + 255) / 256)), dim3(256), 0, st, p.GW, p.Gb, p.L,
                     p.slabs.n_slabs, dim, grad_w_out, grad_b_out, loss_out);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
