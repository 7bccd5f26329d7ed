// n2v_umap.hip -- one epoch of a deterministic UMAP layout optimisation over 2-D points Y[n, 2] (n2v_umap_epoch), and
// the spelled x^b it uses over an array (n2v_umap_powb).  No float atomics; Y_next is a function of the arguments
// alone, bit for bit, on any launch geometry (DESIGN.md "UMAP"; tests/cpu_umap/n2v_umap_cpu.c restates both).
//
// The graph is a symmetric CSR (rowptr int64, col int32 ascending within a row) with an fp32 eps per entry, the
// epochs per sample w_max / w.  Entry t fires in epoch e iff eps[t] is finite, eps[t] >= 1 and
//   floorf((float)(e + 1) / eps[t]) > floorf((float)e / eps[t])                (fp32 divisions, correctly rounded)
// An entry whose column lies outside [0, n) never fires and is never an index.  The entries of a row are clamped to
// [0, nnz).
//
// Row i is ONE sequential chain: y = Y[i]; over the row's entries t ascending, for each that fires, with j = col[t]:
//   attract(y, Y[j]); attract(y, Y[j]);  then for s = 0 .. negative - 1:  k = draw(t, s);  if (k != i) repel(y, Y[k])
// and Y_next[i] = y.  Every other point is read from Y, the snapshot: only y runs ahead.  The second attraction stands
// for the move umap-learn gives the tail of the mirror entry (j, i), which fires in the same epochs.
//
// In fp32, every operation rounded once, no contraction but the fmaf written; clamp(v) = v > 4 ? 4 : (v < -4 ? -4 : v):
//   dx = y.x - o.x;  dy = y.y - o.y;  d2 = fmaf(dy, dy, dx * dx);  pw = (b == 1) ? d2 : powb(d2, b)  (n2v_powb.h)
//   attract:  c = d2 > 0 ? ((m2ab * pw) / d2) / fmaf(a, pw, 1.0f) : 0,  m2ab = -2.0f * (a * b)
//   repel:    d2 > 0:  c = g2b / ((0.001f + d2) * fmaf(a, pw, 1.0f)),  g2b = (2.0f * gamma) * b
//   both:     y.x = y.x + alpha * clamp(c * dx);  y.y = y.y + alpha * clamp(c * dy)
//   repel, d2 == 0:  y.x = y.x + alpha * 4.0f;  y.y = y.y + alpha * 4.0f     (a NaN d2 moves nothing)
// The draws: he = mix64(seed ^ mix64(epoch + 0x9E3779B97F4A7C15));  ht = mix64(he + (t + 1) * 0xD1B54A32D192ED03);
//   k = ((mix64(ht ^ ((s + 1) * 0x8CB92BA72F3D8DD7)) >> 32) * n) >> 32 -- keyed by (seed, epoch, t, s) alone.
//
// Mapping.  The targets of an entry's loads -- its neighbour and its draws -- do not depend on y, so they are requested
// together before the dependent arithmetic.  A block takes 256 consecutive rows and groups them by length in LDS
// (a counting sort on length / 8, longest first; integer LDS atomics decide which lane runs which row, never a
// value).  A row of up to kLong entries is a lane's: the lane skips ahead to its next entry that fires, so a wave
// runs as many rounds as its busiest lane has firing entries, and lanes of one wave hold rows of like length.  A
// longer row (a hub) is a wave's: the lanes test a chunk of entries, draw and fetch its points into LDS side by side,
// and the chain then reads them at one address.
#include "n2v_dense_host.h"
#include "n2v_powb.h"

namespace {

constexpr int kRows = 256;        // rows per block step: a lane per row
constexpr int kWaves = kRows / 64;
constexpr int kLong = 128;        // rows of more entries are chained by a whole wave
constexpr int kBucket = 8;        // lengths per bucket of the block's counting sort
constexpr int kBuckets = kLong / kBucket + 1;
constexpr int kAhead = 8;         // draws of an entry a lane requests together
constexpr int kSlots = 384;       // points a wave stages per chunk: 64 entries of 1 + 5
constexpr int kMaxNegative = 64;

struct Scalars {
  float a, b, m2ab, g2b, alpha, alpha4, ep0, ep1;
  int32_t negative;
  uint64_t he;
  int64_t n;
};

__device__ __forceinline__ bool fires(float e, const Scalars &S) {
  if (!(e >= 1.0f && e <= 0x1.fffffep+127f)) return false;
  return floorf(S.ep1 / e) > floorf(S.ep0 / e);
}

__device__ __forceinline__ uint64_t entry_stream(uint64_t he, int64_t t) {
  return n2v::mix64(he + ((uint64_t)t + 1ULL) * 0xD1B54A32D192ED03ULL);
}

__device__ __forceinline__ int32_t draw(uint64_t ht, int s, int64_t n) {
  const uint64_t r = n2v::mix64(ht ^ (((uint64_t)s + 1ULL) * 0x8CB92BA72F3D8DD7ULL));
  return (int32_t)(((r >> 32) * (uint64_t)n) >> 32);
}

__device__ __forceinline__ float clamp4(float v) { return v > 4.0f ? 4.0f : (v < -4.0f ? -4.0f : v); }

__device__ __forceinline__ void move(float2 &y, float c, float dx, float dy, float alpha) {
  const float gx = clamp4(c * dx), gy = clamp4(c * dy);
  const float sx = alpha * gx, sy = alpha * gy;
  y.x = y.x + sx;
  y.y = y.y + sy;
}

__device__ __forceinline__ void attract(float2 &y, float2 o, const Scalars &S) {
  const float dx = y.x - o.x, dy = y.y - o.y;
  const float d2 = __fmaf_rn(dy, dy, dx * dx);
  float c = 0.0f;
  if (d2 > 0.0f) {
    const float pw = S.b == 1.0f ? d2 : powb(d2, S.b);
    const float num = (S.m2ab * pw) / d2;
    c = num / __fmaf_rn(S.a, pw, 1.0f);
  }
  move(y, c, dx, dy, S.alpha);
}

__device__ __forceinline__ void repel(float2 &y, float2 o, const Scalars &S) {
  const float dx = y.x - o.x, dy = y.y - o.y;
  const float d2 = __fmaf_rn(dy, dy, dx * dx);
  if (d2 > 0.0f) {
    const float pw = S.b == 1.0f ? d2 : powb(d2, S.b);
    const float den = (0.001f + d2) * __fmaf_rn(S.a, pw, 1.0f);
    move(y, S.g2b / den, dx, dy, S.alpha);
  } else if (d2 == 0.0f) {
    y.x = y.x + S.alpha4;
    y.y = y.y + S.alpha4;
  }
}

// a lane's row: entries [lo, hi)
__device__ __forceinline__ void lane_chain(const int32_t *__restrict__ col, const float *__restrict__ eps,
                                           const float2 *__restrict__ Y, float2 *__restrict__ Y_next, int64_t i,
                                           int64_t lo, int64_t hi, const Scalars &S) {
  float2 y = Y[i];
  for (int64_t t = lo;; ++t) {
    int32_t j = -1;
    for (; t < hi; ++t) {  // the next entry that fires
      const float e = eps[t];
      const int32_t c = col[t];
      if (fires(e, S) && (uint32_t)c < (uint32_t)S.n) {
        j = c;
        break;
      }
    }
    if (j < 0) break;
    const float2 yj = Y[j];
    const uint64_t ht = entry_stream(S.he, t);
    for (int s0 = 0;; s0 += kAhead) {
      int32_t k[kAhead];
      float2 yk[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        if (s0 + u < S.negative) {
          k[u] = draw(ht, s0 + u, S.n);
          yk[u] = Y[k[u]];
        }
      }
      if (s0 == 0) {
        attract(y, yj, S);
        attract(y, yj, S);
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (s0 + u < S.negative && (int64_t)k[u] != i) repel(y, yk[u], S);
      if (s0 + kAhead >= S.negative) break;
    }
  }
  Y_next[i] = y;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// a wave's row: every lane carries the same y; js, ks, ys are the wave's staging buffers
__device__ __forceinline__ void wave_chain(const int32_t *__restrict__ col, const float *__restrict__ eps,
                                           const float2 *__restrict__ Y, float2 *__restrict__ Y_next, int64_t i,
                                           int64_t lo, int64_t hi, const Scalars &S, int lane, int32_t *js,
                                           int32_t *ks, float2 *ys) {
  const int per = 1 + S.negative;
  const int chunk = kSlots / per < 64 ? kSlots / per : 64;
  float2 y = Y[i];
  for (int64_t t0 = lo; t0 < hi; t0 += chunk) {
    const int cnt = (int)(hi - t0 < (int64_t)chunk ? hi - t0 : (int64_t)chunk);
    wave_sync();  // the chain has read the chunk before
    if (lane < cnt) {
      const float e = eps[t0 + lane];
      const int32_t c = col[t0 + lane];
      js[lane] = (fires(e, S) && (uint32_t)c < (uint32_t)S.n) ? c : -1;
    }
    wave_sync();
    for (int q = lane; q < cnt * per; q += 64) {
      const int en = q / per, s = q - en * per;
      const int32_t j = js[en];
      if (j < 0) continue;
      const int32_t idx = s == 0 ? j : draw(entry_stream(S.he, t0 + en), s - 1, S.n);
      ks[q] = idx;
      ys[q] = Y[idx];
    }
    wave_sync();
    for (int en = 0; en < cnt; ++en) {
      if (__builtin_amdgcn_readfirstlane(js[en]) < 0) continue;
      const float2 yj = ys[en * per];
      attract(y, yj, S);
      attract(y, yj, S);
      for (int s = 1; s < per; ++s)
        if ((int64_t)ks[en * per + s] != i) repel(y, ys[en * per + s], S);
    }
  }
  if (lane == 0) Y_next[i] = y;
}

__global__ __launch_bounds__(kRows) void umap_epoch_kernel(const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ col,
                                                           const float *__restrict__ eps, int64_t nnz,
                                                           const float2 *__restrict__ Y, float2 *__restrict__ Y_next,
                                                           Scalars S) {
  __shared__ int32_t bucket[kBuckets];
  __shared__ int32_t order[kRows];   // the block's lane rows, longest bucket first
  __shared__ int32_t longs[kRows];   // its wave rows
  __shared__ int32_t n_lane, n_wave;
  __shared__ int32_t js[kWaves][64];
  __shared__ int32_t ks[kWaves][kSlots];
  __shared__ float2 ys[kWaves][kSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row0 = (int64_t)blockIdx.x * kRows; row0 < S.n; row0 += (int64_t)gridDim.x * kRows) {
    if (tid < kBuckets) bucket[tid] = 0;
    if (tid == 0) n_wave = 0;
    __syncthreads();
    const int64_t mine = row0 + tid;
    int64_t lo = 0, hi = 0;
    int key = -1;  // no row, or a wave row
    if (mine < S.n) {
      lo = rowptr[mine];
      hi = rowptr[mine + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > nnz ? nnz : hi;
      hi = hi < lo ? lo : hi;
      if (hi - lo > kLong) {
        longs[atomicAdd(&n_wave, 1)] = tid;
      } else {
        key = kBuckets - 1 - (int)(hi - lo) / kBucket;
        atomicAdd(&bucket[key], 1);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int32_t at = 0;
      for (int b = 0; b < kBuckets; ++b) {
        const int32_t c = bucket[b];
        bucket[b] = at;
        at += c;
      }
      n_lane = at;
    }
    __syncthreads();
    if (key >= 0) order[atomicAdd(&bucket[key], 1)] = tid;
    __syncthreads();
    if (tid < n_lane) {
      const int64_t i = row0 + order[tid];
      int64_t rlo = rowptr[i], rhi = rowptr[i + 1];
      rlo = rlo < 0 ? 0 : rlo;
      rhi = rhi > nnz ? nnz : rhi;
      lane_chain(col, eps, Y, Y_next, i, rlo, rhi, S);
    }
    const int nw = n_wave;
    for (int q = wave; q < nw; q += kWaves) {
      const int64_t i = row0 + longs[q];
      int64_t rlo = rowptr[i], rhi = rowptr[i + 1];
      rlo = rlo < 0 ? 0 : rlo;
      rhi = rhi > nnz ? nnz : rhi;
      wave_chain(col, eps, Y, Y_next, i, rlo, rhi, S, lane, js[wave], ks[wave], ys[wave]);
    }
    __syncthreads();  // the next step rewrites the lists
  }
}

__global__ __launch_bounds__(256) void umap_powb_kernel(const float *__restrict__ x, int64_t n, float b,
                                                        float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    out[i] = v > 0.0f ? (b == 1.0f ? v : powb(v, b)) : 0.0f;
  }
}

inline bool finite_positive(float v) { return v > 0.0f && v <= 0x1.fffffep+127f; }
inline bool finite(float v) { return v >= -0x1.fffffep+127f && v <= 0x1.fffffep+127f; }

}  // namespace

extern "C" {

int n2v_umap_epoch(const int64_t *rowptr, const int32_t *col, const float *eps, int64_t nnz, const float *Y,
                   float *Y_next, int64_t n, int32_t epoch, float a, float b, float gamma, float alpha,
                   int32_t negative, uint64_t seed, int32_t max_blocks, void *stream) {
  if (n < 0 || n >= ((int64_t)1 << 31) || nnz < 0 || negative < 0 || negative > kMaxNegative || epoch < 0 ||
      epoch == INT32_MAX || max_blocks < 0 || !finite_positive(a) || !finite_positive(b) || !finite(gamma) ||
      !finite(alpha))
    return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!rowptr || (nnz > 0 && (!col || !eps)) || !Y || !Y_next || Y == Y_next ||
      (((uintptr_t)Y | (uintptr_t)Y_next) & 7))
    return N2V_EINVAL;
  Scalars S;
  S.a = a;
  S.b = b;
  const float ab = a * b, g2 = 2.0f * gamma;
  S.m2ab = -2.0f * ab;
  S.g2b = g2 * b;
  S.alpha = alpha;
  S.alpha4 = alpha * 4.0f;
  S.ep0 = (float)epoch;
  S.ep1 = (float)(epoch + 1);
  S.negative = negative;
  S.he = n2v::mix64(seed ^ n2v::mix64((uint64_t)epoch + 0x9E3779B97F4A7C15ULL));
  S.n = n;
  int64_t blocks = (n + kRows - 1) / kRows;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  // a block per 256 rows unless the caller caps the launch: the blocks that do not fit at once queue, and a block
  // that drew hubs holds up nobody else's rows
  hipLaunchKernelGGL(umap_epoch_kernel, dim3((unsigned)blocks), dim3(kRows), 0, (hipStream_t)stream, rowptr, col, eps,
                     nnz, reinterpret_cast<const float2 *>(Y), reinterpret_cast<float2 *>(Y_next), S);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_umap_powb(const float *x, int64_t n, float b, float *out, void *stream) {
  if (n < 0 || n >= ((int64_t)1 << 40) || !finite_positive(b)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!x || !out) return N2V_EINVAL;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(umap_powb_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, b, out);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
