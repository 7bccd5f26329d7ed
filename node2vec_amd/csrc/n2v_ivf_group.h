// n2v_ivf_group.h -- what the two scans over an inverted-file index share (n2v_ivf.hip: whole rows of X;
// n2v_ivfpq.hip: product-quantised codes): the (query, probe) pairs grouped by list -- count (integer atomics), scan,
// fill -- so that a block takes a tile of pairs of ONE list, and the kernel that empties the partial lists and checks
// the lists' bounds.  The order inside a group is whatever the atomics give, and no result depends on it
// (DESIGN.md "Approximate nearest neighbours").
#pragma once

#include "n2v_topk_select.h"

namespace {

constexpr int kMaxLists = 1024;  // cluster.MAX_K
constexpr int64_t kMaxBlocks = (int64_t)1 << 22;  // blocks of a scan launch at most (512 threads each)

// the grouping tables, cut from a workspace in this order
struct IvfGroups {
  int32_t *cnt, *cursor, *pair_off, *tile_off, *pair_list;
};

inline IvfGroups take_groups(Carver &carve, int32_t nlist, int64_t pairs) {
  IvfGroups g;
  g.cnt = carve.take<int32_t>(nlist * 4);
  g.cursor = carve.take<int32_t>(nlist * 4);
  g.pair_off = carve.take<int32_t>((nlist + 1) * 4);
  g.tile_off = carve.take<int32_t>((nlist + 1) * 4);
  g.pair_list = carve.take<int32_t>(pairs * 4);
  return g;
}

// every slot empty, the groups' counters zero, and the lists' bounds checked: offsets that descend or a list longer
// than max_list_rows set N2V_ST_RANGE (the scan clamps what it reads)
__global__ __launch_bounds__(256) void ivf_prepare_kernel(const int64_t *__restrict__ list_off, int32_t nlist,
                                                          int64_t max_list_rows, int64_t n_entries,
                                                          float *__restrict__ part_s, int32_t *__restrict__ part_r,
                                                          int32_t *__restrict__ cnt, int32_t *__restrict__ cursor,
                                                          uint32_t *__restrict__ status) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = i0; i < n_entries; i += stride) {
    part_s[i] = -INFINITY;
    part_r[i] = kSentinelRow;
  }
  for (int64_t l = i0; l < nlist; l += stride) {
    cnt[l] = 0;
    cursor[l] = 0;
    const int64_t a = list_off[l], b = list_off[l + 1];
    if (a < 0 || b < a || b - a > max_list_rows) atomicOr(status, N2V_ST_RANGE);
  }
}

// a probe is a list number, or -1 for an unused slot; anything else sets N2V_ST_RANGE and is skipped
__device__ inline bool probe_ok(int32_t l, int32_t nlist, uint32_t *status) {
  if (l >= 0 && l < nlist) return true;
  if (l != -1) atomicOr(status, N2V_ST_RANGE);
  return false;
}

// Entry i of probes [n_queries][nprobe] as the scans take it: a list number that no earlier entry of the same query
// names.  A repeated list sets N2V_ST_RANGE and is skipped like a probe out of range, so that a query's slots never
// hold a row twice (merge_kernel relies on it).  Both grouping kernels decide by this one function.
__device__ inline bool probe_taken(const int32_t *__restrict__ probes, int64_t i, int32_t nprobe, int32_t nlist,
                                   uint32_t *status) {
  const int32_t l = probes[i];
  if (!probe_ok(l, nlist, status)) return false;
  for (int64_t j = i - i % nprobe; j < i; ++j)
    if (probes[j] == l) {
      atomicOr(status, N2V_ST_RANGE);
      return false;
    }
  return true;
}

__global__ __launch_bounds__(256) void ivf_count_kernel(const int32_t *__restrict__ probes, int64_t pairs,
                                                        int32_t nprobe, int32_t nlist, int32_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += stride)
    if (probe_taken(probes, i, nprobe, nlist, status)) atomicAdd(&cnt[probes[i]], 1);
}

// pair_off / tile_off: the exclusive sums over the lists of the pairs and of the tiles of qt pairs; one block
__global__ __launch_bounds__(kMaxLists) void ivf_scan_kernel(const int32_t *__restrict__ cnt, int32_t nlist, int32_t qt,
                                                             int32_t *__restrict__ pair_off,
                                                             int32_t *__restrict__ tile_off) {
  __shared__ int32_t sp[kMaxLists], st[kMaxLists];
  const int i = threadIdx.x;
  const int32_t c = i < nlist ? cnt[i] : 0;
  int32_t p = c, t = (c + qt - 1) / qt;
  sp[i] = p;
  st[i] = t;
  __syncthreads();
  for (int off = 1; off < kMaxLists; off <<= 1) {
    const int32_t ap = i >= off ? sp[i - off] : 0, at = i >= off ? st[i - off] : 0;
    __syncthreads();
    p += ap;
    t += at;
    sp[i] = p;
    st[i] = t;
    __syncthreads();
  }
  if (i == 0) pair_off[0] = tile_off[0] = 0;
  if (i < nlist) {
    pair_off[i + 1] = p;
    tile_off[i + 1] = t;
  }
}

__global__ __launch_bounds__(256) void ivf_group_kernel(const int32_t *__restrict__ probes, int64_t pairs,
                                                        int32_t nprobe, int32_t nlist,
                                                        const int32_t *__restrict__ pair_off,
                                                        int32_t *__restrict__ cursor, int32_t *__restrict__ pair_list,
                                                        uint32_t *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += stride)
    if (probe_taken(probes, i, nprobe, nlist, status)) {
      const int32_t l = probes[i];
      pair_list[pair_off[l] + atomicAdd(&cursor[l], 1)] = (int32_t)i;
    }
}

inline unsigned blocks_for(int64_t items) {
  const int64_t b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// the launches that come before a scan: the slots emptied and the bounds checked, then count, scan, fill
inline int launch_groups(const IvfGroups &g, const int64_t *list_off, int32_t nlist, int64_t max_list_rows,
                         const int32_t *probes, int64_t pairs, int32_t nprobe, int32_t qt, int64_t entries,
                         float *part_s, int32_t *part_r, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(ivf_prepare_kernel, dim3(blocks_for(entries)), dim3(256), 0, st, list_off, nlist, max_list_rows,
                     entries, part_s, part_r, g.cnt, g.cursor, status);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ivf_count_kernel, dim3(blocks_for(pairs)), dim3(256), 0, st, probes, pairs, nprobe,
                     nlist, g.cnt, status);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(kMaxLists), 0, st, g.cnt, nlist, qt, g.pair_off, g.tile_off);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ivf_group_kernel, dim3(blocks_for(pairs)), dim3(256), 0, st, probes, pairs, nprobe, nlist,
                     g.pair_off, g.cursor, g.pair_list, status);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

// the list a tile belongs to: tile_off[l] <= tile < tile_off[l + 1] (tile < tile_off[nlist])
__device__ inline int32_t list_of_tile(const int32_t *__restrict__ tile_off, int32_t nlist, int32_t tile) {
  int32_t l = 0, above = nlist;
  while (above - l > 1) {
    const int32_t m = (l + above) >> 1;
    if (tile_off[m] <= tile) l = m;
    else above = m;
  }
  return l;
}

}  // namespace
