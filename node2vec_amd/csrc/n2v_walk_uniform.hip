// n2v_walk_uniform.hip -- K2 exact mode on a unit-weight graph with p == q == 1 (the
// reference's defaults, constants.py:22,26; BASELINE cfg 4).
//
// With every weight 1.0 and p == q == 1 the table generate_edge_alias_tables builds at a
// step (reference randomwalk.py:193-232) has probs == [1.0] * n exactly (the row sum of
// :172 is the integer n, n / n == 1.0, every x / 1.0 == 1.0), no slot is underfull, the loop
// of :182 never runs, and sampling_from_alias(r1, r2) (:86-99) returns pick = int(r1 * n)
// whatever r2 is.  A step is therefore two dependent gathers -- the row pointer pair of the
// current vertex and col[row + pick] -- and the kernel is bound by the chip's rate of random
// 64-byte sector reads (scripts/micro/gather_ceiling.hip: ~25-27 G such steps/s), so what it
// can save is requests:
//   * one LANE per walker, 8 waves per SIMD, nothing else in flight;
//   * the path is NOT stored word by word into its row (a 4-byte store into a 324-byte-pitch row
//     costs a 32-byte write request each, as many requests as the reads).  The rows of the 64
//     walkers of a wave are one contiguous region of walks_out, and the kernel writes that region
//     STEP-MAJOR: position pos of lane l at word pos * cnt + l of the region, one plain dword store
//     per lane per step, 256 contiguous bytes per wave.  walk_chunk_transpose_kernel, launched right
//     behind on the same stream, turns every region row-major in place through LDS (one block per
//     region).  A p = q = 1 walk is therefore TWO kernels, and a kernel trace shows its time as
//     their sum.
//   * walks too long for the transpose tile (walk_length + 1 > kChunkMaxL1) keep the earlier
//     form, in one kernel: every lane holds the 16 words of the 64-byte sector of walks_out it is
//     filling in registers (selected by a v_cndmask chain, no scratch) and stores the sector
//     whole when it is complete -- four aligned 16-byte stores per 16 steps.
//   * with the hop table (n2v_hops_build, 16 bytes per edge: neighbour id + its row pointer
//     and degree) the two dependent gathers of a step become ONE: the entry that names the next
//     vertex also says where its row starts and how long it is.  The chip sustains ~50 G random
//     64-byte sector reads per second whatever the kernel does (profiles/r02_gather_ceiling.log),
//     so halving the sectors per step is the only lever left; it costs 16 B/edge of HBM
//     (12 GB at cfg 4 of 288 GB).
//   * round 4, the degree-ranked form (n2v_graph.rank_hops): the chip serves random 4-byte reads of
//     a 3 GB table at 52 G/s against 40 G/s for 16-byte reads of a 12 GB one (n2v_mem_probe modes
//     1 / 4, profiles/r4x_probe_classes.log), and an entry can be the neighbour's id alone once
//     vertices are numbered by descending degree: rows lie in rank order, so the row of a rank is
//     offset(class) + (rank - first(class)) * degree(class), the class found by a 13-step search of
//     an LDS table (the probe shows the search is free: 51.6 - 53.2 G/s).  The few top ranks whose
//     degrees are all different are looked up in a small cached table instead.
//   * the pair table (n2v_rank_pairs_build, n2v_graph.rank_emit == 2): the ranked form's frame with
//     entries of 8 bytes, {vertex id, rank} of the neighbour.  The low word goes to the path as it is
//     (vertex ids out without the second gather through rank_vertex that costs the 4-byte form a third
//     of its rate), the high word gives the next row through the class search.  Half the bytes of a
//     16-byte hop entry on any graph the ranked form accepts, no escape read: what serves vertex-id
//     output where the field widths of the 8-byte hop table (hops8) do not fit the graph (cfg 4).
// Same uniform stream as every other kernel (step_bits, n2v_common.h): bit-identical walks.
#include "n2v_walk_host.h"

namespace n2v {

// row start and degree of rank x (degree-ranked form): the head table for the top ranks, else the
// degree class of x by a fixed-depth search of the LDS table (first[0] == head_n <= x; the entry
// after the last class and the padding hold n_vertices / n_edges, never <= x).  8 bytes per class:
// its degree is (offset of the next class - its own) / (its number of ranks).
__device__ __forceinline__ void rank_row(const n2v_graph &g, const uint32_t *first, const uint32_t *off,
                                         uint32_t x, int64_t &vb, int &n) {
  if (x < (uint32_t)g.rank_head_n) {
    const uint64_t e = g.rank_head[x];
    vb = (int64_t)(e & N2V_HOP_ROW_MASK);
    n = (int)(e >> N2V_HOP_DEG_SHIFT);
    return;
  }
  int c = 0;
  for (int half = g.rank_classes >> 1; half > 0; half >>= 1)
    if (first[c + half] <= x) c += half;
  const uint32_t f0 = first[c], o0 = off[c];
  const uint32_t d = (off[c + 1] - o0) / (first[c + 1] - f0);
  n = (int)d;
  vb = (int64_t)(o0 + (x - f0) * d);  // < n_edges < 2^32
}

// The transpose tile of a full region is 64 * L1 words of LDS: 64 KB at L1 == 256, the most a block
// may ask for.  Longer walks take the register-sector path.
constexpr int kChunkMaxL1 = 256;

// Where the words of a path go.  The step-major form: the region of the wave that starts at walker
// `base` holds cnt = min(64, total - base) rows of L1 words, position pos of lane l at word
// pos * cnt + l of it.
template <bool kChunked>
struct path_writer;

template <>
struct path_writer<true> {
  int32_t *at;  // this lane's word of position 0
  int cnt;
  __device__ __forceinline__ path_writer(int32_t *walks_out, int64_t base, int64_t total, int L1, int lane,
                                         int64_t)
      : at(walks_out + base * (int64_t)L1 + lane), cnt((int)(total - base < 64 ? total - base : 64)) {}
  __device__ __forceinline__ void put(int pos, int32_t x, int) { at[pos * cnt] = x; }  // pos * cnt < 2^14
};

// The row-major form without a second kernel: word a of walks_out lives in buf[a & 15] until its
// 64-byte sector (or the row) is complete, and is then stored with it.
template <>
struct path_writer<false> {
  int32_t *walks_out;
  int64_t w0;  // absolute word index of path position 0
  int lo;      // first word of the current sector that belongs to this row
  bool base_aligned;  // whole sectors need a 64-byte aligned output base (torch / hipMalloc give >= 256)
  int32_t buf[16];
  __device__ __forceinline__ path_writer(int32_t *out, int64_t, int64_t, int L1, int, int64_t r)
      : walks_out(out), w0(r * (int64_t)L1), lo((int)((r * (int64_t)L1) & 15)),
        base_aligned((reinterpret_cast<uintptr_t>(out) & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) buf[k] = -1;
  }
  __device__ __forceinline__ void put(int pos, int32_t x, int walk_length) {
    const int64_t a = w0 + pos;
    const int k = (int)(a & 15);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) buf[kk] = (k == kk) ? x : buf[kk];
    if (k != 15 && pos != walk_length) return;
    // words [sector(a) + lo, a] are complete: store them
    int32_t *sec = walks_out + (a & ~(int64_t)15);
    if (lo == 0 && k == 15 && base_aligned) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        reinterpret_cast<int4 *>(sec)[u] =
            make_int4(buf[4 * u], buf[4 * u + 1], buf[4 * u + 2], buf[4 * u + 3]);
    } else {
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
        if (kk >= lo && kk <= k) sec[kk] = buf[kk];
    }
    lo = 0;
  }
};

// kHops: 0 = CSR arrays (two gathers per step), 1 = the 16-byte hop table, 2 = the 8-byte hop
// table (round 3: the chip serves 8-byte gathers over a table half the size a quarter faster),
// 3 = the degree-ranked 4-byte table (blocks of 1024 threads, the class table in LDS: up to 8191
// classes in 64 KB, two blocks per CU), 4 = the same frame on the 8-byte {vertex id, rank} pair table
// (g.rank_hops points at uint64 entries; vertex ids out)
//
// kChunked: the step-major region per wave (walk_chunk_transpose_kernel must follow); otherwise
// whole sectors of the row-major output from registers
template <int kHops, int kThreads, bool kChunked>
__global__ __launch_bounds__(kThreads, 8) void walk_uniform_kernel(
    n2v_graph g, const int32_t *__restrict__ start_ids, int64_t n_start, int32_t num_walks,
    int32_t walk_length, uint64_t seed, int32_t *__restrict__ walks_out,
    uint8_t *__restrict__ valid_out, uint32_t *__restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t total = n_start * (int64_t)num_walks;
  const int L1 = walk_length + 1;
  extern __shared__ uint32_t rank_lds[];
  const uint32_t *cls_first = rank_lds;
  const uint32_t *cls_where = rank_lds + (kHops >= 3 ? g.rank_classes : 0);
  if (kHops >= 3) {
    for (int c = threadIdx.x; c < g.rank_classes; c += kThreads) {
      rank_lds[c] = g.rank_class_first[c];
      rank_lds[g.rank_classes + c] = g.rank_class_off[c];
    }
    __syncthreads();
  }
  const bool emit_rank = kHops == 3 && g.rank_emit != 0;
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&status[1], 64u);
    const int64_t base = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (base >= total) break;
    const int64_t r = base + lane;
    const bool have = r < total;
    int32_t v = -1;
    uint64_t h0 = 0;
    bool alive = have;
    if (have) {
      v = start_ids[r / num_walks];
      const int32_t ordinal = (int32_t)(r % num_walks) + 1;
      h0 = walker_stream(seed, (uint64_t)v * (uint64_t)num_walks + (uint64_t)(ordinal - 1));
      if (v < 0 || (int64_t)v >= g.n_vertices) {
        atomicOr(status, N2V_ST_RANGE);
        alive = false;
      }
    }
    int64_t vb = 0;
    int n = 0;
    int32_t v_emit = v;
    if (kHops >= 3) {
      if (alive) {
        const int32_t rk = g.rank_of[v];
        if (emit_rank) v_emit = rk;
        rank_row(g, cls_first, cls_where, (uint32_t)rk, vb, n);
        alive = n > 0;  // fugue.py:132
      }
    } else if (alive) {
      vb = g.rowptr[v];
      n = (int)(g.rowptr[v + 1] - vb);
      alive = n > 0;  // fugue.py:132
      if (kHops == 2 && g.hop8_rowptr) vb = g.hop8_rowptr[v];  // the padded table's own row start
    }
    bool walking = alive;
    // the path: position pos of this lane's row
    auto emit = path_writer<kChunked>(walks_out, base, total, L1, lane, r);
    if (have) emit.put(0, alive ? v_emit : -1, walk_length);
    for (int step = 0; step < walk_length; ++step) {
      if (ballot64(have) == 0ull) break;
      int32_t x = -1;
      if (walking) {
        const uint64_t bits = step_bits(h0, (uint32_t)step);
        const int pick = pick_index((uint32_t)(bits >> 32), n);  // int(r1 * n); r2 is irrelevant
        if (kHops == 4) {
          const uint64_t e = reinterpret_cast<const uint64_t *>(g.rank_hops)[vb + pick];
          x = (int32_t)(uint32_t)e;  // the neighbour's vertex id; its rank names the next row
          if (step + 1 < walk_length) rank_row(g, cls_first, cls_where, (uint32_t)(e >> 32), vb, n);
        } else if (kHops == 3) {
          const uint32_t xr = g.rank_hops[vb + pick];
          x = emit_rank ? (int32_t)xr : g.rank_vertex[xr];
          if (step + 1 < walk_length) rank_row(g, cls_first, cls_where, xr, vb, n);
        } else if (kHops == 2) {
          const uint64_t h = g.hops8[vb + pick];
          const int cb = g.hop8_col_bits, rb = g.hop8_row_bits;
          x = (int32_t)(h & ((1ull << cb) - 1ull));
          vb = (int64_t)(((h >> cb) & ((1ull << rb) - 1ull)) << g.hop8_align_shift);
          const uint64_t code = h >> (cb + rb), esc = (1ull << (64 - cb - rb)) - 1ull;
          n = (int)code;
          // a high-degree row: its degree is read from rowptr (few such rows: cached)
          if (code == esc) n = (int)(g.rowptr[x + 1] - g.rowptr[x]);
        } else if (kHops == 1) {
          const n2v_hop h = load_hop(g.hops + vb + pick);
          x = h.col;
          vb = hop_row(h);
          n = hop_deg(h);
        } else {
          x = g.col[vb + pick];
          if (step + 1 < walk_length) {
            vb = g.rowptr[x];
            n = (int)(g.rowptr[x + 1] - vb);
          }
        }
        // fugue.py:147: the walker vanishes at a sink, the rest of its row is -1
        if (step + 1 < walk_length && n == 0) {
          walking = false;
          alive = false;
        }
      }
      if (have) emit.put(step + 1, x, walk_length);
    }
    if (have) valid_out[r] = alive ? 1 : 0;
  }
}

// Turns the step-major region of every wave of walk_uniform_kernel<.., true> row-major, in place: a
// block per region at a time (a resident grid whose blocks take regions in turn), the region's
// cnt * L1 words through LDS (dynamic, 4 * 64 * L1 bytes).  Dword accesses to walks, so an output
// base aligned to 4 bytes serves.  A full region's row is rotated on its way into LDS: (pos, l) lies
// at pos * 64 + ((l * m + pos) & 63) with m = L1 | 1.  m is odd, so the 32 lanes of a ds_write
// group, which share pos and hold consecutive l, fall on 32 different banks; on the way out lane i
// reads (pos, row) = (i % L1, i / L1) from bank (row * m + pos) % 32, which is i % 32 for an odd L1
// (no conflict at all, the headline's 81) and (i + row) % 32 for an even one (two lanes of a group
// share a bank where the group crosses into its next row).  The one partial region of a launch is
// not rotated (64 would have to be cnt, and l -> l * m % cnt a bijection).  A thread moves its words
// kBatch at a time, all loads of a batch issued before the first is used.  The kernel reads and
// writes every word of walks_out once (2 x 3.4 GB at the headline) and runs at the HBM rate.
constexpr int kTransposeThreads = 256, kTransposeBatch = 8;

template <int kThreads, int kBatch>
__global__ __launch_bounds__(kThreads) void walk_chunk_transpose_kernel(int32_t *__restrict__ walks,
                                                                        int64_t total, int32_t L1) {
  extern __shared__ int32_t tile[];
  const int m = L1 | 1;
  const int row0 = (int)threadIdx.x / L1, pos0 = (int)threadIdx.x % L1;
  const int drow = kThreads / L1, dpos = kThreads % L1;
  int32_t x[kBatch];
  for (int64_t base = (int64_t)blockIdx.x * 64; base < total; base += (int64_t)gridDim.x * 64) {
    const int cnt = (int)(total - base < 64 ? total - base : 64);
    int32_t *region = walks + base * (int64_t)L1;
    const int n = cnt * L1;
    const bool full = cnt == 64;
    for (int i0 = threadIdx.x; i0 < n; i0 += kThreads * kBatch) {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kThreads;
        x[u] = i < n ? region[i] : 0;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kThreads;
        const int pos = i >> 6, l = i & 63;
        if (i < n) tile[full ? (pos << 6) + ((l * m + pos) & 63) : i] = x[u];
      }
    }
    __syncthreads();
    int row = row0, pos = pos0;
    for (int i0 = threadIdx.x; i0 < n; i0 += kThreads * kBatch) {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        x[u] = i0 + u * kThreads < n ? tile[pos * cnt + (full ? ((row * m + pos) & 63) : row)] : 0;
        row += drow;
        pos += dpos;
        if (pos >= L1) {
          pos -= L1;
          ++row;
        }
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kThreads;
        if (i < n) region[i] = x[u];
      }
    }
    __syncthreads();  // the tile is free for the block's next region
  }
}

template <int kHops, int kThreads>
static auto uniform_instance(bool chunked) {
  return chunked ? walk_uniform_kernel<kHops, kThreads, true> : walk_uniform_kernel<kHops, kThreads, false>;
}

// `form`: the table that serves (the dispatcher checked its fields) -- 4 the 8-byte {id, rank} pairs, 3 the 4-byte
// ranks, 2 hops8, 1 hops, 0 rowptr and col
int launch_walk_uniform(const WalkArgs &a, int form) {
  const int L1 = a.walk_length + 1;
  const bool chunked = L1 <= kChunkMaxL1;
  const auto kernel = form == 4   ? uniform_instance<4, 1024>(chunked)
                      : form == 3 ? uniform_instance<3, 1024>(chunked)
                      : form == 2 ? uniform_instance<2, 256>(chunked)
                      : form == 1 ? uniform_instance<1, 256>(chunked)
                                  : uniform_instance<0, 256>(chunked);
  const int threads = form >= 3 ? 1024 : 256;
  const size_t lds = form >= 3 ? (size_t)a.g->rank_classes * 8 : 0;
  const int64_t total = a.total();
  if (launch_resident(kernel, threads, lds, (total + threads - 1) / threads, a.stream, *a.g, a.start_ids, a.n_start,
                      a.num_walks, a.walk_length, a.seed, a.walks_out, a.valid_out, a.status) != hipSuccess)
    return N2V_ELAUNCH;
  if (!chunked) return N2V_OK;
  // the regions the walk kernel wrote step-major, row-major in place: walks_out is complete when the
  // stream has passed this second kernel
  return launch_status(launch_resident(walk_chunk_transpose_kernel<kTransposeThreads, kTransposeBatch>,
                                       kTransposeThreads, (size_t)64 * (size_t)L1 * sizeof(int32_t),
                                       (total + 63) / 64 /* < 2^26 */, a.stream, a.walks_out, total, L1));
}

}  // namespace n2v
