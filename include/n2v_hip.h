/*
 * n2v_hip.h -- C ABI of libn2v_hip.so, the MI355X (gfx950) node2vec hot path.
 *
 * The reference (graph-embedding/node2vec, node2vec-fugue 0.3.5) is pure Python
 * and has no FFI of its own; the hot path sits behind Python interfaces
 * (SURVEY.md 8b).  This header is the boundary a maintainer of the reference
 * binds to replace that path (ctypes stub: INTEGRATION.md).  Each entry point
 * cites the reference code it replaces, file:line relative to the reference.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA storage) unless
 *    its name ends in _host; the caller owns all buffers;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls
 *    only enqueue work, they never synchronise and never allocate;
 *  - return value: N2V_OK or a negative N2V_E* code for argument / launch
 *    errors detected on the host; data-dependent errors (the reference's
 *    ZeroDivisionError) are OR-ed into the device word status[0] as N2V_ST_*
 *    bits, to be read by the caller after it synchronises.  `status` points to
 *    FOUR uint32 words, zeroed by the caller: [0] status bits, [1] scratch (the exact walk
 *    kernels hand out walkers through it; the library resets it on the stream before a launch),
 *    [2..3] a 64-bit counter that N2V_WALK_FAST increments by its number of
 *    trials (draws, accepted or not; for the algorithmic-bytes accounting of DESIGN.md);
 *  - no global state: re-entrant, any number of streams / devices.
 */
#ifndef N2V_HIP_H
#define N2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define N2V_ABI_VERSION 15

#define N2V_OK 0
#define N2V_EINVAL (-1)  /* maps to ValueError (randomwalk.py:212-217)      */
#define N2V_ELAUNCH (-2) /* HIP launch / runtime error -> RuntimeError      */
#define N2V_ENOGPU (-3)

/* bits of the device status word */
#define N2V_ST_ZERODIV 1u /* sum(weights) == 0: ZeroDivisionError, randomwalk.py:172-173 */
#define N2V_ST_RANGE 2u   /* a start id outside [0, n_vertices)                          */
#define N2V_ST_OVERFLOW 4u /* n2v_partition_forward: a mailbox or the word pool was too small */

/* walk sampler modes */
#define N2V_WALK_EXACT 0 /* per-step biased alias rebuild, bit-identical to the reference */
#define N2V_WALK_FAST 1  /* same transition distribution, not the same draws: on a unit-weight graph
                          * with edge_classes + wedge_off / wedge_pos a step is ONE draw from the
                          * layers of its table (no rejection at q >= 1 with p <= q); otherwise
                          * candidates from the first-order table are rejected by beta / beta_max */

/* One entry of a first-order Walker alias table, packed so that a draw is ONE
 * 16-byte access: the neighbour id, the neighbour id BEHIND the alias index of
 * generate_alias_tables (row[alias[i]], randomwalk.py:140-141 looks it up the same
 * way) and the pseudo-probability (randomwalk.py:157-190). */
typedef struct n2v_slot {
  int32_t col;
  int32_t alias; /* vertex id, not an index */
  double prob;
} n2v_slot;

/* One entry of the hop table (optional, unit-weight graphs; n2v_hops_build): everything a
 * walker needs once it has chosen edge e = (v -> x), in ONE 16-byte access -- the neighbour
 * id, the class counts of that edge (edge_classes[e], needed at the walker's next step) and
 * the row of x: rowptr[x] in the low 40 bits, the out-degree of x in the high 24.  The
 * reference fetches the same facts by two joins per step (fugue.py:146-148); on the GPU each
 * would be a dependent random gather, and random 64-byte sectors per step are what bounds the
 * walk kernels (DESIGN.md "K2").  Costs 16 bytes per edge of HBM. */
typedef struct n2v_hop {
  int32_t col;
  uint32_t classes; /* layout of edge_classes[]; all ones = unknown (the kernels classify) */
  uint64_t row;     /* rowptr[col] | (uint64_t)degree(col) << 40 */
} n2v_hop;
#define N2V_HOP_DEG_SHIFT 40
#define N2V_HOP_ROW_MASK 0xffffffffffull

/* The reference's adjacency DataFrame df_adj (fugue.py:130, randomwalk.py:266-275)
 * as CSR in HBM: one row per vertex id, neighbours sorted by dst ascending,
 * multi-edges kept.  Weights: the reference carries Python floats (randomwalk.py:20,
 * indexer.py:24), so `w64` holds them as fp64; `w` is the 4-byte form for weights that are
 * exactly representable in fp32 (same bits after widening); at most one of the two is set,
 * both NULL = every weight is 1.0 (what index_graph_* produces, indexer.py:20-21) and the
 * walk kernels never read weights.
 * `slots` holds the per-row first-order alias tables written by n2v_alias_build,
 * CSR-aligned (N2V_WALK_FAST on weighted graphs; exact walks with p == q == 1 on weighted
 * graphs).  `pivots` is an optional search index over `col` written by n2v_pivots_build
 * (NULL = plain binary search): the test "x in N_out(src)" of randomwalk.py:226 then
 * touches 2-3 cache lines instead of log2(degree).  `edge_classes` (unit-weight graphs,
 * optional) is written by n2v_edge_classes_build: per edge e = (s -> v) the class counts
 * of the table generate_edge_alias_tables builds at (s, v) -- see there.  `hops` (unit-weight
 * graphs, optional) is written by n2v_hops_build; with it a step of the p == q == 1, the
 * class-count and the rejection kernels is one gather instead of two or three. */
typedef struct n2v_graph {
  int64_t n_vertices;
  int64_t n_edges;
  const int64_t *rowptr; /* [n_vertices + 1] */
  const int32_t *col;    /* [n_edges] */
  const float *w;        /* [n_edges] fp32 storage, or NULL */
  const double *w64;     /* [n_edges] fp64 storage, or NULL */
  const n2v_slot *slots; /* [n_edges] or NULL */
  const int32_t *pivots; /* [(n_edges + 31) / 32]: col[min(32 j + 31, n_edges - 1)], or NULL */
  const uint32_t *edge_classes; /* [n_edges] or NULL */
  const struct n2v_hop *hops;   /* [n_edges] or NULL (unit-weight graphs) */
  const uint64_t *wedge_off;    /* [n_edges] or NULL: see n2v_wedge_build */
  const void *wedge_pos;        /* uint16 / uint32 positions, or NULL */
  int32_t wedge_wide;           /* 0: wedge_pos is uint16 (every degree < 65536), 1: uint32,
                                   T >= 2 (mixed; 65536 in production): the lists of the edges INTO a row
                                   of T entries or more are uint32 and lie behind the uint16 lists of all
                                   other edges -- see n2v_wedge_build */
  int32_t reserved;             /* 0 (diagnostics: N2V_DIAG_NO_TABLES_KERNEL = do not use the all-tables kernel,
                                   N2V_DIAG_NO_SLOTS_KERNEL = do not use wedge_slots) */
  const uint64_t *hops8;        /* the 8-byte hop table (n2v_hops8_build) or NULL */
  int32_t hop8_col_bits;        /* field widths of a hops8 entry, see n2v_hops8_build */
  int32_t hop8_row_bits;
  const int64_t *hop8_rowptr;   /* [n_vertices + 1] row starts of the hops8 table when its rows are
                                   padded (hop8_align_shift > 0), else NULL (= rowptr) */
  int32_t hop8_align_shift;     /* rows of the hops8 table start at multiples of 2^shift entries */
  int32_t reserved2;            /* bit 0 (N2V_HOPS_INLINE_RPOS): the class words of `hops` carry inline
                                   return positions, see n2v_hops_build; bit 1 (N2V_SLOTS_FOLDED): see
                                   n2v_wedge_slots_fold; else 0 */
  const uint16_t *wedge_slots;  /* [n_edges][16] or NULL: see n2v_wedge_slots_build */
  /* The degree-ranked form of a unit-weight graph (p == q == 1 walks; n2v_rank_hops_build), or all
   * NULL / 0.  Vertices are numbered again by descending degree (`rank`), rows are laid out in rank
   * order, so the row of a rank follows from the DEGREE CLASS the rank falls in and an entry of the
   * table is the 4-byte rank of the neighbour alone: a step is one 4-byte gather.
   * The pair table (n2v_rank_pairs_build) is the same layout with 8-byte entries
   * (uint64_t)rank << 32 | vertex id: a walk that writes VERTEX IDS in one 8-byte gather per step, on any
   * graph the ranked form accepts.  A caller passes it through the same fields: rank_hops points at the
   * uint64 entries and rank_emit is 2 (rank_vertex is not read). */
  const uint32_t *rank_hops;        /* [n_edges]: rank of every neighbour; rows in rank order, the entries
                                       of a row in the CSR's order (so pick = int(r1 * n) is unchanged).
                                       rank_emit == 2: const uint64_t [n_edges], the pair table */
  const int32_t *rank_of;           /* [n_vertices]: vertex id -> rank */
  const int32_t *rank_vertex;       /* [n_vertices]: rank -> vertex id */
  const uint64_t *rank_head;        /* [rank_head_n]: row offset | degree << 40 of ranks below rank_head_n
                                       (the few top vertices whose degrees are all different) */
  const uint32_t *rank_class_first; /* [rank_classes]: first rank of every degree class of the ranks from
                                       rank_head_n on, ascending, [0] == rank_head_n; then n_vertices in
                                       the entry after the last class and in the padding */
  const uint32_t *rank_class_off;   /* [rank_classes]: offset in rank_hops of the row of that first rank
                                       (n_edges after the last class; the form needs n_edges < 2^32).
                                       The degree of class c is (off[c+1] - off[c]) / (first[c+1] - first[c]) */
  int32_t rank_head_n;              /* 0 .. 2^22 */
  int32_t rank_classes;             /* a power of two, 2 .. 8192, > the number of classes (the walk kernel
                                       keeps both arrays in LDS: 8 bytes per class) */
  int32_t rank_emit;                /* what the ranked kernel writes to walks_out: 0 = vertex ids (one more
                                       gather per token through rank_vertex), 1 = ranks (the caller
                                       composes rank_vertex into its own per-token lookup, as
                                       n2v_corpus_index's index_of), 2 = vertex ids, and rank_hops points
                                       at the 8-byte pair table of n2v_rank_pairs_build (no second
                                       gather).  Any other value: N2V_EINVAL */
  int32_t reserved3;                /* 0 */
  /* Row sums of the tables of the steps into LONG rows, for ONE (p, q) whose 1/p or 1/q is not dyadic
   * (n2v_edge_row_sums_build; ABI 15), or NULL / 0.  The walk kernels ignore the table unless row_sums_p / _q are
   * the p, q of the walk. */
  const double *row_sums;           /* [n_edges]; valid for the edges into rows of >= row_sums_from entries */
  double row_sums_p;
  double row_sums_q;
  int32_t row_sums_from;
  int32_t reserved4;                /* 0 */
} n2v_graph;

/* edge_classes[e] for e = (s -> v): bits 0..23 = number of entries x of N(v) with
 * x in N_out(s) and x != s ("shared", randomwalk.py:226-227), bits 24..31 = number of
 * entries of N(v) equal to s ("return", :223-224); a field that does not fit is stored
 * saturated (all ones) and the kernels then classify the row themselves. */
#define N2V_EC_SHARED_MASK 0x00ffffffu
#define N2V_EC_RETURN_SHIFT 24
#define N2V_EC_RETURN_SAT 0xffu
/* Inside a hop table built with N2V_HOPS_INLINE_RPOS (never in edge_classes[]): an edge WITHOUT
 * shared neighbours stores  N2V_EC_INLINE | return count (7 bits) << 24 | return position (24
 * bits)  -- the one thing a step that runs the pairing loop still needs of such an edge, so that it
 * does not fetch the edge's wedge slot for it (half of the edges of cfg 4, all of cfg 5). */
#define N2V_EC_INLINE 0x80000000u
#define N2V_HOPS_INLINE_RPOS 1
/* bit 1 of reserved2 (ABI 15): the wedge slots of the edges into rows of wedge_wide .. wedge_wide + 65536 entries are
 * FOLDED slots (n2v_wedge_slots_fold) -- the exact slots kernel then steps those rows like every other */
#define N2V_SLOTS_FOLDED 2
/* the diagnostic bits of `reserved`: an exact biased walk on a unit-weight graph that carries every per-edge table
 * keeps the tables but walks with another kernel (same walks, bit for bit) */
#define N2V_DIAG_NO_TABLES_KERNEL 1 /* bit 0: not the all-tables kernels (a lane per walker, no step needs the wave) */
#define N2V_DIAG_NO_SLOTS_KERNEL 2  /* bit 1: not the one of them that reads wedge_slots */

int n2v_abi_version(void);
const char *n2v_status_string(int code);

/* Number of GPUs visible to the library (no GPU initialisation side effects
 * beyond hipGetDeviceCount). */
int n2v_device_count(void);

/* K1 -- first-order alias tables for every row, exactly
 * generate_alias_tables(weights of the row) (randomwalk.py:157-190): same LIFO
 * pairing order, fp64 arithmetic, leftovers keep alias 0 (= the row's first
 * neighbour).  Rows of degree 0 are skipped; a row whose weights sum to 0 sets
 * N2V_ST_ZERODIV.  slots_out is CSR-aligned ([n_edges]); slot.alias holds the
 * neighbour id the alias index points to, slot.col a copy of col. */
int n2v_alias_build(const n2v_graph *g, n2v_slot *slots_out, uint32_t *status,
                    void *stream);

/* Per-edge class counts for exact walks on a unit-weight graph (g->w == g->w64 == NULL).
 * The table generate_edge_alias_tables builds for a step (s -> v) (randomwalk.py:219-231)
 * is a function of the EDGE (s, v) only, and with unit weights its row sum (:172) and the
 * value probs[i] of every slot before the pairing (:173) follow from two counts: how many
 * neighbours of v are s itself and how many are out-neighbours of s.  The reference
 * recomputes them (a set intersection) at every step; this pass computes them once per
 * edge -- one wave per source row, the shorter list searched in the longer -- and
 * N2V_WALK_EXACT then decides most steps from {rowptr[v], classes[e], col[pick], one
 * membership test}, bit-identical to the per-step rebuild, and only rebuilds the class
 * layout of a row when the pairing loop (:182-189) actually has to run for slot `pick`.
 * classes_out: [n_edges] uint32, layout above.  status: the four words described at the
 * top (word [1] is the kernel's batch counter). */
int n2v_edge_classes_build(const n2v_graph *g, uint32_t *classes_out, uint32_t *status,
                           void *stream);

/* Hop table of a unit-weight graph (struct n2v_hop above): hops_out[e] = {col[e],
 * g->edge_classes ? g->edge_classes[e] : all ones, rowptr[col[e]] | degree(col[e]) << 40}.
 * With g->wedge_off set and g->reserved2 & N2V_HOPS_INLINE_RPOS the class word of an edge whose
 * shared count is 0 is written in the N2V_EC_INLINE form (every return count must be below 128,
 * else N2V_ST_RANGE); such a table serves the wedge-slots kernel of N2V_WALK_EXACT and
 * N2V_WALK_FAST, and n2v_walk returns N2V_EINVAL when it would have to hand it to another exact
 * kernel -- build the plain form for those (the table takes milliseconds).
 * N2V_EINVAL when the graph has weights or 2^40 edges or more; a row of 2^24 entries or more
 * sets N2V_ST_RANGE in status[0] (read after synchronising): the table must then be discarded
 * (walk without it). */
int n2v_hops_build(const n2v_graph *g, struct n2v_hop *hops_out, uint32_t *status, void *stream);

/* The 8-byte hop table of a unit-weight graph for exact walks with p == q == 1 (no class counts
 * needed).  Row v of the table starts at entry T[v] = hop8_rowptr ? hop8_rowptr[v] : rowptr[v] (a
 * multiple of 2^align_shift) and holds, for the k-th neighbour x of v,
 *   x | (T[x] >> align_shift) << col_bits | code << (col_bits + row_bits),
 * code = min(degree(x), 2^(64 - col_bits - row_bits) - 1); the top code is an escape: the degree is
 * then read from rowptr (the few high-degree rows: cache-resident).  The chip delivers ~50 G random
 * 8-byte gathers per second against ~40 G 16-byte gathers over the table of n2v_hops_build
 * (profiles/r3v_probe_gathers.log), and a walk step of this kernel IS one such gather.  Padding
 * the rows (align_shift 3) frees three bits of the row field for the degree code: at cfg 4
 * (27-bit ids) 9 bits instead of 7, so that the escape rows' rowptr entries fit the L2.
 * Requires n_vertices <= 2^col_bits, (table entries >> align_shift) < 2^row_bits and
 * col_bits + row_bits <= 62 (N2V_EINVAL otherwise).  hops8_out: [T[n_vertices]] uint64. */
int n2v_hops8_build(const n2v_graph *g, int32_t col_bits, int32_t row_bits, int32_t align_shift,
                    const int64_t *hop8_rowptr, uint64_t *hops8_out, void *stream);

/* Shared-position lists ("wedge table") of a graph (weights play no part).  For edge e = (s -> v) the list
 *   wedge_pos[off .. off + n_shared)   off = wedge_off[e] & (2^40 - 1), n_shared = low 24 bits
 *                                      of edge_classes[e]
 * holds, ascending, the positions j with N(v)[j] in N_out(s) and N(v)[j] != s -- WHICH slots of
 * the table generate_edge_alias_tables builds at (s, v) carry the unchanged weight
 * (randomwalk.py:226-227) -- and wedge_off[e] >> 40 is the position of the first N(v)[j] == s
 * (the weight / p slots, :223-224; meaningful when the return count of edge_classes[e] is not
 * 0).  With them N2V_WALK_EXACT needs neither a search over N(s) nor a pass over N(v) to lay
 * the table of a step out: the membership test of the drawn slot is a search in its edge's
 * short list, and the steps that must run the pairing loop (:182-189) read the class of every
 * slot off the list.  One entry per (edge, common neighbour) pair: six per triangle.
 *   list_off      [n_edges] exclusive prefix sum of the shared counts (the caller's cumsum over
 *                 edge_classes & N2V_EC_SHARED_MASK); may be the same buffer as wedge_off_out
 *   wedge_pos_out [sum of the counts] uint16 when wide == 0 (every out-degree < 65536), uint32
 *                 when wide == 1.  wide == T >= 2 (T <= 65536; "mixed"): the list of an edge into a
 *                 row of fewer than T entries is uint16, offsets in uint16 units; the list of an
 *                 edge into a row of T entries or more ("wide row": its positions need more than 16
 *                 bits) is uint32, offsets in uint32 units from the same base, and the caller lays
 *                 those lists behind all the uint16 ones (list_off says where, per edge).  A walker
 *                 knows the degree of the row it stands on, so it knows the width of the list it
 *                 reads: a few hubs (the reference caps rows at 100 000, constants.py:6) cost the
 *                 other rows nothing.  The same value goes into n2v_graph.wedge_wide.
 * g->edge_classes must be set.  A list whose length disagrees with its count sets
 * N2V_ST_RANGE in status[0] (the tables must then be discarded). */
#define N2V_WEDGE_RPOS_SHIFT 40
#define N2V_WEDGE_OFF_MASK 0xffffffffffull
int n2v_wedge_build(const n2v_graph *g, const uint64_t *list_off, uint64_t *wedge_off_out,
                    void *wedge_pos_out, int32_t wide, uint32_t *status, void *stream);

/* Wedge slots: the wedge table laid out so that a biased exact step finds the list of the edge it
 * came along with ONE gather at a place it knows a step ahead (slot e = edge index), requested
 * together with the hop entry, instead of wedge_off[e] and then the list behind that offset (two
 * dependent gathers; random 64-byte sectors per step are what bounds the walk kernels).  32 bytes
 * = 16 halfwords per edge:
 *   [0] return position (wedge_off[e] >> 40)   [1] number of list entries below the return position
 *   n_shared <= 14:  [2 .. 2 + n_shared) the list itself
 *   n_shared  > 14:  [4 .. 8) the list's offset in wedge_pos as 64 bits, [8 .. 16) eight pivots
 *                    list[((k + 1) * n_shared) / 9], k = 0 .. 7 (the search enters the right ninth)
 * 16-bit positions only (wedge_wide == 0, or mixed: the slots of the edges into wide rows are left
 * zero and never read -- those steps go through wedge_off); g->edge_classes, g->wedge_off and g->wedge_pos must be
 * set.  At cfg 4 half of the steps need a list and four fifths of those lists are short.
 * slots_out: [n_edges * 16] uint16. */
int n2v_wedge_slots_build(const n2v_graph *g, uint16_t *slots_out, void *stream);

/* Folded lists and slots for the edges into WIDE rows of a mixed wedge table (ABI 15).  The reference trims rows at
 * 100 000 (constants.py:6), so the rows of its hubs hold positions that need 17 bits.  The mixed table keeps the lists
 * of the edges into such rows as uint32 without a slot, and a walker standing there took its step through a second,
 * 32-bit instance of the step (wedge_off, then the list): a wave pays for every code path ONE of its lanes takes, and
 * on cfg 4 trimmed at 100 000 nearly every wave-step has such a lane.  A FOLDED list stores a position below
 * T = wedge_wide as it is and one from T on minus T, in the same order -- both parts ascend, entry k is
 * list[k] + (k >= nlow ? T : 0) with nlow the number of entries below T, and a lower bound is one search in one part --
 * so it is a uint16 list like every other (rows of up to T + 65536 entries), gets a slot like every other, and the
 * exact slots kernel steps such a row with the same instructions as the rest:
 *   n_shared <= 14:  [0] return position (folded)  [1] below | nlow << 4 | upper << 8 (upper: the return position is
 *                    >= T)  [2 .. 2 + n_shared) the folded list
 *   n_shared  > 14:  [0] return position (folded)  [1] below, [2] nlow (low 16 bits)  [3] upper | (below >> 16) << 4 |
 *                    (nlow >> 16) << 8  [4 .. 8) offset of the folded copy in wedge_pos (2-byte units)  [8 .. 16) eight
 *                    pivots of the folded copy, as in n2v_wedge_slots_build
 * g: a graph with a mixed table (wedge_wide = T >= 2), edge_classes, wedge_off, wedge_pos set; fold_off [n_edges]:
 * where the folded copy of edge e's list goes (2-byte units from wedge_pos; read for the edges into rows of T ..
 * T + 65536 entries with more than 14 shared neighbours only); wedge_pos_rw == g->wedge_pos (the caller's buffer, with
 * room behind the uint32 lists); slots [n_edges * 16] as n2v_wedge_slots_build left them (the slots of those edges
 * are rewritten).  The uint32 lists stay: every other kernel reads them.  Set N2V_SLOTS_FOLDED in reserved2 to have
 * the slots kernel use the result; without the bit the same walks come out of the 32-bit instance. */
int n2v_wedge_slots_fold(const n2v_graph *g, const uint64_t *fold_off, void *wedge_pos_rw, uint16_t *slots,
                         void *stream);

/* Row sums for values that are not dyadic (ABI 15).  generate_alias_tables divides every weight of the step's table
 * by sum(node_weights) / n (randomwalk.py:172-173), a sum rounded at every addition in slot order.  With dyadic 1/p,
 * 1/q it is an integer combination of the edge's class counts; otherwise a step whose decision is closer to its
 * threshold than the rounding of that sum (1 % of the steps on long rows) has to add the row up in the reference's
 * order, run by run between the shared positions: O(list) dependent operations by ONE lane while its wave waits
 * (cfg 4 trimmed at 100 000, (3, 0.7): 102 of 149 ms per launch, profiles/r12c_*).  The sum depends on the EDGE walked
 * and on (p, q) only: this pass computes it once for every edge into a row of >= min_row entries -- the same routine,
 * hence the same bits -- and a walk at that (p, q) reads it with one gather.
 *   edges [k]: the edges to compute (the caller lists those into rows of >= min_row entries, longest lists first so
 *   that the lanes of a wave finish together); sums_out [n_edges] (entries of other edges are not written).
 * g: unit weights, edge_classes, wedge_off, wedge_pos set.  Put sums_out, p, q, min_row into n2v_graph.row_sums*. */
int n2v_edge_row_sums_build(const n2v_graph *g, double p, double q, const int64_t *edges, int64_t k,
                            double *sums_out, void *stream);

/* Search index for N2V_WALK_FAST: the last id of every aligned block of 32 entries of
 * `col` (one 128-byte line).  Inside a sorted row the block ends ascend, so a
 * membership query is a binary search over (degree / 32) pivots followed by one over a
 * single line.  pivots_out: [(n_edges + 31) / 32] int32. */
int n2v_pivots_build(const int32_t *col, int64_t n_edges, int32_t *pivots_out, void *stream);

/* K2 -- the whole of fugue.random_walk's loop (fugue.py:137-153) on device:
 * initiate_random_walk (randomwalk.py:279-296), walk_length x
 * next_step_random_walk (randomwalk.py:300-339) and to_path (:343-349).
 *
 *   start_ids   [n_start]   candidate start vertices (walk_start, fugue.py:132-134)
 *   walks_out   [n_start * num_walks, walk_length + 1] int32, row r = start
 *               r / num_walks, ordinal r % num_walks + 1 (randomwalk.py:294)
 *   valid_out   [n_start * num_walks] 1 where the reference emits a row; 0 for
 *               a start vertex without out-edges (fugue.py:132) and for walkers
 *               that reach a vertex without out-edges before the last step
 *               (inner join, fugue.py:147)
 *
 * The two uniforms of randomwalk.py:336-337 come from the counter-based stream
 * of DESIGN.md "RNG", keyed by (seed, start vertex, ordinal, step): results do
 * not depend on launch geometry or on how start_ids are sharded over GPUs.
 * mode N2V_WALK_EXACT reproduces generate_edge_alias_tables + sampling_from_alias
 * bit for bit; N2V_WALK_FAST draws from the same distribution by rejection.
 * With return_param == inout_param == 1 (the reference's defaults) and g->slots set,
 * exact mode reads the K1 tables instead of rebuilding them: same bits, one gather per
 * step.  On a unit-weight graph a return_param == inout_param == 1 walk of up to 255 steps
 * enqueues TWO kernels on `stream` (the walk, which stores each wave's rows step-major, and an
 * in-place transpose of those regions): walks_out is complete when the stream has passed both. */
int n2v_walk(const n2v_graph *g, const int32_t *start_ids, int64_t n_start,
             int32_t num_walks, int32_t walk_length, double return_param,
             double inout_param, uint64_t seed, int32_t mode,
             int32_t *walks_out, uint8_t *valid_out, uint32_t *status,
             void *stream);

/* ONE STEP of exact walks on a WEIGHTED graph (g->w or g->w64), one lane per walker
 * (csrc/n2v_walk_wlanes.hip) -- the step-synchronous form of n2v_walk for the graphs whose tables have
 * no closed form: every value of the table generate_edge_alias_tables builds (randomwalk.py:193-232)
 * is different, so a step is O(row) with two serial parts, the left-to-right row sum (:172) and the
 * pairing loop (:182-189).  n2v_walk gives a walker a wave and runs those on one lane of it; here 64
 * walkers share a wave and their serial chains run side by side -- which pays when the lanes of a
 * wave stand on rows of similar length, hence `order`.  The caller keeps the state and loops:
 *     walks  [n_rows, walk_length + 1] int32, row r = start r / num_walks, ordinal r % num_walks + 1;
 *            before step 0: walks[r][0] = the start vertex, or -1 (and valid[r] = 0) for a start
 *            vertex out of range or without out-edges (fugue.py:132); everything else -1
 *     valid  [n_rows] 1 while the walker walks; the step clears it when the walker reaches a vertex
 *            without out-edges before the last step (fugue.py:147) or its row sums to 0
 *            (N2V_ST_ZERODIV)
 *     edge_state [n_rows] the edge (index into col) every walker walked last; the step writes it
 *     order  [n_rows] the rows in the order lanes take them -- sorted by the out-degree of
 *            walks[r][step], descending, vanished walkers last (the ascending sort of
 *            n2v_walk_weighted_keys' keys) -- or NULL (row order).  PRECONDITION when scratch and
 *            row_sums are given: the order IS sorted that way.  The wave-per-walker kernels stop at the
 *            first row at or below the cut between the two kernels and at the first vanished walker
 *            (everything behind it is the lane kernel's, or nobody's), so a long row BEHIND a short one
 *            in an unsorted order would not be stepped and no status bit would say so.  The library
 *            cannot check a device-side permutation without a pass and a host read; it does not.
 *   for step = 0 .. walk_length - 1:  n2v_walk_weighted_step(..., step, ...)
 * and the result is n2v_walk's, bit for bit (same uniform stream, keyed by start vertex, ordinal and
 * step).  For return_param or inout_param != 1 the steps after the first read the classes of the
 * slots from g->edge_classes, g->wedge_off and g->wedge_pos (n2v_edge_classes_build, n2v_wedge_build:
 * they depend on the ids alone and are built for a weighted graph as for a unit one).
 *     scratch  int64 [2 (n_rows + 2)] or NULL, row_sums fp64 [n_vertices + 2] or NULL: the sum of the stored
 *            weights of every row, in any order (all weights finite and >= 0), then row_sums[n_vertices] =
 *            a power of two that divides every stored weight (fp32 weights: 2^(e - 24) of the smallest
 *            one, w = m 2^e; 0 = none known: then the margins are the general ones) and
 *            row_sums[n_vertices + 1] = the largest stored weight.  With an order AND both of
 *            these no walker's pairing loop is replayed: the one slot the draw asks for is DECIDED from
 *            sums over the row -- by a lane per walker on rows below 768 slots, by a wave per walker on the
 *            rows above -- (the k-th
 *            overfull slot is demoted where the running sum of the underfull slots' deficits passes that
 *            of the overfull slots' excess; the row sum itself comes from row_sums and the shared and
 *            return slots: no pass), every comparison with a margin that covers the roundings of the
 *            reference's loop (16 n^2 2^-52 and up); a walker whose draw some comparison cannot decide
 *            by that margin gets a second chance in a launch of its own -- the row sum in the
 *            reference's order, hence the margins of an exact sum -- and, if still undecided, is stepped by
 *            the exact wave-per-walker kernel, all in the same call (after it scratch[0] = how many had the
 *            second chance, scratch[n_rows + 2] = how many the exact kernel stepped; their rows follow each
 *            count).  Same bits as without them.
 *     hubs   NULL or the summaries of the long rows (n2v_weighted_hubs, above): the wave kernel then takes
 *            the sums of a step over such a row from them instead of a pass over the row.  Same bits. */
/* Summaries of the HUB rows of a weighted graph for n2v_walk_weighted_step (optional): for every row of at least
 * min_slots slots, cut into blocks of 256 slots in row order, the weights of each block SORTED ascending (the last
 * block padded with +inf) and their prefix sums -- with them the sums of a step over such a row (the deficits and
 * excesses of its slots at the walker's own threshold) are one binary search per block instead of a pass over the
 * row; the slots that are not "other" (shared positions, return run) are corrected from the wedge list.
 *   block0  int32 [n_vertices]: the first block of the row in sorted / prefix, -1 = the row has no summary
 *   sorted  [n_blocks][256] weights as stored (fp32 beside n2v_graph.w, fp64 beside w64)
 *   prefix  fp64 [n_blocks][257]: prefix[b][k] = the sum of the k smallest weights of block b */
typedef struct n2v_weighted_hubs {
  const int32_t *block0;
  const void *sorted;
  const double *prefix;
  int32_t min_slots;
  int32_t lane_cut;   /* 0 = chosen by the library from the number of walkers; > 0: rows of at least this many slots
                       * are decided by a wave per walker, shorter ones by a lane per walker (tuning, tests).  A struct
                       * with block0 == NULL carries this field alone. */
} n2v_weighted_hubs;

/* The sort keys of n2v_walk_weighted_step's `order`, one pass: keys[r] = rank_of[walks[r][step]] (rank_of: the
 * place of every vertex in the order of descending out-degree, ties by id) for a walker that walks, 0x7fffffff
 * for one that has vanished or never started -- sorting them ascending gives the order the step wants. */
int n2v_walk_weighted_keys(const int32_t *walks, const uint8_t *valid, const int32_t *rank_of,
                           int64_t n_vertices, int64_t n_rows, int32_t step, int32_t walk_length,
                           int32_t *keys, void *stream);
int n2v_walk_weighted_step(const n2v_graph *g, const int32_t *start_ids, int32_t num_walks,
                           const int64_t *order, int64_t n_rows, int32_t step, int32_t walk_length,
                           double return_param, double inout_param, uint64_t seed,
                           int64_t *edge_state, int32_t *walks, uint8_t *valid, uint32_t *status,
                           int64_t *scratch, const double *row_sums, const n2v_weighted_hubs *hubs,
                           void *stream);

/* n2v_walk with a workspace lent by the caller, kept for callers of earlier releases.  No walk kernel
 * takes a workspace (passes over walker records kept in one were measured SLOWER than the one-launch
 * kernel on every BASELINE graph, DESIGN.md 5, and are gone): n2v_walk_workspace_bytes always returns 0,
 * and n2v_walk_ws is n2v_walk whatever it is lent (workspace may be NULL). */
int64_t n2v_walk_workspace_bytes(const n2v_graph *g, int64_t n_start, int32_t num_walks,
                                 int32_t walk_length, double return_param, double inout_param,
                                 int32_t mode);
int n2v_walk_ws(const n2v_graph *g, const int32_t *start_ids, int64_t n_start,
                int32_t num_walks, int32_t walk_length, double return_param,
                double inout_param, uint64_t seed, int32_t mode,
                int32_t *walks_out, uint8_t *valid_out, uint32_t *status,
                void *workspace, int64_t workspace_bytes, void *stream);

/* The reference's transformer-level protocol on MATERIALISED tables, one partition (a batch of
 * walker rows) per call.  n2v_walk never builds the table of a step; next_step_random_walk
 * (randomwalk.py:300-339) and the reference's known-answer tests (tests/test_randomwalk.py:
 * 131-189, 268-306) are stated on it, with the two uniforms supplied by the caller
 * (random.random(), :336-337).  Rows are CSR-packed: row r holds the neighbour list of the
 * walker's current vertex, ids[rowptr[r] .. rowptr[r+1]) sorted by id (fugue.py:130).
 *
 *   n2v_edge_bias    w_out[e] = the unnormalised probability generate_edge_alias_tables gives
 *                    entry e (randomwalk.py:219-231): weight / return_param if ids[e] ==
 *                    src_id[r], weight if ids[e] is in the row's src_nbs list (sorted; the
 *                    caller's set src_nbs_id, :318), weight / inout_param otherwise; rows with
 *                    src_id[r] < 0 (first step, :319-320) and src_id == NULL keep the weight.
 *                    w / w64: fp32 or fp64 weights (both NULL = 1.0).  N2V_EINVAL when
 *                    return_param or inout_param is 0 (ValueError, :214-217).
 *   n2v_alias_build  on {rowptr, ids, w64 = w_out} then IS generate_alias_tables(biased row)
 *                    (:232, :157-190).
 *   n2v_alias_draw   sampling_from_alias(r1, r2) (:86-99) followed by the neighbour lookup of
 *                    RandomPath.append (:140-144): vertex_out[r] = the id behind the drawn
 *                    index.  r2 == NULL selects sampling_from_alias_wiki(r1) (:70-84).  A row
 *                    without neighbours yields -1; r1 outside [0, 1) sets N2V_ST_RANGE (the
 *                    reference raises IndexError). */
int n2v_edge_bias(const int64_t *rowptr, const int32_t *ids, const float *w, const double *w64,
                  const int32_t *src_id, const int64_t *src_rowptr, const int32_t *src_nbs,
                  int64_t n_rows, int64_t nnz, double return_param, double inout_param,
                  double *w_out, void *stream);
int n2v_alias_draw(const int64_t *rowptr, const n2v_slot *slots, int64_t n_rows,
                   const double *r1, const double *r2, int32_t *vertex_out, uint32_t *status,
                   void *stream);

/* The two uniforms n2v_walk draws for walker `key[i]` (= start vertex * num_walks + ordinal - 1)
 * at step `step[i]` (0-based), as the fp64 numbers u / 2^32 the reference's random.random()
 * stands for (randomwalk.py:336-337).  With them n2v_edge_bias + n2v_alias_build +
 * n2v_alias_draw reproduce one step of n2v_walk's exact mode bit for bit: the step function of
 * graph-partitioned walking (node2vec_amd/partitioned.py), where a walker's two rows live on
 * different GPUs and the step is taken where the current vertex is stored. */
int n2v_walk_uniforms(uint64_t seed, const int64_t *key, const int32_t *step, int64_t n,
                      double *r1_out, double *r2_out, void *stream);

/* a9 -- trim_hotspot_vertices (randomwalk.py:238-262): rows with more than
 * max_out_degree edges keep a uniform sample without replacement of exactly
 * max_out_degree of them (max_out_degree <= 0 means 100000, constants.py:6).
 * keep_out[e] = 1 for surviving edges; weights are untouched. */
int n2v_trim_mark(const int64_t *rowptr, int64_t n_rows, int64_t max_out_degree,
                  uint64_t seed, uint8_t *keep_out, void *stream);

/* K3 -- one pass of skip-gram negative-sampling SGD over a block of walks: the
 * arithmetic behind gensim.models.Word2Vec(sentences, sg=1, hs=0, negative=k) at
 * the reference's call site embedding.py:126 (algorithm: DESIGN.md "SGNS"; the
 * trainer itself is third-party gensim 3.8, absent from the reference tree).
 *
 *   walks       [n_walks, walk_len] int32 vocabulary indices, < 0 = token outside
 *               the vocabulary (dropped before windowing, as gensim does)
 *   syn0        [n_vocab, dim] fp32 input vectors  (model.wv.vectors), in place
 *   syn1neg     [n_vocab, dim] fp32 output vectors (model.trainables.syn1neg)
 *   cum_table   [n_vocab] uint32 cumulative count^0.75, scaled to 2^31 - 1
 *   sample_int  [n_vocab] uint32 keep-thresholds of frequent-word subsampling,
 *               or NULL when `sample` == 0
 *   exp_table   [1000] fp32 sigmoid table over [-6, 6) (word2vec EXP_TABLE)
 *   pairs_out   TWO device uint64 (or NULL): [0] += number of (centre, context) pairs
 *               trained; [1] scratch, the kernel hands out rows through it (reset by the
 *               library on the stream before the launch)
 *
 * params->batched = 1 selects the opt-in BATCHED trainer (dim 64 / 128 / 256, window <= 7,
 * negative <= 15, else N2V_EINVAL): the `negative` draws are made once per centre position and
 * shared by its <= 2 * window pairs, and the pairs of a position are trained from one snapshot of
 * the rows -- NOT gensim's sampling (Ji et al. 2016).  A position then is three small dense
 * products on v_mfma_f32_16x16x4_f32 and moves 8 * dim * (2 + negative) bytes per position
 * instead of per pair.  Its deterministic mode is bit-identical to its own CPU restatement
 * (oracle/n2v_oracle_sgns.c, the batched function).
 *
 * One wave trains one walk (sentence); walks are spread over the grid hogwild
 * (unsynchronised updates, as gensim's worker threads).  deterministic != 0 runs
 * every walk in order on a single wave: bit-identical to oracle/n2v_oracle_sgns.c.
 * All randomness is counter-based on (seed, sentence_base + row, draw index), so
 * results do not depend on launch geometry in deterministic mode. */
typedef struct n2v_sgns_params {
  int64_t n_vocab;
  int64_t sentence_base; /* global index of walks[0] (RNG key, multi-GPU shards) */
  uint64_t seed;
  int32_t dim;      /* 1 .. 1024 */
  int32_t window;   /* 1 .. 32  (the reference allows 5 .. 30, embedding.py:110) */
  int32_t negative; /* 1 .. 32 */
  float alpha;      /* learning rate of this pass (host applies the linear decay) */
  int32_t deterministic;
  int32_t cum_index_bits;   /* log2 of the number of buckets of cum_index (1 .. 30) */
  const int32_t *cum_index; /* device, [2^bits + 1] from n2v_cum_index_build, or NULL */
  int32_t max_waves; /* 0: hogwild concurrency = one wave per 32 vocabulary rows, up to the whole
                        chip; > 0: at most this many waves train concurrently */
  int32_t batched;   /* 0: gensim's sampling -- k negatives drawn per (centre, context) pair;
                        1 (opt-in, NOT gensim's sampling): the k negatives are drawn once per
                        centre position and shared by its <= 2 * window pairs, which turns a
                        position into one small dense product (see n2v_sgns_train) */
  int32_t window_cache; /* 1: the default kernel keeps the syn0 rows of the window in LDS (read and
                           written once per position instead of once per pair; same values, bit
                           for bit in deterministic mode; dim 64 / 128 and window <= 7, else
                           N2V_EINVAL).  Measured slower than 0 on MI355X (the ring costs 3 of 8
                           waves per SIMD and the kernel is bound by rows in flight): off by default */
  int32_t hub_rows;     /* hogwild mode only: rows [0, hub_rows) of syn0 / syn1neg (the most frequent
                           words: the vocabulary is in descending count order) are updated by
                           atomic adds of each wave's contribution instead of read-modify-write
                           stores, so that concurrent waves do not overwrite each other on hubs.
                           0 = off (gensim's unsynchronised updates everywhere).  The batched
                           trainer always returns its context rows as atomic deltas; hub_rows
                           adds the same for its target rows (8 adds per lane and row: measured
                           -34 % at 4096 on cfg 3, link AUC 0.886 -> 0.899 on cfg 2) */
  const float *row_alpha; /* [n_walks] or NULL: the learning rate of every row of the launch (gensim
                             lowers it per job of sentences: n2v_sgns_job_alpha writes such an
                             array); NULL = `alpha` for every row */
} n2v_sgns_params;

#define N2V_SGNS_MAX_SENTENCE 256 /* longer walks: split rows on the host */

/* Optional index over cum_table for the negative draws of K3: index_out[b] =
 * bisect_left(cum_table, b << (31 - bits)) for b = 0 .. 2^bits.  A draw r then needs
 * bisect_left only inside [index[r >> (31 - bits)], index[(r >> (31 - bits)) + 1]]: the same
 * word as gensim's bisect over the whole table, in one or two memory sectors instead of
 * log2(n_vocab) dependent probes (at 10^8 words the probes were a fifth of the kernel's read
 * sectors).  index_out: [2^bits + 1] int32. */
int n2v_cum_index_build(const uint32_t *cum_table, int64_t n_vocab, int32_t bits,
                        int32_t *index_out, void *stream);

/* gensim's learning-rate schedule, per row of a launch.  gensim.models.Word2Vec (embedding.py:126)
 * lowers the rate per JOB -- a batch of consecutive sentences of at most batch_words raw words
 * (constants.py:58: 1000) -- to  max(end, start - (start - end) * (epoch + pushed / total) / epochs),
 * pushed = sentences queued before the job (word2vec.py _job_producer, _get_next_alpha; Python
 * doubles, then cast to fp32).  out[i] = that rate for sentence row0 + i of epoch `epoch`, whose job
 * is (row0 + i) / job_rows (job_rows = max(1, batch_words / sentence length) for the equal-length
 * sentences of a walk corpus): the same double operations in the same order.  Pass `out` as
 * n2v_sgns_params.row_alpha.  out: [n] fp32. */
int n2v_sgns_job_alpha(int32_t job_rows, int32_t epoch, int32_t epochs, int64_t row0, int64_t rows,
                       double alpha0, double alpha_min, int64_t n, float *out, void *stream);

/* How many waves n2v_sgns_train(P, n_walks, walk_len) keeps in flight on this device (its hogwild
 * concurrency rule, max_waves and the occupancy of the kernel instance it picks, all applied) --
 * nothing is launched.  The host chooses n2v_sgns_params.hub_rows from it (node2vec_amd/sgns.py
 * auto_hub_rows: a row held by more than one wave at a time on average gets atomic adds).  With
 * P->batched the waves of the batched trainer's launch; a negative status for parameters
 * n2v_sgns_train would refuse. */
int64_t n2v_sgns_hogwild_waves(const n2v_sgns_params *P, int64_t n_walks, int32_t walk_len);

int n2v_sgns_train(const int32_t *walks, int64_t n_walks, int32_t walk_len,
                   float *syn0, float *syn1neg, const uint32_t *cum_table,
                   const uint32_t *sample_int, const float *exp_table,
                   const n2v_sgns_params *params_host,
                   unsigned long long *pairs_out, void *stream);

/* The exchange step of the multi-GPU SGNS path.  The reference trains on
 * one machine: gensim's worker threads share syn0 / syn1neg (embedding.py:126).  Sharded
 * over GPUs, every rank trains its own walks on a full replica and the replicas are
 * averaged every few launches by an all-reduce (RCCL) between these two elementwise passes:
 *
 *   n2v_delta_pack   before_out[i] = cur[i] (snapshot), and the rank's contribution
 *                    wire_out[i] = cur[i]                        N2V_WIRE_F32 (fp32 [n])
 *                                = bf16(cur[i] - ref_bf16[i])    N2V_WIRE_BF16 (bf16 [n])
 *   (caller: all-reduce SUM of wire over the ranks)
 *   n2v_delta_apply  mean = wire_sum[i] / world                       (F32)
 *                         = ref_bf16[i] + wire_sum[i] / world         (BF16; ref := bf16(mean))
 *                    cur[i] += mean - before[i]
 *   ("/ world" is one correctly rounded fp32 division by (float)world, never a product with
 *   1 / world: the two differ for every world that is no power of two)
 *
 * so that updates made to cur while the collective was in flight survive.  With
 * before_out / before == NULL no snapshot is taken and apply stores cur[i] = mean exactly
 * (a blocking exchange: every rank ends with the same bits).  ref_bf16 is a
 * bf16 reference copy shared by all ranks (n2v_delta_ref_init writes bf16(cur) once, on
 * identical replicas); the F32 form needs no reference at all. */
#define N2V_WIRE_F32 0
#define N2V_WIRE_BF16 1
int n2v_delta_ref_init(const float *cur, int64_t n, uint16_t *ref_bf16_out, void *stream);
int n2v_delta_pack(const float *cur, const uint16_t *ref_bf16, int64_t n, float *before_out,
                   void *wire_out, int32_t wire_dtype, void *stream);
int n2v_delta_apply(float *cur, uint16_t *ref_bf16, const float *before, const void *wire_sum,
                    int32_t wire_dtype, int32_t world, int64_t n, void *stream);
/* The sum itself, when the caller moves bytes instead of calling an all-reduce (so that the result
 * does not depend on the collective library's reduction order or accumulator type): `parts` holds
 * `world` contributions of m elements each, rank after rank (what an all-to-all of the ranks' wire
 * buffers delivers for this rank's shard); out[i] = parts[0][i] + parts[1][i] + ... in fp32, in
 * rank order, stored in the wire type (bf16: ONE rounding of the fp32 sum).  An all-gather of the
 * shards then gives every rank the same wire_sum for n2v_delta_apply. */
int n2v_delta_reduce(const void *parts, int32_t wire_dtype, int32_t world, int64_t m, void *out,
                     void *stream);

/* The two elementwise passes between K2 and K3 when the corpus is streamed batch by batch
 * (node2vec_amd/pipeline.py; the reference materialises the walks as strings and lets gensim's
 * build_vocab count them, embedding.py:125-126):
 *   n2v_corpus_count  counts[v] += occurrences of v in the rows with valid[row] != 0 (valid NULL =
 *                     every row); tokens outside [0, n_vertices) are ignored.  counts: uint64.
 *   n2v_corpus_index  idx_out[r][t] = index_of[walks[r][t]] for tokens of valid rows, else -1
 *                     (the int32 vocabulary indices n2v_sgns_train takes). */
int n2v_corpus_count(const int32_t *walks, const uint8_t *valid, int64_t n_rows, int32_t len,
                     int64_t n_vertices, unsigned long long *counts, void *stream);
int n2v_corpus_index(const int32_t *walks, const uint8_t *valid, const int32_t *index_of,
                     int64_t n_rows, int32_t len, int64_t n_vertices, int32_t *idx_out, void *stream);

/* Graph-partitioned walking (node2vec_amd/partitioned.py): one step of the k
 * walkers resident on ONE part of a vertex-range partition -- the reference's per-step join
 * (fugue.py:146-149: walker row x adjacency row of its current vertex, the row of its previous
 * vertex carried along) followed by next_step_random_walk (randomwalk.py:300-339), in one launch,
 * one wave per walker, no table materialised.
 *   rowptr / col / w / w64   the part's rows [lo, lo + n_local) (rowptr rebased to 0; ids global;
 *                            at most one of w, w64; both NULL = unit weights)
 *   head      int64 [k][head_cols] (head_cols >= 4): (output row, RNG key = start * num_walks +
 *             ordinal - 1, s << 32 | v, step[, classes]); s = -1 (high word all ones) on the
 *             first step (:320-321)
 *   src_ptr / src_ids        what travelled with the walkers, packed (int64 [k + 1] offsets):
 *     src_kind N2V_SRC_ROWS    the rows N(s), sorted ids; read only when q != 1 and s >= 0 (may
 *                              be NULL otherwise)
 *     src_kind N2V_SRC_WEDGES  (unit weights, head_cols >= 5) the WEDGE LIST of the edge (s -> v)
 *                              walked last -- the positions in N(v) of the neighbours v shares
 *                              with s, ascending, 32-bit -- cut from the wedge table of the rank
 *                              that stores that edge (n2v_wedge_build on its part), with
 *                              head[.][4] = edge_classes[e] | return position << 32: the class of
 *                              every slot of the step's table is then known by position and
 *                              neither N(s) nor a pass over N(v) is needed.  With q == 1 the
 *                              lists are empty (only the return run matters), with p == q == 1
 *                              nothing is read beyond the first four header words
 *   A header whose output row (head[i][0]) is NEGATIVE is an EMPTY SLOT of a capacity-bounded
 *   mailbox: n2v_partition_step draws nothing for it and n2v_partition_forward neither logs nor
 *   forwards it, so a mailbox of fixed capacity can be stepped whole, without its count on the host.
 *   next_out  int32 [k]: the vertex drawn (-1 when status reports an error for that walker)
 *   edge_out  int64 [k] or NULL: the index (into the part's col) of the edge drawn
 *   status    uint32 [4] as for n2v_walk; [1] is used as the walker counter.
 * Draws are those of n2v_walk's exact mode (same stream keyed by (seed, key, step)), so walks are
 * bit-identical to n2v_walk over the unpartitioned graph wherever the walker happens to be.
 *   n2v_gather_rows    out[out_ptr[j] ..) = ids[ptr[rows[j]] .. ptr[rows[j] + 1]) for j < k: packs
 *                      the rows that leave with migrating walkers (out_ptr = their prefix sums)
 *   n2v_gather_wedges  the same for wedge lists: out[out_ptr[j] ..) = the list of edge edges[j]
 *                      widened to 32 bits, and head[j][4] = edge_classes | return position << 32 */
#define N2V_SRC_ROWS 0
#define N2V_SRC_WEDGES 1
#define N2V_SRC_WEDGES_AT 2 /* as N2V_SRC_WEDGES, but src_ptr is int64 [k]: where the list of walker i
                               STARTS in src_ids (its length is the shared count in head[i][4]) -- the
                               form n2v_partition_forward leaves the lists in */
int n2v_partition_step(const int64_t *rowptr, const int32_t *col, const float *w, const double *w64,
                       int64_t lo, int64_t n_local, const int64_t *head, int32_t head_cols,
                       const int64_t *src_ptr, const int32_t *src_ids, int32_t src_kind, int64_t k,
                       double p, double q, uint64_t seed, int32_t *next_out, int64_t *edge_out,
                       uint32_t *status, void *stream);
/* The elementwise half of the routing that follows a step: for walker i the path record
 * log_out[i] = (output row, step + 1, next) -- or (row, -1, -1) when next < 0: the vertex it stood
 * on has no out-edges, it vanished on arrival (fugue.py:147) --, the header it travels on with,
 * dest_out[i] = the part that owns `next` (bounds: first vertex of every part, ascending) or
 * n_parts when the walk is complete or the walker vanished, len_out[i] / src_out[i] = how many
 * words travel with it and where they come from (carry 0: none; N2V_SRC_ROWS + 1: the row of its
 * vertex, src = local row; N2V_SRC_WEDGES + 1: the wedge list of edge[i], src = that edge;
 * N2V_SRC_WEDGES + 2: src = that edge but no words -- q == 1, only the counts and the return
 * position of the edge travel, in the header).  The caller groups the walkers by a stable sort
 * of dest_out, or calls n2v_partition_group. */
int n2v_partition_route(const int64_t *head_in, int32_t head_cols, const int32_t *next,
                        const int64_t *edge, int64_t k, int32_t walk_length, const int64_t *bounds,
                        int32_t n_parts, int32_t carry, const int64_t *rowptr, int64_t lo,
                        const uint32_t *edge_classes, int64_t *log_out, int64_t *head_out,
                        int32_t *dest_out, int64_t *len_out, int64_t *src_out, void *stream);
/* Groups what n2v_partition_route wrote by destination, keeping the order inside a destination
 * (a stable counting sort: per-block counts, one scan, one scatter): head_out / len_out / src_out
 * = the rows of head / len / src ordered by dest (0 .. n_parts, n_parts = not forwarded, last);
 * cuts_out int64 [n_parts + 1]: where destination d starts (cuts_out[n_parts] = the number of
 * forwarded walkers).  n_parts <= 64.  work: int64 scratch of ((k + 255) / 256 + 1) * (n_parts + 1)
 * words. */
int n2v_partition_group(const int32_t *dest, const int64_t *head, int32_t head_cols,
                        const int64_t *len, const int64_t *src, int64_t k, int32_t n_parts,
                        int64_t *work, int64_t *head_out, int64_t *len_out, int64_t *src_out,
                        int64_t *cuts_out, void *stream);
/* Route, group and gather in ONE launch, no size known to the host (round 4).  For walker i: the
 * path record -- log_out[i] as n2v_partition_route writes it, or, when log_out is NULL, straight
 * into walks_out[row][step + 1] (valid_out[row] = 0 for a walker that vanished): the single-process
 * form, where the emitting rank's arrays are at hand --; then, if the walk goes on, the walker is
 * APPENDED to the mailbox of the part that owns `next`:
 *   box_head  int64 [n_parts][cap][head_cols]   headers (head[.][4] = edge_classes | return position
 *                                               << 32 of the edge drawn when carry != 0)
 *   box_off   int64 [n_parts][cap]              where its list starts in the destination's pool
 *   box_words int32 [n_parts][wcap]             the wedge lists (carry N2V_SRC_WEDGES + 1): one pool per
 *                                               destination, so that what goes to one part is
 *                                               contiguous (an exchange sends pool d to rank d)
 *   box_count uint64 [2 n_parts]                walkers appended per destination, then words used per
 *                                               destination.  The caller zeroes it before the first
 *                                               launch of a step; several source parts may append to
 *                                               the same boxes (one atomic add per block and
 *                                               destination).
 * A full mailbox or pool sets N2V_ST_OVERFLOW in status[0] (the step must be repeated with larger
 * ones; nothing is written out of bounds).  carry: 0 (headers only: p == q == 1), N2V_SRC_WEDGES + 1
 * (the list of edge[i]), N2V_SRC_WEDGES + 2 (q == 1: counts and return position only); rows do not
 * travel this way.  The next n2v_partition_step takes mailbox d as head = box_head[d] / src_ptr =
 * box_off[d] / src_ids = box_words[d] with src_kind N2V_SRC_WEDGES_AT.  Replaces n2v_partition_route +
 * n2v_partition_group + a prefix sum + n2v_gather_wedges and the host read between them; the order
 * of the walkers in a mailbox is not defined, the walks are (the RNG is keyed by walker and step).
 *   wide: the width of a UNIFORM wedge table only -- 0: every list uint16, 1: every list uint32; any other value
 *   is N2V_EINVAL before anything is launched, here, in n2v_partition_forward_boxes and in n2v_gather_wedges.  A
 *   mixed table (n2v_wedge_build with wide = T >= 2, n2v_graph.wedge_wide of such a graph) cannot be cut by edge
 *   ranges: it is rebuilt with 32-bit lists throughout (wide = 1) first, as partition_graph does. */
int n2v_partition_forward(const int64_t *head_in, int32_t head_cols, const int32_t *next,
                          const int64_t *edge, int64_t k, int32_t walk_length, const int64_t *bounds,
                          int32_t n_parts, int32_t carry, const uint32_t *edge_classes,
                          const uint64_t *wedge_off, const void *wedge_pos, int32_t wide,
                          int64_t *box_head, int64_t *box_off, int32_t *box_words,
                          unsigned long long *box_count, int64_t cap, int64_t wcap, int64_t *log_out,
                          int32_t *walks_out, uint8_t *valid_out, uint32_t *status, void *stream);
/* n2v_partition_forward into mailboxes with a capacity PER DESTINATION, laid out back to back (what an
 * all-to-all with fixed split sizes sends as it lies): box_starts int64 [2 * n_parts + 2] -- mailbox d
 * is box_head / box_off [box_starts[d], box_starts[d + 1]), its word pool box_words
 * [box_starts[n_parts + 1 + d], box_starts[n_parts + 2 + d]); box_off holds the list start INSIDE the
 * pool of its destination.  The path records go to log_out.  With empty slots (see n2v_partition_step)
 * this is the step of a rank of a multi-GPU walk that reads nothing on the host: capacities fixed
 * once, overflow reported in the status word (N2V_ST_OVERFLOW) and looked at after the last step.
 * Replaces the shuffle of fugue.py:146-149. */
int n2v_partition_forward_boxes(const int64_t *head_in, int32_t head_cols, const int32_t *next,
                                const int64_t *edge, int64_t k, int32_t walk_length,
                                const int64_t *bounds, int32_t n_parts, int32_t carry,
                                const uint32_t *edge_classes, const uint64_t *wedge_off,
                                const void *wedge_pos, int32_t wide, int64_t *box_head, int64_t *box_off,
                                int32_t *box_words, unsigned long long *box_count,
                                const int64_t *box_starts, int64_t *log_out, uint32_t *status,
                                void *stream);
int n2v_gather_rows(const int64_t *ptr, const int32_t *ids, const int64_t *rows,
                    const int64_t *out_ptr, int64_t k, int32_t *out, void *stream);
int n2v_gather_wedges(const uint32_t *edge_classes, const uint64_t *wedge_off, const void *wedge_pos,
                      int32_t wide, const int64_t *edges, const int64_t *out_ptr, int64_t k,
                      int32_t *out, int64_t *head, int32_t head_cols, void *stream);

/* Fills the entry table of the degree-ranked form (n2v_graph.rank_hops) of a unit-weight graph.
 * The caller ranks the vertices -- any STABLE sort by descending degree: rank_vertex[r] = the vertex
 * of rank r, rank_of its inverse -- and passes rank_rowptr[r] = the sum of the degrees of ranks
 * below r ([n_vertices + 1], int64).  out[rank_rowptr[r] + k] = rank_of[col[rowptr[v] + k]] for
 * v = rank_vertex[r].  The head and class tables of n2v_graph are a few thousand words the caller
 * derives from the sorted degrees (node2vec_amd/graph.py build_ranked shows how).  Replaces nothing
 * in the reference (its adjacency rows are Python lists, fugue.py:130); it is the layout that lets
 * a p == q == 1 step (randomwalk.py:86-99 with probs == 1.0) be one 4-byte gather.
 * out: [g->n_edges] uint32. */
int n2v_rank_hops_build(const n2v_graph *g, const int32_t *rank_of, const int32_t *rank_vertex,
                        const int64_t *rank_rowptr, uint32_t *out, void *stream);

/* The pair table: the rows of n2v_rank_hops_build (same arguments, same order of rows and of the entries
 * inside a row) with 8-byte entries that hold the neighbour's vertex id beside its rank:
 *   out[rank_rowptr[r] + k] = (uint64_t)rank_of[c] << 32 | (uint32_t)c,  c = col[rowptr[rank_vertex[r]] + k].
 * A p == q == 1 walk over it (n2v_graph.rank_hops = out, rank_emit = 2, the head and class tables as for
 * the ranked form) writes the low word to the path and finds the next row from the high word: vertex
 * ids out in one 8-byte gather per step, where the 4-byte form needs a second gather through
 * rank_vertex and the 8-byte hop table (n2v_hops8_build) needs field widths the graph may not have.
 * out: [g->n_edges] uint64. */
int n2v_rank_pairs_build(const n2v_graph *g, const int32_t *rank_of, const int32_t *rank_vertex,
                         const int64_t *rank_rowptr, uint64_t *out, void *stream);

/* Measurement aid (bench.py; nothing on the product path calls it): the rate this device
 * sustains for the access shapes of K2 and K3 on the CALLER's buffer, so that the ceilings the
 * kernels are compared with are observed on the box the bench runs on.  One launch; the caller
 * times it (HIP events on `stream`).
 *   mode 0  independent random reads (a hop-table gather), 4 in flight per lane; element width
 *           = row_bytes (16, 8 or 4; 0 = 16)
 *   mode 1  one dependent chain of such reads per lane (a walker)
 *   mode 2  random rows of row_bytes (256 | 512 | 1024 | 2048) read by one wave each (a syn0 row)
 *   mode 3  the same rows read, modified and written back (a trained row)
 *   mode 4  one dependent chain of random 4-byte reads per lane with a binary search over an LDS
 *           table of row_bytes degree classes (a power of two, 64 .. 8192) between them: a walker on
 *           a graph numbered by descending degree whose entries are the neighbour id alone
 *   mode 5  the shape of a biased exact step: a dependent chain of hop entries of row_bytes (16 | 8)
 *           bytes, and with 49 % of the steps an independent 32-byte read of a wedge slot; the buffer
 *           is cut into E hop entries followed by E slots (E = buffer_bytes / (row_bytes + 32)); six
 *           waves per SIMD as the walk kernel runs
 * iters: accesses per lane (modes 0, 1) / rows per wave (modes 2, 3), a multiple of 4.
 * *accesses_host (host pointer, optional) receives the number of accesses the launch makes.
 * buffer: 16-byte aligned device memory, overwritten in mode 3.  sink: one device word. */
int n2v_mem_probe(void *buffer, int64_t buffer_bytes, int32_t mode, int32_t iters,
                  int32_t row_bytes, int64_t *accesses_host, uint32_t *sink, void *stream);

/* Nearest neighbours by cosine over trained vectors: exact fp32 brute force over a row-major
 * X[n, dim] (1 <= dim <= 1024, 0 <= n < 2^31), what gensim 3.8 KeyedVectors.init_sims /
 * most_similar compute on the Word2Vec model the reference returns (embedding.py:120-127).
 * score(q, r) = dot(q_hat, x_r) * inv_norm[r] with q_hat = q * (1 / sqrtf(sum q^2)) -- or, for a
 * query given as row r' of X, x_r' * inv_norm[r'] -- in fp32 products and sums, every score in one
 * fixed order (DESIGN.md "Nearest neighbours"): results do not depend on the batch of queries, and
 * n2v_knn_topk's scores equal n2v_knn_scores' bit for bit.  A row (or query) of norm 0 scores 0
 * where gensim gives NaN.  Exactly one of queries ([n_queries, dim] fp32) / query_rows
 * ([n_queries] int64, each in [0, n)) is non-NULL.  Argument errors are N2V_EINVAL before any
 * launch; n == 0 or n_queries == 0 is N2V_OK and launches nothing. */

/* inv_norm[r] = 1 / sqrtf(sum_d X[r, d]^2), 0 for a zero row: init_sims' norms, without the
 * normalised copy of X.  inv_norm: [n] fp32. */
int n2v_knn_inv_norms(const float *X, int64_t n, int32_t dim, float *inv_norm, void *stream);
/* Bytes of workspace n2v_knn_topk needs for these sizes (1 <= k <= 1024), or n2v_knn_scores
 * (k == 0); -1 for sizes the calls refuse. */
int64_t n2v_knn_workspace_bytes(int64_t n, int32_t dim, int64_t n_queries, int32_t k);
/* The k best rows of every query (most_similar's argsort of the score vector, topn = k), fused:
 * the n_queries x n score matrix is never written.  out_rows / out_scores: [n_queries, k] int64 /
 * fp32, by score descending, then row ascending; for k > n the tail is row -1, score -inf.
 * 1 <= k <= 1024; workspace: 16-byte aligned, workspace_bytes >= n2v_knn_workspace_bytes. */
int n2v_knn_topk(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                 const int64_t *query_rows, int64_t n_queries, int32_t k, int64_t *out_rows,
                 float *out_scores, void *workspace, int64_t workspace_bytes, void *stream);
/* Every score (most_similar with topn=None): out_scores [n_queries, n] fp32, row-major.
 * n_queries < 2^20; workspace as above with k == 0. */
int n2v_knn_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                   const int64_t *query_rows, int64_t n_queries, float *out_scores, void *workspace,
                   int64_t workspace_bytes, void *stream);

/* Skip-gram with HIERARCHICAL SOFTMAX (what Spark ML's Word2Vec trains behind the reference's
 * Node2VecSpark, embedding.py:182-285): word2vec.c's Huffman tree and skip-gram HS update,
 * DESIGN.md "Hierarchical softmax".
 *
 * n2v_hs_tree_build (host memory, no GPU): the Huffman tree of counts[n_vocab] (descending, as
 * the vocabulary is ordered; >= 0), built exactly as word2vec.c CreateBinaryTree.  Word w's path
 * is points[path_off[w] .. path_off[w + 1]) (syn1 rows, root n_vocab - 2 first) and its code bit d
 * is (codes[w] >> d) & 1.  path_off_out: [n_vocab + 1] int64, codes_out: [n_vocab] uint64,
 * points_out: [path_off[n_vocab]] int32 or NULL (then only path_off / codes are written: the caller
 * sizes points from path_off[n_vocab] and calls again).  N2V_EINVAL for counts that are not
 * descending, a code longer than 64 bits, or points_capacity < path_off[n_vocab].  n_vocab == 1:
 * code length 0. */
int n2v_hs_tree_build(const int64_t *counts, int64_t n_vocab, int64_t *path_off_out, uint64_t *codes_out,
                      int32_t *points_out, int64_t points_capacity);

typedef struct n2v_hs_params {
  int64_t n_vocab;
  int64_t sentence_base; /* global index of walks[0] (RNG key) */
  uint64_t seed;
  int32_t dim;           /* 1 .. 1024 */
  int32_t window;        /* 1 .. 32 */
  float alpha;           /* rate of every row when row_alpha is NULL */
  int32_t deterministic; /* 1: one wave, rows in order: bit-identical to the CPU restatement */
  const float *row_alpha; /* [n_walks] or NULL: the rate of every row of the launch */
  int32_t max_waves;     /* 0: one wave per 32 vocabulary rows, up to the whole chip */
  int32_t hot_nodes;     /* must be 0 (N2V_EINVAL otherwise): atomic adds on the nodes nearest the root
                            were measured slower and worse than plain stores */
  int32_t path_cache;    /* 1: the top path rows of a centre position are held in LDS across its
                            contexts (same values); 0: every pair reads and writes them in HBM */
  int32_t reserved;
} n2v_hs_params;

/* One pass of skip-gram HS over a block of rows.  walks: [n_walks, walk_len] int32 vocabulary
 * indices (< 0 or >= n_vocab: dropped before windowing; walk_len <= N2V_SGNS_MAX_SENTENCE); syn0
 * [n_vocab, dim], syn1 [n_vocab - 1, dim] fp32 in place; path_off / points / codes from
 * n2v_hs_tree_build, on the device; exp_table [1000] fp32; pairs_out: TWO device uint64 or NULL,
 * as n2v_sgns_train.  Argument errors are N2V_EINVAL before anything is launched. */
int n2v_hs_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1,
                 const int64_t *path_off, const int32_t *points, const uint64_t *codes, const float *exp_table,
                 const n2v_hs_params *params_host, unsigned long long *pairs_out, void *stream);

/* The waves n2v_hs_train keeps in flight for such a launch on this device (nothing is launched), or
 * a negative status for parameters it would refuse. */
int64_t n2v_hs_hogwild_waves(const n2v_hs_params *P, int64_t n_walks, int32_t walk_len);

/* CBOW (sg = 0) with negative sampling: what gensim.models.Word2Vec trains at the reference's call
 * site embedding.py:126 when `negative` is set and `sg` is left at gensim's default 0 (gensim 3.8
 * train_batch_cbow / fast_sentence_cbow_neg; DESIGN.md "CBOW").  Arguments, sentence preparation,
 * launch geometry and pairs_out as n2v_sgns_train, on the same syn0 / syn1neg; pairs_out[0] grows by
 * one per trained POSITION (a centre word with at least one context word).  The `negative` draws are
 * made once per position.  cbow_mean 1: the context vectors are averaged (gensim's default), 0: summed
 * and the error divided by their number.  deterministic != 0: one wave, rows in order, bit-identical
 * to tests/cpu_cbow/n2v_cbow_cpu.c.  params->batched != 0, params->window_cache != 0, cbow_mean
 * outside {0, 1} and everything n2v_sgns_train refuses are N2V_EINVAL before anything is launched;
 * n_walks == 0 is N2V_OK. */
int n2v_cbow_train(const int32_t *walks, int64_t n_walks, int32_t walk_len,
                   float *syn0, float *syn1neg, const uint32_t *cum_table,
                   const uint32_t *sample_int, const float *exp_table,
                   const n2v_sgns_params *params_host, int32_t cbow_mean,
                   unsigned long long *pairs_out, void *stream);

/* The waves n2v_cbow_train keeps in flight for such a launch on this device (nothing is launched), or
 * a negative status for parameters it would refuse. */
int64_t n2v_cbow_hogwild_waves(const n2v_sgns_params *P, int64_t n_walks, int32_t walk_len);

/* Link prediction over trained vectors (node2vec paper, section 4.4; csrc/n2v_pairs.hip, DESIGN.md "Link
 * prediction").  ADDITIONS ONLY: nothing that existed changes and N2V_ABI_VERSION stays 15, as when CBOW was
 * added.  X: row-major fp32 [n, dim], 1 <= dim <= 1024, 0 <= n < 2^31; a, b: [n_pairs] int64 row numbers.
 * All three calls only read X and the graph.  Argument errors are N2V_EINVAL before any launch (sizes, an
 * unknown metric / op, an n_pairs whose grid of ceil(n_pairs / 256) blocks does not fit, then NULL pointers);
 * n_pairs == 0 is N2V_OK and launches nothing.  A pair with an index outside [0, n) (outside
 * [0, n_vertices) for n2v_pairs_in_graph) is never dereferenced: its score or feature row is NaN, its
 * mask 0. */
#define N2V_PAIR_DOT 0    /* dot(x_a, x_b) */
#define N2V_PAIR_COSINE 1 /* dot(x_a, x_b) * (inv_norm[a] * inv_norm[b]) */
/* the binary operators of the paper's Table 1, element by element */
#define N2V_PAIR_AVERAGE 0  /* (x_a + x_b) * 0.5f */
#define N2V_PAIR_HADAMARD 1 /* x_a * x_b */
#define N2V_PAIR_L1 2       /* fabsf(x_a - x_b) */
#define N2V_PAIR_L2 3       /* (x_a - x_b) * (x_a - x_b) */

/* out_scores[i] = score of (a[i], b[i]), fp32 [n_pairs].  inv_norm: the output of n2v_knn_inv_norms,
 * required for N2V_PAIR_COSINE, ignored (may be NULL) for N2V_PAIR_DOT; a zero row scores 0, NaN or inf
 * propagates, as in n2v_knn_*.  The dot is summed by fp32 fmaf and adds in ONE fixed order that depends on
 * dim alone (written out in csrc/n2v_pairs.hip and restated in tests/cpu_pairs/n2v_pairs_cpu.c): not on
 * n_pairs, the pair's place in the list or the launch; and score(a, b) == score(b, a) bit for bit. */
int n2v_pair_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *a,
                    const int64_t *b, int64_t n_pairs, int32_t metric, float *out_scores, void *stream);
/* out[i, :] = op(x_a[i], x_b[i]), fp32 [n_pairs, dim] row-major: one or two correctly rounded fp32
 * operations per element, no contraction (bit-identical to numpy float32).  64-bit offsets throughout. */
int n2v_pair_features(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                      int64_t n_pairs, int32_t op, float *out, void *stream);
/* out_mask[i] = 1 if row a[i] of the CSR (rowptr int64 [n_vertices + 1], col int32, ascending within a
 * row, multi-edges adjacent, empty rows allowed) holds b[i], else 0.  uint8 [n_pairs]. */
int n2v_pairs_in_graph(const int64_t *rowptr, const int32_t *col, int64_t n_vertices, const int64_t *a,
                       const int64_t *b, int64_t n_pairs, uint8_t *out_mask, void *stream);

/* k-means (Lloyd) over trained vectors (the node2vec paper's case study, section 4.1; csrc/n2v_kmeans.hip,
 * DESIGN.md "Clustering").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  X: row-major fp32 [n, dim],
 * 1 <= dim <= 1024, 0 <= n < 2^31; centroids: fp32 [k, dim], 1 <= k <= 1024; labels: int32 [n], -1 = no
 * cluster; inv_norm: the output of n2v_knn_inv_norms, required for N2V_KMEANS_COSINE, ignored otherwise.
 * Every result is a function of the arguments alone, bit for bit (no float atomics; the orders are written
 * out in csrc/n2v_kmeans.hip and restated in tests/cpu_kmeans/n2v_kmeans_cpu.c).  Argument errors are
 * N2V_EINVAL before any launch: sizes or metric out of range, cosine without inv_norm, then (n > 0) a NULL
 * required pointer, a workspace that is NULL, not 16-byte aligned or smaller than
 * n2v_kmeans_workspace_bytes, centroids_out == the input centroids.  n == 0 is N2V_OK and launches nothing. */
#define N2V_KMEANS_EUCLIDEAN 0 /* t(c, r) = fmaf(-2, dot(c, r), sum c^2);  dist = fmaxf(t_min + sum x_r^2, 0) */
#define N2V_KMEANS_COSINE 1    /* unit centroids: t(c, r) = -dot(c, r);  dist = 1 - dot_best * inv_norm[r] */

/* Rows per slab of the update's fixed order of summation (a multiple of 64; -1 for sizes the calls refuse):
 * round_up(ceil(n / S), 64) with S = min(2048, 512 MiB / (4 k dim)) slabs at most. */
int64_t n2v_kmeans_slab_rows(int64_t n, int32_t dim, int32_t k);
/* Bytes of workspace of the three calls below (-1 for sizes they refuse, 0 for n == 0): the padded centroids
 * and their squared norms, 4 round_up(k, 64) (round_up(dim, 16) + 1), plus one fp32 [k, dim] partial sum per
 * slab, 4 k dim ceil(n / slab_rows) <= 512 MiB whatever n is (each part rounded up to 256 bytes). */
int64_t n2v_kmeans_workspace_bytes(int64_t n, int32_t dim, int32_t k);
/* labels_out[r] = the lowest c with the smallest t(c, r); a row whose every t is NaN or +inf gets -1 and
 * dist NaN; a zero row gets label 0 and dist 1 by cosine.  dist_out: fp32 [n] or NULL. */
int n2v_kmeans_assign(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *centroids,
                      int32_t k, int32_t metric, int32_t *labels_out, float *dist_out, void *workspace,
                      int64_t workspace_bytes, void *stream);
/* centroids_out[c] = the mean of the rows of label c (cosine: the unit vector of the sum of their unit
 * vectors); a cluster without rows (cosine: or with a zero sum) keeps prev_centroids[c] bit for bit.
 * counts_out: int64 [k].  A label outside [-1, k) is treated as -1 and never used as an index. */
int n2v_kmeans_update(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int32_t *labels,
                      int32_t k, int32_t metric, const float *prev_centroids, float *centroids_out,
                      int64_t *counts_out, void *workspace, int64_t workspace_bytes, void *stream);
/* One Lloyd iteration that reads X once: n2v_kmeans_assign against centroids_in followed by
 * n2v_kmeans_update with centroids_in as the previous centroids, bit for bit.  labels_inout: the previous
 * labels in (any values), the new ones out; stats_out: int64 [2] = {labels that changed, rows left at -1}. */
int n2v_kmeans_step(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *centroids_in,
                    int32_t k, int32_t metric, int32_t *labels_inout, float *dist_out, float *centroids_out,
                    int64_t *counts_out, int64_t *stats_out, void *workspace, int64_t workspace_bytes,
                    void *stream);

/* One-vs-rest L2 logistic regression over trained vectors (the node2vec paper's multi-label classification,
 * section 4.3; csrc/n2v_logreg.hip, DESIGN.md "Node classification").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.
 * X: row-major fp32 [n, dim], 1 <= dim <= 1024, 0 <= n < 2^31; W: fp32 [c, dim], b: fp32 [c], 1 <= c <= 1024;
 * y_bits: uint32 [n][ceil(c / 32)], bit j of word w of a row is its label of class 32 w + j.
 * z[r][k] = dot(W_k, x_r) + b[k], dot being the fixed fmaf chain of the nearest-neighbour and k-means kernels.
 * Every result is a function of the arguments alone, bit for bit (no float atomics; the orders and the spelled
 * exp / log1p are written out in csrc/n2v_logreg.hip and restated in tests/cpu_logreg/n2v_logreg_cpu.c).
 * Argument errors are N2V_EINVAL before any launch: sizes out of range, then (n > 0) a NULL pointer, a
 * workspace that is NULL, not 16-byte aligned or smaller than n2v_logreg_workspace_bytes.  n == 0 is N2V_OK,
 * launches nothing and writes nothing. */

/* Rows per slab of the gradient's fixed order of summation (a multiple of 64; -1 for sizes the calls refuse):
 * round_up(max(1, ceil(n / S)), 64) with S = min(2048, 512 MiB / (4 c (dim + 3))) slabs at most. */
int64_t n2v_logreg_slab_rows(int64_t n, int32_t dim, int32_t c);
/* Bytes of workspace of the two calls below (-1 for sizes they refuse, 0 for n == 0): W padded to
 * [round_up(c, 64)][round_up(dim, 16)], plus per slab fp32 [c, dim] and [c] and fp64 [c] partials, <= 512 MiB
 * whatever n is, plus one more fp64 block (each part rounded up to 256 bytes). */
int64_t n2v_logreg_workspace_bytes(int64_t n, int32_t dim, int32_t c);
/* scores_out[r, k] = z[r][k], fp32 [n, c] row-major. */
int n2v_logreg_scores(const float *X, int64_t n, int32_t dim, const float *W, const float *b, int32_t c,
                      float *scores_out, void *workspace, int64_t workspace_bytes, void *stream);
/* One pass over X: loss_out[0] = sum over (r, k) of the logistic loss l(z[r][k], y[r][k]), grad_w_out[k, d] =
 * sum_r (sigmoid(z[r][k]) - y[r][k]) x_r[d] (fp64 [c, dim]), grad_b_out[k] = sum_r (sigmoid - y) (fp64 [c]):
 * unregularised sums, not means; fp32 chains per slab of rows, folded over the slabs in fp64. */
int n2v_logreg_loss_grad(const float *X, const uint32_t *y_bits, int64_t n, int32_t dim, const float *W,
                         const float *b, int32_t c, double *loss_out, double *grad_w_out, double *grad_b_out,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* The link-prediction classifier (node2vec paper, section 4.4; csrc/n2v_edge_logreg.hip, DESIGN.md
 * "Link-prediction classifier"): binary logistic regression on the edge feature f = op(x_a, x_b) of a list of pairs,
 * without the [n_pairs, dim] feature matrix.  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.
 * X: row-major fp32 [n, dim], 1 <= dim <= 1024, 0 <= n < 2^31; a, b: int64 [n_pairs] row numbers, 0 <= n_pairs <
 * 2^31; y: uint8 [n_pairs], nonzero is a positive; w: fp32 [dim]; b0: one fp32, by pointer (device memory); op: one
 * of N2V_PAIR_AVERAGE .. N2V_PAIR_L2.  f[d] are the bits n2v_pair_features writes; z = dot(w, f) + b0, dot in the
 * fixed order of n2v_pair_scores with (w, f) in the place of (x_a, x_b); the logistic functions are those of
 * n2v_logreg_*.  Every result is a function of the arguments alone, bit for bit, and does not change when a and b
 * are swapped (no float atomics; the order of summation is written out in csrc/n2v_edge_logreg.hip and restated in
 * tests/cpu_edge_logreg/n2v_edge_logreg_cpu.c).  Both calls only read X.  A pair with an index outside [0, n) is
 * never dereferenced: its score is NaN, and so are a loss and a gradient that include it.
 * Argument errors are N2V_EINVAL before any launch: sizes out of range, an unknown op, then (n_pairs > 0) a NULL
 * pointer, then a workspace that is NULL, not 16-byte aligned or smaller than n2v_edge_logreg_workspace_bytes.
 * n_pairs == 0 is N2V_OK, launches nothing and writes nothing. */

/* Pairs per slab of the gradient's fixed order of summation: n2v_logreg_slab_rows(n_pairs, dim, 1) (a multiple of
 * 64; -1 for sizes the calls refuse). */
int64_t n2v_edge_logreg_slab_pairs(int64_t n_pairs, int32_t dim);
/* Bytes of workspace of n2v_edge_logreg_loss_grad (-1 for sizes it refuses, 0 for n_pairs == 0): per slab (at most
 * 2048 of them) fp32 [dim] and [1] and fp64 [1] partials, each part rounded up to 256 bytes. */
int64_t n2v_edge_logreg_workspace_bytes(int64_t n_pairs, int32_t dim);
/* z_out[i] = z of pair i, fp32 [n_pairs]. */
int n2v_edge_logreg_scores(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                           int64_t n_pairs, int32_t op, const float *w, const float *b0, float *z_out,
                           void *stream);
/* One pass over the pairs: loss_out[0] = sum over i of the logistic loss l(z_i, y_i), grad_w_out[d] = sum_i
 * (sigmoid(z_i) - y_i) f_i[d] (fp64 [dim]), grad_b_out[0] = sum_i (sigmoid(z_i) - y_i): unregularised sums, not
 * means; fp32 chains per slab of pairs, folded over the slabs in fp64. */
int n2v_edge_logreg_loss_grad(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                              const uint8_t *y, int64_t n_pairs, int32_t op, const float *w, const float *b0,
                              double *loss_out, double *grad_w_out, double *grad_b_out, void *workspace,
                              int64_t workspace_bytes, void *stream);

/* The moments principal components need (csrc/n2v_pca.hip, DESIGN.md "Principal components").  ADDITIONS ONLY:
 * N2V_ABI_VERSION stays 15.  X: row-major fp32 [n, dim], 1 <= dim <= 1024, 0 <= n < 2^31; inv_norm: fp32 [n] or
 * NULL.  Row r enters as xh[d] = x[d] * inv_norm[r] (one fp32 multiply; NULL: x[d]) and is USED when all dim values
 * of xh are finite; every other row is skipped by both calls and not counted in n_used_out[0].  Every result is a
 * function of the arguments alone, bit for bit (no float atomics; the orders are written out in csrc/n2v_pca.hip
 * and restated in tests/cpu_pca/n2v_pca_cpu.c).  Argument errors are N2V_EINVAL before any launch: sizes out of
 * range, then (n > 0) a NULL pointer, a workspace that is NULL, not 16-byte aligned or smaller than
 * n2v_pca_workspace_bytes.  n == 0 is N2V_OK, launches nothing and writes nothing. */

/* Rows per slab of both calls' fixed order of summation (a multiple of 64; -1 for sizes the calls refuse):
 * round_up(max(1, ceil(n / S)), 64) with S = min(2048, 512 MiB / (4 round_up(dim, 16)^2)) slabs at most. */
int64_t n2v_pca_slab_rows(int64_t n, int32_t dim);
/* Bytes of workspace of the two calls below (-1 for sizes they refuse, 0 for n == 0): per slab an fp32
 * [round_up(dim, 16)]^2 partial scatter, an fp64 [dim] partial sum and a count (each part rounded up to 256). */
int64_t n2v_pca_workspace_bytes(int64_t n, int32_t dim);
/* mean_out[d] = (sum over the used rows of (double)xh[r][d]) / n_used, fp64 [dim]; zeros when no row is used. */
int n2v_pca_mean(const float *X, const float *inv_norm, int64_t n, int32_t dim, double *mean_out,
                 int64_t *n_used_out, void *workspace, int64_t workspace_bytes, void *stream);
/* scatter_out[a][b] = sum over the used rows of xc[r][a] xc[r][b], xc[r][d] = xh[r][d] - center[d] (one fp32
 * subtraction; center fp32 [dim], NULL: uncentred), fp64 [dim, dim], symmetric to the bit: fp32 fmaf chains per
 * slab of rows on the upper triangle, folded over the slabs in fp64 and written to both halves. */
int n2v_pca_scatter(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *center,
                    double *scatter_out, int64_t *n_used_out, void *workspace, int64_t workspace_bytes,
                    void *stream);

/* Approximate nearest neighbours over an inverted-file (IVF-flat) index of X (csrc/n2v_ivf.hip, DESIGN.md
 * "Approximate nearest neighbours").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  The index is device data over X in
 * place: list_off int64 [nlist + 1] and row_ids int32 [list_off[nlist]], the rows of X in list order (ascending
 * inside a list); max_list_rows >= the longest list.  probes: int32 [n_queries, nprobe], for every query the lists
 * it scans, -1 for an unused slot; a list a query names twice is refused (below).  A query's candidates are the rows of
 * its probed lists; out_rows / out_scores [n_queries, k] are the k best of them, every score equal to
 * n2v_knn_scores' of the same (query, row) bit for bit, by score descending, then row number ascending; a NaN score
 * is never selected; the tail is row -1, score -inf.  Nothing else is approximate: with every list probed the
 * result is n2v_knn_topk's.  Bounds: X as n2v_knn_*; 1 <= nlist <= 1024; 1 <= nprobe <= nlist; 1 <= k <= 128;
 * 1 <= max_list_rows <= n; n_queries < 2^20; exactly one of queries / query_rows non-NULL.  Argument errors are
 * N2V_EINVAL before any launch; n == 0 or n_queries == 0 is N2V_OK and launches nothing.  A list longer than
 * max_list_rows, offsets that descend, a probe outside [-1, nlist), a list number that an earlier entry of the same
 * query's probes names already, or a row id outside [0, n) sets N2V_ST_RANGE in status[0] (a device word, read after
 * synchronising): such a probe is skipped like an unused slot, the call still runs, reads nothing out of bounds or
 * uninitialised, and its results must be discarded. */

/* Bytes of workspace n2v_ivf_topk needs; -1 for sizes it refuses (also: more scan blocks than one launch takes --
 * split the queries), 0 for n == 0 or n_queries == 0.  Non-decreasing in n_queries, nprobe and k. */
int64_t n2v_ivf_workspace_bytes(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t n_queries,
                                int32_t nprobe, int32_t k);
/* The launch shape, for tests (host memory): plan3 = {(query, probe) pairs per tile: 16 or 64, rows per chunk of a
 * list: a multiple of 128, chunks per list = ceil(max_list_rows / rows per chunk)}. */
int n2v_ivf_plan(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t n_queries, int32_t nprobe,
                 int32_t k, int64_t *plan3);
/* workspace: 16-byte aligned, workspace_bytes >= n2v_ivf_workspace_bytes. */
int n2v_ivf_topk(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *list_off,
                 const int32_t *row_ids, int32_t nlist, int64_t max_list_rows, const float *queries,
                 const int64_t *query_rows, int64_t n_queries, const int32_t *probes, int32_t nprobe, int32_t k,
                 int64_t *out_rows, float *out_scores, uint32_t *status, void *workspace, int64_t workspace_bytes,
                 void *stream);

/* Product-quantised codes for the inverted-file index (IVF-PQ; csrc/n2v_ivfpq.hip, DESIGN.md "Product-quantised
 * codes").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  Beside list_off and row_ids (as n2v_ivf_*) the index is
 * codebooks fp32 [m, 256, dsub], dsub = ceil(dim / m) (the last sub-space padded; dims at or past dim are never
 * read), and codes uint8 [list_off[nlist], stride], 16-byte aligned, stride = m rounded up to 4, 8, 16, 32 or 64
 * (plan5[4]); row p of codes belongs to row_ids[p], bytes m .. stride are not looked at.  1 <= m <= min(dim, 64).
 * X is read only for a query given as a row (query_rows; X and inv_norm may be NULL with queries).  The arithmetic,
 * fp32, every product and sum rounded once, in an order no tile, chunk or launch size enters:
 *   lut[q][j][c] = ((+0 + q_hat[j dsub] w_j[c][0]) + q_hat[j dsub + 1] w_j[c][1]) + .., t ascending, j dsub + t < dim,
 *                  q_hat as n2v_knn_* build it;
 *   score(q, position p in the list of probe ordinal o) = ((coarse[q][o] + lut[q][0][codes[p][0]]) +
 *                  lut[q][1][codes[p][1]]) + .., j ascending.
 * coarse: fp32 [n_queries, nprobe], the first term of every probe (the query's score against that list's centroid).
 * out_rows / out_scores [n_queries, k]: the k best positions of the probed lists as ORIGINAL row numbers, by score
 * descending, then row number ascending; a NaN score (a NaN coarse score, a NaN table entry) is never selected;
 * the tail is row -1, score -inf.  Bounds and status as n2v_ivf_topk: 1 <= k <= 128, argument errors N2V_EINVAL
 * before any launch, n == 0 or n_queries == 0 N2V_OK without a launch; a list longer than max_list_rows, offsets
 * that descend, a probe outside [-1, nlist), a list number a query's probes repeat, or a row id outside [0, n) sets
 * N2V_ST_RANGE in status[0]: the call still runs, reads nothing out of bounds or uninitialised, and its results must
 * be discarded. */

/* Bytes of workspace n2v_ivfpq_topk needs (q_hat, fp32 [n_queries, m, 256] tables, the grouping tables, the slots);
 * -1 for sizes it refuses (also: more scan blocks than one launch takes -- split the queries), 0 for n == 0 or
 * n_queries == 0.  k == 0: the workspace of n2v_ivfpq_lut (q_hat alone; n, nlist, max_list_rows and nprobe are not
 * looked at). */
int64_t n2v_ivfpq_workspace_bytes(int64_t n, int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows,
                                  int64_t n_queries, int32_t nprobe, int32_t k);
/* The launch shape (host memory): plan5 = {(query, probe) pairs per tile T: 16 (m <= 7), 8 (m <= 16), 4 (m <= 32)
 * or 2, positions per chunk of a list: a multiple of 128, chunks per list = ceil(max_list_rows / positions per
 * chunk), bytes of LDS of a scan block (<= 160 KiB), bytes from one row of codes to the next}. */
int n2v_ivfpq_plan(int64_t n, int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows, int64_t n_queries,
                   int32_t nprobe, int32_t k, int64_t *plan5);
/* lut_out fp32 [n_queries, m, 256], the tables n2v_ivfpq_topk sums from.  workspace: 16-byte aligned, at least
 * n2v_ivfpq_workspace_bytes(.., k = 0). */
int n2v_ivfpq_lut(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                  const int64_t *query_rows, int64_t n_queries, const float *codebooks, int32_t m, float *lut_out,
                  void *workspace, int64_t workspace_bytes, void *stream);
/* workspace: 16-byte aligned, workspace_bytes >= n2v_ivfpq_workspace_bytes. */
int n2v_ivfpq_topk(const uint8_t *codes, const float *codebooks, int32_t m, const float *X, const float *inv_norm,
                   int64_t n, int32_t dim, const int64_t *list_off, const int32_t *row_ids, int32_t nlist,
                   int64_t max_list_rows, const float *queries, const int64_t *query_rows, int64_t n_queries,
                   const int32_t *probes, const float *coarse, int32_t nprobe, int32_t k, int64_t *out_rows,
                   float *out_scores, uint32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* Silhouette coefficients of a clustering of trained vectors (csrc/n2v_silhouette.hip, DESIGN.md "Cluster
 * quality").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  X, inv_norm, labels, k and metric as for n2v_kmeans_*
 * (metric: N2V_KMEANS_EUCLIDEAN, the true distance sqrt(max(|x_i|^2 + |x_j|^2 - 2 dot, 0)), or N2V_KMEANS_COSINE,
 * 1 - dot * inv_norm[i] * inv_norm[j]).  A row whose label is outside [0, k) belongs to no cluster: it is never
 * counted and never an index.  rows: int64 [m], the rows to score (any order, repeats allowed), or NULL for every
 * row (then m == n); 0 <= m < 2^31.  For scored row i of label L, n_c rows of label c and S(i, c) = the sum of
 * d(i, j) over the rows j != i of label c: a = S(i, L) / (n_L - 1); b = the smallest S(i, c) / n_c over c != L with
 * n_c > 0 (ties: the lowest c; NaN never wins), nearest = that c, or -1 and b = +inf when there is none;
 * s = (b - a) / max(a, b), and 0 when n_L == 1, nearest == -1 or max(a, b) == 0.  A scored row of no cluster, or
 * an entry of rows outside [0, n) (never dereferenced), gets a = b = s = NaN and nearest = -1.  a_out, b_out,
 * s_out: fp64 [m]; nearest_out: int32 [m]; counts_out: int64 [k] (n_c) or NULL.  Distances are fp32, the sums and
 * all that follows fp64, in one fixed order (no float atomics; written out in csrc/n2v_silhouette.hip and restated
 * in tests/cpu_silhouette/n2v_silhouette_cpu.c): the result is a function of the arguments alone, bit for bit, and
 * a row's values do not depend on which other rows are scored with it.  Argument errors are N2V_EINVAL before any
 * launch: sizes or metric out of range, cosine without inv_norm, rows NULL with m != n, then (n > 0 and m > 0) a
 * NULL required pointer, a workspace that is NULL, not 16-byte aligned or smaller than
 * n2v_silhouette_workspace_bytes.  n == 0 or m == 0 is N2V_OK, launches nothing and writes nothing. */

/* Bytes of workspace n2v_silhouette needs (-1 for sizes it refuses, 0 for n == 0 or m == 0): the scored rows padded
 * to [round_up(m, 64)][round_up(dim, 16)] fp32, fp32 [n] squared norms, the row list int32 [n + 16 k], int32
 * [ceil(n / slab)][k] counts with slab = round_up(max(1, ceil(n / 2048)), 1024), int32 [k] and int64 [k + 1] (each
 * part rounded up to 256 bytes). */
int64_t n2v_silhouette_workspace_bytes(int64_t n, int32_t dim, int32_t k, int64_t m);
int n2v_silhouette(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int32_t *labels, int32_t k,
                   int32_t metric, const int64_t *rows, int64_t m, double *a_out, double *b_out, double *s_out,
                   int32_t *nearest_out, int64_t *counts_out, void *workspace, int64_t workspace_bytes,
                   void *stream);

/* Exact t-SNE of 2-D points (csrc/n2v_tsne.hip, DESIGN.md "t-SNE").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.
 * Y: row-major fp32 [n, 2], 8-byte aligned, 0 <= n < 2^31.  A pair (i, j) in fp32, one rounding per operation:
 * dx = yi.x - yj.x; dy = yi.y - yj.y; d2 = fmaf(dy, dy, dx * dx); w = 1.0f / (1.0f + d2), correctly rounded.
 * Every result is a function of the arguments alone, bit for bit (no float atomics; the orders below are restated
 * in tests/cpu_tsne/n2v_tsne_cpu.c).  Argument errors are N2V_EINVAL before any launch: n out of range, then
 * (n > 0) a NULL or misaligned pointer, a workspace that is NULL, not 16-byte aligned or smaller than
 * n2v_tsne_workspace_bytes, Y_next == Y.  n == 0 is N2V_OK, launches nothing and writes nothing. */

/* The fixed order of the repulsion as numbers, a pure function of n: columns are cut into tiles of *tile (1024)
 * and into *n_slabs slabs of *slab_cols columns (whole tiles; n_slabs * slab_cols >= n), so that
 * ceil(n / 256) * n_slabs is about 2048 blocks at most. */
int n2v_tsne_plan(int64_t n, int32_t *tile, int64_t *slab_cols, int32_t *n_slabs);
/* Bytes of workspace n2v_tsne_repulse needs (-1 for an n it refuses, 0 for n == 0): fp64 [n_slabs][n][3] partials,
 * fp64 [ceil(n / 256)] block sums and a ticket (each part rounded up to 256 bytes). */
int64_t n2v_tsne_workspace_bytes(int64_t n);
/* rep_out fp64 [n, 2]: rep_i = sum_{j != i} w_ij^2 (y_i - y_j); zrow_out fp64 [n]: sum_{j != i} w_ij; z_out fp64
 * [1]: their sum.  j == i is skipped by index.  Order: per (row, slab) and tile, j ascending from +0 in fp32:
 * sw = sw + w; w2 = w * w; sx = fmaf(w2, dx, sx); sy = fmaf(w2, dy, sy); at the tile's end the three sums are added
 * (as doubles) to the slab's fp64 partials, tiles ascending from 0.0; the slabs' partials are added ascending from
 * 0.0.  z = 0.0 + b_0 + b_1 + .., b_k = 0.0 + zrow[256 k] + zrow[256 k + 1] + .. (at most 256 rows), all fp64. */
int n2v_tsne_repulse(const float *Y, int64_t n, double *rep_out, double *zrow_out, double *z_out, void *workspace,
                     int64_t workspace_bytes, void *stream);
/* One iteration's attraction, gradient and update in one launch.  P as CSR: rowptr int64 [n + 1], col int32 [nnz],
 * val fp32 [nnz] (a row's range is clamped to [0, nnz); a column outside [0, n) contributes nothing).  rep, Z:
 * n2v_tsne_repulse's of the same Y.  Row i: lane l of 16 takes entries rowptr[i] + l, + 16, .. ascending, a = val *
 * w; ax = fmaf(a, dx, ax); ay likewise, from +0; the 16 sums fold by v[l] = v[l] + v[l ^ m], m = 8, 4, 2, 1.  Per
 * coordinate: r = (float)(rep / Z[0]); g = 4.0f * (exaggeration * a - r); gain = ((g > 0) != (vel > 0)) ? gain +
 * 0.2f : gain * 0.8f; gain = fmaxf(gain, min_gain); vel = momentum * vel - learning_rate * (gain * g); y_next = y +
 * vel -- every product, sum and difference rounded once.  vel, gain: fp32 [n, 2], updated in place; Y_next, grad_out:
 * fp32 [n, 2], Y_next a buffer other than Y (other rows still read Y). */
int n2v_tsne_step(const int64_t *rowptr, const int32_t *col, const float *val, int64_t nnz, const float *Y,
                  const double *rep, const double *Z, int64_t n, float exaggeration, float learning_rate,
                  float momentum, float min_gain, float *vel, float *gain, float *Y_next, float *grad_out,
                  void *stream);

/* Filtered link-prediction ranks over trained vectors (csrc/n2v_linkrank.hip, DESIGN.md "Link ranking"): where the
 * held-out endpoint of an edge stands among ALL rows, the statistic behind filtered MRR, mean rank and Hits@K.
 * ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  X, inv_norm as for n2v_knn_* (the dot product: inv_norm all ones); a, b:
 * [n_queries] int64 row numbers (u_q, v_q), 0 <= n_queries < 2^31.  With s(u, w) the score n2v_knn_scores gives query
 * row u against row w, bit for bit, thr_q = s(u_q, v_q) and F(u) the distinct columns of row u of the filter CSR
 * (rowptr int64 [n + 1], col int32, ascending within a row, multi-edges adjacent, empty rows allowed; both NULL: no
 * filter):
 *   counts_out[q, 0] = #{ w in [0, n) : w != u_q, w != v_q, w not in F(u_q), s(u_q, w) >  thr_q }
 *   counts_out[q, 1] = the same with ==
 * A NaN on either side counts in neither: a NaN thr_q gives (0, 0).  thr_out: [n_queries] fp32 or NULL.  The
 * [n_queries, n] score matrix is never written: a scan over (query tile, chunk of rows) counts every row in integers
 * (integer atomic adds, no float atomics), then a pass over the lists {u, v} + F(u) takes their comparisons away again
 * with the same bits.  Argument errors are N2V_EINVAL before anything is launched (sizes, exactly one of rowptr / col,
 * NULL pointers, a workspace that is NULL, not 16-byte aligned or smaller than n2v_link_rank_workspace_bytes);
 * n_queries == 0 or n == 0 is N2V_OK and launches nothing.  a, b and col are device memory, which the host cannot
 * read without a synchronisation: a query with a row outside [0, n) is never dereferenced and answers thr NaN,
 * counts (0, 0) (callers check the rows where they are made, as for n2v_knn_*' query_rows); a column outside [0, n)
 * is skipped. */
/* Bytes of workspace n2v_link_rank needs (q_hat, the thresholds, the checked rows); -1 for sizes it refuses. */
int64_t n2v_link_rank_workspace_bytes(int64_t n, int32_t dim, int64_t n_queries);
/* The scan's launch shape for these sizes: chunks of *chunk_rows_out rows (a multiple of 128), *n_chunks_out of them,
 * the last one ragged. */
int n2v_link_rank_plan(int64_t n, int32_t dim, int64_t n_queries, int64_t *chunk_rows_out, int32_t *n_chunks_out);
int n2v_link_rank(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                  int64_t n_queries, const int64_t *rowptr, const int32_t *col, float *thr_out, int64_t *counts_out,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* Fold-in: rows for NEW vertices against a frozen skip-gram negative-sampling model (csrc/n2v_foldin.hip, DESIGN.md
 * "Fold-in").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.  walks: [n_walks, walk_len] int32, walk_len <=
 * N2V_SGNS_MAX_SENTENCE, n_walks < 2^31; a token in [0, n_vocab) is a known word, one in [n_vocab, n_vocab + n_new) is
 * new vertex tok - n_vocab, any other is dropped.  params: n_vocab, sentence_base, seed, dim, window, negative, alpha,
 * cum_index(_bits), row_alpha and max_waves as for n2v_sgns_train; deterministic is not read (the result is the same
 * bits on any launch geometry); batched and window_cache must be 0.  Sentence preparation is n2v_sgns_train's, but
 * a new token is always kept (sample_int has no entry for it).  A pair (centre position i, context position j) of
 * n2v_sgns_train is TRAINABLE when sent[j] is new and sent[i] is known; it is trained as there, on the new vertex's row,
 * with the same negative draws, and without the updates of syn1neg.  Everything but new_rows is only read.
 *
 * A record names one trainable pair; the pairs of one new vertex are trained in (row, i, j) ascending order. */
typedef struct n2v_foldin_record {
  int32_t vertex; /* the new index, tok - n_vocab */
  int32_t row;    /* the walk: the sentence is sentence_base + row */
  int32_t pos;    /* i | rel << 16: the centre's position in the prepared sentence, and the window slot
                     rel = j - i + window - (j > i) */
  int32_t centre; /* the known word sent[i] */
} n2v_foldin_record;

/* The pair listing, in two passes with the caller's exclusive prefix sum over rows in between:
 * row_count_out[r] = trainable pairs of walk r; then records_out[row_off[r] ...] = those pairs in (i, j) order, so that
 * the records stand in (row, i, j) order and no atomic decides an order.  Argument errors (whatever n2v_sgns_train
 * refuses, n_new < 0, n_vocab + n_new past the int32 tokens, NULL pointers) are N2V_EINVAL before anything is launched;
 * n_walks == 0 is N2V_OK. */
int n2v_foldin_pair_counts(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_new,
                           const uint32_t *sample_int, const n2v_sgns_params *params_host, int64_t *row_count_out,
                           void *stream);
int n2v_foldin_pair_records(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_new,
                            const uint32_t *sample_int, const n2v_sgns_params *params_host, const int64_t *row_off,
                            n2v_foldin_record *records_out, void *stream);

/* One pass (epoch) of chain training, one wave per new vertex.  records: the listing's, grouped by vertex with a STABLE
 * sort (the order inside a vertex stays (row, i, j)); vertex_off: int64 [n_new + 1], vertex u owns records
 * [vertex_off[u], vertex_off[u + 1]); new_rows: fp32 [n_new, dim], in place -- a vertex without records keeps its row.
 * params, n_walks and walk_len as for the listing that made the records (the draws are keyed on them).  A record whose
 * row, position or centre lies outside them is not trained.  Argument errors as above, a NULL new_rows with
 * n_new > 0 included, are N2V_EINVAL before anything is launched; n_new == 0 or n_walks == 0 is N2V_OK. */
int n2v_foldin_train(const n2v_foldin_record *records, const int64_t *vertex_off, int64_t n_new, int64_t n_walks,
                     int32_t walk_len, float *new_rows, const float *syn1neg, const uint32_t *cum_table,
                     const float *exp_table, const n2v_sgns_params *params_host, void *stream);

/* UMAP layouts of 2-D points (csrc/n2v_umap.hip, DESIGN.md "UMAP").  ADDITIONS ONLY: N2V_ABI_VERSION stays 15.
 * One epoch: rowptr int64 [n + 1], col int32 [nnz] ascending within a row, eps fp32 [nnz] (the epochs per sample,
 * w_max / w) are a symmetric CSR; Y, Y_next: row-major fp32 [n, 2], 8-byte aligned, Y_next a buffer other than Y.
 * Entry t fires in epoch e iff eps[t] is finite and >= 1 and floorf((float)(e + 1) / eps[t]) > floorf((float)e /
 * eps[t]); an entry whose column is outside [0, n) never fires; a row's range is clamped to [0, nnz).  Row i is one
 * sequential chain from y = Y[i] over its firing entries t ascending: two attractions towards Y[col[t]], then
 * `negative` repulsions from Y[k], k = ((mix64(ht ^ ((s + 1) * 0x8CB92BA72F3D8DD7)) >> 32) * n) >> 32 for s ascending
 * (k == i skipped), ht = mix64(he + (t + 1) * 0xD1B54A32D192ED03), he = mix64(seed ^ mix64(epoch +
 * 0x9E3779B97F4A7C15)); every other point is read from Y; Y_next[i] = y.  The fp32 operations of the two moves are
 * spelled at the top of csrc/n2v_umap.hip and restated in tests/cpu_umap/n2v_umap_cpu.c: the result is a function of
 * the arguments alone, bit for bit, whatever max_blocks (> 0: at most that many blocks; 0: a block per 256 rows).
 * No float atomics.  N2V_EINVAL before any launch: n outside [0, 2^31), nnz < 0, negative outside [0, 64], epoch
 * outside [0, 2^31 - 1), max_blocks < 0, a or b not finite and positive, gamma or alpha not finite; then (n > 0) a
 * NULL or misaligned pointer or Y_next == Y.  n == 0 is N2V_OK and launches nothing. */
int n2v_umap_epoch(const int64_t *rowptr, const int32_t *col, const float *eps, int64_t nnz, const float *Y,
                   float *Y_next, int64_t n, int32_t epoch, float a, float b, float gamma, float alpha,
                   int32_t negative, uint64_t seed, int32_t max_blocks, void *stream);
/* out[i] = the epoch's x[i]^b for x[i] > 0 (b == 1: x[i] itself; otherwise the spelled sequence of csrc/n2v_powb.h),
 * 0 for any other x[i].  N2V_EINVAL: n outside [0, 2^40), b not finite and positive, (n > 0) a NULL pointer. */
int n2v_umap_powb(const float *x, int64_t n, float b, float *out, void *stream);

/* DBSCAN of trained vectors (csrc/n2v_dbscan.hip, DESIGN.md "Density clustering").  ADDITIONS ONLY: N2V_ABI_VERSION
 * stays 15.  X, inv_norm and metric as for n2v_kmeans_*; 0 <= n < 2^31.  Rows i and j are WITHIN EPS when, in fp32
 * with one rounding per spelled operation and dot(i, j) the chain of n2v_silhouette,
 *   N2V_KMEANS_EUCLIDEAN  fmaxf(fmaf(-2, dot, xn_i + xn_j), 0) <= eps * eps   (xn: the row's sum of squares)
 *   N2V_KMEANS_COSINE     1 - dot * (inv_norm[i] * inv_norm[j]) <= eps
 * a test that is symmetric in (i, j) bit for bit; a row is always within eps of itself (added by index, not
 * computed).  The canonical result: row i is core when counts[i] = #{j within eps of i, i included} >= min_samples;
 * a cluster is a connected component of the core rows, numbered by its lowest core row; a row that is not core takes
 * the lowest-numbered cluster with a core row within eps of it, or -1.  It depends on the set of pairs alone: the
 * integer atomics that carry it cannot show, and max_blocks (> 0: at most that many blocks a scan; 0: what the device
 * holds at once, twice over) never changes a value.  Nothing of size n x n is stored.  The rows should be finite
 * (fmaxf drops a NaN: a Euclidean pair with a non-finite row counts as within eps).  The three calls are three scans
 * over (tile of columns x chunk of rows); the lists are device memory: an entry outside [0, n) is skipped, never
 * dereferenced.  N2V_EINVAL before any launch: sizes or metric out of range, cosine without inv_norm, eps negative
 * or not finite, min_samples < 1, max_blocks < 0, a list length outside [0, n]; then (n > 0) a NULL required pointer,
 * a workspace that is NULL, not 16-byte aligned or smaller than n2v_dbscan_workspace_bytes.  n == 0 is N2V_OK and
 * launches nothing. */

/* Bytes of workspace of each of the three calls (-1 for sizes they refuse, 0 for n == 0): the scan's columns padded
 * to [round_up(n, 64)][round_up(dim, 16)] fp32 and fp32 [n] squared norms (each part rounded up to 256 bytes). */
int64_t n2v_dbscan_workspace_bytes(int64_t n, int32_t dim);
/* Scan 1, every row against every row: counts_out int32 [n]; core_out uint8 [n] (counts >= min_samples) or NULL. */
int n2v_dbscan_count(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                     int32_t min_samples, int32_t *counts_out, uint8_t *core_out, void *workspace,
                     int64_t workspace_bytes, int32_t max_blocks, void *stream);
/* Scan 2, core rows against core rows (pairs on or above the diagonal of the list): core int32 [n_core], the core
 * rows; root_out int32 [n]: for a core row the lowest core row of its connected component (a lock-free union-find,
 * csrc/n2v_unionfind.h, then flattened), for any other row its own index. */
int n2v_dbscan_union(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                     const int32_t *core, int64_t n_core, int32_t *root_out, void *workspace,
                     int64_t workspace_bytes, int32_t max_blocks, void *stream);
/* Scan 3, rows that are not core against core rows: labels int32 [n] holds the cluster id of every core row and -1
 * elsewhere; labels[b] of every row b of border int32 [n_border] becomes the smallest labels[c] over the rows c of
 * core within eps of b (unchanged when there is none).  n_core == 0 or n_border == 0 is N2V_OK. */
int n2v_dbscan_border(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                      const int32_t *core, int64_t n_core, const int32_t *border, int64_t n_border, int32_t *labels,
                      void *workspace, int64_t workspace_bytes, int32_t max_blocks, void *stream);

#ifdef __cplusplus
}
#endif
#endif
