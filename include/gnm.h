/*
 * gnm.h -- C ABI of libgnm.so, the MI355X (gfx950) GatedGCN edge-logit engine.
 *
 * The reference (lvrcek/GNNome-assembly) has no FFI of its own: its hot path is ~120
 * lines of Python that call torch and DGL (un-vendored).  Each entry point below replaces
 * one group of those implicit kernels; the reference call site is cited per function
 * (paths relative to the reference repository root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the function says "host";
 *  - all float tensors are fp32, row-major, contiguous unless an explicit leading
 *    dimension (ld*, in elements) is given; all indices are int32;
 *  - the library never allocates, frees or keeps a pointer across calls; scratch space
 *    is a caller-provided workspace (gnm_*_workspace_bytes tells how much);
 *  - kernels are enqueued on `stream` (a hipStream_t passed as void*), no internal
 *    synchronisation, re-entrant;
 *  - return value: 0 ok, <0 invalid argument, >0 a hipError_t; gnm_last_error() returns a
 *    thread-local message for the last non-zero return.
 *  - "internal edge order" = edges stably sorted by destination (gnm_graph_build_index);
 *    all [E,*] tensors inside the layer stack are in that order, the model boundary
 *    (e_raw in, scores out, labels) is in the caller's edge-id order.
 *  - H (hidden width) must be one of 32, 64, 128, 256.
 */
#ifndef GNM_H
#define GNM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNM_ABI_VERSION 7   /* 2: per-call max_blocks_per_cu (edge_bwd_src, node_proj_bwd_tn), locality order; 3: sweep plans, two-sided sweeps; 4: H = 256 fused kernels; 5: LayerNorm entry points take the real width, node_bgrad its row pitch, fused node-side entry points, composite layer entry points; 6: matmul mode 2 (f16x2, the default), the pre-split image entry points (gnm_*_s3) and the Bs argument of gnm_tn128_bgrad removed, gnm_ln_edge_gate2_fwd; 7: gnm_edge_bwd_fused_gt (gt given: the LayerNorm backward's fused edge pass), gnm_ln_edge_bwd_top / gnm_ln_edge_bwd_src_fix (its two-sided sweep), gnm_ln_edge_bwd_chain (its chained form), gnm_debug_set_variant("gate2_wg") */

/* GEMM operand modes: C[M,N] = op(A) * op(B) (+bias +resid, relu) */
#define GNM_GEMM_NT 0 /* A[M,K] row-major, B[N,K] row-major  : y = x W^T   (nn.Linear forward)   */
#define GNM_GEMM_NN 1 /* A[M,K] row-major, B[K,N] row-major  : gx = gy W    (nn.Linear input grad) */
#define GNM_GEMM_TN 2 /* A[K,M] row-major, B[K,N] row-major  : gW = gy^T x  (nn.Linear weight grad)*/

int gnm_abi_version(void);
const char* gnm_last_error(void);
/* number of compute units of the current device (grid sizing / partial-buffer sizing) */
int gnm_num_cus(void);
/* upper bound on the number of per-block partial rows any kernel writes (see *_partials) */
int gnm_max_partial_blocks(void);
/* Process-wide configuration knobs (NOT per-call state; set them before the first launch, never while another
 * thread is inside the library).  Everything a launch needs beyond them travels in its arguments, so the entry
 * points themselves are re-entrant: two host threads, or one host on two streams, may call concurrently.
 *   gnm_set_matmul_mode     (below) which matrix-core arithmetic the fused kernels use;
 *   gnm_set_occupancy_cap   tools/ only: a default cap on workgroups per CU for every persistent kernel
 *                           (0 = none).  A host that co-schedules two kernels on two streams does NOT use it: the
 *                           entry points it needs take the cap per call (max_blocks_per_cu; 0 = none).       */
int gnm_set_occupancy_cap(int blocks_per_cu);

/* ---- graph index (HOST pointers; replaces DGL's lazy CSR/CSC build + dgl.reverse,
 *      layers/gated_gcn_full.py:115, graph_parser.py:297 edge-id order) -------------------
 * perm[j]    = caller edge id stored at internal position j (stable sort by dst)
 * isrc/idst  = endpoints in internal order; in_ptr[N+1] = CSC row pointer over internal order
 * out_ptr[N+1], out_pos[E], out_dst[E]: out-edges grouped by source (ascending internal
 *              position inside a source): internal position and destination of each. */
int gnm_graph_build_index(const int32_t* src, const int32_t* dst, int64_t N, int64_t E,
                          int32_t* perm, int32_t* isrc, int32_t* idst, int32_t* in_ptr,
                          int32_t* out_ptr, int32_t* out_pos, int32_t* out_dst);

/* ---- locality order of the nodes (HOST pointers).  The reference never sorts reads by position
 *      (pipeline.py:46-61,160-169 keep the simulator's read order; graph_parser.py:297-304 numbers nodes by
 *      read id), while the gather kernels rely on node ids that follow the genome (the node rows of the edges in
 *      flight must fit the 4 MB per-XCD L2).  The host renumbers the nodes INTERNALLY, once per graph:
 * edge_locality:  *frac_out = fraction of the edges with |src - dst| <= window in the caller's numbering
 *                 (decides whether a renumbering is needed at all);
 * locality_order: order[new] = old, rank[old] = new: breadth-first over the symmetrised graph restricted to the
 *                 triangle-supported edges (true overlaps are transitive; repeat-induced shortcuts would fold
 *                 the order) when those are at least half of the edges, every component started from a
 *                 pseudo-peripheral node; *core_frac_out (optional) = fraction of triangle-supported edges.   */
int gnm_graph_edge_locality(const int32_t* src, const int32_t* dst, int64_t N, int64_t E, int64_t window,
                            double* frac_out);
int gnm_graph_locality_order(const int32_t* src, const int32_t* dst, int64_t N, int64_t E, int32_t* order,
                             int32_t* rank, double* core_frac_out);

/* ---- sweep plan (HOST pointers): lets ONE destination-sorted sweep also form the by-SOURCE sums the reference takes
 *      on dgl.reverse(g) (gated_gcn_full.py:115,133-143 and their autograd duals) instead of a second pass over the
 *      [E,H] tensors.  Input: the internal index (isrc / idst / in_ptr of gnm_graph_build_index) and the partition of
 *      the sweep kernels (gnm_sweep_partition).  Output, per internal row j:
 *        sinfo[j] != 0 iff row j is the first row of its source inside its tile AND the sweep serves that source:
 *          bits 0-15 tile rows sharing the source | bits 16-21 accumulator slot | bit 22 first tile | bit 23 last tile
 *        dinfo[j]: the same for the row's destination (contiguous rows, two alternating slots);
 *      fix_nodes[0 .. *nfix_out): the nodes the sweep does not serve (out-edges in more than one workgroup, no free
 *      slot, farther than `margin` ids from the workgroup's node range, or no out-edges at all): the *_fix kernels
 *      cover them.  tile_rows <= 16, nslots <= 64; *peak_live_out (optional) = most slots ever in use.
 *      Returns 3 (nothing written, gnm_last_error() says which workgroup) when the node partition gives one workgroup more
 *      rows than the sweep kernels' 32-bit row offsets reach (> 2^21 - 64: a hub-heavy graph): such a graph has no plan and
 *      runs the separate by-source passes.                                                                              */
int gnm_graph_build_sweep_plan(const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr, int64_t N, int64_t E,
                               int64_t nodes_per_block, int tile_rows, int nslots, int64_t margin, uint32_t* sinfo,
                               uint32_t* dinfo, int32_t* fix_nodes, int64_t* nfix_out, int32_t* peak_live_out);
/* The same plan built ON THE DEVICE (device pointers, kernels queued on `stream`, no host synchronisation), bit for bit the
 * words of gnm_graph_build_sweep_plan: for graphs whose index never visits the host (the induced sub-graphs of the mini-batch
 * mode, train.py:288-343).  served[N] (bytes): 1 for the sources the sweep serves; fix_nodes[N] (optional): v for the nodes it does
 * not serve, -1 for the others -- the *_fix kernels skip negative entries, so the list is used as it is with nfix = N.
 * first / last [N] int32: scratch; peak [1] int32 (optional): most slots in use.  tile_rows = 16, nslots <= 64.          */
int gnm_graph_build_sweep_plan_device(const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr, int64_t N, int64_t E,
                                      int64_t nodes_per_block, int tile_rows, int nslots, int64_t margin, uint32_t* sinfo,
                                      uint32_t* dinfo, uint8_t* served, int32_t* fix_nodes, int32_t* first, int32_t* last,
                                      int32_t* peak, void* stream);
/* the partition of a sweep kernel on the current device: workgroup w owns the destination nodes
 * [w * nodes_per_block, (w+1) * nodes_per_block); *grid_out (optional) = workgroups launched.
 * wg_per_cu: 1 for gnm_edge_bwd_chain_src, 2 for gnm_edge_gate2_fwd (a plan serves ONE partition)            */
int gnm_sweep_partition(int64_t N, int wg_per_cu, int64_t* nodes_per_block, int* grid_out);

/* ---- the index of an induced sub-graph, derived from its parent's index (additive, ABI 7 unchanged) ----
 * dgl's g.subgraph(nodes) of the ClusterGCN mini-batches (train.py:288-293): nodes relabelled in ascending id, induced edges in
 * ascending edge id.  The parent's index (gnm_graph_build_index over its internal node numbering) is sorted already and both
 * relabellings are monotone, so every array of the sub-graph's index is the parent's with the dropped entries removed and the
 * kept ones renumbered: flags -> exclusive prefix sums -> gather / scatter.  No sort, no atomics, no allocation; DEVICE pointers,
 * kernels queued on `stream`.  node_mask [N] bytes (0 = dropped; 4-byte aligned); src / dst [E] the caller's edge list;
 * perm .. out_dst the parent's index; nperm / nrank: the parent's internal numbering, both NULL when it has none.
 * induce_count: writes the flags and the five prefix sums (new caller id, new internal id, new edge id, new destination-order
 *   and new by-source position) into ws (gnm_graph_induce_workspace_bytes(N, E), 16-byte aligned) and sizes[0] = n', sizes[1] = e'
 *   (device int64): the only two numbers the host has to read.  The prefix sums run over fixed blocks of
 *   gnm_graph_induce_scan_block() elements in three phases (block sums, one workgroup per sequence over the block sums, apply);
 *   no workgroup waits for another.  N, E >= 2^31 - 1 are rejected.
 * induce_fill: with n' and e' from the count on the same stream and ws untouched since, writes nid [n'] / eid [e'] (the kept
 *   nodes' / edges' ids, ascending), s_sub / d_sub [e'] (their ends, relabelled), the seven index arrays (in_ptr / out_ptr
 *   [n' + 1], the others [e']) and, when nrank is given, nrank_sub / nperm_sub [n'].  Arrays of length 0 may be NULL.  Sizes
 *   that are not the count's give wrong numbers but no access outside the arrays as sized by n_sub / e_sub.                */
int gnm_graph_induce_scan_block(void);
size_t gnm_graph_induce_workspace_bytes(int64_t N, int64_t E);
int gnm_graph_induce_count(int64_t N, int64_t E, const int32_t* src, const int32_t* dst, const uint8_t* node_mask,
                           const int32_t* perm, const int32_t* out_pos, const int32_t* nperm, void* ws, size_t ws_bytes,
                           int64_t* sizes, void* stream);
int gnm_graph_induce_fill(int64_t N, int64_t E, int64_t n_sub, int64_t e_sub, const int32_t* src, const int32_t* dst,
                          const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                          const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nrank,
                          const void* ws, size_t ws_bytes, int32_t* nid, int32_t* eid, int32_t* s_sub, int32_t* d_sub,
                          int32_t* perm_sub, int32_t* isrc_sub, int32_t* idst_sub, int32_t* in_ptr_sub, int32_t* out_ptr_sub,
                          int32_t* out_pos_sub, int32_t* out_dst_sub, int32_t* nrank_sub, int32_t* nperm_sub, void* stream);

/* ---- greedy decode (HOST pointers, sequential CPU work; inference.py:31-77,182-253) ----------
 * build_adjacency: successors / predecessors of every node in edge-id order, as the reference's
 *   succ / pred dicts (graph_parser.py:13-73); *_eid[p] = edges[(node, nbr)] of its edges dict, i.e. the
 *   LAST edge id of a duplicated (src, dst) pair.  ptr arrays hold N+1, nbr / eid arrays E entries.
 * decode_iteration: one pass of get_contigs' loop body for `nb` sampled start edges
 *   (start_src[i] -> start_dst[i]): greedy forward walk from the head, backward walk from the tail
 *   (forced single-neighbour moves, otherwise the best-scored neighbour that is neither in visited[]
 *   nor consumed by this walk; a node consumes its reverse complement node ^ 1), the walk with the
 *   greatest reconstructed length (sum of prefix_length over its edges + read_length of its last node)
 *   wins.  Returns its node count, the nodes in walk_out, the length in *best_length_out; when the count is
 *   >= len_threshold, visited[] (N bytes, in/out) absorbs the walk, the complements and the jumped-over
 *   nodes.  < 0: error (-3: a cycle of forced moves, on which the reference does not terminate).     */
int gnm_decode_build_adjacency(const int32_t* src, const int32_t* dst, int64_t N, int64_t E,
                               int32_t* succ_ptr, int32_t* succ_nbr, int32_t* succ_eid,
                               int32_t* pred_ptr, int32_t* pred_nbr, int32_t* pred_eid);
int64_t gnm_decode_iteration(int64_t N, const float* scores, const int64_t* prefix_length,
                             const int64_t* read_length, const int32_t* succ_ptr, const int32_t* succ_nbr,
                             const int32_t* succ_eid, const int32_t* pred_ptr, const int32_t* pred_nbr,
                             const int32_t* pred_eid, uint8_t* visited, int nb, const int32_t* start_src,
                             const int32_t* start_dst, int len_threshold, int32_t* walk_out,
                             int64_t walk_cap, int64_t* best_length_out);
/* decode_iteration_mt: the same iteration, the nb candidates dealt out to min(threads, nb) host threads (each with its own
 *   seen arrays; the choice of the winner and the visited[] update happen in the calling thread after the join).  Identical
 *   results: the first of equally long walks, the same visited[], the same error codes (of the lowest failing candidate).
 *   threads <= 1 IS gnm_decode_iteration.                                                                                  */
int64_t gnm_decode_iteration_mt(int64_t N, const float* scores, const int64_t* prefix_length,
                                const int64_t* read_length, const int32_t* succ_ptr, const int32_t* succ_nbr,
                                const int32_t* succ_eid, const int32_t* pred_ptr, const int32_t* pred_nbr,
                                const int32_t* pred_eid, uint8_t* visited, int nb, const int32_t* start_src,
                                const int32_t* start_dst, int len_threshold, int32_t* walk_out,
                                int64_t walk_cap, int64_t* best_length_out, int threads);

/* ---- decode: start edges sampled on the device (DEVICE pointers; inference.py:256-277) ----------
 * For edge k = (src[k] -> dst[k]) with logit scores[k] and visited[N] (uint8):
 *   w_k = 0 if visited[src[k]] | visited[dst[k]] | (src[k] == dst[k]) (get_subgraph, self loops are no candidates),
 *         else max(sigmoid(scores[k]), 1e-9f) (the fp32 number nearest to the fp64 sigmoid)
 *   C_k = w_0 + ... + w_k in fp64;  pick(u) = the smallest k with w_k > 0 and C_k > u * C_{E-1}, u in [0, 1)
 * -- the distribution of the reference's sample_edges (p = w / sum over the candidate edges), drawn by inverse CDF.
 * decode_candidate_sums: one streaming pass forms the fp64 sums of w over FIXED blocks of 2048 edge ids (the summation tree does
 *   not depend on the grid, the CU count or gnm_set_occupancy_cap; no atomics: two runs are bit-identical), one workgroup turns
 *   them into the block prefix in `ws` (gnm_decode_sample_workspace_bytes(E), 16-byte aligned) and writes `stats` (32 bytes:
 *   double total = C_{E-1}; int64 count = #{w_k > 0}; int64 the last block with a candidate; int64 the block count).
 *   w_out: NULL, or [E] fp32 that receives w (tests; the product path recomputes w in decode_pick).  E == 0: stats zeroed, no launch.
 * decode_pick: picks[i] = pick(u[i]) for i < nb, one wave per draw: binary search over the block prefix, then a scan of that
 *   block's weights in edge-id order.  Same scores / src / dst / visited / ws / stats as the decode_candidate_sums call before it
 *   on the same stream.  u * total rounding up to total gives the LAST edge with w > 0; an edge with w = 0 is never picked;
 *   count == 0 leaves picks untouched.  E == 0 or nb == 0: no launch.                                                       */
size_t gnm_decode_sample_workspace_bytes(int64_t E);
int gnm_decode_candidate_sums(int64_t E, int64_t N, const float* scores, const int32_t* src, const int32_t* dst,
                              const uint8_t* visited, void* ws, size_t ws_bytes, float* w_out, void* stats, void* stream);
int gnm_decode_pick(int64_t E, int64_t N, const float* scores, const int32_t* src, const int32_t* dst,
                    const uint8_t* visited, const void* ws, const void* stats, int nb, const double* u, int32_t* picks,
                    void* stream);

/* ---- dense (fp32 MFMA v_mfma_f32_32x32x2_f32): nn.Linear call sites
 *      gated_gcn_full.py:107-113, full_graph.py:23-26, score_predictor.py:15-17 and their
 *      autograd duals.  TN mode reduces over K with split-K partials in the workspace. */
size_t gnm_gemm_f32_workspace_bytes(int mode, int64_t M, int64_t N, int64_t K);
int gnm_gemm_f32(int mode, int64_t M, int64_t N, int64_t K,
                 const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc,
                 const float* bias,                 /* [N] or NULL */
                 const float* resid, int64_t ldr,   /* [M,N] added to the result, or NULL */
                 int relu, void* ws, size_t ws_bytes, void* stream);

/* column sums out[c] = sum_m X[m*ld + c], c < W (bias gradients). ws: gnm_colsum_workspace_bytes */
size_t gnm_colsum_workspace_bytes(int64_t M, int64_t W);
int gnm_colsum_f32(int64_t M, int64_t W, const float* X, int64_t ld, float* out,
                   void* ws, size_t ws_bytes, void* stream);

/* Weight AND bias gradient of a Linear in one call (autograd of nn.Linear under loss.backward(), train.py:257):
 * C[M,N] = A[K,M]^T B[K,N], colsum[m] = sum_k A[k][m].  One pass over A where the split-mode kernel applies
 * (bf16x3 matmul mode, M and N multiples of 128, K >= 4096), gnm_gemm_f32(TN) + gnm_colsum_f32 otherwise. */
size_t gnm_gemm_tn_colsum_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gnm_gemm_tn_colsum(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                       float* C, int64_t ldc, float* colsum, void* ws, size_t ws_bytes, void* stream);

/* out[j, 0:W] = X[idx[j], 0:W]  (edge features: caller edge-id order -> internal order) */
int gnm_gather_rows_f32(int64_t M, int64_t W, const float* X, const int32_t* idx, float* out,
                        void* stream);
/* x = (ref > 0) ? x : 0, elementwise over n floats (relu backward for the tiny encoders) */
int gnm_relu_mask_f32(int64_t n, float* x, const float* ref, void* stream);

/* ---- BatchNorm1d(track_running_stats=False) statistics: gated_gcn_full.py:122,147 ------
 * partials: double[nblk][2][H] = per-block (sum x, sum x^2) written by the *_stats kernels.
 *           The buffer must hold (gnm_max_partial_blocks() + 1) * 2 * 256 doubles: the row
 *           after the last possible partial row is the finalisers' reduction scratch.
 * stat out: float[4][H] = mean, rstd, scale = gamma*rstd, shift = beta - mean*scale.      */
int gnm_bn_finalize(const double* partials, int nblk, int64_t count, int H,
                    const float* gamma, const float* beta, float eps, float* stat, void* stream);
/* backward: partials = per-block (sum gy, sum gy*xhat).  bstat: float[2][H] = mean(gy),
 * mean(gy*xhat); ggamma[H] = sum gy*xhat, gbeta[H] = sum gy. */
int gnm_bn_bwd_finalize(const double* partials, int nblk, int64_t count, int H,
                        float* bstat, float* ggamma, float* gbeta, void* stream);

/* ---- GatedGCN layer, forward (gated_gcn_full.py:120-152) --------------------------------
 * P = [A1h|A2h|A3h|B1h|B2h] is the [N,5H] node projection (ld 5H).
 * edge_t_stats: t[j] += B1h[isrc j] + B2h[idst j]  (t holds B3e on entry), per-block
 *               (sum t, sum t^2) -> partials.                                   (:120-121) */
int gnm_edge_t_stats_fwd(int64_t E, int H, float* t, const float* P, const int32_t* isrc,
                         const int32_t* idst, double* partials, int* nblk_out, void* stream);
/* (e_in == NULL / h_in == NULL in the four forward kernels below and their LayerNorm twins: no residual --
 *  GatedGCN_1d(residual=False), or in_channels != out_channels which drops it: gated_gcn_full.py:41-42,124-125,151-152)
 * edge_gate: e_out = relu(t*scale+shift) + e_in; sigma = sigmoid(e_out);
 *            hf[v] = sum_{in(v)} sigma*A2h[src] / (sum sigma + 1e-6); inv_f = 1/(sum sigma + 1e-6)
 *                                                                      (:122-130) */
int gnm_edge_gate_fwd(int64_t N, int64_t E, int H, const float* t, const float* e_in,
                      const float* stat_e, const float* P, const int32_t* isrc,
                      const int32_t* in_ptr, float* e_out, float* hf, float* inv_f, void* stream);
/* edge_gate2 (H = 128; H = 256: the sweep is column-separable and runs once per 128-column half with row pitch 256):
 *   gnm_edge_gate_fwd AND gnm_node_agg_src_fwd as ONE two-sided sweep over the destination-sorted
 *   rows (same outputs: e_out, hf, inv_f, hb, inv_b, z, BatchNorm_h partials; e_out is not re-read): the by-source
 *   sums through the sweep plan (sinfo / dinfo / fix_nodes of gnm_graph_build_sweep_plan over
 *   gnm_sweep_partition(N, 2)); the plan's fix_nodes are covered by gathers.  inv_f == inv_b == NULL: a forward
 *   without a backward (torch.no_grad: inference.py:444) does not store what only the backward reads.  (:122-147) */
int gnm_edge_gate2_fwd(int64_t N, int64_t E, int H, const float* t, const float* e_in, const float* stat_e,
                       const float* P, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                       const uint32_t* sinfo, const uint32_t* dinfo, int64_t plan_nodes_per_block, int64_t nfix,
                       const int32_t* fix_nodes, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                       float* e_out, float* hf, float* inv_f, float* hb, float* inv_b, float* z, double* partials,
                       int* nblk_out, void* stream);
/* the same sweep for a LayerNorm layer (batch_norm = False; H = 128; width = the layer's real out_channels, see the gnm_ln_*
 * entry points): gnm_ln_edge_gate_fwd AND gnm_node_agg_src_fwd in one pass, e_out bit-identical to gnm_ln_edge_gate_fwd's.
 * `partials` receives column sums nobody needs (z is formed by the same kernel as in the BatchNorm form).          (:122-147) */
int gnm_ln_edge_gate2_fwd(int64_t N, int64_t E, int H, const float* t, const float* e_in, const float* gamma_e,
                          const float* beta_e, int width, const float* P, const int32_t* isrc, const int32_t* idst,
                          const int32_t* in_ptr, const uint32_t* sinfo, const uint32_t* dinfo, int64_t plan_nodes_per_block,
                          int64_t nfix, const int32_t* fix_nodes, const int32_t* out_ptr, const int32_t* out_pos,
                          const int32_t* out_dst, float* e_out, float* hf, float* inv_f, float* hb, float* inv_b, float* z,
                          double* partials, int* nblk_out, void* stream);
/* node_agg_src: hb[v] = sum_{out(v)} sigma*A3h[dst] / (sum sigma + 1e-6), inv_b likewise;
 *               z = A1h + hf + hb; per-block (sum z, sum z^2) -> partials   (:133-145) */
int gnm_node_agg_src_fwd(int64_t N, int64_t E, int H, const float* e_out, const float* P,
                         const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                         const float* hf, float* hb, float* inv_b, float* z, double* partials,
                         int* nblk_out, void* stream);
/* node_update: h_out = relu(z*scale+shift) + h_in                             (:147-152) */
int gnm_node_update_fwd(int64_t N, int H, const float* z, const float* stat_h, const float* h_in,
                        float* h_out, void* stream);
/* ---- GatedGCN layer, backward (autograd of the above) -------
 * node_bwd_stats: gw = gh_out*[relu(bn(z))>0]; partials (sum gw, sum gw*zhat)            */
int gnm_node_bwd_stats(int64_t N, int H, const float* z, const float* stat_h, const float* gh_out,
                       double* partials, int* nblk_out, void* stream);
/* node_bwd_apply: gz = gamma*rstd*(gw - m1 - zhat*m2) -> gP[:,0:H];
 *                 Q[N,2H] = Qf | Qb = gz*inv_f | gz*inv_b                                 */
int gnm_node_bwd_apply(int64_t N, int H, const float* z, const float* stat_h, const float* bstat_h,
                       const float* gamma_h, const float* gh_out, const float* inv_f, const float* inv_b,
                       float* gP, float* Q, void* stream);
/* edge_bwd_dst (internal order, by destination), Rf = Qf*hf, Rb = Qb*hb formed from the saved hf / hb rows:
 *   gsigma = Qf[d]*A2h[s] - Rf[d] + Qb[s]*A3h[d] - Rb[s];  ge <- ge + gsigma*sigma*(1-sigma)
 *   gu = ge*[t*scale+shift > 0];  partials (sum gu, sum gu*that)
 *   gP[:,2H:3H][d] = sum sigma*Qb[s];  Ud[d] = sum gu;  Td[d] = sum that                 */
int gnm_edge_bwd_dst(int64_t N, int64_t E, int H, const float* e_out, const float* t,
                     const float* stat_e, float* ge, const float* P, const float* Q,
                     const float* hf, const float* hb,
                     const int32_t* isrc, const int32_t* in_ptr, float* gP, float* Ud, float* Td,
                     double* partials, int* nblk_out, void* stream);
/* edge_bwd_src (by source, after bn_bwd_finalize):
 *   gP[:,H:2H][v]  = sum_{out(v)} sigma*Qf[dst]
 *   gP[:,3H:4H][v] = c*(sum_{out(v)} gu - outdeg*m1 - m2*sum_{out(v)} that)   (= sum gt)
 *   gP[:,4H:5H][v] = c*(Ud[v] - indeg*m1 - m2*Td[v]),  c = gamma_e*rstd_e                */
int gnm_edge_bwd_src(int64_t N, int64_t E, int H, const float* e_out, const float* t,
                     const float* stat_e, const float* bstat_e, const float* gamma_e,
                     const float* ge, const float* Q, const int32_t* in_ptr,
                     const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                     const float* Ud, const float* Td, float* gP, int max_blocks_per_cu, void* stream);
/* edge_bwd_gt: gt = gamma*rstd*(gu - m1 - that*m2), gu = ge*[t*scale+shift > 0]          */
int gnm_edge_bwd_gt(int64_t E, int H, const float* ge, const float* t, const float* stat_e,
                    const float* bstat_e, const float* gamma_e, float* gt, void* stream);

/* ---- LayerNorm mode (batch_norm=False: nn.LayerNorm(H) for bn_h / bn_e, gated_gcn_full.py:57-59) ---
 * Row-wise normalisation, no global barrier.  The projections, t (gnm_edge_t_stats_fwd or the fused
 * form) and gnm_node_agg_src_fwd are shared with BatchNorm mode (their column partials are unused).
 * ln_edge_gate_fwd   e_out = relu(LN(t)*gamma+beta) + e_in, sigma, by-destination gated mean
 * ln_node_update_fwd h_out = relu(LN(z)*gamma+beta) + h_in
 * ln_node_bwd        gz -> gP[:,0:H], Q[N,4H]; partials (sum gw, sum gw*zhat) -> gnm_bn_bwd_finalize
 * ln_edge_bwd_dst    ge <- ge + gsigma*sigma'; gt = LNbwd(ge*[u>0]) -> gt[E,H]; gP[:,2H:3H] = sum
 *                    sigma*Qb[s]; gP[:,4H:5H] = sum_dst gt; partials (sum gu, sum gu*that)
 * ln_edge_bwd_src    gP[:,H:2H] = sum_src sigma*Qf[d]; gP[:,3H:4H] = sum_src gt
 * (B_3 gradients and ge_in then come from gnm_gemm_f32 TN/NN + gnm_colsum_f32 on gt.)
 * width (ABI 5): the layer's REAL channel count, 1 <= width <= H.  nn.LayerNorm(out_channels) takes its mean and
 * variance over out_channels; a layer that runs on the next kernel width up (H > width: the channels width .. H-1 are
 * dead -- zero weights, zero inputs) must not count them: they get xhat = 0 and are left out of every row mean.  */
int gnm_ln_edge_gate_fwd(int64_t N, int64_t E, int H, const float* t, const float* e_in,
                         const float* gamma, const float* beta, const float* P, const int32_t* isrc,
                         const int32_t* in_ptr, float* e_out, float* hf, float* inv_f, int width, void* stream);
int gnm_ln_node_update_fwd(int64_t N, int H, const float* z, const float* gamma, const float* beta,
                           const float* h_in, float* h_out, int width, void* stream);
int gnm_ln_node_bwd(int64_t N, int H, const float* z, const float* gamma, const float* beta,
                    const float* gh_out, const float* hf, const float* inv_f, const float* hb,
                    const float* inv_b, float* gP, float* Q, double* partials, int* nblk_out,
                    int width, void* stream);
int gnm_ln_edge_bwd_dst(int64_t N, int64_t E, int H, const float* e_out, const float* t,
                        const float* gamma, const float* beta, float* ge, const float* P, const float* Q,
                        const int32_t* isrc, const int32_t* in_ptr, float* gP, float* gt,
                        double* partials, int* nblk_out, int width, void* stream);
int gnm_ln_edge_bwd_src(int64_t N, int64_t E, int H, const float* e_out, const float* gt, const float* Q,
                        const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                        float* gP, void* stream);
/* LayerNorm layers wider than 256 channels (additive, ABI 7 unchanged).  Such a layer runs zero-padded to Hp = 256 C columns as C
 * chunks on contiguous [rows,256] copies, like the BatchNorm wide path, but LayerNorm's row statistics span the chunks: they are
 * formed once per row and handed to the per-chunk kernels, and the two row means of the backward are summed chunk by chunk.
 * Every per-chunk call takes c0 >= 0, c0 % 4 == 0 (the chunk's first column in the layer) and width >= 1 (the layer's real channel
 * count): the channels c0 + j >= width are dead.  gamma / beta point at the chunk's 256 entries.  Call the chunks of one phase in
 * ASCENDING c0 on one stream: c0 == 0 starts a row sum, every later chunk adds to it.  No atomics; bit-reproducible.
 *
 * gnm_ln_wide_row_stats: stat[r] = (mean, rstd = 1/sqrt(var + 1e-5)) over the live channels of row r, r < R, whose chunk c is
 *   x[c * chunk_stride + r * 256 .. + 255] (a [C,R,256] stack: chunk_stride = 256 R).  Centred variance, mean with one correction step.
 * gnm_ln_wide_edge_gate_fwd / gnm_ln_wide_node_update_fwd: gnm_ln_edge_gate_fwd / gnm_ln_node_update_fwd at H = 256 on one chunk
 *   with xhat = (x - mean) rstd from stat ([E,2] / [N,2]).  e_in / h_in NULL: no residual.
 * gnm_ln_wide_node_bwd_sums (phase A): rowsum[v] (+)= (sum a, sum a zhat), a = gamma gh_out [w > 0]; partials = the chunk's
 *   (sum gw, sum gw zhat) for gnm_bn_bwd_finalize.  gnm_ln_wide_node_bwd_apply (phase B, after phase A of EVERY chunk): gz ->
 *   gP[:,0:256] of the chunk's [N,1280] and Q [N,1024] = Qf | Rf | Qb | Rb as gnm_ln_node_bwd.
 * gnm_ln_wide_edge_bwd_sums (phase A): gnm_ln_edge_bwd_dst up to gu -- ge <- ge + gsigma sigma' in place, gP[:,512:768] = gA3h,
 *   partials (sum gu, sum gu that) -- and rowsum[j] (+)= (sum gamma gu, sum gamma gu that) instead of gt.
 *   gnm_ln_wide_edge_bwd_apply (phase B, after phase A of EVERY chunk): gt [E,256] and gP[:,1024:1280] = gB2h; then
 *   gnm_ln_edge_bwd_src (H = 256) for gA2h / gB1h.                      autograd of gated_gcn_full.py:120-152 under nn.LayerNorm */
int gnm_ln_wide_row_stats(int64_t R, int C, const float* x, int64_t chunk_stride, int width, float* stat, void* stream);
int gnm_ln_wide_edge_gate_fwd(int64_t N, int64_t E, const float* t, const float* e_in, const float* gamma,
                              const float* beta, const float* stat, const float* P, const int32_t* isrc,
                              const int32_t* in_ptr, float* e_out, float* hf, float* inv_f, int c0, int width,
                              void* stream);
int gnm_ln_wide_node_update_fwd(int64_t N, const float* z, const float* stat, const float* gamma, const float* beta,
                                const float* h_in, float* h_out, int c0, int width, void* stream);
int gnm_ln_wide_node_bwd_sums(int64_t N, const float* z, const float* stat, const float* gamma, const float* beta,
                              const float* gh_out, float* rowsum, double* partials, int* nblk_out, int c0, int width,
                              void* stream);
int gnm_ln_wide_node_bwd_apply(int64_t N, const float* z, const float* stat, const float* gamma, const float* beta,
                               const float* gh_out, const float* rowsum, const float* hf, const float* inv_f,
                               const float* hb, const float* inv_b, float* gP, float* Q, int c0, int width, void* stream);
int gnm_ln_wide_edge_bwd_sums(int64_t N, int64_t E, const float* e_out, const float* t, const float* stat,
                              const float* gamma, const float* beta, float* ge, const float* P, const float* Q,
                              const int32_t* isrc, const int32_t* in_ptr, float* gP, float* rowsum, double* partials,
                              int* nblk_out, int c0, int width, void* stream);
int gnm_ln_wide_edge_bwd_apply(int64_t N, int64_t E, const float* t, const float* stat, const float* gamma,
                               const float* beta, const float* ge, const float* rowsum, const int32_t* in_ptr, float* gt,
                               float* gP, int c0, int width, void* stream);
/* round 6 (ABI 7), H = 128 with a sweep plan: gnm_ln_edge_bwd_dst + gnm_ln_edge_bwd_src as ONE two-sided sweep (the LayerNorm form of
 * gnm_edge_bwd_top): ge <- ge + gsigma sigma' in place, gt [E,H] written for gnm_edge_bwd_fused_gt, gP[:, H:5H] = gA2h | gA3h | gB1h | gB2h
 * of the nodes the plan serves, partials = (sum gu, sum gu that); then the plan's unserved sources by gathers.  Q = gnm_ln_node_bwd's [N,4H].
 * ws >= gnm_edge_bwd_fused_workspace_bytes().                        autograd of gated_gcn_full.py:120-143 under nn.LayerNorm (:57-59) */
int gnm_ln_edge_bwd_top(int64_t N, int64_t E, int H, float* ge, const float* e_out, const float* t, const float* gamma_e,
                        const float* beta_e, int width, const float* P, const float* Q, const float* hf, const float* hb,
                        const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr, float* gP, float* gt,
                        double* partials, const uint32_t* sinfo, int64_t plan_nodes_per_block, int* nblk_out, void* ws,
                        size_t ws_bytes, void* stream);
int gnm_ln_edge_bwd_src_fix(int64_t nfix, const int32_t* fix_nodes, int64_t N, int64_t E, int H, const float* e_out,
                            const float* gt, const float* Q, const int32_t* out_ptr, const int32_t* out_pos,
                            const int32_t* out_dst, float* gP, void* stream);
/* The chained form (split matmul modes): gnm_edge_bwd_fused_gt of layer i (gt_hi: the gt layer i's own sweep wrote) AND gnm_ln_edge_bwd_top of
 * layer i-1 in one sweep: ge (in place) holds d loss / d e_out(i) on entry and ge_tot(i-1) on exit, gt_lo receives layer i-1's gt; gW3_hi / gb3_hi
 * the B_3 gradients of layer i.  partials_hi [grid][128] and partials_lo [grid][2][128] must differ.      train.py:257 under nn.LayerNorm */
int gnm_ln_edge_bwd_chain(int64_t N, int64_t E, int H, float* ge, const float* gt_hi, const float* e_mid, const float* W3_hi,
                          float* gW3_hi, float* gb3_hi, double* partials_hi, const float* t_lo, const float* gamma_lo,
                          const float* beta_lo, int width, const float* P_lo, const float* Q_lo, const float* hf_lo,
                          const float* hb_lo, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr, float* gP_lo,
                          float* gt_lo, double* partials_lo, const uint32_t* sinfo, int64_t plan_nodes_per_block,
                          int* nblk_out, void* ws, size_t ws_bytes, void* stream);

/* ---- fused W-stationary MFMA kernels (H = 128 only; other H use the unfused entry points) ---
 * edge_t_fused_fwd: t = e_in W3^T + b3 + B1h[isrc] + B2h[idst] and the BatchNorm partials in ONE
 *                   pass (gemm NT + gnm_edge_t_stats_fwd).            gated_gcn_full.py:113,120-122
 * node_proj_fwd:    Pout[N,ncols] = h W^T + b, W [ncols,128] row-major, ncols % 128 == 0 (:107-112)
 * node_proj_bwd:    gh_in = gh_out + gP W;  gW = gP^T h_in;  gb = sum gP   (gP [N,ncols])
 *                   (gemm NN + gemm TN + colsum).                        autograd of :107-112
 * edge_bwd_fused:   gt = gamma*rstd*(gu - m1 - that*m2), gu = ge*[t*scale+shift > 0];
 *                   ge_out = ge + gt W3 (ge_out may alias ge);  gW3 = gt^T e_in;  gb3 = sum gt
 *                   (gnm_edge_bwd_gt + gemm TN + gemm NN + colsum).  autograd of :113,:122
 * ws: gnm_rowtile_workspace_bytes(ncols) / gnm_node_proj_bwd_workspace_bytes(ncols) /
 *     gnm_edge_bwd_fused_workspace_bytes().  partials: the BatchNorm partials buffer.      */
size_t gnm_rowtile_workspace_bytes(int ncols);
/* How the fused kernels multiply a fp32 tile by a fp32 weight block (process-wide, default 2):
 *   0  v_mfma_f32_32x32x2_f32 -- fp32 operands on the matrix cores;
 *   1  "bf16x3": each fp32 operand is split EXACTLY into three bf16 terms (3 x 8 = 24 significand
 *      bits) and the product is formed from six v_mfma_f32_32x32x16_bf16 (all partial products
 *      above 2^-24 |x w|), accumulated in fp32;
 *   2  "f16x2" (round 5): x s = h1 + h2 with two fp16 terms (2 x 11 = 22 significand bits) of a
 *      POWER-OF-TWO multiple -- s puts the largest magnitude of the operand's row (of a weight's
 *      output column) at 2^14, so nothing overflows or leaves the fp16 exponent range, and the fp32
 *      accumulator is multiplied by the exact 1 / s afterwards -- and THREE v_mfma_f32_32x32x16_f16
 *      per product (h1 w1, h1 w2, h2 w1), accumulated in fp32.  In every matrix kernel of a 128-wide
 *      layer (node_proj_fwd, edge_t_fused_fwd, node_proj_bwd_nn(_stats), tn128*, edge_bwd_chain*,
 *      edge_bwd_fused), in the fused H = 256 edge kernels and in the general rows / weight-gradient
 *      GEMMs of the wide models.
 *      The step runs at the package power cap: half the matrix instructions come back as time;
 *      distance to fp64 per mode: profiles/r05_f16x2_accuracy.txt (mode 2 <= mode 1 <= mode 0).
 * Applies to the NT / NN contractions of edge_t_fused_fwd, node_proj_fwd/bwd, edge_bwd_fused.   */
int gnm_debug_set_variant(const char* what, int v);   /* A/B switches between kernel generations (tests, tools) */
int gnm_set_matmul_mode(int mode);
int gnm_get_matmul_mode(void);
/* H = 128 in every matmul mode; H = 256 (the reference's default dim_latent, hyperparameters.py:8) in the split modes (1, 2; bf16x3 arithmetic): a
 * workgroup of eight waves keeps one 128-column half of W3 stationary, the two halves of the contraction meet in LDS
 * (ws >= gnm_rowtile_workspace_bytes(5 * H)).                                    gated_gcn_full.py:113,120-122 */
int gnm_edge_t_fused_fwd(int64_t E, int H, const float* e_in, const float* W3, const float* b3,
                         const float* P, const int32_t* isrc, const int32_t* idst, float* t,
                         double* partials, int* nblk_out, void* ws, size_t ws_bytes, void* stream);
/* H = 256, bf16x3 mode: gt = gamma*rstd*(gu - m1 - that*m2) (what gnm_edge_bwd_gt writes) AND ge_out = ge + gt W3 in one
 * pass over ge and t; gt is kept for the weight-gradient GEMM (gW3 = gt^T e_in).  ge_out and gt must not alias ge.
 * ws >= gnm_rowtile_workspace_bytes(5 * H).                                 autograd of gated_gcn_full.py:113,122 */
int gnm_edge_bwd_gt_nn(int64_t E, int H, const float* ge, const float* t, const float* stat_e, const float* bstat_e,
                       const float* gamma_e, const float* W3, float* gt, float* ge_out, void* ws, size_t ws_bytes,
                       void* stream);
int gnm_node_proj_fwd(int64_t N, int H, int ncols, const float* h, const float* W, const float* b,
                      float* Pout, void* ws, size_t ws_bytes, void* stream);
/* edge_bwd_chain (bf16x3 mode, H = 128): gnm_edge_bwd_fused of layer i ("hi": ge, t_hi, e_mid = e_in(i) = e_out(i-1),
 * stat/bstat/gamma/W3 of layer i -> gW3_hi, gb3_hi) CHAINED with gnm_edge_bwd_dst of layer i-1 ("lo": t_lo, stat_lo,
 * P_lo, Q_lo, hf_lo, hb_lo -> gP_lo[:,2H:3H], Ud_lo, Td_lo, BatchNorm partials in partials_lo, *nblk_out rows) in
 * one sweep: ge_out (may alias ge) receives what gnm_edge_bwd_dst would have written after gnm_edge_bwd_fused, the
 * intermediate d loss / d e_out(i-1) never leaves the chip.  partials_hi: scratch, >= gnm_max_partial_blocks()*128
 * doubles, distinct from partials_lo.  ws as gnm_edge_bwd_fused.  autograd of gated_gcn_full.py:113,120-130      */
int gnm_edge_bwd_chain(int64_t N, int64_t E, int H, const float* ge, float* ge_out, const float* t_hi,
                       const float* e_mid, const float* stat_hi, const float* bstat_hi, const float* gamma_hi,
                       const float* W3_hi, float* gW3_hi, float* gb3_hi, double* partials_hi,
                       const float* t_lo, const float* stat_lo, const float* P_lo, const float* Q_lo,
                       const float* hf_lo, const float* hb_lo, const int32_t* isrc, const int32_t* idst,
                       const int32_t* in_ptr, float* gP_lo, float* Ud_lo, float* Td_lo, double* partials_lo,
                       int* nblk_out, void* ws, size_t ws_bytes, void* stream);
/* edge_bwd_chain_src: gnm_edge_bwd_chain as a TWO-SIDED sweep -- layer i-1's by-SOURCE sums (what gnm_edge_bwd_src
 * re-reads e_out, t and ge for) are formed in the same pass from the per-edge terms that are on chip, through the
 * sweep plan (sinfo of gnm_graph_build_sweep_plan, built for plan_nodes_per_block = gnm_sweep_partition(N, 1)'s), RAW:
 *   gP_lo[:,H:2H] = sum_out sigma*Qf[dst],  UT_lo[N,2H] = [ sum_out gu | sum_out that ]    (served sources only)
 * gnm_edge_bwd_src_fix then writes the same three sums for the plan's fix_nodes (gathers; needs layer i-1's
 * e_out, t, stat_e, Q and ge = this call's ge_out), and once layer i-1's BatchNorm-backward means are known
 * gnm_node_bgrad turns the raw sums into gP[:,3H:4H] = gB1h = c (Us - outdeg m1 - m2 Ts) and gP[:,4H:5H] = gB2h =
 * c (Ud - indeg m1 - m2 Td).  Together = gnm_edge_bwd_src.  Ud_lo / Td_lo: two [N,H] arrays or the halves of one [N,2H]
 * array (Td_lo == Ud_lo + H); gnm_node_bgrad takes the row pitch of Ud / Td (H or 2H, in floats) as ud_pitch (ABI 5).
 *                                                                     autograd of gated_gcn_full.py:133-143 */
int gnm_edge_bwd_chain_src(int64_t N, int64_t E, int H, const float* ge, float* ge_out, const float* t_hi,
                           const float* e_mid, const float* stat_hi, const float* bstat_hi, const float* gamma_hi,
                           const float* W3_hi, float* gW3_hi, float* gb3_hi, double* partials_hi,
                           const float* t_lo, const float* stat_lo, const float* P_lo, const float* Q_lo,
                           const float* hf_lo, const float* hb_lo, const int32_t* isrc, const int32_t* idst,
                           const int32_t* in_ptr, float* gP_lo, float* Ud_lo, float* Td_lo, double* partials_lo,
                           const uint32_t* sinfo, int64_t plan_nodes_per_block, float* UT_lo,
                           int* nblk_out, void* ws, size_t ws_bytes, void* stream);
/* edge_bwd_top (H = 128; H = 256 with a sweep plan: once per 128-column half with row pitch 256 -- the by-destination and
 * by-source backward of EVERY layer of a 256-wide stack, followed by gnm_edge_bwd_src_fix / gnm_node_bgrad at H = 256):
 * the top layer of the stack (no layer above to chain with): gnm_edge_bwd_dst on the chained kernel's sweep
 * (ge updated in place to ge + gsigma*sigma', gP[:,2H:3H], Ud, Td, BatchNorm_e backward partials) plus, with sinfo, the
 * by-source sums exactly as gnm_edge_bwd_chain_src leaves them (then gnm_edge_bwd_src_fix, gnm_node_bgrad).          */
int gnm_edge_bwd_top(int64_t N, int64_t E, int H, float* ge, const float* e_out, const float* t, const float* stat_e,
                     const float* P, const float* Q, const float* hf, const float* hb, const int32_t* isrc,
                     const int32_t* idst, const int32_t* in_ptr, float* gP, float* Ud, float* Td, double* partials,
                     const uint32_t* sinfo, int64_t plan_nodes_per_block, float* UT, int* nblk_out, void* ws,
                     size_t ws_bytes, void* stream);
int gnm_edge_bwd_src_fix(int64_t nfix, const int32_t* fix_nodes, int64_t N, int64_t E, int H, const float* e_out,
                         const float* t, const float* stat_e, const float* ge, const float* Q, const int32_t* out_ptr,
                         const int32_t* out_pos, const int32_t* out_dst, float* gP, float* UT, void* stream);
int gnm_node_bgrad(int64_t N, int H, const float* stat_e, const float* bstat_e, const float* gamma_e,
                   const int32_t* in_ptr, const int32_t* out_ptr, const float* UT, const float* Ud, const float* Td,
                   int64_t ud_pitch, float* gP, void* stream);
size_t gnm_node_proj_bwd_workspace_bytes(int ncols);
int gnm_node_proj_bwd(int64_t N, int H, int ncols, const float* gP, const float* h_in, const float* W,
                      const float* gh_out, float* gh_in, float* gW, float* gb, double* partials,
                      void* ws, size_t ws_bytes, void* stream);
/* the two kernels behind gnm_node_proj_bwd on their own (same ws layout and size): gh_in = gh_out + gP W, and
 * gW = gP^T h_in, gb = sum gP                                                  autograd of :107-112 */
int gnm_node_proj_bwd_nn(int64_t N, int H, int ncols, const float* gP, const float* W, const float* gh_out,
                         float* gh_in, void* ws, size_t ws_bytes, void* stream);
int gnm_node_proj_bwd_tn(int64_t N, int H, int ncols, const float* gP, const float* h_in, float* gW, float* gb,
                         double* partials, void* ws, size_t ws_bytes, int max_blocks_per_cu, void* stream);
/* ---- the node side of the chained backward without its elementwise launches (ABI 5; bf16x3 mode, H = 128) ----
 * node_proj_bwd_nn_stats = gnm_node_proj_bwd_nn + gnm_node_bwd_stats of the layer BELOW in its epilogue: gh_in IS that layer's
 *   gh_out, so (sum gw, sum gw zhat), gw = gh_in [bn_h(z_lo) > 0], are taken from the rows on chip and one read of z_lo;
 *   partials / *nblk_out as gnm_node_bwd_stats leaves them (-> gnm_bn_bwd_finalize).         autograd of :107-112 and :147
 * tn128_bgrad = gnm_tn128 over the column groups gB1h | gB2h of gP (out = gW5[3H:5H], colsum = gb5[3H:5H]) with
 *   gnm_node_bgrad in its operand load: the groups are FORMED from the raw sums the two-sided sweep left (UT = [Us | Ts] with
 *   pitch 2H; Ud, Td with pitch ud_pitch = H or 2H) and the BatchNorm_e backward means, and WRITTEN to gP[:, 3H:5H] (row
 *   pitch 5H) for gnm_node_proj_bwd_nn*, which must run behind this call.  B = the layer's h_in [M,128].
 *   ws >= gnm_tn128_workspace_bytes().                                                  autograd of :107-112,120-122 */
int gnm_node_proj_bwd_nn_stats(int64_t N, int H, int ncols, const float* gP, const float* W, const float* gh_out,
                               float* gh_in, const float* z_lo, const float* stat_h_lo, double* partials, int* nblk_out,
                               void* ws, size_t ws_bytes, void* stream);
int gnm_tn128_bgrad(int64_t M, int H, const float* UT, const float* Ud, const float* Td, int64_t ud_pitch,
                    const float* stat_e, const float* bstat_e, const float* gamma_e, const int32_t* in_ptr,
                    const int32_t* out_ptr, float* gP, const float* B, float* out, float* colsum,
                    double* partials, void* ws, size_t ws_bytes, void* stream);
size_t gnm_edge_bwd_fused_workspace_bytes(void);
int gnm_edge_bwd_fused(int64_t E, int H, const float* ge, float* ge_out, const float* t, const float* e_in,
                       const float* stat_e, const float* bstat_e, const float* gamma_e,
                       const float* W3, float* gW3, float* gb3, double* partials, void* ws,
                       size_t ws_bytes, void* stream);
/* The same pass with gt GIVEN (round 6; H = 128, split matmul modes): the LayerNorm backward (layers/gated_gcn_full.py:58-59 selects
 * nn.LayerNorm) forms gt in its by-destination pass; this replaces its gemm_tn_colsum(gt, e_in) + gemm NN(gt, W3) + residual add:
 * gW3 = gt^T e_in, gb3 = sum gt, ge_out = ge + gt W3 (ge_out may alias ge, not gt).   autograd of gated_gcn_full.py:113 */
int gnm_edge_bwd_fused_gt(int64_t E, int H, const float* ge, float* ge_out, const float* gt, const float* e_in,
                          const float* W3, float* gW3, float* gb3, double* partials, void* ws, size_t ws_bytes, void* stream);

/* ---- edge-feature encoder (full_graph.py:24-26), H = 128 or 256, edge_features F = 2, hidden Q = 16 ----
 * fwd: e0[j] = W2 relu(W1 e_raw[perm j] + b1) + b2, internal order, one pass writing [E,H]
 *      (gnm_gather_rows + 2 gemm NT).
 * bwd: from ge0 [E,H]: gW2 [H,Q], gb2 [H], gW1 [Q,F], gb1 [Q] in one pass reading ge0 once
 *      (2 gemm TN + gemm NN + relu mask + 2 colsum).  ws: gnm_edge_encoder_bwd_workspace_bytes(). */
int gnm_edge_encoder_fwd(int64_t E, int H, int F, int Q, const float* e_raw, const int32_t* perm,
                         const float* W1, const float* b1, const float* W2, const float* b2,
                         float* e0, void* stream);
size_t gnm_edge_encoder_bwd_workspace_bytes(void);
int gnm_edge_encoder_bwd(int64_t E, int H, int F, int Q, const float* ge0, const float* e_raw,
                         const int32_t* perm, const float* W1, const float* b1, const float* W2,
                         float* gW1, float* gb1, float* gW2, float* gb2, void* ws, size_t ws_bytes,
                         void* stream);
/* the same pass, and also d loss / d e_raw: ge_raw [E,F] in the caller's edge-id order (row j of the internal order
 * written to ge_raw[perm j], every row exactly once: a permutation, no accumulation).  Same ws as gnm_edge_encoder_bwd. */
int gnm_edge_encoder_bwd_dx(int64_t E, int H, int F, int Q, const float* ge0, const float* e_raw,
                            const int32_t* perm, const float* W1, const float* b1, const float* W2,
                            float* gW1, float* gb1, float* gW2, float* gb2, float* ge_raw, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- ScorePredictor (score_predictor.py:12-25), split-W1 form ---------------------------
 * hid[j] += Ps[isrc j] + Pd[idst j] (hid holds e*W1e^T+b1 on entry; Pn=[Ps|Pd] is [N,2*HS]);
 * score[perm j] = W2 . relu(hid[j]) + b2                                                 */
int gnm_predictor_score_fwd(int64_t E, int HS, float* hid, const float* Pn, const int32_t* isrc,
                            const int32_t* idst, const float* W2, const float* b2,
                            const int32_t* perm, float* scores, void* stream);
/* ghid[j] = gscore[perm j]*W2*[hid>0] (in place over hid);
 * partials double[nblk][2][HS]: (sum gscore*relu(hid)) -> gW2, and [.,1,0] = sum gscore -> gb2 */
int gnm_predictor_score_bwd(int64_t E, int HS, float* hid, const float* gscore, const float* W2,
                            const int32_t* perm, double* partials, int* nblk_out, void* stream);
/* Fused single-pass forms for H = 128, HS = 64 (fp32 MFMA, W1e stationary in registers):
 * fwd: hid = e W1e^T + b1 + Ps[isrc] + Pd[idst] (written only if hid != NULL), score[perm j] = W2 . relu(hid[j]) + b2.
 *      W1e = &W1[0][2H] with row stride ldw (= 3H): the e-columns of predictor.W1 (score_predictor.py:15-17).
 * bwd: ghid = gscore[perm j] W2 [hid>0] (in place over hid), ge = ghid W1e, gW1e[HS,H] = ghid^T e,
 *      gsums[0:HS] = gW2, gsums[HS:2HS] = gb1, gsums[2HS] = gb2 (gsums holds 3*HS floats).
 *      partials: the BatchNorm partials buffer.  ws: gnm_predictor_fused_workspace_bytes().          */
size_t gnm_predictor_fused_workspace_bytes(void);   /* sized for H = 256; the two kernels are built for H = 128 and 256, HS = 64 */
int gnm_predictor_fused_fwd(int64_t E, int H, int HS, const float* e, const float* W1e, int64_t ldw,
                            const float* b1, const float* Pn, const int32_t* isrc, const int32_t* idst,
                            const int32_t* perm, const float* W2, const float* b2, float* hid,
                            float* scores, void* ws, size_t ws_bytes, void* stream);
int gnm_predictor_fused_bwd(int64_t E, int H, int HS, float* hid, const float* gscore,
                            const int32_t* perm, const float* W2, const float* e, const float* W1e,
                            int64_t ldw, float* ge, float* gW1e, float* gsums, double* partials,
                            void* ws, size_t ws_bytes, void* stream);
/* Weight-gradient shape of a Linear with a 128-wide input: out[cg*128+n][c] = sum_r A[r][cg*128+n] B[r][c],
 * colsum[cg*128+n] = sum_r A[r][cg*128+n];  A [M, lda >= ncg*128], B [M,128], ncg <= 16.              */
size_t gnm_tn128_workspace_bytes(void);
int gnm_tn128(int64_t M, const float* A, int64_t lda, int ncg, const float* B, float* out, float* colsum,
              double* partials, void* ws, size_t ws_bytes, void* stream);
/* reduce double partials [nblk][rows][W] -> float out[rows][W] */
int gnm_reduce_partials(const double* partials, int nblk, int rows, int W, float* out, void* stream);
/* out[v*ldo + c] = sum_{m in [ptr[v],ptr[v+1])} X[(pos ? pos[m] : m)*W + c], c < W        */
int gnm_seg_sum_rows(int64_t N, int W, const float* X, const int32_t* ptr, const int32_t* pos,
                     float* out, int64_t ldo, void* stream);

/* ---- input feature preparation ("next" row: utils.py:67-74, 97-138; train.py:245-251) -------------
 * pagerank_pe: pe[N, 2+pe_dim] = in_deg | out_deg | pe_dim PageRank steps (alpha = 0.95 in the
 *              reference), fp64 iterate, from the graph index.  ws: gnm_pagerank_pe_workspace_bytes(N).
 *              N > 0; E = 0 is a graph (degrees 0, every step (1-alpha)/N) and isrc may then be null.
 * edge_feats_zscore: e[E,2] = z-scored (overlap_length, overlap_similarity), unbiased std, in the
 *              caller's edge-id order.  ws: 4 * gnm_max_partial_blocks() doubles.                    */
size_t gnm_pagerank_pe_workspace_bytes(int64_t N);
int gnm_pagerank_pe(int64_t N, int64_t E, const int32_t* isrc, const int32_t* in_ptr,
                    const int32_t* out_ptr, int pe_dim, double alpha, float* pe, void* ws,
                    size_t ws_bytes, void* stream);
int gnm_edge_feats_zscore(int64_t E, const float* overlap_length, const float* overlap_similarity,
                          float* e, void* ws, size_t ws_bytes, void* stream);

/* ---- loss (train.py:210-211,253-255): BCEWithLogitsLoss(pos_weight), mean ---------------
 * loss_out[0] = mean_k(pw*y*softplus(-x) + (1-y)*softplus(x)); gscore = dloss/dx.
 * ws: double[gnm_max_partial_blocks()] */
int gnm_bce_fwd_bwd(int64_t E, const float* scores, const float* y, float pos_weight,
                    float* loss_out, float* gscore, void* ws, size_t ws_bytes, void* stream);
/* The same loss and gradient (bit for bit: same per-element arithmetic, grid and summation order) with the step's metric
 * counts and the epoch's running sums from the same pass over the logits (utils.calculate_tfpn, utils.py:217-223;
 * train.py:259-262 epoch sums).
 * counts_out[4] = TP TN FP FN (overwritten) of p = round(sigmoid(x)), half to even, against y: p == 1 exactly when x >= 0x1.800002p-24
 *             (the smallest fp32 logit whose fp32 sigmoid exceeds 0.5), p == 0 when x is below it; a NaN logit and a label that is
 *             neither 0 nor 1 are counted nowhere, as in torch.
 * gscore:     NULL under no_grad: no per-edge output is stored.
 * epoch_acc:  NULL, or a device {double loss_sum; int64_t steps; int64_t counts[4]} (48 bytes, 8-byte aligned) that the call ADDS
 *             to: loss_out[0] widened to double, 1, the four counts.  Calls on one stream add in call order.
 * ws:         gnm_bce_stats_workspace_bytes() bytes, 16-byte aligned; its previous content is not read.  No atomics: two runs
 *             give the same bits.  E must be positive, as for gnm_bce_fwd_bwd.                                                  */
size_t gnm_bce_stats_workspace_bytes(void);
int gnm_bce_stats_fwd_bwd(int64_t E, const float* scores, const float* y, float pos_weight,
                          float* loss_out, float* gscore, int64_t* counts_out, void* epoch_acc,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- node-output dropout of the layer stack (gated_gcn_full.py:154) with a counter-based mask, nothing stored --------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes, and the binding checks
 * every symbol by name when it loads.)
 * The keep decision of element (row r, channel c) is a pure function of (seed, step, layer, v, c), v = node_ids[r] (the caller's
 * node id of internal row r: the index's internal -> caller array; NULL: v = r): Philox4x32-10 with key (seed low word, seed
 * high word) and counter (q low, q high, layer, step), q = (v * H + c) >> 2 in 64 bits; word c & 3 of its output is the draw x,
 * u = (x >> 8) * 2^-24, kept iff u >= (float)p, compared in fp32 (p travels as a double so that the scale float(1 / (1 - p)) is
 * rounded once).  It does not depend on the internal node numbering, the grid or the occupancy cap.
 *   gnm_node_dropout_apply  y[r, c] = kept ? x[r, c] * float(1 / (1 - p)) : +0 for c < H; rows ld >= H elements apart in x and y
 *                           (a padded width, a column chunk: columns H .. ld-1 are neither read nor written).  y == x (in place)
 *                           is allowed, any other overlap is not.  The backward is the same call on the gradient.
 *                           H % 4 == 0, ld % 4 == 0 and 16-byte aligned x, y: one float4 per Philox call; else element by element.
 *   gnm_node_dropout_mask   mask[r * H + c] = kept (uint8 0 / 1, contiguous [N,H]): the same decisions, for inspection.
 * 0 <= p < 1, layer >= 0, N >= 0.                                                                                             */
int gnm_node_dropout_apply(int64_t N, int H, int64_t ld, const float* x, float* y, const int32_t* node_ids, double p,
                           uint64_t seed, uint32_t step, int layer, void* stream);
int gnm_node_dropout_mask(int64_t N, int H, uint8_t* mask, const int32_t* node_ids, double p, uint64_t seed, uint32_t step,
                          int layer, void* stream);

/* ---- the optimizer step over the flat buffers: Adam, gradient-norm clip, non-finite guard ------------------------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: three new symbols, no existing signature changes.)
 * torch.optim.Adam (train.py:209,256-258; no weight decay, no amsgrad) over flat fp32 buffers of n elements -- the layout
 * models.flatten_parameters and dp.FlatGradients share -- in two launches on one stream, with no host read-back:
 *   gnm_optim_grad_stats   one pass over g: per block of 2048 elements the fp64 sum of squares of the finite entries and the count
 *                          of the non-finite ones, one pair per block into `workspace`; it also copies *step into the workspace,
 *                          so that every workgroup of the step kernel sees the count of before the call, however late it starts.
 *   gnm_optim_adam_step    consumes the workspace of the gnm_optim_grad_stats call before it on the stream (same n, g, step):
 *                            c          = 1, or 1 / max(*inv_count, 1) with inv_count (device float: a contributor count)
 *                            total_norm = c * sqrt(sum of squares);  clip = max_norm > 0 ? min(1, max_norm / (total_norm + 1e-6)) : 1
 *                            guard:       a non-finite entry anywhere in g -> p, m, v and *step keep their bits, stats.skipped += 1
 *                            otherwise    t = *step + 1 -> *step;  gh = g * c * clip;  m = beta1 m + (1 - beta1) gh;
 *                                         v = beta2 v + (1 - beta2) gh^2;
 *                                         p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *                            zero_grad != 0: g is left all zeros, in the skipped case too.
 *                          Scalars in fp64; each element evaluated in fp64 from the fp32 inputs and rounded once per stored value.
 * step:      device float, the step count (the dtype of torch's fused Adam); written by one thread.
 * stats:     device gnm_optim_stats, 8-byte aligned; total_norm, nonfinite and clip are overwritten by every call (in a skipped
 *            call total_norm covers the finite entries), skipped accumulates: zero it once.  Read it whenever convenient.
 * workspace: gnm_optim_workspace_bytes(n) bytes, 8-byte aligned; its previous content is not read by gnm_optim_grad_stats.
 * Bit-identical between runs and independent of the grid, the CU count and gnm_set_occupancy_cap: a block partial depends on its
 * 2048 elements alone, the combination on the number of blocks alone; no atomics.  16-byte loads and stores when every buffer is
 * 16-byte aligned, element by element otherwise and in the tail -- same bits.  n == 0: nothing is launched, *step stays.
 * lr >= 0, 0 <= beta < 1, eps >= 0, max_norm >= 0 (0: no clipping), all finite.                                                 */
typedef struct gnm_optim_stats { double total_norm; int64_t nonfinite; int64_t skipped; double clip; } gnm_optim_stats;
size_t gnm_optim_workspace_bytes(int64_t n);
int gnm_optim_grad_stats(int64_t n, const float* g, const float* step, void* workspace, size_t workspace_bytes, void* stream);
int gnm_optim_adam_step(int64_t n, float* p, float* g, float* m, float* v, float* step, void* stats, const void* workspace,
                        size_t workspace_bytes, double lr, double beta1, double beta2, double eps, double max_norm,
                        const float* inv_count, int zero_grad, void* stream);

/* ---- threshold-free validation metrics: a per-label histogram of the logits from one pass, no sort ----------------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes.)
 * The key of an fp32 logit x that is not NaN:  u = bits(x + 0.0f) (-0 counts as +0);  u ^= (u >> 31) ? 0xFFFFFFFF : 0x80000000;
 * key = u >> 18: sign, 8 exponent bits, 5 mantissa bits.  It is monotone non-decreasing in x; -inf has the lowest key a value can
 * take (31) and +inf the highest (16352).  Bin k of hist[l] counts the edges with label l and key k: AUROC with exact lower and
 * upper bounds, average precision, the ROC / PR curves and the best-F1 threshold follow from the record on the host
 * (train.RankingMetrics.from_counts).
 *   gnm_rank_hist   ADDS one call's E (score, label) pairs to *record: y == 1 is a positive, y == 0 a negative, any other label
 *                   (NaN included) adds to tail[2] alone; a NaN score adds to tail[0] (y == 1) or tail[1] (y == 0) and to no bin;
 *                   tail[3] += 1 per call.  E == 0 is a valid call that adds 1 to tail[3] and nothing else (scores and y may then
 *                   be NULL).  The caller zeroes the record; records add across calls, graphs and ranks.
 * record:    device gnm_rank_record, 8-byte aligned.
 * workspace: gnm_rank_hist_workspace_bytes(E) bytes -- currently 0, and ws may then be NULL: every workgroup keeps its histogram
 *            in LDS and adds its non-zero bins to the record with 64-bit integer atomics.
 * The record is a function of (scores, y, previous record) alone: all of its fields are integer sums, which commute, so it does
 * not depend on the grid, the CU count, gnm_set_occupancy_cap or the order in which the atomics land, and two runs give the same
 * bits.  E < 0, a NULL record, NULL scores or y with E > 0, a short workspace and an E that would give one workgroup 2^31 or more
 * elements (its bins are 32-bit) are errors, returned before anything is launched.                                              */
typedef struct gnm_rank_record { int64_t hist[2][16384]; int64_t tail[4]; /* nan_pos, nan_neg, other_label, calls */ } gnm_rank_record;
size_t gnm_rank_hist_workspace_bytes(int64_t E);
int gnm_rank_hist(int64_t E, const float* scores, const float* y, void* record, void* ws, size_t ws_bytes, void* stream);

/* ---- read-masking coverage augmentation: which reads a training step keeps, and the degrees of the thinned graph --------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes.)
 * A training step may run on the sub-graph induced by a random subset of the READS: to first order a read set thinned to the
 * fraction f is the same genome sequenced at f times the coverage.  Nodes 2i and 2i+1 are the two strands of read i; a read is
 * kept or dropped as a whole.  The mask is a pure function of (key, epoch, graph_index, node), never a stored draw:
 *   gnm_read_mask      mask[v] (uint8 0 / 1, the caller's node order, N entries) for v < N:  r = v >> 1 the read, q = r >> 2;
 *                      Philox4x32-10 with key (key low word, key high word) and counter (q low, q high, graph_index, epoch);
 *                      word r & 3 of its output is the draw x, u = (x >> 8) * 2^-24, the read is kept iff u < (float)f, compared
 *                      in fp32 (f travels as a double and is rounded once).  f = 1 keeps every read, f = 0 none; masks of one
 *                      (key, epoch, graph_index) are nested in f, and the mask for N is a prefix of the mask for N + k.  An odd N
 *                      (the last read with one strand only) is legal.  One Philox call serves four reads = eight nodes: one
 *                      8-byte store where `mask` is 8-byte aligned, byte stores otherwise and in the tail -- same bits.
 *                      key: the training loop passes (the dropout key of the rank: seed ^ rank * 0x9E3779B97F4A7C15) ^
 *                      GNM_READ_MASK_KEY_XOR, a fixed odd constant, so that the mask and the dropout stream of one seed never
 *                      share a (key, counter) pair.
 *                      It does not depend on the internal node numbering, the grid or gnm_set_occupancy_cap.  0 <= f <= 1 and
 *                      N >= 0, else -1 before anything is launched; N == 0 returns 0 without a launch (mask may then be NULL).
 *   gnm_index_degrees  for every internal node i < n of an index (in_ptr, out_ptr [n + 1], internal numbering):
 *                        pe[nperm[i] * ld + 0] = (float)(in_ptr[i + 1] - in_ptr[i])      the in-degree
 *                        pe[nperm[i] * ld + 1] = (float)(out_ptr[i + 1] - out_ptr[i])    the out-degree
 *                      pe: row-major [n, ld] fp32 in the CALLER's node order, ld >= 2; columns 2 .. ld-1 are neither read nor
 *                      written.  nperm: internal -> caller's node id, NULL: the identity.  A row nperm[i] outside [0, n) is
 *                      checked before use and never written.  On the sub-graph of a read mask these are the THINNED graph's
 *                      degrees: the first two columns of the model's `pe` input.  n == 0 returns 0 without a launch.
 * No atomics, no LDS, no scratch memory, nothing allocated: two runs give the same bits.                                         */
#define GNM_READ_MASK_KEY_XOR 0xA0761D6478BD642FULL
int gnm_read_mask(int64_t N, double f, uint64_t key, uint32_t epoch, uint32_t graph_index, uint8_t* mask, void* stream);
int gnm_index_degrees(int64_t n, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* nperm, float* pe, int64_t ld,
                      void* stream);

/* ---- symmetry loss: the original and the edge-reversed scores of one graph in one pass ------------------------------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: four new symbols, no existing signature changes.)
 *   l_k = bce(org_k, y_k) + bce(rev_k, y_k) + alpha |org_k - rev_k|,  L = (1/E) sum_k l_k,  bce as in gnm_bce_fwd_bwd.
 * loss_out[0] = (float)((S_org + S_rev + alpha S_abs) * (1.0 / E)) from the three fp64 sums;  parts_out[3] = their means: mean
 *             bce(org), mean bce(rev), mean |org - rev| (the last is the "symmetry gap", reported unscaled by alpha).
 * g_org, g_rev: dL/d org = (bce'(org_k) + alpha sgn(org_k - rev_k)) / E, dL/d rev = (bce'(rev_k) - alpha sgn(org_k - rev_k)) / E,
 *             sgn(0) = 0 (torch.abs's subgradient).  Both NULL: no per-edge output is stored.  Exactly one NULL is an error.
 * counts_out: NULL, or [4] = TP TN FP FN of ORG by gnm_bce_stats_fwd_bwd's rule.   epoch_acc: NULL, or the same 48-byte record; it
 *             receives loss_out[0], 1 and the counts of org.
 * Same per-element BCE arithmetic, grid, element-to-thread assignment and summation trees as gnm_bce_fwd_bwd: with alpha = 0, g_org
 * and parts_out[0] have the bits of gnm_bce_fwd_bwd(org)'s gradient and loss, g_rev and parts_out[1] those of gnm_bce_fwd_bwd(rev).
 * No atomics: two runs give the same bits.  16-byte loads and stores when org, rev, y (and g_org, g_rev) are 16-byte aligned,
 * element by element otherwise and at the ragged end -- same bits.
 * ws: gnm_sym_bce_workspace_bytes() bytes, 16-byte aligned; counts_out and epoch_acc 8-byte aligned.
 * E <= 0, a NULL org / rev / y / loss_out / parts_out, exactly one of g_org / g_rev, a short or misaligned workspace and an alpha
 * that is negative or not finite are errors, returned before anything is launched.
 *   gnm_mirror_add     g[i] += scratch[pi[i]], i < n: folds the gradient of a pass run on mirrored parameters (flat[pi]) into the
 *                      flat gradient buffer.   gnm_mirror_gather   out[i] = src[pi[i]] (out != src).
 *                      pi: a permutation of [0, n), n < 2^31; an entry outside [0, n) is skipped.  n == 0: no launch.           */
size_t gnm_sym_bce_workspace_bytes(void);
int gnm_sym_bce_fwd_bwd(int64_t E, const float* org, const float* rev, const float* y, float pos_weight, float alpha,
                        float* loss_out, float* parts_out, float* g_org, float* g_rev, int64_t* counts_out, void* epoch_acc,
                        void* ws, size_t ws_bytes, void* stream);
int gnm_mirror_add(int64_t n, float* g, const float* scratch, const int32_t* pi, void* stream);
int gnm_mirror_gather(int64_t n, float* out, const float* src, const int32_t* pi, void* stream);

/* ---- walk decisions: per node the best-scored out- and in-edge, and how often that choice is a correct edge, in one pass --------
 * (Added without raising GNM_ABI_VERSION, which stays 7: one new symbol, no existing signature changes.)
 * The greedy decode follows, at a node with several free successors, the out-edge with the top score (inference.py:45-51) and on
 * the way back the top-scored in-edge; a contig breaks or goes chimeric when that one choice is wrong, which no edge-wise figure
 * (loss, TP..FN, AUROC) shows.  DEVICE pointers; perm .. out_dst: the graph's index (gnm_graph_build_index), nperm: internal ->
 * caller's node id, NULL: the identity.  scores, y [E]: fp32 in EDGE-ID order (y may be NULL).
 * Candidates of internal node i.  Successors: p in [out_ptr[i], out_ptr[i+1]) -> internal position out_pos[p] -> edge id
 *   perm[out_pos[p]], other end out_dst[p].  Predecessors: j in [in_ptr[i], in_ptr[i+1]) -> edge id perm[j], other end isrc[j].
 *   A self loop is no candidate (the decode drops self loops from its candidates); duplicate edges are separate candidates.
 *   idst is not read (in-edge j of node i ends in i) and may be NULL.
 * Choice: the candidate with the largest score, the lowest edge id among equal scores.  -0 equals +0; denormals are not flushed;
 *   a NaN orders below every number, -inf included, and NaNs tie (lowest edge id).  Compared on the full 32-bit form of the key
 *   above: k(x) = 0 for a NaN, else u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000) with u = bits(x == -0 ? +0 : x); (k, -eid) under
 *   a plain integer maximum.
 * best_succ / best_pred [n] (int32, either may be NULL): the chosen edge id of node v in the CALLER's numbering, -1 when v has no
 *   candidate.  A row nperm[i] outside [0, n) is checked before use and never written.
 * record: ADDS, per direction d (0: successors, 1: predecessors), to
 *   dir[d][0] dead             nodes with no candidate
 *   dir[d][1] forced           nodes with exactly one candidate         dir[d][2] forced_ok        ... whose label y == 1
 *   dir[d][3] branch           nodes with two or more candidates        dir[d][4] branch_solvable  ... some candidate has y == 1
 *   dir[d][5] branch_ok        ... the chosen edge has y == 1           dir[d][6] branch_nan       ... the chosen score is NaN
 *   and calls += 1.  A label other than 1 (0.5, NaN) counts as not 1.  y == NULL: only dead, forced, branch and branch_nan move.
 *   n == 0 or E == 0 is a valid call (E == 0: every node is dead).  The caller zeroes the record; records add across calls,
 *   graphs and ranks.  8-byte aligned.
 * One launch: eight lanes per node stride over its candidates and reduce by shuffles; counters go through registers and LDS to one
 * 64-bit integer atomic per counter and workgroup.  All fields are integer sums, which commute, and a table entry depends on its
 * node alone: neither depends on the grid, gnm_set_occupancy_cap or the order in which the atomics land, and two runs give the
 * same bits.  No float atomics, no workspace, nothing allocated.  Every position and edge id read from the index is range-checked
 * before it addresses anything (an entry outside [0, E) drops that candidate).
 * n or E negative or >= 2^31 - 1, a NULL or misaligned record, NULL row pointers with n > 0 and NULL perm / isrc / out_pos /
 * out_dst / scores with E > 0 are errors, returned before anything is launched.                                                 */
typedef struct gnm_decision_record { int64_t dir[2][7]; int64_t calls; } gnm_decision_record;
int gnm_decision_stats(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                       const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                       const float* scores, const float* y, void* record, int32_t* best_succ, int32_t* best_pred, void* stream);

/* ---- best-overlap contigs: mutual-best links, cycles cut, list ranking by pointer jumping, contig layout -- all on the device ------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes.)
 * The best-overlap graph of overlap-layout assemblers on the tables gnm_decision_stats writes: a deterministic decoder that needs
 * no sampling and no host walk.  DEVICE pointers; everything in the CALLER's node numbering and edge-id order.
 * Inputs: src, dst [E] int32; best_succ, best_pred [n] int32 (gnm_decision_stats); scores [E] fp32; y [E] fp32 or NULL;
 *   prefix_length [E] int64; read_length [n] int64; min_logit (-inf: no cut).
 * Links.  Edge k = (u -> v) is a link iff u != v, best_succ[u] == k, best_pred[v] == k, scores[k] is not NaN and
 *   scores[k] >= min_logit.  A table entry outside [-1, E) or a src / dst entry outside [0, n) drops that candidate; each is
 *   checked before it addresses anything.  Then next[u] = v, prev[v] = u, pedge[v] = k; else -1.
 * Cycles.  A component in which every node has a prev is a cycle; it is cut at its smallest node id m: prev[m] = pedge[m] = -1
 *   and next[old prev of m] = -1.  (Two mutual-best edges u -> v, v -> u are the smallest case.)
 * Ranking.  Every node now lies on exactly one path (a node with no link is a path of one).  head(v): the path's first node;
 *   rank(v): hops from the head; off(v): the int64 sum of prefix_length[pedge[w]] over the path from the head (excluded) to v
 *   (included); wrong(v): the same sum over [y[pedge[w]] != 1], 0 everywhere when y == NULL.
 * Contigs.  The heads in ascending node id are contigs 0 .. C-1.  Outputs (contig_ptr [n+1], the others [n]; of contig_ptr,
 *   contig_bases and contig_wrong only the first C+1 / C / C entries are defined):
 *   contig_ptr [C+1] int32; walk_nodes [n] int32 with walk_nodes[contig_ptr[c] + rank(v)] = v; walk_edges [n] int32 = pedge in
 *   the same layout (-1 at a contig's first node); contig_bases [C] int64 = off(tail) + read_length[tail] (get_contig_length,
 *   inference.py:20-28); contig_wrong [C] int32 = wrong(tail).
 * record: ADDS to  contigs (C), links (kept links, after the cuts: n - C), cycles_cut, dropped (mutual-best edges refused for a
 *   NaN score or min_logit), wrong_links (the sum of contig_wrong), multi_nodes (nodes on paths of >= 2 nodes), multi_contigs,
 *   calls (+1).  The caller zeroes it; the host reads C from it -- the call's one synchronisation, and the caller's.  8-byte aligned.
 * gnm_bog_contigs issues every launch on `stream`: 2 K + 6 of them, K = ceil(log2(max(n, 2))).  Pointer jumping runs as K fixed
 * rounds per pass, one launch per round, reading one generation of the per-node state and writing the other: pass one carries the
 * minimum id (a node whose pointer is still live after K rounds is on a cycle), pass two carries head, rank, off and wrong.  Head
 * numbers and contig offsets are exclusive prefix sums over node-ordered flags / lengths in fixed blocks (block sums, one workgroup
 * over the block sums, in-block scan).  No workgroup waits for another inside a kernel, nothing is read back between launches, no
 * float arithmetic (the score enters through the one comparison), integer atomics on the eight record words only (one per counter
 * and workgroup): the results depend on the inputs alone, not on the grid, gnm_set_occupancy_cap or timing.
 * ws: gnm_bog_workspace_bytes(n) bytes (72 n and two block-sum arrays; 0 for n == 0 and for an n that is refused), 16-byte aligned.
 * n == 0 and E == 0 are valid (E == 0: n contigs of one node).  n or E negative or >= 2^31 - 1, a NULL or misaligned record, NULL
 * tables / read_length / outputs with n > 0, NULL src / dst / scores / prefix_length with E > 0 and a workspace that is NULL, short
 * or misaligned are errors, returned before anything is launched.                                                                 */
typedef struct gnm_bog_record {
  int64_t contigs, links, cycles_cut, dropped, wrong_links, multi_nodes, multi_contigs, calls;
} gnm_bog_record;
size_t gnm_bog_workspace_bytes(int64_t n);
int gnm_bog_contigs(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int32_t* best_succ, const int32_t* best_pred,
                    const float* scores, const float* y, const int64_t* prefix_length, const int64_t* read_length, float min_logit,
                    void* record, int32_t* contig_ptr, int32_t* walk_nodes, int32_t* walk_edges, int64_t* contig_bases,
                    int32_t* contig_wrong, void* ws, size_t ws_bytes, void* stream);

/* ---- cover rounds: the greedy path cover by iterated mutual-best links (locally-dominant matching) -- all on the device -------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes.)
 * gnm_decision_stats + gnm_bog_contigs keep an edge only when both of its ends rank it first, and stop.  That is round one of this
 * sequence: take the mutual-best edges, mark their out-slot and in-slot as used, let every node with a free slot choose again
 * among the edges whose other end is still free, repeat.  The fixed point is the greedy path cover of overlap-layout assemblers:
 * the edges by descending score (lowest edge id among equals), an edge accepted when its source has no successor and its
 * destination no predecessor yet.  Cycles can close; they are cut afterwards by gnm_bog_contigs, which takes link_succ /
 * link_pred unchanged in place of best_succ / best_pred (the tables are mutual by construction: it never refuses an entry).
 * DEVICE pointers; perm .. out_dst, nperm: the graph's index as for gnm_decision_stats (idst is not needed); scores [E] fp32 in
 * EDGE-ID order.
 * State, per node in the index's internal numbering, kept in ws between calls: msucc / mpred, the edge id of the accepted out- /
 *   in-edge, or -1.
 * Candidates: an edge k = (u -> w) with u != w, every position and id in range (row pointers are clamped, an entry outside [0, E)
 *   or [0, n) drops the candidate before it addresses anything), scores[k] not NaN and scores[k] >= min_logit (-inf: no cut).
 *   Order: the 32-bit key of "walk decisions" above, the lowest edge id among equal keys; -0 ties +0, -inf is the lowest number.
 * Round r, on the state after round r - 1 (two launches: propose, link):
 *   propose  u with msucc[u] < 0 takes cs[u], its best candidate out-edge whose destination w has mpred[w] < 0, or -1; w with
 *            mpred[w] < 0 takes cp[w], its best candidate in-edge whose source u has msucc[u] < 0, or -1.
 *   link     u sets msucc[u] = k when k = cs[u] >= 0 and cp[dst k] == k; w sets mpred[w] = k when k = cp[w] >= 0 and
 *            cs[src k] == k.  Every node writes its own words only.
 *   round_links[j] (int64 [rounds], j = r - first_round) = the links round r added.  The call zeroes its `rounds` entries first.
 * gnm_cover_rounds: first_round == 0 sets the state to -1; then rounds first_round .. first_round + rounds - 1 run on it; then
 *   link_succ[v] / link_pred[v] (int32 [n], the CALLER's numbering through nperm; a row outside [0, n) is never written) receive
 *   the state so far: they are valid after every call.  first_round > 0 continues on the ws of the previous call, which the caller
 *   leaves untouched in between.  2 rounds + 2 launches on `stream` (none for n == 0 and rounds == 0), nothing read back: the
 *   caller reads round_links and stops at the first 0 -- a round that adds nothing leaves a fixed point, and further rounds add
 *   nothing and change nothing.  The state after any number of rounds is a set of disjoint paths and cycles.
 * Eight lanes per node stride over its candidates and reduce by shuffles (the decision kernel's layout); a node whose two slots
 * are taken costs its two state loads.  No cooperative launch, no workgroup waits for another, no float arithmetic, one 64-bit
 * integer atomic per workgroup and round: the outputs depend on the inputs alone, not on the grid, gnm_set_occupancy_cap or timing.
 * ws: gnm_cover_workspace_bytes(n) bytes (24 n; 0 for n == 0 and for an n that is refused), 16-byte aligned.
 * n or E negative or >= 2^31 - 1, first_round or rounds negative or >= 2^31 - 1, a NULL or misaligned round_links with rounds > 0,
 * NULL row pointers / link_succ / link_pred with n > 0, NULL perm / isrc / out_pos / out_dst / scores with E > 0 and a workspace
 * that is NULL, short or misaligned are errors, returned before anything is launched.                                             */
size_t gnm_cover_workspace_bytes(int64_t n);
int gnm_cover_rounds(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* in_ptr, const int32_t* out_ptr,
                     const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm, const float* scores, float min_logit,
                     int64_t first_round, int64_t rounds, int64_t* round_links, int32_t* link_succ, int32_t* link_pred, void* ws,
                     size_t ws_bytes, void* stream);

/* ---- contig sequences: a packed read store + walks in CSR form -> the contigs' bases as ASCII, on the device ----------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: four new symbols, no existing signature changes.)
 * evaluate.walk_to_sequence (evaluate.py:36-47) without a string per node.  DEVICE pointers except for gnm_decode_walk_edges.
 * Store.  One entry per READ, + strand only: packed [packed_bytes] uint8, 4 bits per base in the BAM code "=ACMGRSVTWYHKDBN"
 *   (A=1 C=2 G=4 T=8, an ambiguity code the OR of its bases, N=15), two bases per byte, low nibble first; base_off [R] int64, the
 *   nibble index of read r's first base; length [R] int64.  packed_bytes is a multiple of 16 and packed is 4-byte aligned.  Node v
 *   of the graph (n nodes) is read v >> 1; an odd v is the reverse complement: the read's nibbles in reverse order, the four bits
 *   of each reversed (complement = bit reversal for every code).
 * Walks.  contig_ptr [C+1] int32, walk_nodes [P] int32, walk_edges [P] int32 (walk_edges[p] joins positions p-1 and p; the entry
 *   at a contig's first position is not read): the layout gnm_bog_contigs leaves.  prefix_length [E] int64.
 * Pieces.  Position p of contig c (contig_ptr[c] <= p < contig_ptr[c+1]) with node v contributes the first k bases of v's strand:
 *   k = length[v >> 1] at the contig's last position, else k = clamp(prefix_length[walk_edges[p+1]], 0, length[v >> 1]).  The
 *   clamp is deliberate: a Python slice takes a negative prefix from the END of the read, which is not reproduced but counted.
 *   A position is INVALID, gets k = 0 and has nothing read through it when: it lies in no contig (contig_ptr not ascending from
 *   0 to P), v is outside [0, n), v >> 1 >= R, the read's [base_off, base_off + length) does not lie inside the store, or
 *   (inner positions) the edge id is outside [0, E).  Every index is checked before it addresses anything.
 * gnm_seq_layout (4 launches; 2 for P == 0): piece_len [P], piece_off [P+1] = the exclusive prefix sum of piece_len (blocked
 *   integer scan: block sums, one workgroup over the block sums, in-block scan), contig_base_ptr [C+1] = piece_off[contig_ptr[c]].
 *   record: ADDS  contigs (C), pieces (P), bases (piece_off[P]), clamped (prefix below 0 or above the read's length), empty (valid
 *   pieces of 0 bases), reverse (valid pieces of odd nodes), invalid, calls (+1).  The caller zeroes it and reads `bases` to size
 *   the output: the one host synchronisation.  ws: gnm_seq_workspace_bytes(P) bytes, 16-byte aligned.
 * gnm_seq_emit (1 launch; none when total == 0): out[g] for g < total = the ASCII letter of output base g, the contigs back to
 *   back (contig c at contig_base_ptr[c]); out_bytes is a multiple of 16 >= total and the bytes of the last 16-byte group at and
 *   past `total` are written as 0.  total: `bases` of the layout call; the kernel never goes past piece_off[P].  A workgroup owns
 *   chunks of GNM_SEQ_CHUNK_BASES output bases and every lane writes 16 bases with one aligned 16-byte store: from one window of
 *   the store when they lie in one piece (forward: nibbles [s, s+16); reverse: the same window with all 64 bits reversed), base by
 *   base when pieces end among them.  The emit pass re-checks node, read and window against the store: a piece whose source does
 *   not check out is written as '=' (code 0), never read.  Callers refuse to emit when record.invalid != 0.
 * No float arithmetic, no workgroup waits for another, integer atomics on the record only: the bytes and the record depend on the
 * inputs alone.  Negative or >= 2^31 - 1 counts, a packed_bytes that is no multiple of 16, NULL or misaligned record / ws / out /
 * packed and an out_bytes below total are errors, returned before anything is launched.
 * gnm_decode_walk_edges (HOST pointers): walk_edges for walks given as node lists.  src, dst [E] and succ_ptr [N+1] as in
 *   gnm_decode_build_adjacency; contig_ptr [C+1], walk_nodes [P].  walk_edges[p] = the LOWEST edge id k with src[k] ==
 *   walk_nodes[p-1] and dst[k] == walk_nodes[p]; -1 at a contig's first position.  -2: a node outside [0, N) or a step that is
 *   no edge; bad[0..3] = contig, position in the contig, u, v of the first one, also named in gnm_last_error.                       */
#define GNM_SEQ_CHUNK_BASES 4096
typedef struct gnm_seq_record {
  int64_t contigs, pieces, bases, clamped, empty, reverse, invalid, calls;
} gnm_seq_record;
size_t gnm_seq_workspace_bytes(int64_t P);
int gnm_seq_layout(int64_t C, int64_t P, int64_t E, int64_t n, int64_t R, const int32_t* contig_ptr, const int32_t* walk_nodes,
                   const int32_t* walk_edges, const int64_t* prefix_length, const int64_t* base_off, const int64_t* length,
                   int64_t packed_bytes, void* record, int64_t* piece_len, int64_t* piece_off, int64_t* contig_base_ptr, void* ws,
                   size_t ws_bytes, void* stream);
int gnm_seq_emit(int64_t P, int64_t n, int64_t R, const int32_t* walk_nodes, const int64_t* piece_off, const int64_t* base_off,
                 const int64_t* length, const uint8_t* packed, int64_t packed_bytes, int64_t total, uint8_t* out, int64_t out_bytes,
                 void* stream);
int gnm_decode_walk_edges(const int32_t* src, const int32_t* dst, int64_t N, int64_t E, const int32_t* succ_ptr, int64_t C,
                          const int32_t* contig_ptr, const int32_t* walk_nodes, int32_t* walk_edges, int64_t* bad);

/* ---- transitive support: the string-graph reduction of the candidate edges ahead of the cover decoders -- one launch ---------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: one new symbol, no existing signature changes.)
 * The overlap graph is not transitively reduced: a read overlaps its next several neighbours, and a path cover that takes a -> c
 * over a -> b -> c leaves b to a parallel contig.  This marks the edges a two-step path of shorter prefix explains.
 * DEVICE pointers; perm .. out_dst, nperm: the graph's index as for gnm_cover_rounds (only perm and the by-source half -- out_ptr,
 * out_pos, out_dst -- are read); scores [E] fp32, prefix_length [E] int64, y [E] fp32 or NULL: EDGE-ID order.
 * Candidates: gnm_cover_rounds' -- k = (u -> w) with u != w, scores[k] not NaN and scores[k] >= min_logit (-inf: no cut).
 * support[k] (int32 [E], edge-id order), for every edge k = (a -> c) with a != c, candidate or not: the number of out-edges
 *   j = (a -> b) of a with j a candidate, b != a, b != c, prefix_length[j] < prefix_length[k] STRICTLY, and at least one candidate
 *   m = (b -> c) -- with fuzz >= 0 one that also has |prefix_length[j] + prefix_length[m] - prefix_length[k]| <= fuzz (int64,
 *   wrapping); fuzz == -1: no length test.  Parallel a -> b edges each count, several parallel b -> c edges make one witness, a
 *   self loop has support 0.  k is REDUCED when it is a candidate and support[k] > 0.  The strict < keeps two edges from removing
 *   each other through one another and never reduces a node's candidate out-edge of uniquely smallest prefix.
 * masked_scores (fp32 [E] or NULL): scores[k], or the quiet NaN 0x7FC00000 where k is reduced -- what gnm_decision_stats,
 *   gnm_cover_rounds and gnm_bog_contigs take as scores: they treat a NaN as no candidate.  May not alias scores.
 * record: ADDS  edges (edges seen), candidates, reduced, reduced_label1 (reduced edges with y == 1; 0 when y == NULL), witnesses
 *   (the sum of support), self_loops, calls (+1), and raises max_support to the largest support seen.  8-byte aligned.
 * Eight lanes per source node stride over its out-edges k and each walks the row again for j; "a candidate b -> c exists" is a
 * binary search in b's by-source row, whose destinations ascend, and a scan of the equal range: d^2 log d steps for out-degree d.
 * Every edge is written by the one lane that owns it: plain stores, no atomics but one integer atomic per record word and
 * workgroup, no workspace, no float arithmetic, no cooperative launch: the outputs depend on the inputs alone, not on the grid or
 * gnm_set_occupancy_cap.  Row pointers are clamped; a position or edge id outside [0, E) or a node outside [0, n) drops that edge
 * (not counted, not written) or witness before it addresses anything.
 * n == 0 and E == 0 are valid: nothing is launched and the record stays as it is.  n or E negative or >= 2^31 - 1, fuzz < -1, a
 * NULL or misaligned record, NULL out_ptr with n > 0 and NULL perm / out_pos / out_dst / scores / prefix_length / support with
 * E > 0 are errors, returned before anything is launched.                                                                         */
typedef struct gnm_reduce_record {
  int64_t edges, candidates, reduced, reduced_label1, witnesses, max_support, self_loops, calls;
} gnm_reduce_record;
int gnm_transitive_support(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* in_ptr,
                           const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                           const float* scores, const int64_t* prefix_length, const float* y, float min_logit, int64_t fuzz,
                           int32_t* support, float* masked_scores, void* record, void* stream);

/* ---- overlap alignment: the banded edit distance of every edge's overlap, from the packed read store -- one launch ---------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: two new symbols, no existing signature changes.)
 * The second column of the model's edge input: graph_parser.py:268-282 copies overlap_similarity out of the overlapper's line and
 * writes 0 where it is missing; this computes an edit-distance identity from the reads instead.  It is NOT the overlapper's own
 * number, which has no formula in the reference.
 * gnm_overlap_align takes DEVICE pointers, gnm_overlap_align_host HOST pointers; both run csrc/gnm_align.h.  src, dst int32 [E] and
 * prefix_length int64 [E] in EDGE-ID order; the store (packed .. R, n) as for "contig sequences".
 * Rule, integers only.  Edge k = (a -> c), p = prefix_length[k], la / lc the lengths of the two nodes' reads (node v: read v >> 1,
 *   reverse-complemented when v is odd).  p < 0 or p > la is clamped (counted).  Q = bases [p, la) of a's strand, m = la - p;
 *   T = bases [0, min(lc, m + K)) of c's strand, K = max_errors.  dist[k] = min over 0 <= j <= |T| of Levenshtein(Q, T[0:j]):
 *   all of Q is aligned, both start at their first base, the end in T is free; substitution, insertion and deletion cost 1; two
 *   bases match when their 4-bit codes are EQUAL (N matches N and nothing else, and so every ambiguity code).  A distance above K
 *   is reported as K + 1 (the edge is `exceeded`); a path of cost <= K never leaves the diagonals |i - j| <= K, so the band gives
 *   the exact answer otherwise.  overlap_length[k] = m (graph_parser.py:281).  similarity[k] = max(0, 1 - dist / m), ONE fp32
 *   division of the two integers converted to fp32.  m == 0: dist 0, similarity 0 (`empty`).  A node outside [0, n), a read index
 *   >= R or a read outside the store: dist -1, overlap_length 0, similarity 0 (`invalid`), nothing is read through it.
 * max_errors: 0 .. 255.  The band is 1, 2, 4 or 8 words of 64 diagonals (K <= 31, 63, 127, 255), held in registers.
 * record: ADDS  edges (E), aligned (dist <= K, m > 0), exceeded, empty, clamped, invalid, cells (the sum of m * |T| over the
 *   aligned edges), calls (+1).  edges == aligned + exceeded + empty + invalid.  8-byte aligned; the caller zeroes it.
 * One lane per edge, plain stores at the edge's id, one integer atomic per record word and workgroup: outputs and record depend on
 * the inputs alone, not on the grid or gnm_set_occupancy_cap.  The column loop of an edge runs m times, m taken from the store
 * before it starts.  E == 0: nothing is launched, the record stays as it is.  E negative or >= 2^31 - 1, max_errors outside
 * [0, 255], a packed_bytes that is no multiple of 16, a NULL or misaligned record / packed, NULL arrays with E > 0 and (host)
 * threads outside [1, 1024] are errors, returned before anything runs.                                                           */
typedef struct gnm_align_record {
  int64_t edges, aligned, exceeded, empty, clamped, invalid, cells, calls;
} gnm_align_record;
int gnm_overlap_align(int64_t E, const int32_t* src, const int32_t* dst, const int64_t* prefix_length, const uint8_t* packed,
                      int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int64_t n, int max_errors,
                      int32_t* dist, int64_t* overlap_length, float* similarity, void* record, void* stream);
int gnm_overlap_align_host(int64_t E, const int32_t* src, const int32_t* dst, const int64_t* prefix_length, const uint8_t* packed,
                           int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int64_t n, int max_errors,
                           int32_t* dist, int64_t* overlap_length, float* similarity, void* record, int threads);

/* ---- resolve strands: one strand per read over the contigs of a path cover -- all on the device ----------------------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: four new symbols, no existing signature changes.)
 * Nodes 2i and 2i+1 are the two strands of read i; a cover usually holds a contig and its reverse complement.  The rule (the
 * host's decode.resolve_strands): the contigs are taken in the order `order` gives (descending bases, ascending contig index among
 * equals); a contig of fewer than len_threshold nodes is never walked; a node whose read is taken ends the current piece and
 * belongs to none; a piece of at least len_threshold nodes is kept and takes its reads, a shorter one is dropped and takes none; a
 * read met twice inside one piece ends it too (kept: the node is skipped; dropped: the node starts the next piece).
 * DEVICE pointers.  contig_ptr [C+1], walk_nodes [P], walk_edges [P]: the layout gnm_bog_contigs leaves; order int32 [C]: a
 * permutation of the contigs, first contig first; prefix_length [E], read_length [n] int64; y [E] fp32 or NULL.
 * Every node may occur at most ONCE in walk_nodes (a path cover).  Then taken[r] is written only by the contig of either strand
 * of r, and the rule runs in rounds: a contig is READY when every contig that holds the other strand of one of its reads is the
 * contig itself, comes later in `order`, or was finished in an earlier round; ready contigs share no read and are cut side by
 * side, one wave each: ballots find the runs of free positions (the open run is carried across chunks of 64), a second pass keeps
 * the runs of at least len_threshold.  A contig that holds both strands of some read is cut by one lane, by the rule as written.
 * The first unfinished contig of `order` is always ready, so every round finishes at least one.
 * gnm_resolve_prepare (3 launches): resets ws, checks the input, classifies the contigs.  record ADDS contigs (C), eligible,
 *   serial (eligible contigs that hold both strands of a read), invalid, calls (+1).  INVALID: a contig_ptr row that does not
 *   ascend inside [0, P], a node outside [0, n), an inner edge id outside [0, E), an order entry outside [0, C), and every
 *   position (order entry) whose node (contig) is listed twice.  With invalid != 0 the later calls launch kernels that return at
 *   once: nothing is written but undecided, which reads -1.
 * gnm_resolve_rounds (1 + rounds launches): rounds first_round .. first_round + rounds - 1 on the state in ws; undecided[j]
 *   (int64 [rounds]) = the eligible contigs not finished after round first_round + j (-1: invalid input).  The caller stops at the
 *   first 0; a round on a finished state changes nothing.  record ADDS dropped (the non-empty pieces below the threshold).
 * gnm_resolve_layout (5 launches), once the rounds have ended: the kept pieces, by the order of their contigs and then by
 *   position, as a cover of their own -- out_ptr [K+1] (room for P+1), out_nodes, out_edges [N] (room for P; -1 at a piece's first
 *   node), out_bases int64 [K] (the sum of prefix_length over the inner links + read_length of the last node), out_wrong [K] (inner
 *   links with y != 1; 0 when y == NULL), room for P each.  record ADDS pieces (K), nodes (N): the caller reads them to size its views.
 * ws: gnm_resolve_workspace_bytes(C, P, n) bytes, 16-byte aligned, the same for the three calls and untouched in between.
 * Integers only; one integer atomic per workgroup and counter; no workgroup waits for another: outputs and record depend on the
 * inputs alone, not on the grid or gnm_set_occupancy_cap.  Counts negative or >= 2^31 - 1, len_threshold < 1, NULL or misaligned
 * record / ws / undecided, NULL arrays that the sizes need are errors, returned before anything is launched.                      */
typedef struct gnm_resolve_record {
  int64_t contigs, eligible, pieces, dropped, nodes, serial, invalid, calls;
} gnm_resolve_record;
size_t gnm_resolve_workspace_bytes(int64_t C, int64_t P, int64_t n);
int gnm_resolve_prepare(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                        const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, void* record, void* ws,
                        size_t ws_bytes, void* stream);
int gnm_resolve_rounds(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                       const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, int64_t first_round, int64_t rounds,
                       int64_t* undecided, void* record, void* ws, size_t ws_bytes, void* stream);
int gnm_resolve_layout(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                       const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, const int64_t* prefix_length,
                       const int64_t* read_length, const float* y, void* record, int32_t* out_ptr, int32_t* out_nodes,
                       int32_t* out_edges, int64_t* out_bases, int32_t* out_wrong, void* ws, size_t ws_bytes, void* stream);

/* ---- overlap graph: all-versus-all overlaps of the reads of a packed store -- minimizer sketch, seed hits, chains ---------------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: eleven new symbols, no existing signature changes.)
 * What the reference gets from an external overlapper (graph_dataset.py:120) and graph_parser.py: the edges of the assembly graph,
 * for accurate long reads (errors of about 1 %), by exact minimizer matches.  Integers only; csrc/gnm_overlap.h is the arithmetic,
 * run by the kernels and by the *_host entries alike.  The store (packed .. R) as for "contig sequences"; node 2r is read r, node
 * 2r + 1 its reverse complement.  Between the stages the CALLER sorts (stable sorts; the package uses torch.sort).
 *
 * Stage 1, sketch.  A, C, G, T (codes 1, 2, 4, 8) are 0 .. 3; a k-mer that holds any other code is invalid.  k in [8, 31].  For
 *   a valid k-mer at position p of the + strand, f is its 2k-bit value, first base most significant, r the value of its reverse
 *   complement; f == r: skipped.  c = min(f, r), strand bit s = (r < f), h = fmix64(c) (the murmur3 64-bit finaliser, constants
 *   0xff51afd7ed558ccd and 0xc4ceb9fe1a85ec53; a bijection).  Order key: (h, p), h unsigned.  nk = L - k + 1 (<= 0: nothing);
 *   w in [1, 64], W = min(w, nk); every window [j, j + W), 0 <= j <= nk - W, selects its valid k-mer of smallest key, if it has
 *   one; the read's sketch is the set of selected positions.  Output: hash (h's bit pattern as int64), read, pos int32, strand
 *   uint8, ordered by read, then position.  A read that lies outside the store or has 2^31 - 1 bases or more gives nothing on the
 *   device (gnm_sketch_host, which can see the lengths, refuses the latter).
 *   gnm_sketch_count: the tile table (tiles of GNM_SKETCH_TILE k-mer positions; tile_ptr int64 [R + 1]), the entries of every tile
 *   and their scan (tile_off int64 [tile_bound + 1], tile_bound = gnm_sketch_tile_bound(R, packed_bytes)); record ADDS reads (R),
 *   kmers_valid, minimizers, calls (+1).  The caller reads `minimizers` (M), sizes the outputs, calls gnm_sketch_emit.
 * Stage 2, seed hits.  Input: the M entries sorted by hash AS SIGNED int64, stably.  A run of equal hash longer than max_occ
 *   (1 .. 4096) is skipped (skipped_runs, skipped_entries).  Otherwise every pair of its entries j < i is a hit unless both are of
 *   one read (same_read).  With a the entry of the lower read id, b the other: rel = s_a ^ s_b; q = p_b when rel == 0, else
 *   L_b - k - p_b; diag = p_a - q (int32): node 2a is compared with node 2b + rel, whose first base falls at diag in a.
 *   key = a << 32 | b << 1 | rel (int64).  Order of the hits: by i, then by j ascending.
 *   gnm_seed_pairs_count: off int64 [M + 1]; record ADDS runs, skipped_runs, skipped_entries, same_read, hits.  The caller reads
 *   `hits` (N), calls gnm_seed_pairs_emit.
 *   Stage 2 in read-range chunks (five more symbols, same rule: GNM_ABI_VERSION stays 7).  a(hit) is the lower read id of the hit's two
 *   entries, the `a` of its key.  Every hit of a chain group carries the same a, and hits sorted by key are a-major; so the hits with
 *   a_lo <= a(hit) < a_hi, sorted and chained on their own, give the slots of exactly the groups whose a lies in the range, and
 *   consecutive ranges, concatenated, give the unchunked call's arrays.  Same input as gnm_seed_pairs_count.
 *   gnm_seed_pairs_lower_hits: lower_hits int64 [R], which the caller zeroes: lower_hits[r] += #{hits : a(hit) == r}, the entries of
 *   each entry's run that have a larger read id (counted directly: no order inside a run is assumed; 64-bit integer atomics, near one
 *   per entry).  An entry whose read id is outside [0, R) counts in no lower_hits word (then sum(lower_hits) < hits); a sketch
 *   of R reads has none.  record ADDS exactly what gnm_seed_pairs_count adds.  ws is not used (NULL, 0 are accepted).
 *   gnm_seed_pairs_count_range / _emit_range: gnm_seed_pairs_count / _emit restricted to the hits with a_lo <= a(hit) < a_hi
 *   (0 <= a_lo <= a_hi <= R), in the same order; the record stays as it is (gnm_seed_pairs_lower_hits added the totals); the
 *   range's size is off[M].  With a_lo = 0, a_hi = R: the outputs of gnm_seed_pairs_count / _emit.
 * Stage 3, chains.  Input: the N hits sorted by diag, then stably by key: group (a, b, rel) holds its diagonals ascending, d_0 ..
 *   d_{g-1}.  c_i = #{j >= i : d_j <= d_i + band}; the window is the i of largest c_i, the lowest among equals; hits = c_i,
 *   D = d_{i + (c_i - 1) / 2}.  hits < min_hits: rejected (few_hits).  With la, lb the reads' lengths:
 *     D > 0 and D + lb > la: forward, ov = la - D: edge 2a -> 2b+rel, prefix D; twin (2b+rel)^1 -> 2a+1, prefix lb - ov;
 *     D < 0 and D + lb < la: backward, ov = lb + D: edge 2b+rel -> 2a, prefix -D; twin 2a+1 -> (2b+rel)^1, prefix la - ov;
 *     otherwise containment: b is contained when D >= 0 and D + lb <= la, else a; contained[read] = 1 (a plain store of the same
 *     value by every writer; the caller zeroes the array); no edge (contained_groups).
 *   An edge with ov < min_overlap is rejected (too_short).  Group g (in sorted order) owns slots 2g (the edge) and 2g + 1 (the
 *   twin) of src, dst int32, prefix_length, overlap_length int64, valid uint8; a rejected group's slots read -1, -1, 0, 0, 0.  A
 *   key that names a read outside [0, R) -- none of gnm_seed_pairs does -- is rejected under few_hits.
 *   gnm_chain_count: off int64 [N + 1] (the group number of every group's first hit); record ADDS groups.  The caller reads
 *   `groups` (G), calls gnm_chain_pairs, which ADDS few_hits, too_short, contained_groups, links.
 *   One lane walks a whole group: a launch takes as long as its longest group (at most max_occ^2 hits per pair of k-mer runs).
 * Every emit call writes nothing at or past the size it is given.  ws: gnm_overlap_scan_workspace_bytes(items) bytes, 16-byte
 * aligned (sketch: items = max(R, tile_bound)).  *_host: HOST pointers; with capacity < 0 only *total is written (the
 * size to allocate) and the record stays as it is; otherwise capacity >= *total is required and the record is added to as by the
 * device calls of the stage.  One integer atomic per record word and workgroup; no workgroup waits for another: outputs and
 * record depend on the inputs alone, not on the grid or gnm_set_occupancy_cap.  k, w, max_occ, band, min_hits out of range,
 * counts negative or too large, a_lo / a_hi out of order or range, a NULL or misaligned record / ws / packed / lower_hits, NULL arrays that the sizes need and (host) threads
 * outside [1, 1024] are errors, returned before anything runs.                                                                      */
#define GNM_SKETCH_TILE 512
typedef struct gnm_overlap_record {
  int64_t reads, kmers_valid, minimizers, runs, skipped_runs, skipped_entries, hits, same_read, groups, few_hits, too_short,
      contained_groups, links, calls;
} gnm_overlap_record;
size_t gnm_overlap_scan_workspace_bytes(int64_t items);
int64_t gnm_sketch_tile_bound(int64_t R, int64_t packed_bytes);
int gnm_sketch_count(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int k,
                     int w, int64_t* tile_ptr, int64_t* tile_off, int64_t tile_bound, void* record, void* ws, size_t ws_bytes,
                     void* stream);
int gnm_sketch_emit(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int k,
                    int w, const int64_t* tile_ptr, const int64_t* tile_off, int64_t tile_bound, int64_t M, int64_t* hash,
                    int32_t* read, int32_t* pos, uint8_t* strand, void* stream);
int gnm_sketch_host(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int k,
                    int w, int64_t capacity, int64_t* hash, int32_t* read, int32_t* pos, uint8_t* strand, int64_t* total,
                    void* record, int threads);
int gnm_seed_pairs_count(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* off, void* record, void* ws,
                         size_t ws_bytes, void* stream);
int gnm_seed_pairs_emit(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                        const int64_t* length, int64_t R, int k, int max_occ, const int64_t* off, int64_t N, int64_t* key,
                        int32_t* diag, void* stream);
int gnm_seed_pairs_host(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                        const int64_t* length, int64_t R, int k, int max_occ, int64_t capacity, int64_t* key, int32_t* diag,
                        int64_t* total, void* record, int threads);
int gnm_seed_pairs_lower_hits(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* lower_hits, int64_t R,
                              void* record, void* ws, size_t ws_bytes, void* stream);
int gnm_seed_pairs_lower_hits_host(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* lower_hits, int64_t R,
                                   void* record, int threads);
int gnm_seed_pairs_count_range(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t a_lo, int64_t a_hi, int64_t R,
                               int64_t* off, void* record, void* ws, size_t ws_bytes, void* stream);
int gnm_seed_pairs_emit_range(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                              const int64_t* length, int64_t R, int k, int max_occ, int64_t a_lo, int64_t a_hi, const int64_t* off,
                              int64_t N, int64_t* key, int32_t* diag, void* stream);
int gnm_seed_pairs_range_host(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                              const int64_t* length, int64_t R, int k, int max_occ, int64_t a_lo, int64_t a_hi, int64_t capacity,
                              int64_t* key, int32_t* diag, int64_t* total, void* record, int threads);
int gnm_chain_count(int64_t N, const int64_t* key, int64_t* off, void* record, void* ws, size_t ws_bytes, void* stream);
int gnm_chain_pairs(int64_t N, const int64_t* key, const int32_t* diag, const int64_t* off, int64_t G, const int64_t* length, int64_t R,
                    int64_t band, int64_t min_hits, int64_t min_overlap, int32_t* src, int32_t* dst, int64_t* prefix_length,
                    int64_t* overlap_length, uint8_t* valid, uint8_t* contained, void* record, void* stream);
int gnm_chain_pairs_host(int64_t N, const int64_t* key, const int32_t* diag, const int64_t* length, int64_t R, int64_t band,
                         int64_t min_hits, int64_t min_overlap, int64_t capacity, int32_t* src, int32_t* dst, int64_t* prefix_length,
                         int64_t* overlap_length, uint8_t* valid, uint8_t* contained, int64_t* total, void* record, int threads);

/* ---- ground-truth labels: y per edge from the reads' positions -- components, forward and backward reachability, emit ----------------
 * (Added without raising GNM_ABI_VERSION, which stays 7: six new symbols, no existing signature changes.)
 * What the reference computes with algorithms.get_gt_graph (graph_parser.py:307-309), restated so that it does not depend on a walk
 * order.  Per node (the caller's numbering; v and v^1 are the two strands of a read) start, end, strand int64 with
 * 0 <= start < end < 2^32 and strand +1 or -1.  Edge s -> d is VALID when strand[s] == strand[d] == +1, s != d and
 * start[s] <= start[d] < end[s]; every other edge falls under the first that applies of wrong_strand, self_loops, gap
 * (start[d] >= end[s]), backward (start[d] < start[s]).  Over the + strand nodes and the valid edges: the weakly connected
 * components, the ROOT of each the node of smallest (start, id); fwd = what a root reaches; the TOP of a component = the node of fwd
 * with the largest end, the smallest id among equals; bwd = what reaches the top; backbone = fwd and bwd (a component of one node
 * is its own backbone and labels nothing).  y = 1 for every valid edge with both ends on the backbone and for every copy of its
 * mirror d^1 -> s^1, else 0.  twin_missing counts the copies of such edges whose mirror the graph does not hold.
 * Device calls, over the index of gnm_graph_build_index (nperm / nrank: both NULL, or the internal numbering and its inverse):
 * gnm_gt_prepare (a memset and 2 launches): checks the nodes, classifies the edges; record ADDS edges, valid, wrong_strand,
 *   self_loops, gap, backward, invalid (unusable nodes; everything later then does nothing), calls (+1).
 * gnm_gt_rounds (1 - 3 + rounds launches): rounds first_round .. first_round + rounds - 1 of stage 0 (components: min-label hooking
 *   with pointer jumping over the valid edges, 64-bit atomicMin), 1 (fwd) or 2 (bwd; its first round selects the tops by a 64-bit
 *   atomicMax); changed[j] (int64 [rounds]) = what round first_round + j lowered or reached, -1 for invalid input.  The caller runs a
 *   stage until a round reports 0 and the stages in order; a round on a finished stage changes nothing.  How many rounds a stage
 *   takes depends on the schedule; what it ends in does not.
 * gnm_gt_emit (2 launches), after stage 2: y fp32, valid uint8 [E] in edge-id order; backbone uint8, component (the root's id),
 *   top int32 [n] (-1 on - strand nodes); record ADDS components, singletons, backbone, positives, twin_missing.  twin: NULL (the
 *   mirror is searched in the out-row), or int64 [E] mirror edge ids with src, dst the caller's edge list: an entry is believed only
 *   when it names the mirrored pair.
 * ws: gnm_gt_workspace_bytes(n, E) bytes, 16-byte aligned, the same for all calls of one graph and untouched in between.
 * gnm_gt_sweeps(): the sweeps a workgroup makes over its nodes per fwd / bwd round.
 * gnm_gt_labels_host: all of it on HOST pointers over the caller's edge list (union-find and queues over the same header,
 *   csrc/gnm_labels.h); invalid input is an error and writes nothing but record.invalid.
 * Integers only; the outputs and the record depend on the inputs alone, not on the grid or gnm_set_occupancy_cap.  Counts negative
 * or >= 2^31 - 1, a NULL or misaligned record / ws / changed and NULL arrays that the sizes need are errors, returned before
 * anything is launched.                                                                                                            */
typedef struct gnm_gt_record {
  int64_t edges, valid, wrong_strand, self_loops, gap, backward, components, singletons, backbone, positives, twin_missing, invalid,
      calls;
} gnm_gt_record;
size_t gnm_gt_workspace_bytes(int64_t n, int64_t E);
int gnm_gt_sweeps(void);
int gnm_gt_prepare(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                   const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm, const int32_t* nrank,
                   const int64_t* start, const int64_t* end, const int64_t* strand, void* record, void* ws, size_t ws_bytes,
                   void* stream);
int gnm_gt_rounds(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                  const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm, const int32_t* nrank,
                  int stage, int64_t first_round, int64_t rounds, int64_t* changed, void* ws, size_t ws_bytes, void* stream);
int gnm_gt_emit(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm, const int32_t* nrank,
                const int64_t* twin, const int32_t* src, const int32_t* dst, float* y, uint8_t* valid, uint8_t* backbone,
                int32_t* component, int32_t* top, void* record, void* ws, size_t ws_bytes, void* stream);
int gnm_gt_labels_host(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int64_t* start, const int64_t* end,
                       const int64_t* strand, const int64_t* twin, float* y, uint8_t* valid, uint8_t* backbone, int32_t* component,
                       int32_t* top, void* record);

/* ---- composite entry points (ABI 5): the measured path's launch sequences behind one call each -------------------------
 * For hosts that do not want to schedule the kernels themselves (a C++ trainer, a Go / Rust / Java binding).  Host code only:
 * every arithmetic step is one of the entry points above, called in the order the Python engine calls them on ONE stream, so
 * the results are the engine's bit for bit (tests/cabi/host_step.cpp runs both and compares).  H = 128, BatchNorm mode.  Memory
 * stays the caller's: every output, intermediate and scratch buffer is passed in (device pointers unless noted).
 *   gnm_layer_forward    GatedGCN_1d.forward (gated_gcn_full.py:99-157): projections, t + BatchNorm_e statistics, the
 *                        two-sided gate sweep (or, without a forward plan, gate + by-source pass), BatchNorm_h, node update.
 *   gnm_stack_backward   autograd of L stacked layers (processor.py:15-20 reversed; train.py:257): gh = dL/dh_out(L-1) (read),
 *                        ge = dL/de_out(L-1), UPDATED IN PLACE to dL/de_in(0); gh_in = dL/dh_in(0); parameter gradients into
 *                        gr[i].  The chained two-sided schedule (bf16x3 mode; needs the backward sweep plan).
 * gnm_graph_view: the internal index (gnm_graph_build_index) and the sweep plans (gnm_graph_build_sweep_plan over
 * gnm_sweep_partition(N, 2) for the forward, (N, 1) for the backward; fwd_sinfo == NULL: no forward plan).
 * gnm_layer_state: a layer's inputs and everything its forward leaves for its backward (h_out / e_out of layer i are
 * h_in / e_in of layer i+1).  gnm_scratch: partials* hold gnm_compose_partials_doubles() doubles each, ws / ws2 hold
 * gnm_compose_workspace_bytes(H) bytes each (partials2, partials3, ws2: gnm_stack_backward only).                        */
typedef struct gnm_graph_view {
  int64_t N, E;
  const int32_t *isrc, *idst, *in_ptr, *out_ptr, *out_pos, *out_dst;
  const uint32_t *fwd_sinfo, *fwd_dinfo; int64_t fwd_nodes_per_block, fwd_nfix; const int32_t* fwd_fix_nodes;
  const uint32_t* bwd_sinfo; int64_t bwd_nodes_per_block, bwd_nfix; const int32_t* bwd_fix_nodes;
} gnm_graph_view;
typedef struct gnm_layer_weights { const float *W5, *b5, *W3, *b3, *gamma_e, *beta_e, *gamma_h, *beta_h; } gnm_layer_weights;
typedef struct gnm_layer_state {
  const float *h_in, *e_in;                                   /* [N,H], [E,H] (internal edge order) */
  float *P, *t, *e_out;                                       /* [N,5H], [E,H], [E,H] */
  float *hf, *inv_f, *hb, *inv_b, *z, *h_out;                 /* [N,H] each */
  float *stat_e, *stat_h;                                     /* [4,H] each */
} gnm_layer_state;
typedef struct gnm_layer_grads { float *gW5, *gb5, *gW3, *gb3, *g_gamma_e, *g_beta_e, *g_gamma_h, *g_beta_h; } gnm_layer_grads;
typedef struct gnm_backward_work {
  float* gP[2];                                               /* [N,5H] each */
  float *Q, *UT, *DT;                                         /* [N,2H] each */
  float* gh_tmp[2];                                           /* [N,H] each */
  float* bstat_e[2];                                          /* [2,H] each */
  float* bstat_h;                                             /* [2,H] */
} gnm_backward_work;
typedef struct gnm_scratch { double *partials, *partials2, *partials3; void* ws; size_t ws_bytes; void* ws2; size_t ws2_bytes; } gnm_scratch;
size_t gnm_compose_workspace_bytes(int H);
size_t gnm_compose_partials_doubles(void);
int gnm_layer_forward(const gnm_graph_view* g, int H, const gnm_layer_weights* w, const gnm_layer_state* s, const gnm_scratch* sc,
                      void* stream);
int gnm_stack_backward(const gnm_graph_view* g, int H, int L, const gnm_layer_weights* w, const gnm_layer_state* s,
                       const gnm_layer_grads* gr, const float* gh, float* ge, float* gh_in, const gnm_backward_work* wk,
                       const gnm_scratch* sc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNM_H */
