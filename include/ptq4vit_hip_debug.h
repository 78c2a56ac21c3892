/* ptq4vit_hip_debug.h -- measurement / test-only entry points of libptq4vit_hip.so.
 *
 * NOT part of the drop-in boundary (include/ptq4vit_hip.h): nothing here replaces a reference interface, production code
 * never calls it, and it is the only PROCESS-WIDE mutable state of the library (SURVEY.md s8-b3 asks for none beyond the
 * per-thread error string on the boundary itself).  The scripts under tools/, bench.py --tune / --variant and the kernel-vs-kernel
 * agreement tests use it.
 */
#ifndef PTQ4VIT_HIP_DEBUG_H
#define PTQ4VIT_HIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A/B switches for measurements and kernel-vs-kernel agreement tests; never needed in production (default 0).
 * `variant` selects reference kernel paths (bits 1, 2, 4, 2048, 32768, 65536, 131072, 524288, 1048576, 2097152, 4194304,
 * 8388608, 134217728; list in csrc/p4v_api.hip), `force_generic` routes every int8 sweep through the generic kernel.  Any
 * other bit selected a path that was measured and removed: P4V_ERR_INVALID.  Process-wide, relaxed atomics: set them while
 * no call is in flight. */
int p4v_debug_set_variant(int variant, int force_generic);
/* Overrides of launch heuristics: key 0 / 1 / 2 / 3 = candidate groups of k_sweep6 / k_sweep2 / k_sweep2g / k_sweep7
 * (0 = cost model), key 4 = print the launch plans to stderr, key 5 = workgroup order of k_sweep7 + 1, key 6 = k_sweep6 prologue
 * of the cost model (0.1 us), keys 9-15 = slice sizes / tiers / thresholds of the pruned passes, key 12 = reference path switches (7 cosine
 * on the generic kernel, 9 no per-score-block ranges, 11 the round-4 quantiser, >= 16 k_bound timing ablations, 4 the previous
 * stage-B1 kernel of Linear passes (k_bound, 64 x 32 wave tile); 1, 2, 3, 5, 6, 8, 10 and 12 selected removed paths:
 * P4V_ERR_INVALID). */
int p4v_debug_set_tuning(int key, int value);
/* The stage-B1 totals (the bound) of the pruned search passes of the calling thread.  out == NULL and count == NULL: start
 * keeping them (costs one small copy and a stream synchronise per pruned pass; not inside p4v_calibrate_group).  Otherwise:
 * stop, *count = how many were kept, out receives min(capacity, *count) of them -- per pass, the evaluated entries of its
 * [candidate][score block] table in table order.  Nothing but the bound may depend on these numbers (csrc/p4v_api.hip::
 * run_pass_pruned); exposed so that a test can hold two stage-B1 kernels against each other within prune_margin. */
int p4v_debug_bound_totals(float* out, int64_t capacity, int64_t* count);
/* The stage tables of the pruned search passes of the calling thread (csrc/p4v_api.hip::run_pass_pruned_impl,
 * run_sos_split_pruned_impl).  out == NULL and count == NULL: start keeping them (costs copies of every table and a stream
 * synchronise per staged pass; not inside p4v_calibrate_group).  Otherwise: stop, *count = the 32-bit words kept, out receives
 * min(capacity, *count) of them.  One record per staged pass (p4v_prune_counters[0] counts the same passes), appended at
 * whichever exit the pass takes, floats by their bits:
 *   [0] words of the record  [1] 0 search pass, 1 split search  [2] search round, [3] side (0 = w / A / split, 1 = a / B) of the
 *   fused call, -1 outside one  [4] eq_n  [5] nj  [6] virt  [7] hull_selects  [8] b1_bound  [9] the second tier ran
 *   [10] the host read the survivors  [11] the margin (float)  [12] rows of stage B1's table (virt: 1, the synthetic candidate)
 *   [13] SA2 follows  [14] S2 follows (stage B2 ran; after the merge)  [15] per-block ranges kept  [16..21] r1, r2, r3 (lo, hi)
 *   [22], [23] rows per segment of the two slices;
 *   then best_idx [nj], rblk2 [2 nj], rblk3 [2 nj], SA [eq_n][nj], SB [rows][nj], SA2 [eq_n][nj], S2 [eq_n][nj].
 * What the pass did not write is -1 (r3, rblk3, best_idx) or absent (SA2, S2).  For the tests of the two premises of the exact
 * pruning: the stage-A scores are upper bounds of the totals, and the decision kernels pick what k_select picks from the totals. */
int p4v_debug_prune_tables(int32_t* out, int64_t capacity, int64_t* count);
/* The decision chain of a pruned pass on tables of the caller: k_prune_pick -> stage B1 -> k_prune_hull (-> stage A2 ->
 * k_prune_hull) -> stage B2 -> k_merge_scores / k_merge_virtual -> k_select through the launchers of run_pass_pruned_impl, with
 * no sweep: the stages are what k_finish would leave of the full totals d_T [C][nj] -- stage B1 holds T on r1 for every block
 * and -inf elsewhere (virt: T[best[j]][j] in row 0), stage A2 holds d_SA2 (optional: no second tier without it) and stage B2
 * holds T where the candidate lies in the hull's range and, with honour_blk, in the block's own range; -inf elsewhere.
 * d_SA [C][nj]: the stage-A scores.  d_cands [C + 1][nj]: the candidate table (row c, column j: the interval candidate c gives
 * block j).  virt: stage B1 on the synthetic candidate (needs nj > 1).  host_reads: the host reads the survivor ranges and a pass
 * without survivors ends without stage B2.  hull_selects follows plan_prune's rule.
 * Out, all on the device: d_ranges [6] = r1, r2, r3; d_rblk [4 nj] = the per-block ranges of the two hulls; d_best [nj] = the
 * stage-A winners (virt); d_interval [nj], d_best_out [nj] = the selection.  What a branch does not write is -1.  info (host,
 * [3]): hull_selects, the second tier ran, the exit (0 merge and k_select, 1 / 2 no stage B2 after the first / second hull).
 * Null pointers, C < 1, nj < 1, nj > 4096 and virt with nj == 1 are P4V_ERR_INVALID before anything is launched.  Synchronises
 * the stream (several times: it builds the stage tables on the host). */
int p4v_debug_prune_decide(const float* d_SA, const float* d_SA2, const float* d_T, const float* d_cands, int C, int nj, int virt,
                           int honour_blk, int host_reads, int32_t* d_ranges, int32_t* d_rblk, int32_t* d_best, float* d_interval,
                           int32_t* d_best_out, int32_t* info, void* stream);
/* The arena that carves the caller's workspace, for the tests of the workspace contract (include/ptq4vit_hip.h, Conventions).
 * p4v_debug_set_arena_gap: with a non-zero value every allocation of the arena -- from the bottom and from the top, in the sizing
 * run of *_workspace_bytes() as well, which then includes the gaps -- leaves that many bytes unused behind it; a poisoned workspace
 * then shows a kernel that stores past ANY carved buffer, not only past the last one.  A multiple of 256 (the arena's alignment;
 * the gaps move buffers, they never change a buffer's alignment); anything else is P4V_ERR_INVALID.  0 (the default): off.
 * Process-wide, relaxed atomic: set it while no call is in flight, and size the workspace after setting it. */
int p4v_debug_set_arena_gap(size_t bytes);
/* While the arena gap is on (recorded only then: with the gap at 0 the library does nothing for this word and reports no range):
 * the byte ranges [begin, end), offsets from d_workspace, that any allocation of the LAST call with a workspace made by the calling
 * thread ever covered, merged and ascending: out receives min(cap, n) pairs {begin, end}, the return value is n.  A pass that
 * rewinds the arena does not erase its ranges.  Kept on the host per thread, nothing is launched for it.  The members of a
 * p4v_calibrate_group call run on the library's own threads: their ranges are not reported. */
int p4v_debug_arena_ranges(uint64_t* out, int cap);
/* Where the calling thread's last p4v_mlp_quant_forward left fc2's row plane(s): out[0], out[1] = byte offsets of plane 1 / 2 from
 * d_ws (plane 2: 0 unless out[4]), out[2] x out[3] = padded rows x columns of a plane (row-major int8), out[4] = 1 for the twin
 * pair.  The planes outlive the call: fc2's scratch lies behind them.  For the tests; nothing is launched. */
int p4v_debug_mlp_planes(uint64_t* out);
/* The same for the calling thread's last p4v_attn_quant_forward or p4v_wattn_quant_forward (the window call shares the chain
 * and its record) and matmul2's row plane(s), [batch*heads][Mp][Kp]: out[2] = batch * heads * Mp (all rows of a plane),
 * out[3] = Kp. */
int p4v_debug_attn_planes(uint64_t info[5]);
/* Where the calling thread's last p4v_qkv_attn_quant_forward left the three operand planes k_qkv_heads wrote (matmul2's row
 * plane(s) of that call: p4v_debug_attn_planes): info[0..2] = byte offsets of Q(q), Q(k^T), Q(v) from ws, info[3] = Z = batch *
 * heads, info[4], info[5] = padded rows of a z of the q / k^T plane, info[6] = their row length K1p ([Z][rows][K1p] at [tok][d]),
 * info[7] x info[8] = rows x row length of a z of the v plane ([Z][NpB][Kp] at [d][tok]).  The planes outlive the call. */
int p4v_debug_qkv_planes(uint64_t info[9]);
/* ONE sweep of the split-of-softmax split search (k_sos_split + k_finish) on the operands of `desc`, over the first n_cands of
 * the 20 splits: d_scores [n_cands] receives the score table, entries outside [c_lo, c_hi) as k_finish leaves them (-inf).
 * c_lo < 0: no candidate range.  known_cands: what the caller tells the sweep about the number of candidates in the range
 * (< 0: unknown) -- it selects the kernel instance, never the result.  Synchronises the stream.  For tests that hold the
 * instances of the kernel against each other on ranges the search itself does not produce. */
int p4v_debug_sos_sweep(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out, const float* d_grad,
                        int n_cands, int c_lo, int c_hi, int known_cands, float* d_scores, void* d_workspace, size_t workspace_bytes,
                        void* stream);
/* The row selection of the exact pruning alone (k_topk_rows; csrc/p4v_api.hip::slice_fill runs it on the per-sample metric
 * weight): for each of `segs` segments of `n` fp32 masses, d_mass [segs][n], the segment-local indices of the k heaviest
 * entries in ASCENDING index order, d_idx [segs][k]; among equal masses the lowest indices are taken; negative masses
 * count as the lightest.  Exposed for the tests: a repeated or missing row would make the slice's partial sums an
 * invalid bound.  1 <= k <= n. */
int p4v_debug_topk_rows(const float* d_mass, int segs, int n, int k, int32_t* d_idx, void* stream);
/* The two fixed int8 planes of a twin row operand from one read of the source (k_pack_dual, the search's kernel for them):
 * d_x [rows][cols] fp32 -> d_q1, d_q2 [rows][cols_padded] (cols_padded % 64 == 0, zero padded).  sos = 0: the post-GELU
 * pair clamp(rint(x / *d_scale), 0, hi) and clamp(rint(x / const_scale), lo, 0); sos = 1: the split-of-softmax pair
 * PACK_SOS_HI / PACK_SOS_LO of the split *d_scale with q - 1 = qmax - 1.  Exposed for the bit-exactness tests. */
int p4v_debug_pack_dual(const float* d_x, long rows, long cols, long cols_padded, int sos, int lo, int hi, int qmax,
                        const float* d_scale, float const_scale, int8_t* d_q1, int8_t* d_q2, void* stream);
/* The candidate planes of one operand as the search packs them (k_pack; k_pack1 for a single plane and for the one
 * candidate of a range with live_max == 1): d_x [rows][cols] fp32 ->
 * clamp(rint(x / d_scales[c]), lo, hi) for the candidates c < n_cands, zero padded to [rows_padded][cols_padded]
 * (cols_padded % 64 == 0).  layout 0: [c][row][k]; 1: [row][c][k]; 2: [row][c / 2][k / 64][c % 2][64] (an odd n_cands padded
 * to a pair); 3: MFMA-fragment order of ONE plane (rows_padded % 64 == 0; every packed candidate lands in it).  d_crange
 * (optional, two ints on the device): only the candidates in [d_crange[0], d_crange[1]) are packed, and of those only the
 * ones whose d_done flag (optional, one byte per candidate) is 0; live_max >= 0: what the host knows of that range -- an upper
 * bound of its length (0: empty, nothing is launched) --, < 0: nothing.  general != 0: k_pack also where k_pack1 would
 * take the launch.  Bytes of candidates that are not packed are left as they were.  Exposed for the bit-exactness tests. */
int p4v_debug_pack_cands(const float* d_x, long rows, long cols, long rows_padded, long cols_padded, int layout, int lo, int hi,
                         const float* d_scales, int n_cands, const int* d_crange, const unsigned char* d_done, int live_max,
                         int general, int8_t* d_q, void* stream);
/* Rows of the im2col matrix of a conv input as the pruned passes gather them (k_gather_im2col, the search's kernel for the
 * slice rows of a Conv2d weight search): d_x [batch][in_channels][height][width] fp32, zero padded, groups = 1; row
 * r = (image, oy, ox) of the [batch * fh * fw][in_channels * kernel_h * kernel_w] matrix, column (ci, ki, kj) -- the element
 * F.unfold(x, ...).transpose(1, 2) holds there.  d_idx [k]: the rows to gather, 0 <= d_idx[i] < batch * fh * fw; d_dst
 * [k][in_channels * kernel_h * kernel_w].  A copy: every element is bit-identical to its source or 0 (padding).  A geometry
 * whose dilated kernel exceeds the padded input is P4V_ERR_INVALID.  Exposed for the geometry tests. */
int p4v_debug_gather_im2col(int batch, int in_channels, int height, int width, int kernel_h, int kernel_w, int stride_h, int stride_w,
                            int pad_h, int pad_w, int dil_h, int dil_w, const float* d_x, const int32_t* d_idx, int k, float* d_dst,
                            void* stream);
/* k_sweep6's epilogue operands in fragment order (k_prep_epi6): raw_out d_o (element (s, t) at s * o_ss + t * o_ts, s < sr
 * stationary rows, t < tr streaming rows), the metric weight d_wt (wt_mode 1), the bias (indexed by t if bias_on_t, else
 * by s) -> d_e, ceil(sr / 256) * ceil(tr / 64) tiles of 256 * 64 * 2 floats.  Exposed for the layout tests. */
int p4v_debug_prep_epi6(const float* d_o, const float* d_wt, const float* d_bias, long o_ss, long o_ts, int sr, int tr,
                        int bias_on_t, int wt_mode, int transposed, float* d_e, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTQ4VIT_HIP_DEBUG_H */
