/*
 * dmpfold_hip.h - C ABI of libdmpfold_hip.so: the DMPfold2 alignment -> coordinates
 * hot path as hand-written HIP for MI355X (gfx950).
 *
 * The reference (psipred/DMPfold2) has no FFI / plugin interface: its boundary is the
 * Python function dmpfold.aln_to_coords() (reference dmpfold/predict.py:74-158) whose
 * arithmetic lives in PyTorch operator calls.  Every entry point below replaces the
 * operator call sites named in its comment (file:line relative to the reference tree).
 * The Python shim dmpfold2_amd/predict.py binds them with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; `d_` = device pointer, `h_` = host pointer;
 *   - every function returns 0 on success or a negative dmp_status; the message of the
 *     last failure on the calling thread is dmp_last_error();
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only
 *     enqueue work, they never synchronise unless stated;
 *   - all floating point buffers are float32 row-major unless stated;
 *   - one dmp_ctx per GPU and per host thread; contexts are independent.
 */
#ifndef DMPFOLD_HIP_H
#define DMPFOLD_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 6): 65 functions.  New: the dmp_pipeline_* family (16 functions) - the throughput scheduler behind the C ABI;
 *    option "precision" accepts 2 (exact three-piece bf16 convolution and vertical GRU: full-width operands at the
 *    16-bit matrix cores' rate; "vgru_f32" accepts 2 for the latter alone).
 * 4 (round 5): 49 functions.  New: dmp_block_conv5x5_maxout_winners (the training slice's forward: maxout output + the
 *    winners autograd saves), dmp_head_conv_bwd, dmp_stem_maxout_winners and dmp_stem_bwd; dmp_block_conv5x5_maxout_bwd takes the saved winners (d_idx, NULL = run
 *    the forward again: the ABI-3 behaviour).  New options: precision (0 split-f16 / 1 the reference's float32 end to end),
 *    vgru_f32, gj_diag_blocked.
 * 3 (round 4): 45 functions instead of 60.  Removed: the experimental scheduler entry points that were measured
 *    slower (detached group chain, chain on its own stream, features ahead: six functions), the convenience wrappers
 *    predict_begin / predict_pass / predict_end_refine - dmp_predict and the unit calls cover them -, clear_faults and
 *    sync_check - dmp_sync_faults reports and clears -, profile_conv_ms and time_conv5x5 - dmp_profile_conv_intervals
 *    holds every launch's interval; the three lane functions became dmp_ctx_share_lane.  Options vgru_legacy and gj_lds are gone;
 *    act_scaling and vgru_persistent are new; fault bit DMP_FAULT_VGRU_HANDOFF is new.
 * 2: dmp_sync_faults clears what it reports, dmp_ctx_get_option and dmp_dca_features added. */
#define DMP_ABI_VERSION 5
#define DMP_MAX_SEQS 3000 /* predict.py:130-132: deeper MSAs are truncated */

typedef struct dmp_ctx dmp_ctx;

typedef enum dmp_status {
  DMP_OK = 0,
  DMP_ERR_ARG = -1,     /* bad argument (sizes, NULL, L < 8 ...) */
  DMP_ERR_HIP = -2,     /* a HIP runtime call failed */
  DMP_ERR_WEIGHTS = -3, /* unknown key, wrong shape, or weights incomplete */
  DMP_ERR_CAPACITY = -4, /* L or N exceeds what the context was created for */
  DMP_ERR_FAULT = -5     /* a device-side fault was recorded: results invalid */
} dmp_status;

/* Device-side fault bits (dmp_sync_faults).  A prediction during which a bit was raised returns NaN
 * coordinates and confidences. */
#define DMP_FAULT_SEQ_HANDOFF 1    /* sequence-GRU workgroup hand-off timed out */
#define DMP_FAULT_F16_RANGE 2      /* conv_mode 0: an activation reached |x| >= 6e4 (re-run in conv_mode 2) */
#define DMP_FAULT_REFINE_HANDOFF 4 /* minimiser workgroup hand-off timed out */
#define DMP_FAULT_EIG_HANDOFF 16   /* tridiagonalisation cluster: workgroup hand-off timed out */
#define DMP_FAULT_VGRU_HANDOFF 32  /* persistent vertical GRU: a row barrier between the workgroups of an XCD timed out */
#define DMP_FAULT_BAD_CODE 8       /* residue code > 21: the reference's embedding raises IndexError
                                      (network.py:223) */

int dmp_abi_version(void);
const char* dmp_last_error(void);

/* ---- context ------------------------------------------------------------------------
 * Allocates every device buffer the path needs for alignments up to max_N x max_L
 * (max_N is clamped to DMP_MAX_SEQS).  No allocation happens after this call.
 * DEVIATION from the reference, which has no length limit (network.py:218-221): 8 <= max_L <= DMP_MAX_L.
 * The eigensolver's kernels are instantiated per range of the order (<= 384: everything of the inverse iteration in
 * one workgroup's LDS; <= 1280: the vectors in LDS; <= 2048: in global memory; 8 x 256 rows per thread block of the
 * Householder step); every element count up to 442 L^2 and (21 L)^2 stays below 2^31 at 2048.  dmp_ctx_create answers
 * DMP_ERR_ARG ("max_L must be in [8, 2048]") for more, and the Python front end raises RuntimeError naming the
 * alignment's length before anything is computed.  The largest configuration of BASELINE.json (L = 1000) needs
 * 8.5 GB of the 288; L = 2048 with 3000 rows about 60 GB. */
#define DMP_MAX_L 2048
/* option "search_structures" (dmp_ctx_set_option): the most entries one prediction searches, and the scratch budget in
 * MiB that decides how many of them are in flight at a time */
#define DMP_SEARCH_MAX 4096
#define DMP_SEARCH_BUDGET_MIB 256
#define DMP_PASSES_BUDGET_MIB 64      /* option "score_passes": scratch of a chunk of passes */
int dmp_ctx_create(int device, int max_L, int max_N, dmp_ctx** out);
void dmp_ctx_destroy(dmp_ctx* ctx);
/* (device memory held by the context: option "device_mib" of dmp_ctx_get_option, read only) */

/* Options (additive).  "conv_mode" selects how the 5x5 convolutions form their float32 products:
 *   0            each float32 operand split into two f16 pieces, 3 f16 MFMA products, float32
 *                accumulation - same error against float64 as a float32 convolution, 5.3x the
 *                f32 matrix-core rate; activations must stay inside the f16 range (|x| < 6e4,
 *                checked on the device, reported by dmp_sync_faults);
 *   1            the f32 matrix-core instruction (bitwise an fmaf chain);
 *   2 (default)  exact 3-way bf16 split, 6 bf16 MFMA products (no range limit, 2.7x the f32 rate).
 * "conv_f32_exact" = 1 is shorthand for conv_mode 1 (0 restores the default).
 * "precision" = 0 / 1 / 2 is the end-to-end switch: 0 = the FAST mode (split-f16 products of 22-23-bit operands in the
 * convolutions AND in the vertical GRU, whose gates use the hardware v_exp_f32 / v_rcp_f32; 1.8 x the speed of 2);
 * 1 = the reference's arithmetic instruction for instruction - conv_mode 1 and the float32 vertical GRU
 * (v_mfma_f32_16x16x4_f32 products, the device library's expf / tanhf in the gates: nn.GRU in float32, network.py:189,
 * 223-224); with it no f16 / bf16 matrix-core kernel runs; 2 (round 6) = FULL-WIDTH operands at the 16-bit matrix cores'
 * rate - conv_mode 2 (every float32 operand as three exact bf16 pieces = 24 significand bits, the six piece products
 * above 2^-24 accumulated in float32) and the vertical GRU the same way ("vgru_f32" 2: three bf16 pieces per operand
 * of its three products, float32 accumulation, the library gate functions of setting 1): A CONTEXT'S INITIAL SETTING (the
 * reference computes in float32: predict.py:136, network.py:25-31) and what the drop-in entry points run; 1.7 x the
 * speed of setting 1.
 * Reads back 0 / 1 / 2, or -1 for a mixed setting.
 * "vgru_f32" = -1 / 0 / 1 / 2: the vertical GRU alone (initially 2, with "precision" 2); -1 follows the convolution (float32 exactly when
 * conv_mode is 1, so "conv_mode" 1 and "precision" 1 select the same thing), 0 / 1 / 2 force the split-f16 / the float32
 * / the three-piece bf16 form whatever the convolution does.  Reads back what the next prediction will run (0 / 1 / 2).  The float32 form costs
 * 5.3 x the matrix-core time of the split form (41 against 15 ms for one alignment of 2000 x 300, 196 against 72 ms
 * for a chain of eight); its fallback without the persistent launch ("vgru_persistent" = 0) is the same kernel, one
 * launch per row, the same bits.
 * "tridiag_single" = 1 runs the Householder tridiagonalisation of the MDS eigensolver in a single
 * workgroup (one launch) instead of one multi-workgroup launch per step; same algorithm, different
 * summation order (results agree to float64 rounding).
 * "tridiag_cluster" (default 1): orders up to 640 run
 * every Householder step in ONE launch on a cluster of 32 workgroups of one XCD; 0 = one launch per step (hipGraph
 * chain).  The same algorithm with the float64 partial sums associated differently: the float32 results are the same bits
 * on full-rank matrices, the near-null columns of a rank-deficient Gram matrix can differ in their last bits (a
 * bit-for-bit comparison of two predictions needs the same setting); the cluster is faster for one prediction (0.9 against 1.9 ms at
 * order 300), the launches disturb the convolutions of other contexts less (the multi-engine scheduler sets 0).
 * "cluster_local" (default 1): the cluster kernels (sequence GRU, minimiser, tridiagonalisation) publish their
 * hand-off granules with plain stores when they find all their workgroups on one XCD (run-time check); 0 = always
 * agent-scope stores, the protocol that does not depend on placement.  Same bits, 1.84 against 2.8 us per GRU step.
 * "gj_diag_groups" = 2 / 4 / 8: threads (x 128) of the one-workgroup diagonal sweep of the inverse; same bits; 4 is the
 * default (8.9 against 10.0 ms per inverse at D = 6300 with 2, the form of rounds 1-3).
 * "gj_diag_blocked" (round 5, default 0): 1 = the 128 x 128 diagonal block of a block step is swept in 8 sub-blocks of 16
 * pivots (the pivot block inside one wave, W = T P and the rank-16 update on the f32 matrix cores) instead of as a chain
 * of 128 barrier-synchronised pivots (0: the arithmetic of rounds 1-4; "gj_diag_groups" applies to it).  The blocked form
 * is faster (6.6 against 7.65 ms per inverse at D = 6300, 18.4 against 20.2 at D = 10 500) and closer to the float64
 * inverse (4.5e-7 against 8.7e-7 of max |inv| at D = 630); the two agree to 1.1e-6, not bit for bit - and on three of the
 * reference's recycling fixtures (L = 200, ten passes; the x 4 weight set) that difference, amplified by eleven trunk
 * passes, moves a confidence by 1.4 .. 2.0e-4 from the reference's where the chain's stays below 1e-4, so the chain
 * remains the default of the prediction path.
 * "gj_pairs" (default 1): the inverse takes its 128-column block steps in pairs - one pass of the trailing update over
 * the matrix tiles per two steps (119 against 173 ms at D = 21 000, 20.4 against 26.0 at D = 10 500, equal at D = 6300);
 * 0 = one pass per step.  Same bits.
 * "gj_lookahead" = 0 / 1 / 2 (with gj_pairs = 0 only): the inverse's look-ahead - the next block step's diagonal sweep and panels on the context's
 * second stream beside this step's trailing update - where one prediction has the device to itself (dmp_predict,
 * dmp_spd_inverse, dmp_dca_features): 0 never, 1 (default) from 64 tile rows on (D > 8064: 23.5 against 25.4 ms at
 * D = 10500; at D = 6300 it loses, 8.7 against 7.7 ms), 2 at every size.  Same bits in every mode.
 * "conv_tile_bands" = 0 / 1 / 2 (round 6): pixel tile of the split-product convolutions - 1 = 16 x 16, 2 = 8 rows x 16
 * columns (twice the workgroups), 0 (default) = 8 x 16 where the 16 x 16 shape would leave half the CUs without a workgroup
 * (L <= 80), 16 x 16 above.  The same bits in every setting.
 * "act_scaling" (default 1): conv_mode 0 takes the f16 pieces of 2^e x activation, with e chosen per residual block
 * at dmp_weights_finalize from the InstanceNorm weights of the blocks before it (a bound of the residual stream), so the
 * low pieces of the bulk of the activations are normal f16 numbers whether the trunk sits at 1e-3 or at 1e4, and a trunk
 * that would leave the f16 range unscaled is scaled down instead of faulting; 0 = unscaled pieces (the round-3
 * arithmetic).  "act_scale_log2_block<k>" (k = 1..16, read only) answers e of block k's input.
 * "vgru_persistent" (default 1): the vertical GRU's chain as ONE weight-stationary launch (columns partitioned over the
 * XCDs, hidden units over the CUs of an XCD, XCD-local row barriers); 0 = one launch per alignment row (the round-3
 * group step kernel, also the fallback on a device without 256 CUs).  Reads back 0 where the persistent form is not
 * available.  The two forms sum K in different orders: results agree to float32 rounding.
 * "vgru_debug_drop_wg" = 1 (TESTS ONLY): the persistent chain is launched one workgroup short, so one XCD's row barrier can
 * never complete - the situation of a second process holding CUs.  The kernel must time out ONCE (a quarter of a second),
 * raise DMP_FAULT_VGRU_HANDOFF and leave its row loop; the Python layer then repeats with one launch per row.
 * "refine_single" = 1 runs the minimiser (dmp_refine_coords, dmp_predict*) in one workgroup instead
 * of a cluster of 16 that hands the coordinates over every step; same iteration, different
 * partial-sum slices (results agree to float32 rounding).
 * "recycle_tol_mA" (default 0 = off; negative: DMP_ERR_ARG): stop recycling once the C-alpha trace has converged.  The
 * value is a tolerance in milli-Angstrom, read when a prediction begins.  With it > 0 the tail unit of every pass p
 * launches one more kernel (recycle_delta, csrc/coords.hip) that computes
 *   d_p = sqrt(mean over i < j of (D(ca_p)_ij - D(seed_p)_ij)^2),  D(x)_ij = sqrt(max(|x_i - x_j|^2, 1e-8)),
 * the RMS change, in Angstrom, between the distance map that seeded pass p (seed_p: the refined pass-0 trace for p = 1,
 * ca_(p-1) after that) and the one pass p's own trace would seed (the traces "ca_pass" records; float64, fixed summation
 * order: the same bits on every run).  Pass 0 has no delta (+inf is recorded).  If (float)d_p <= tol_mA * 1e-3f (false for
 * NaN) for a p >= 1, pass p is the last one: best-of, final refinement and backbone run exactly as if nloops had been p,
 * so A CONVERGED PREDICTION THAT STOPPED AFTER PASS k IS BIT-IDENTICAL TO A PLAIN ONE WITH nloops = k, and one that
 * never meets the tolerance to the plain one with the nloops given.  The decision is the host's, between passes: the
 * kernel leaves {pass, stop} in a word of pinned host memory, and it is read in front of unit 0 of every pass >= 2 once
 * the tail unit before it has completed - see dmp_predict and dmp_predict_next_unit below.  With the option 0 no extra
 * kernel is launched and nothing ever waits.
 * "passes_run" (read only): the trunk passes of this context's last prediction, valid after dmp_predict_end (nloops + 1
 * unless "recycle_tol_mA" stopped it earlier).  The tickets of a pipeline do not carry their own count - that would take
 * a new entry point (an ABI 6); dmp_pipeline_stats has the sums (and "emit_distmap" hands every prediction, a
 * pipeline's tickets included, its own count).
 * "emit_distmap" (0 or 1, default 0; any other value: DMP_ERR_ARG): return the predicted C-alpha distance map of the pass
 * the best-of rule chose.  Read when a prediction begins (dmp_predict, dmp_predict_begin_units) and held for it.  With it
 * 0 no extra kernel is launched, nothing extra is written, and every output is bit for bit what it is without the
 * option.  With it 1 THE d_conf ARGUMENT OF dmp_predict, dmp_predict_end AND dmp_pipeline_submit MUST HOLD
 * L + L*L + 3 FLOATS (the library cannot check the size):
 *   [0, L)          the confidences, unchanged
 *   [L, L + L*L)    dm, row-major: dm[i][j] = |(h0[i][j] + h0[j][i]) * 0.5f| of the chosen pass, h0 the head's channel 0
 *                   (network.py:237-243) - bit for bit the values that pass's Gram matrix, and through it the MDS
 *                   embedding and the trace, were formed from.  dm is exactly symmetric.  Its DIAGONAL IS WHAT THE
 *                   NETWORK PREDICTS, NOT ZERO.
 *   L + L*L         best_pass: the 0-based pass the strict '>' rule on the mean confidence logit (network.py:302) kept,
 *                   as a float
 *   L + L*L + 1     passes_run: trunk passes run, as a float (nloops + 1, or fewer with "recycle_tol_mA"; exact below 2^24)
 *   L + L*L + 2     map_rms = sqrt(mean over i < j of (dm[i][j] - |ca_i - ca_j|)^2) in Angstrom, ca the final, refined
 *                   C-alpha trace the backbone is built from: how well the model realises the map it was derived from.
 *                   The distances are formed in float64 from the float32 coordinates, sqrt((dx*dx + dy*dy) + dz*dz)
 *                   with no clamp, the squares summed in float64 in a fixed order (the same bits on every run), and
 *                   the result is rounded once to float32.  The reference has no such quantity.
 * A prediction that latched a device-side fault returns NaN in all L + L*L + 3 floats.  Cost: one store in the best-of
 * kernel always; with the option on one kernel per pass tail (keep_best_dm: workgroups of a pass that was not taken leave
 * at once) and one in dmp_predict_end (emit_distmap), csrc/coords.hip.  A context holds max_L^2 floats for the map.
 * "score_native" (0 or 1, default 0; any other value: DMP_ERR_ARG): score the model against a native C-alpha trace on the
 * device.  Read when a prediction begins and held for it.  With it 0 nothing is launched, nothing extra is read or written,
 * and every output is bit for bit what it is without the option.  With it 1 THE d_conf ARGUMENT OF dmp_predict,
 * dmp_predict_end AND dmp_pipeline_submit MUST HOLD S0 + 5L + 24 FLOATS, S0 = L, OR L + L*L + 3 WITH "emit_distmap" ON AS
 * WELL (the library cannot check the size): behind the confidences (and the distance-map extension) sits the SCORE BLOCK.
 * THE CALLER WRITES ITS TWO INPUTS BEFORE THE CALL (on a pipeline: the submission's ready_event is behind those writes);
 * dmp_predict_end reads them from d_conf itself.  Offsets relative to S0:
 *   [0, 3L)         in   native C-alpha trace, one row (x, y, z) per alignment column; a row whose x is NaN: no native
 *                        residue here
 *   3L              in   lnorm, the length TM-score and GDT are normalised by; 0: the number of rows present
 *   3L + 1          out  n_pairs: rows present
 *   3L + 2          out  rmsd: Kabsch RMSD over all present rows [Angstrom]
 *   3L + 3          out  tm
 *   3L + 4          out  gdt_ts = (c1 + c2 + c4 + c8) / 4 / lnorm, c the counts below
 *   3L + 5          out  gdt_ha = (c0.5 + c1 + c2 + c4) / 4 / lnorm
 *   3L + 6          out  lddt: global lDDT-C-alpha
 *   3L + 7 .. 11    out  the five counts of rows deviating by less than 0.5, 1, 2, 4, 8 Angstrom, each its own maximum over
 *                        every superposition the search visited
 *   3L + 12 .. 23   out  R (row-major 3 x 3) and t of the superposition that gave tm: native ~ R model + t
 *   [3L+24, 4L+24)  out  per-residue lDDT-C-alpha; NaN where the native row is absent, 0 where the residue has no partner
 *                        inside the radius
 *   [4L+24, 5L+24)  out  per-residue deviation [Angstrom] under that superposition; NaN where the native row is absent
 * The model trace is the final, refined C-alpha trace the backbone is built from (d_coords[:, 1]).  n_pairs < 3: NaN in
 * every out slot except n_pairs, no fault.  A prediction that latched a device-side fault returns NaN in every out slot;
 * the inputs are left alone.
 * The scores (the reference has none of them; float64 from the float32 coordinates, each output rounded once to float32).
 * The n present rows in sequence order are k = 0 .. n-1; d0 = max(1.24 (lnorm - 15)^(1/3) - 1.8, 0.5) for lnorm > 15, else
 * 0.5; d_cut = min(max(d0, 4.5), 8).  Seeds: the fragment lengths are the distinct values of f_0 = n and
 * f_k = max(n >> k, min(4, n)), k = 1..5; every start s = 0 .. n - f of every length is a seed, numbered by (level,
 * start): at most 1 + 5 max_L, a context holds records for 6 max_L.  One seed starts with S = its fragment and repeats at
 * most 20 times: Kabsch superposition of the model on the native over S; deviations d_k of all n rows;
 * TM = sum_k 1 / (1 + (d_k / d0)^2) / lnorm and the five counts #{d_k < c}; the seed's best TM (with its R, t) and each of
 * its five best counts are updated; S' = {k : d_k < d_cut}; stop if |S'| < 3 or S' = S, else S = S'.  Seed 0 (the whole
 * chain), iteration 0, also yields rmsd.  tm is the maximum over the seeds, ties to the lowest seed number (R, t are
 * reproducible); each count is its own maximum over all seeds.  lDDT-C-alpha is superposition-free: over the ordered pairs
 * i != j of present rows with native distance below 15 Angstrom, a pair is preserved at threshold 0.5, 1, 2, 4 if
 * |d_model - d_native| is below it; per residue preserved / (4 x partners), globally total preserved / (4 x total pairs)
 * (0 without any pair), from integer counts: exact and order-free.
 * THIS IS THE TM-SCORE PROGRAM'S KIND OF SEARCH, NOT ITS BITS: any superposition gives a lower bound of the true maximum,
 * and nobody has compared the values with that program's.  MaxSub is not offered; a sequence-independent alignment is
 * what option "align_structure" below gives.
 * Cost with the option on: three launches in dmp_predict_end (csrc/score.hip: score_prep, score_lddt, score_search - one
 * workgroup per seed, both traces and the set S in LDS, 6L floats + L flags; sums in a fixed order, the same bits on
 * every run).  A context holds 6 max_L records of 20 doubles.
 * "score_map" (0 or 1, default 0; any other value: DMP_ERR_ARG): score the chosen pass's predicted distance map - the map
 * "emit_distmap" returns - against the native trace of "score_native" on the device: contact precision of the top L, L/2
 * and L/5 predictions in the short, medium and long sequence-separation classes, and the distance error of the map itself,
 * per residue and in total.  Beside "score_native"'s lddt of the MODEL it tells which half of a prediction lost the
 * accuracy: the network that produces the map, or the embedding, coordinate GRU and minimiser that realise it.  Read when a
 * prediction begins and held for it.  IT NEEDS "emit_distmap" = 1 AND "score_native" = 1: a prediction begun with it on and
 * either of them off fails with DMP_ERR_ARG and a message naming the missing option.  With it 0 nothing is launched, read,
 * written or allocated, and every offset and output is bit for bit what it is without the option.  With it 1 THE d_conf
 * ARGUMENT MUST HOLD M0 + 64 + L FLOATS, M0 = THE END OF THE SCORE BLOCK = L + L*L + 3 + 5L + 24: there sits the MAP-SCORE
 * BLOCK, all of it outputs (its inputs are the score block's native trace and lnorm), and A0 and B0 below move behind it.
 * The coordinates, the confidences, the map extension and the score block do not change by a bit.
 * Rows and pairs.  P = the rows whose native x is not NaN, n = |P|; ln = lnorm if lnorm > 0, else n.  Candidates are the
 * pairs i < j, both in P, by their separation s = j - i in alignment columns: class c = 0 (short) 6 <= s <= 11, c = 1
 * (medium) 12 <= s <= 23, c = 2 (long) s >= 24, c = 3 (medium + long) s >= 12; N_c = the candidates of class c.
 * Contacts.  A native contact holds iff (dx*dx + dy*dy) + dz*dz < 64.0f in float32 from the float32 native coordinates,
 * every operation rounded, nothing contracted, no square root.  A predicted contact holds iff dm[i][j] < 8.0f.  The
 * diagonal of dm is never used.
 * Ranked lists.  The candidates of a class are ordered by the key (bit pattern of dm[i][j] as an unsigned 32-bit integer, i,
 * j), ascending: dm is not negative, so this is numeric order, NaN last, ties to the lower (i, j).  For d in {1, 2, 5}:
 * k_d = max(1, floor(ln / d)), t_{c,d} = min(k_d, N_c), h_{c,d} = the native contacts among the first t_{c,d} candidates.
 * Distance agreement.  The pair set and the native distance are those of "score_native"'s lDDT-C-alpha - the ordered pairs
 * i != j of present rows with native distance dn < 15 Angstrom, float64 from the float32 coordinates - and the model's
 * distance is replaced by dm[i][j]: a pair is preserved at 0.5, 1, 2, 4 if |dm - dn| is below it; map_lddt per residue and
 * in total from integer counts, preserved / (4 x partners) (in total 0 without any pair).  Over the same pairs map_mae =
 * mean |dm - dn|, map_rmse = sqrt(mean (dm - dn)^2), map_bias = mean (dm - dn): float64 sums in a fixed order, each output
 * rounded once to float32.  Offsets relative to M0:
 *   0                    n
 *   1                    ln
 *   2 + 12c + 0          N_c                                          (c = 0 .. 3)
 *   2 + 12c + 1          native contacts among the candidates of class c
 *   2 + 12c + 2 .. 4     h_{c,d} for d = 1, 2, 5
 *   2 + 12c + 5 .. 7     t_{c,d} for d = 1, 2, 5
 *   2 + 12c + 8          true positives at the threshold: candidates that are a predicted AND a native contact
 *   2 + 12c + 9          predicted contacts among the candidates
 *   2 + 12c + 10, 11     zero
 *   50                   ordered pairs within 15 Angstrom
 *   51 .. 54             map_lddt, map_mae, map_rmse, map_bias
 *   55 .. 63             zero
 *   [64, 64 + L)         per-residue map_lddt; NaN where the native row is absent, 0 where the residue has no partner
 * Every count is an integer below 2^24 stored as a float.  The precisions h / t, and precision, recall and F1 at the
 * threshold, are formed on the host (NaN where a denominator is 0).  n < 2: the counts are 0, offsets 51 .. 54 NaN, no
 * fault.  A prediction that latched a device-side fault returns NaN in every slot.
 * THE REFERENCE HAS NO SUCH QUANTITY, and nobody has compared these figures with another contact-evaluation program's;
 * the definition above is the only one (tests/test_mapscore_cpu.py restates it in NumPy).
 * Cost with the option on: two launches in dmp_predict_end behind "score_native" (csrc/mapscore.hip).  mapscore_count:
 * rows dealt to at most 64 workgroups; integer counts go thread -> LDS -> one integer atomic per workgroup and counter,
 * the three error sums through the fixed-order float64 grid sum, whose last arriver writes the header.  mapscore_select:
 * one workgroup per (class, list), twelve; a radix select of the t-th smallest of the unique 54-bit keys bits(dm) << 22 |
 * (i L + j) - digit histograms in LDS, the class's pairs re-read once per digit, the pair index's digits only where a list
 * ends inside a run of equal values - then h as the count of native contacts
 * with a key not above it, so ties are no separate path.  No float atomics: the same bits on every run.  A context holds
 * 1.7 KB for this (14 counters, 3 x 64 partial sums, 3 totals, 3 tickets).  Measured cost: 6.6 ms at L = 2048, 0.2 ms at
 * L = 300 (profiles/mapscore.txt).
 * "score_passes" (0 or 1, default 0; any other value: DMP_ERR_ARG): score EVERY recycling pass's C-alpha trace against the
 * native trace of "score_native" on the device, not only the pass the best-of rule kept, and hand out beside the scores the
 * number that rule compared and the convergence measure of "recycle_tol_mA": one full-depth run then tells how many passes
 * were worth running, whether the confidence picked the right one, and what any convergence tolerance would have cost
 * (dmpfold2_amd/score.py: simulate_converge).  Read when a prediction begins and held for it.  IT NEEDS "score_native" = 1:
 * a prediction begun with it on and that option off fails with DMP_ERR_ARG and a message naming the missing option.  With
 * it 0 nothing is launched, read, written or allocated, and every offset and output is bit for bit what it is without the
 * option.  With it 1 THE d_conf ARGUMENT MUST HOLD T0 + 16 + 8R FLOATS, T0 = THE END OF THE MAP-SCORE BLOCK (THE END OF THE
 * SCORE BLOCK WITHOUT "score_map"), R = min(nloops + 1, 128) WITH THE nloops THE PREDICTION WAS BEGUN WITH: there sits the
 * PASS BLOCK, all of it outputs, and A0 and B0 below move behind it.  128 is the number of passes a context records a trace
 * for; later passes run and may be kept, but have no row.  Everything else in the buffer does not change by a bit.
 * Offsets relative to T0:
 *   0                    rows = min(passes run, 128): the rows that hold a pass (fewer than R after a convergence stop)
 *   1                    best_pass: the pass the best-of rule kept (the value "emit_distmap" reports)
 *   2                    tm_pass: the row with the largest tm (float32 comparison, ties to the lowest pass, NaN rows skipped);
 *                        NaN if there is none
 *   3                    lddt_pass: the same for lddt
 *   4                    regret_tm = tm[tm_pass] - tm[best_pass], one float32 subtraction of the stored floats; NaN if
 *                        best_pass >= 128 or either operand is NaN
 *   5                    regret_lddt, likewise
 *   6 .. 15              zero
 *   16 + 8p + 0          conf_mean of pass p: the mean confidence logit the strict '>' of the best-of rule compared
 *   16 + 8p + 1          delta of pass p: d_p exactly as "recycle_tol_mA" defines it (+inf for pass 0), computed whether or
 *                        not that option is on
 *   16 + 8p + 2 .. 6     tm, gdt_ts, gdt_ha, rmsd, lddt of pass p
 *   16 + 8p + 7          zero
 * Rows at and beyond `rows` are NaN in all eight floats.  THERE IS ONE DEFINITION, BY REFERENCE: row p's five scores are
 * exactly what "score_native" returns when the model trace is the one recorded for pass p - the same native, lnorm, seeds,
 * iteration and summation order, evaluated by the same device functions, so where the final trace IS that pass's trace
 * (refine_steps = 0) the row has the bits of the score block - and its delta is exactly what "recycle_tol_mA" records for
 * that pass, evaluated by the same device function.  THE TRACE OF PASS 0 IS THE REFINED ONE WHEN refine_steps > 0 (the trace
 * that seeded pass 1); THE LATER PASSES' TRACES ARE UNREFINED, as the network produced them: with refine_steps > 0 the row
 * of best_pass is therefore not the score block's, which scores the final, refined trace.  A native with fewer than 3
 * present rows gives NaN at offsets 2 .. 6 of every row and 2 .. 5 of the header; conf_mean and delta stay; no fault.  A
 * prediction that latched a device-side fault returns NaN in the whole block.  No per-pass R, t, per-residue arrays or map
 * scores are kept.
 * Cost with the option on: in dmp_predict_end behind "score_map" and in front of "align_structure", on the prediction's
 * stream, nothing synchronises - pass_fill, pass_delta (coords.hip: the delta's sum with the pass as blockIdx.y), then per
 * chunk of passes score_pass_prep, score_lddt and score_search (csrc/score.hip: the kernels of "score_native" with the pass
 * as blockIdx.y; the packed native and the row index are those score_prep made for the score block of the same call; each
 * pass has its own packed model, lDDT totals, seed records and ticket), then pass_header, one workgroup.  No float atomics:
 * the same bits on every run.  Scratch: a slot per pass in flight - score_seeds(L) <= 1 + 5L records of 20 doubles (8262 records,
 * 1.3 MB at L = 2048), the packed trace, the totals - under a budget of DMP_PASSES_BUDGET_MIB (64 MiB): C = clamp(budget / slot,
 * 1, 128) consecutive passes per chunk, 49 at L = 2048, every pass in one chunk up to about L = 790.  Chunk boundaries do not
 * change a bit.  The scratch (the largest chunk of any length up to max_L, plus 66 KB of tickets and partial sums) is
 * allocated when the option first becomes 1 on a context and counted in "device_mib"; an allocation failure is an error of
 * dmp_ctx_set_option and leaves the option as it was.  Measured cost: profiles/passes.txt.
 * "score_passes_chunk" (TESTS ONLY; n >= 0, default 0): at most n passes per chunk when n > 0.
 * THE NATIVE ENTITY of "assign_ss", "exposure" and "domains" below, stated once (csrc/entity.hip).  Each of the three has a
 * leg for the native of "score_native" and each states its own predicate for "the native is whole"; the inputs of those legs
 * are prepared once per prediction, whichever of the three are on.  Front end, with "assign_ss" or "exposure" on: one launch
 * (entity_row, beside the alignment's weights) keeps the L residue codes of the alignment's first row for the end - a proline
 * donates no hydrogen bond ("assign_ss"), a glycine has no CB atom ("exposure").  dmp_predict_end, with "score_native" and any
 * of the three on, in front of "assign_ss": one launch of one workgroup (entity_whole) reads the 3L floats of the native trace
 * and writes two words - whole_x: every row has an x that is no NaN (the predicate of "assign_ss" and "exposure"); whole_xyz:
 * no coordinate is NaN (the predicate of "domains") - and, with "assign_ss" or "exposure" on, one more launch rebuilds the
 * native's backbone from its trace by the very device function that builds the model's (csrc/coords.hip, float32).  A native
 * with a NaN only in some y or z is therefore whole to the first two options and not to "domains".  Scratch: the two words,
 * the first row and the backbone - 61 max_L + 16 bytes, 122 KiB at max_L = 2048 - allocated when the first of the three options
 * becomes 1 on a context, counted in "device_mib", and kept until the context is destroyed.
 * "assign_ss" (0 or 1, default 0; any other value: DMP_ERR_ARG): assign secondary structure to the final backbone that
 * dmp_predict_end has just written into d_coords, from its hydrogen bonds, on the device - helix, strand and coil content
 * and the strand pairing without a native, a partner structure or a second program.  Read when a prediction begins and held
 * for it.  With it 0 nothing is launched, read, written or allocated, and every offset and output is bit for bit what it is
 * without the option.  With it 1 THE d_conf ARGUMENT MUST HOLD U0 + 32 + 8L FLOATS, U0 = THE END OF WHAT "emit_distmap",
 * "score_native", "score_map" AND "score_passes" GIVE (the end of the pass block, T0 + 16 + 8R, with "score_passes"): there
 * sits the SS BLOCK, all of it outputs, and A0 and B0 below move behind it (search_prep's rule for B0 starts from the moved
 * A0).  Everything else in the buffer does not change by a bit.  If "score_native" is on too and every one of the L native
 * rows is present (no NaN x), the native is assigned as well: its trace is rebuilt into a backbone by the very device
 * function that builds the model's from its trace (csrc/coords.hip, float32; the native entity above), the same P_i apply, and the
 * block gains the native's codes and the Q3 / Q8 agreement counts; otherwise has_native = 0.  So a native that is exactly
 * the model's returned C-alpha trace gives ss_native equal to ss, bit for bit.  Counts are integers below 2^24, stored as
 * floats.  Offsets relative to U0:
 *   0                    n_hb: pairs (i, j) with hb(i, j) true (model)
 *   1 .. 8               residues of the model with code 0 .. 7
 *   9, 10                parallel and antiparallel bridge pairs, i < j (model)
 *   11                   has_native (0 or 1)
 *   12, 13               q3_match, q8_match: residues whose three-state / eight-state code equals the native's (0 if
 *                        has_native = 0)
 *   14 .. 21             residues of the native with code 0 .. 7 (0 if has_native = 0)
 *   22 .. 31             zero
 *   [32, 32 + L)         ss: code of model residue i
 *   [32 + L, 32 + 2L)    e_acc[i]: min over the valid j of E(i, j), float64 rounded once to float32; 0 if there is no valid j
 *   [32 + 2L, 32 + 3L)   p_acc[i]: that j, ties to the lower j; -1 if none
 *   [32 + 3L, 32 + 5L)   e_don[j] and p_don[j], likewise over i (the bond residue j's N-H donates)
 *   [32 + 5L, 32 + 7L)   bp1, bp2: the two lowest-numbered bridge partners of i, of either type; -1 where absent
 *   [32 + 7L, 32 + 8L)   ss_native: code of native residue i; NaN in all L if has_native = 0
 * A prediction that latched a device-side fault returns NaN in the whole block.
 * The definition, the only one (Kabsch & Sander, Biopolymers 22, 2577, 1983, restated; tests/test_ss_cpu.py restates it in
 * NumPy).  Arithmetic: float64 formed from the float32 coordinates, contraction off, every operation in the order written.
 * Residue i has atoms N_i, CA_i, C_i, O_i from d_coords; P_i is true if column i of the alignment's first row is proline
 * (code 14); d(a, b) = sqrt((dx dx + dy dy) + dz dz).
 * Amide hydrogen: for i >= 1, v = C_{i-1} - O_{i-1}, vv = (vx vx + vy vy) + vz vz, H_i = N_i + v / sqrt(vv) per component.
 * Residue i is a DONOR iff i >= 1, P_i is false and vv > 0.
 * Energy E(i, j), the C=O of i accepting the N-H of j, is defined for j a donor and |i - j| >= 2: if any of d(O_i, N_j),
 * d(C_i, H_j), d(O_i, H_j), d(C_i, N_j) is below 0.5 then E = -9.9, otherwise E = max(27.888 (((1 / d(O_i, N_j) +
 * 1 / d(C_i, H_j)) - 1 / d(O_i, H_j)) - 1 / d(C_i, N_j)), -9.9).  hb(i, j) = E(i, j) < -0.5, false where E is not defined
 * or an index is outside [0, L).  The valid j of e_acc[i] are those for which E(i, j) is defined; a minimum is taken by
 * strict '<' over rising index.
 * Turns: t_n(i) = hb(i, i + n), n = 3, 4, 5.
 * Helices: Hf(k) iff some i in [1, L - 5] has t_4(i - 1), t_4(i) and i <= k <= i + 3.  Gf: for every i in [1, L - 4] with
 * t_3(i - 1) and t_3(i) and no k in i .. i + 2 having Hf, residues i .. i + 2 get Gf.  If: for every i in [1, L - 6] with
 * t_5(i - 1) and t_5(i) and no k in i .. i + 4 having Hf or Gf, residues i .. i + 4 get If.  All three are functions of hb
 * inside a fixed window.
 * Bridges, defined for 1 <= i, j <= L - 2 with |i - j| >= 3 (false elsewhere): P(i, j) = [hb(i - 1, j) and hb(j, i + 1)] or
 * [hb(j - 1, i) and hb(i, j + 1)]; A(i, j) = [hb(i, j) and hb(j, i)] or [hb(i - 1, j + 1) and hb(j - 1, i + 1)].  Ef(i) iff
 * some j has P(i, j) and (P(i - 1, j - 1) or P(i + 1, j + 1)), or A(i, j) and (A(i - 1, j + 1) or A(i + 1, j - 1)).  Bf(i)
 * iff i has a bridge at all.  The bridge partners of i are the j with P(i, j) or A(i, j).
 * Turn residues: Tf(k) iff some n, i has t_n(i) and i < k < i + n.
 * Bends: for 2 <= k <= L - 3, a = CA_k - CA_{k-2}, b = CA_{k+2} - CA_k, Sf(k) iff a.b < 0.3420201433256687 (sqrt(a.a)
 * sqrt(b.b)), each dot product as (x x + y y) + z z.
 * Code(k) is the first that holds of H = 7 (Hf), E = 6 (Ef), B = 5 (Bf), G = 4 (Gf), I = 3 (If), T = 2 (Tf), S = 1 (Sf),
 * else 0 ('-').  The three-state reduction formed for Q3: 7, 4, 3 -> helix; 6, 5 -> strand; the rest -> coil.
 * THIS IS DSSP'S KIND OF ASSIGNMENT, NOT ITS BITS: there is no two-best-partner rule, no bulges, no sheet labels and no
 * chain breaks, and NOBODY HAS COMPARED THE STRINGS WITH THAT PROGRAM'S.  The backbone is the one the reference's
 * Levitt-style reconstruction places from the C-alpha trace (network.py:141-177), not an experimental one.
 * Cost with the option on: the native entity's launches above (one in the front end; two in dmp_predict_end with the
 * native, shared with "exposure" and "domains") and, in dmp_predict_end behind "score_passes" and in front of
 * "align_structure", on the prediction's stream, three launches (csrc/ss.hip) - ss_prep (hydrogens and donor flags), ss_hbond (one
 * workgroup per residue, entity and side: the energies of a row of acceptor i or a column of donor j by the same device
 * function, the minimum of (E, index) pairs, the row of the bit matrix hb or of its transpose from the waves' ballots),
 * ss_assign (one thread per residue: the helix flags through LDS, the bridges from the set bits of two rows, integer
 * counts thread -> LDS -> one integer atomic per workgroup and counter, the last arriver writes the header).  No float
 * atomics: the same bits on every run.  Scratch, beside the native entity's: both bit matrices of both entities (4 x max_L x
 * 2 ceil(max_L / 64) words, 2 MiB at max_L = 2048), the hydrogens, the donor flags, 21 counters and a ticket - 2.1 MiB at
 * max_L = 2048 - allocated when the option first becomes 1 on a context and counted in "device_mib"; an allocation failure is
 * an error of dmp_ctx_set_option and leaves the option and the count as they were.  Measured cost of dmp_predict_end with the option on (profiles/ss.txt; a collapsed model with 2.6 million hydrogen
 * bonds at L = 2048): 0.11 ms at L = 96, 0.29 ms at 300, 1.29 ms at 1000, 2.78 ms at 2048; with the native's leg 0.14,
 * 0.31, 1.35 and 2.86 ms - above "score_native" alone (1.10 ms at L = 2048) from L = 300 on.
 * "exposure" (0 or 1, default 0; any other value: DMP_ERR_ARG): count the solvent exposure of the final backbone that
 * dmp_predict_end has just written into d_coords, on the device - is the model compact, are its hydrophobic positions buried,
 * does each residue see as many neighbours as a folded chain's would - without a native, a partner structure or a second
 * program.  Three measures: a Shrake-Rupley accessible surface (for every backbone atom the number of exposed sphere
 * points), the half-sphere exposure of every residue (Hamelryck, Proteins 59, 38, 2005, the CB variant) and a CB contact
 * number.  Read when a prediction begins and held for it.  With it 0 nothing is launched, read, written or allocated, and
 * every offset and output is bit for bit what it is without the option.  With it 1 THE d_conf ARGUMENT MUST HOLD X0 + 32 +
 * 16L FLOATS, X0 = THE END OF THE SS BLOCK (U0 + 32 + 8L with "assign_ss", U0 without): there sits the EXPOSURE BLOCK, all
 * of it outputs, and A0 and B0 below move behind it (search_prep's rule for B0 starts from the moved A0).  Everything else
 * in the buffer does not change by a bit.  If "score_native" is on too and every one of the L native rows is present (no NaN
 * x - the condition of "assign_ss"), the native gets the same three measures: its trace is rebuilt into a backbone by the
 * very device function that builds the model's (csrc/coords.hip, float32; the native entity above), and the same glycines apply;
 * otherwise has_native = 0.  So a native that is exactly the model's returned C-alpha trace gives native arrays equal to the
 * model's, bit for bit.  Counts are integers below 2^24, stored as floats.  Offsets relative to X0:
 *   0                    P = 256, the sphere points per atom
 *   1                    atoms present in the model (5L - glycines)
 *   2 .. 6               sum of n over the model's N, CA, C, O, CB atoms
 *   7                    atoms of the model with n = 0
 *   8                    has_native (0 or 1)
 *   9 .. 15              the native's atoms present, five sums, atoms with n = 0 (0 if has_native = 0)
 *   16 .. 31             zero
 *   [32 + aL, 32 + (a + 1)L), a = 0 .. 4   n of atom a (N, CA, C, O, CB) of model residue i; -1 for a glycine's CB
 *   a = 5, 6, 7          hse_up, hse_down, cn10 of model residue i
 *   a = 8 .. 15          the same eight arrays of the native; NaN in all 8L if has_native = 0
 * A prediction that latched a device-side fault returns NaN in the whole block.  AREAS ARE NOT FORMED ON THE DEVICE: the
 * accessible area of an atom is 4 pi R_a^2 n / 256, which the host computes in float64 (dmpfold2_amd/score.py).
 * The definition, the only one (tests/exposure_ref.py restates it in NumPy).  Arithmetic: float64 formed from the float32
 * coordinates, contraction off, every operation in the order written.
 * Atoms: residue i has N, CA, C, O and CB from d_coords, atom index a = 0 .. 4.  G_i is true if column i of the alignment's
 * first row is glycine (code 7): the CB of such a residue is ABSENT from the surface calculation - it neither has points nor
 * blocks any.  The CB POSITION in d_coords exists for every residue and is used by the two pair counts, glycine included.
 * Radii: R_a = the atom's radius plus a 1.4 A probe, with the radii of Kabsch & Sander 1983 (N 1.65, CA 1.87, C 1.76, O 1.40,
 * a side-chain atom 1.80): the double literals 3.05, 3.27, 3.16, 2.80, 3.20.
 * Sphere points: P = 256 unit vectors u_k on a golden-spiral lattice, z = 1 - (2k + 1) / 256, r = sqrt(1 - z z), phi = k pi
 * (3 - sqrt 5), u_k = (r cos phi, r sin phi, z), formed in float64 and ROUNDED ONCE TO FLOAT32.  The 768 floats are the
 * generated header csrc/exposure_points.h (tools/make_exposure_points.py; hexadecimal literals);
 * dmp_debug_fetch("exposure_points") answers them as the device holds them.
 * Point test: point k of atom i is p = c_i + R_i u_k, per component one multiply, then one add.  It is BURIED iff some present
 * atom j != i, from any residue including i's own, has (dx dx + dy dy) + dz dz < R_j R_j with d = p - c_j.  n_i = the points
 * that are not buried, an integer in [0, 256].  A NaN fails the comparison, as everywhere in this library.  The result is
 * defined over ALL atoms: the kernel's neighbour filter (|c_i - c_j| < R_i + R_j + 0.01 for some atom i of the residue) only
 * leaves out atoms that cannot hold a point, with a margin far above the rounding of the test.
 * Half-sphere exposure: v = CB_i - CA_i; for j != i, w = CA_j - CA_i; near iff (w_x w_x + w_y w_y) + w_z w_z < 169.0; up iff
 * near and (v_x w_x + v_y w_y) + v_z w_z > 0; down iff near and not up.  hse_up[i], hse_down[i] = the j that are up / down.
 * Contact number: cn10[i] = #{j != i : |CB_j - CB_i|^2 < 100.0}, d = CB_j - CB_i, the same parenthesisation.
 * THIS IS SHRAKE & RUPLEY'S KIND OF SURFACE ON A MODEL WITH NO SIDE CHAINS: IT IS NOT DSSP'S ACC, no relative accessibility
 * is offered, and NOBODY HAS COMPARED THE FIGURES WITH ANOTHER PROGRAM'S.  The backbone is the one the reference's
 * Levitt-style reconstruction places from the C-alpha trace, not an experimental one.
 * Cost with the option on: the native entity's launches above (one in the front end; two in dmp_predict_end with the native,
 * shared with "assign_ss" and "domains") and, in dmp_predict_end behind "assign_ss" and in front of "align_structure", on the
 * prediction's stream and without synchronising, two launches (csrc/exposure.hip) - exposure_surface (one workgroup of 256
 * threads per residue and entity, thread k owning point k of the residue's five atoms: the threads scan all 5L atoms and
 * compact the candidates into an LDS list of (x, y, z, R^2) doubles with wave ballots and a prefix; the list is walked by
 * every wave in step with early exit, in chunks of at most 1024 entries (32 KiB) with the buried bits carried in registers,
 * so that chunk boundaries do not change a bit; the counts are popcounts of the waves' ballots, the sums go through one
 * integer atomic per workgroup and counter, the last arriver writes the header) and exposure_pairs (one thread per residue:
 * the two half-sphere counts and cn10 over LDS tiles).  No float atomics, no waiting between workgroups: the same bits on
 * every run.  Scratch, beside the native entity's: 14 counters and a ticket - 256 bytes - allocated when the option first
 * becomes 1 on a context and counted in "device_mib"; an allocation failure is an error of dmp_ctx_set_option and leaves the
 * option and the count as they were.  Measured cost of dmp_predict_end with the option on (profiles/exposure.txt; a collapsed model, 98 % of
 * its atoms without an exposed point at L = 2048): 0.27 ms at L = 96, 0.69 ms at 300, 2.13 ms at 1000, 5.18 ms at 2048 -
 * about twice "assign_ss" on the same model (0.11, 0.29, 1.29, 2.78 ms, profiles/ss.txt) and 2.4 times "score_native" in
 * the same run at L = 2048; a folded-like native's leg adds under 0.03 ms, a collapsed native's 0.3 to 2.0 ms.
 * "exposure_chunk" (TESTS ONLY; n >= 0, default 0): at most n list entries per chunk when 0 < n < 1024.
 * "domains" (0 or 1, default 0; any other value: DMP_ERR_ARG) with "domains_tau_milli" (1 .. 1000, default 250),
 * "domains_min_size" (8 .. 1024, default 40) and "domains_min_segment" (1 .. 64, default 10; dmp_predict_begin_units answers
 * DMP_ERR_ARG if it exceeds "domains_min_size" with "domains" on): split the final C-alpha trace into structural domains on
 * the device - how many domains the model has, where their boundaries are, which of them are discontinuous - without a
 * native or a second program.  All four are read when a prediction begins and held for it.  With "domains" 0 nothing is
 * launched, read, written or allocated, and every offset and output is bit for bit what it is without the option.  With it 1
 * THE d_conf ARGUMENT MUST HOLD D0 + 32 + 2L + 256 FLOATS, D0 = THE END OF THE EXPOSURE BLOCK (X0 + 32 + 16L with
 * "exposure", X0 without): there sits the DOMAIN BLOCK, all of it outputs, and A0 and B0 below move behind it.  Everything
 * else in the buffer does not change by a bit.  If "score_native" is on too and every one of the L native rows is present (no
 * NaN coordinate: whole_xyz of the native entity above - NOT the condition of "assign_ss" and "exposure", which look at x
 * alone), the native's trace is parsed the same way as a second leg.  Every value is an integer below 2^24, stored as
 * a float.  Offsets relative to D0:
 *   0                    number of domains of the model (1 .. 16)
 *   1                    contact pairs of the chain
 *   2, 3, 4              tau_milli, min_size, min_segment as the prediction held them
 *   5                    domains of more than one segment
 *   6                    the deepest level a domain lies at: 0 = the chain is whole, v = a domain of level v - 1 was split
 *   7                    1 if a domain of level 4, which is never examined, has n >= 2 min_size residues
 *   8 .. 15              zero
 *   16 .. 31             the same fields of the native's leg; all zero without it
 *   [32, 32 + L)         label_model: the domain of residue i, domains numbered from 0 by their lowest residue
 *   [32 + L, 32 + 2L)    label_native; NaN without the native's leg
 *   32 + 2L + 8d + c     table of the model, row d = 0 .. 15 of 8 floats; rows d >= the number of domains are zero
 *     c = 0 size  1 segments  2 lowest residue  3 contact pairs inside  4 contact pairs to the rest of the chain
 *     c = 5, 6 ext and denominator of the cut that made the domain (0, 0 for an unsplit chain)  7 its level
 *   32 + 2L + 128 + 8d + c   the same table of the native; zero without its leg
 * A prediction that latched a device-side fault returns NaN in the whole block.
 * The definition, the only one (tests/domains_ref.py restates it in NumPy; the library agrees with it in every label and
 * count).  Contacts: residues i and j are in contact iff |i - j| >= 3 and (dx dx + dy dy) + dz dz < 100.0, d = c_i - c_j in
 * float64 formed from the float32 coordinates, contraction off, every operation in the order written; a NaN fails the
 * comparison.  Everything behind that is integer arithmetic.  A domain is the ascending list of its n residues; list
 * positions are virtual indices 0 .. n.  A cut (I, J), 0 <= I < J <= n, (I, J) != (0, n), puts list positions [I, J) into A
 * and the rest into B (I = 0 or J = n: a plain boundary; otherwise B is discontinuous in the list).  int_A, int_B = contact
 * pairs inside A, inside B; ext = pairs between them; each pair once, the domain's own residues only.  A cut is admissible iff
 * J - I >= min_size, n - (J - I) >= min_size, (I = 0 or I >= min_segment), (J = n or n - J >= min_segment) and
 * min(int_A, int_B) > 0.  Its quality is the rational q = ext / (min(int_A, int_B) + ext); the best cut has the smallest q,
 * compared exactly by cross-multiplication in int64 (at L = 2048 every product is below 2^44), ties to the lexicographically
 * smallest (I, J): a strict weak order with a total tie-break, so the order of the reduction cannot change the answer.  A
 * domain with n >= 2 min_size is split at its best admissible cut iff ext * 1000 < tau_milli * (min(int_A, int_B) + ext).
 * Levels: level 0 is the whole chain; every domain of a level is examined independently; the children of split domains form
 * the next level; levels 0 .. 3 are examined, so there are at most 16 domains; children at level 4 are final.
 * THIS IS A CONTACT-DENSITY BISECTION IN THE MANNER OF DOMAK (Siddiqui & Barton 1995) AND HOLM & SANDER (1994), NOT THEIR
 * BITS: no smoothing of short stray segments, no sheet rule, and NO VALIDATION ON REAL DOMAINS - tau = 0.25 comes from
 * synthetic compact traces only (two globules placed side by side have a best q of 0.008 .. 0.165; of 90 single globules of
 * 80 .. 250 residues 85 have one of 0.26 .. 0.54 and stay whole, 5 one of 0.22 .. 0.25 and are split); nobody has compared
 * the parse with a domain benchmark or with another program.  The reference has no such quantity.
 * Cost with the option on: in dmp_predict_end behind "exposure" and in front of "align_structure", on the prediction's stream
 * and without synchronising - the host reads nothing back between the levels - behind the native entity's launch for
 * whole_xyz (with the native; no backbone is rebuilt for this option) 24 launches (csrc/domains.hip): the reset; the L x L contact table as bytes; per level, the slot (at most 2^level domains) as a grid dimension and
 * empty or final slots returning at once, the compaction of each domain's residue list by ballot prefix sums, the rows of its
 * summed-area table in int32 by wave scans, the columns by one thread per column, every admissible (I, J) from five table
 * reads reduced per I and then per domain with the int64 comparison, the children's labels; the contacts inside and outside
 * every domain; the numbering by lowest residue, the labels, the table and the header.  Integer atomics only: the same bits
 * on every run.  Scratch, both legs, beside the native entity's: 2560 + 48 max_L + 2 max_L^2 + 8 (max_L + 16)^2 bytes - the contact tables and
 * the summed-area tables of one level, (n_s + 1)^2 int32 per domain, together at most (max_L + 16)^2 - 0.9 MiB at max_L =
 * 300, 40.6 MiB at max_L = 2048; allocated when the option first becomes 1 on a context and counted in "device_mib"; an
 * allocation failure is an error of dmp_ctx_set_option and leaves the option and the count as they were.  Measured cost of
 * dmp_predict_end with the option on (profiles/domains.txt; the collapsed model of profiles/exposure.txt, which stays whole at the defaults):
 * 0.07 ms at L = 96, 0.07 ms at 300, 0.17 ms at 1000, 0.41 ms at 2048; forced through all four levels (tau_milli 1000,
 * min_size 8, min_segment 2) 0.08, 0.12, 0.39 and 0.83 ms - against 5.15 ms for "exposure" and 17.0 ms for "align_structure"
 * at L = 2048 in the same run; a native's leg adds 0.01 to 0.32 ms.
 * "restrain_milli" (0 .. 100000, default 0 = off; any other value: DMP_ERR_ARG) and "restrain_cut_mA" (0 .. 100000, default
 * 15000): restrain the prediction's FINAL refinement to the predicted distance map.  THE REFERENCE HAS NO SUCH TERM: its
 * minimiser (network.py:106-137) knows steric repulsion and the bond and never sees the map.  Both are read when a prediction
 * begins and held for it; k = (float)restrain_milli / 1000.0f, cut = (float)restrain_cut_mA / 1000.0f (Angstrom).  With
 * "restrain_milli" 0 nothing changes by a bit.  With it > 0 the pass tails keep the chosen pass's map exactly as they do for
 * "emit_distmap" (t_ij below; exactly symmetric), and each of the refine_steps steps that dmp_predict_end applies to the best
 * trace gains a third term.  Float32, every operation in the order written, as the minimiser's own: for residue j and
 * partner i, dx = x_j - x_i (dy, dz likewise), d_raw = sqrtf((dx dx + dy dy) + dz dz); the steric term is the reference's,
 * from clamp(d_raw, 0.01, 10); then, if |i - j| >= 2 and t = t_ij < cut (a NaN fails the test and the pair is skipped),
 *   dr = fmaxf(d_raw, 0.01f), e = fminf(fmaxf(dr - t, -3.0f), 3.0f), a_j -= (k e) (dx / dr)   per component.
 * The partners are summed in the slices and the order of the plain minimiser, the two bond terms, the clamp of the total
 * acceleration to +-100 and the step 0.001 are the reference's.  Nothing else changes: the refinement of pass 0's trace that
 * seeds pass 1, recycling, the best-of choice, "recycle_tol_mA", the recorded ca_pass traces and the layout of d_conf are
 * what they are without the option; the score, SS, align and search blocks see the restrained trace because they read the
 * final coordinates.  refine_steps = 0: nothing runs.  "restrain_cut_mA" = 0: no pair qualifies and the result is the plain
 * refinement's, bit for bit.  No scratch, no allocation; one more read of the map per step (csrc/coords.hip).  Measured
 * cost of dmp_predict_end with refine_steps = 100, option on against off (profiles/restrain.txt): +0.02 ms at L = 96,
 * +0.08 ms at 300, +1.04 ms at 1000, +3.93 ms at 2048.  dmp_debug_fetch("best_dm") answers L x L floats when this option
 * or "emit_distmap" kept the map.
 * "align_structure" (0 or 1, default 0; any other value: DMP_ERR_ARG): align the model with a structure of any length and
 * sequence on the device - a structural alignment found by superposition and dynamic programming in turn.  Read when a
 * prediction begins and held for it.  With it 0 nothing is launched, nothing extra is read or written, and every output is
 * bit for bit what it is without the option.  With it 1 dmp_predict_end launches the alignment behind "score_native", on
 * the final, refined C-alpha trace (d_coords[:, 1], n = L rows); the coordinates, the confidences, the map extension and
 * the score block do not change by a bit.  THE d_conf ARGUMENT MUST THEN HOLD A0 + 25 + 2L + 3m FLOATS, A0 = THE END OF
 * WHAT THE OTHER OPTIONS GIVE (L, + L*L + 3 with "emit_distmap", + 5L + 24 with "score_native", + 64 + L with "score_map",
 * + 16 + 8R with "score_passes", + 32 + 8L with "assign_ss", + 32 + 16L with "exposure", + 32 + 2L + 256 with "domains", + (400 + 2L) K with "search_domains", + 1040 + 4L with "score_domains", + 48 + 20L with "flex", + 128 + 8L (+ L*L) with "msa_report" = 1 (2); the library cannot check the size): there sits the ALIGN BLOCK.  THE CALLER WRITES ITS TWO INPUTS BEFORE THE CALL, as with the score block.
 * Every output lies at an offset that does not depend on m; the variable-length input comes last.  Offsets relative to A0:
 *   0                    in   m, the number of rows of the structure, as a float
 *   1                    out  n_ali: aligned pairs
 *   2                    out  rmsd_ali: Kabsch RMSD over the aligned pairs [Angstrom]
 *   3                    out  tm_model: TM-score normalised by L
 *   4                    out  tm_struct: TM-score normalised by m
 *   5 .. 16              out  R (row-major 3 x 3) and t of the superposition that gave tm_struct: structure ~ R model + t
 *   17, 18               out  d0_model = d0(L), d0_struct = d0(m)
 *   19                   out  seed_offset: the k of the winning seed (may be negative)
 *   20                   out  seeds: how many offsets stage 1 scored
 *   21 .. 24             out  zero
 *   [25, 25 + L)         out  ali[i]: row of the structure aligned with model residue i, or -1
 *   [25 + L, 25 + 2L)    out  deviation of residue i from its partner under R, t [Angstrom]; NaN where ali[i] = -1
 *   [25 + 2L, .. + 3m)   in   the structure's C-alpha trace, (x, y, z) per row, in chain order
 * An m that is not an integer in [3, max_L], or a NaN among the 3m coordinates, gives NaN in every out slot and no fault;
 * with such an m nothing beyond offset 0 is read.  A prediction that latched a device-side fault returns NaN in every out
 * slot; the inputs are left alone.
 * The definition (float64 from the float32 coordinates, contraction off, every sum in a fixed order, each output rounded
 * once to float32).  For a length l, d0(l) = max(1.24 (l - 15)^(1/3) - 1.8, 0.5) for l > 15, else 0.5.  lmin = min(n, m),
 * d0s = d0(lmin), d_cut = min(max(d0s, 4.5), 8).
 * superpose(A, d0, lnorm), for an alignment A = pairs (i, j) in increasing order, is the loop of one seed of "score_native"
 * on the packed pairs: start with S = A and repeat at most 20 times: Kabsch superposition of the model on the structure
 * over S; deviations d of all pairs of A; tm = sum 1 / (1 + (d / d0)^2) / lnorm; keep the best tm with its R, t (strict
 * comparison: the earliest of equals stays); S' = {d < d_cut}; stop if |S'| < 3 or S' = S.
 * Stage 1 scores every gapless threading: minov = max(lmin / 2 (integer division), min(5, lmin)); seed k pairs i with
 * j = i + k for every k whose overlap is at least minov, numbered by rising k (n + m - 2 minov + 1 <= 2 max_L seeds); its
 * score is superpose(A_k, d0s, lmin).tm.  The 16 best seeds go on (by score, ties to the lower number; all, if fewer).
 * Stage 2 refines each of them in at most 10 rounds from A = A_k: (1) (tm, R, t) = superpose(A, d0s, lmin); if tm beats the
 * seed's best so far (strict) record (tm, A); (2) s_ij = 1 / (1 + d_ij^2 / d0s^2), d_ij^2 = |R p_i + t - q_j|^2; (3) the
 * dynamic programme over i = 1..n, j = 1..m, H = 0 and D = 0 on the border: a = H[i-1][j-1] + s_ij,
 * b = H[i-1][j] + (D[i-1][j] ? -0.6 : 0), c = H[i][j-1] + (D[i][j-1] ? -0.6 : 0), H[i][j] = max(a, b, c), the direction diag
 * if a >= max(b, c), else up if b >= c, else left, D[i][j] = (direction is diag); (4) trace back from (n, m) along the
 * directions until i = 0 or j = 0, every diag step aligns (i, j): A'; (5) stop if A' = A or |A'| < 3, else A = A'.  (The
 * tenth round ends after (1): what a further programme gave would never be scored.)  Every candidate of (3) is a single
 * float64 add of two defined values, so H does not depend on the order the cells are evaluated in.
 * The result: the seed with the largest recorded tm, ties to the lower seed number; A* its alignment.  tm_model =
 * superpose(A*, d0(n), n).tm; tm_struct, R, t = superpose(A*, d0(m), m); rmsd_ali = the RMSD of the plain Kabsch
 * superposition over all of A*; ali from A*, the deviations from R, t.
 * THIS IS TM-ALIGN'S KIND OF SEARCH, NOT ITS BITS: one family of initial alignments (the gapless threadings), one gap
 * penalty, 16 refinements.  Any alignment it returns gives a valid lower bound of the best TM-score; nobody has compared
 * the values with that program's.
 * Cost with the option on: three launches in dmp_predict_end (csrc/align.hip: align_prep; align_thread - one workgroup per
 * offset, L + max_L + 1 launched; align_refine - 16 workgroups of 256 threads, the programme as an anti-diagonal wavefront:
 * three rotating diagonals of H and D in LDS, one barrier per diagonal, s_ij formed on the fly, the traceback serial).
 * A context holds, ALLOCATED AT ITS CREATION and counted in "device_mib", 16 (max_L + 1)^2 bytes for the directions (one
 * byte per cell and workgroup; 64 MiB at max_L = 2048), 16 alignments of 2 max_L ints and 2 max_L + 1 seed records.
 * "search_structures" (0, the default, or K = 1 .. DMP_SEARCH_MAX = 4096; any other value: DMP_ERR_ARG): align the model with
 * each of the K structures of a library in the one call, and rank them - fold recognition with the prediction that is
 * already on the device.  Read when a prediction begins and held for it.  With it 0 nothing is launched, read or written, and
 * every output is bit for bit what it is without the option.  THE RESULT FOR ENTRY k IS DEFINED AS EXACTLY WHAT
 * "align_structure" RETURNS FOR THAT STRUCTURE ALONE: the definition above is the only one, and the same device functions
 * evaluate it (csrc/align.hip), so the floats are equal bit for bit.  The coordinates, the confidences and the blocks of the
 * other options do not change by a bit.
 * "search_max_m" (0, the default = the context's max_L, or 3 .. max_L; anything else: DMP_ERR_ARG): the caller's bound on
 * every entry's length.  The library sizes its scratch slots, its launches and the LDS of align_refine from (L,
 * search_max_m) on the host; it never reads a length back from the device, and dmp_predict_end stays asynchronous.
 * "search_chunk" (TESTS ONLY; n >= 0, default 0): at most n entries per chunk when n > 0 (see below).
 * WITH K > 0 THE d_conf ARGUMENT MUST HOLD THE SEARCH BLOCK AT B0 = THE END OF WHAT THE OTHER OPTIONS GIVE: A0 (above)
 * without "align_structure"; with it B0 = A0 + 25 + 2L + 3m', m' = the align block's m if that is an integer in [3, max_L],
 * else 0 (search_prep forms B0 on the device by this rule; a host layer that knows m uses the same).  THE CALLER WRITES ITS
 * TWO INPUTS BEFORE THE CALL.  Every output lies at an offset that depends on K and L only; the variable-length input comes
 * last.  Offsets relative to B0, M = the sum of the m_k:
 *   [0, K)                        in   m_k, the rows of entry k, as floats
 *   [K, 2K)                       out  rank[r]: the index of the entry with the r-th largest tm_model
 *   [2K, 26K)                     out  entry k's header at 2K + 24k: the 24 floats an align block holds at offsets 1 .. 24
 *   [26K, 26K + 2LK)              out  entry k's ali[L] then deviation[L] at 26K + 2Lk, as offsets 25 .. 25 + 2L of an align block
 *   [26K + 2LK, .. + 3M)          in   the entries' C-alpha traces, entry after entry, (x, y, z) per row
 * Ranking: by falling tm_model (the float32 value of the header), ties to the lower index; entries whose tm_model is NaN
 * come last, in index order.  The ranks are floats, exact below 2^24.
 * If any m_k is not an integer in [3, search_max_m], nothing beyond [0, K) is read, every out slot behind the ranks is NaN,
 * rank is 0 .. K-1, and there is no fault.  A NaN among entry k's coordinates makes that entry's 24 + 2L floats NaN and no
 * other's (it is ranked last).  A prediction that latched a device-side fault returns NaN in every out slot, the ranks
 * included (search_rank reads the fault word; the latch kernel does not know B0); the inputs are left alone.
 * Launches with the option on, all on the prediction's stream, behind "align_structure": search_prep (one workgroup: the m_k
 * validated, the prefix sums of the trace offsets, B0, NaN into every out slot), then per CHUNK of C consecutive entries
 * align_prep (1 x c workgroups), align_thread (L + search_max_m + 1 by c) and align_refine (16 by c; c = the chunk's entries,
 * the entry is blockIdx.y), then search_rank (one workgroup: rank by counting, order-free): 2 + 3 ceil(K / C) launches.
 * A SLOT holds one entry's working set, every part rounded up to 16 bytes: 16 (L + 1)(search_max_m + 1) bytes of
 * directions, L + search_max_m + 1 seed records of 8 bytes, 16 candidate alignments of 1 + 2L ints, both traces (12 L and
 * 12 search_max_m bytes) and 272 bytes of header, survivors and their scores.  C = clamp(DMP_SEARCH_BUDGET_MIB (256 MiB) /
 * slot, 1, 256); "search_chunk" lowers it.  Chunk boundaries do not change a bit of any output.  align_refine's dynamic LDS
 * is sized from search_max_m in these launches (24 (L + 1) + max(25 L, 12 search_max_m + 3 (L + 1)) + 12 L bytes: 17.9 KB at
 * L = 300, search_max_m = 500, against 35.5 KB with search_max_m = 2048), so that several workgroups share a CU.
 * THE SCRATCH - the largest chunk over every L <= max_L at this search_max_m, 66 KB of head in front (the table of trace
 * offsets, two tickets per slot, and the two tables of "search_refine" below) - IS
 * ALLOCATED WHEN "search_structures" FIRST BECOMES POSITIVE ON A CONTEXT (again, larger, if "search_max_m" grows later) and
 * counted in "device_mib"; an allocation failure is an error of dmp_ctx_set_option and leaves the option as it was.  Nothing
 * is allocated for a context that never turns the option on.  Read-only, of the last prediction that searched:
 * "search_chunk_used" (C) and "search_wg_per_cu" (resident align_refine workgroups per CU at that shape).
 * "search_refine" (0, the default, or R = 1 .. DMP_SEARCH_MAX; any other value: DMP_ERR_ARG): the search in two stages -
 * every entry SCREENED by stage 1 alone, the R most promising entries REFINED.  Read when a prediction begins and held for
 * it.  With R = 0, or R >= K, the launches are exactly the ones above and every float of the search block is bit for bit
 * what it is without the option.  With 0 < R < K:
 *   A SCREENED ENTRY is the definition with stage 2 left out: A* = A_s, the gapless threading of the best seed s of stage 1
 *   (by score, ties to the lower number), and the result formulae applied to it - tm_model = superpose(A*, d0(n), n).tm;
 *   tm_struct, R, t = superpose(A*, d0(m), m); rmsd_ali, n_ali = |A*|, seed_offset = the k of s, seeds, d0_model, d0_struct,
 *   ali and the deviations as above - and OFFSET 21 OF ITS HEADER IS 1.0: "screened, not refined".  It is a valid alignment,
 *   and its TM-scores are valid lower bounds of the best like every other number of this option (never above the refined
 *   entry's: stage 2 starts from A_s).
 *   THE SELECTION is by the screened tm_model (the float32 value): the R entries that rank first by the rule of the
 *   ranking above - falling value, ties to the lower index, NaN last in index order - are refined.
 *   A REFINED ENTRY is computed again from nothing by the three stages above, so its 24 + 2L floats are, bit for bit, what
 *   "align_structure" gives for that structure alone, and offset 21 of its header is 0.  (Offset 21 stays one of the zero
 *   slots of an align block: "align_structure" never screens.)
 *   The ranking is by the header's tm_model as always: refined and screened entries are ranked together.
 * AN ENTRY WHOSE FOLD ONLY SHOWS ONCE GAPS ARE OPENED CAN BE MISSED: its best gapless threading may screen below R
 * unrelated entries, and it then keeps the screen's numbers.  Nobody has compared the recall with another program's;
 * profiles/search_refine.txt has what was measured on made-up libraries.
 * An entry with a NaN coordinate screens as NaN, is selected last and stays NaN if selected; a bad m_k gives the all-NaN
 * answer above; a latched fault likewise (search_rank writes the NaNs).
 * Launches with 0 < R < K: search_prep; per chunk of C consecutive entries over all K: align_prep, align_thread and
 * align_screen (1 x c workgroups, the dynamic LDS of align_thread: 6 L floats and L flags; it also leaves the entry's
 * screened tm_model, NaN for an entry without a result, in a table); search_select (one workgroup: the R entries by
 * counting, into a second table; the identity if search_prep found a bad m_k); per chunk of C over the R selected entries,
 * taken through that table: align_prep, align_thread, align_refine; search_rank: 3 + 3 ceil(K / C) + 3 ceil(R / C)
 * launches.  Nothing comes back from the device in between: the grids are sized from (L, search_max_m, K, R) on the host
 * and dmp_predict_end stays asynchronous.  The two tables (4 DMP_SEARCH_MAX bytes each) lie in the head of the scratch,
 * behind the tickets; the slots and the budget are the same.  Stage 1 runs twice for the R selected entries: R / K of the
 * screen pass, for one definition of a refined entry.
 * THIS IS TM-ALIGN'S KIND OF SEARCH, a lower bound of the best TM-score per entry, not compared with that program
 * (see "align_structure").  Measured cost: profiles/search.txt, profiles/search_refine.txt.
 * "search_domains" (0, the default, or 1; 2 is FOR TESTS ONLY; any other value: DMP_ERR_ARG): search the library of
 * "search_structures" with EVERY DOMAIN of the model as well - the tm_model of a multi-domain model against a library of
 * single-domain folds is nearly meaningless, and "domains" says when that is so.  Read when a prediction begins and held for
 * it; dmp_predict_begin_units answers DMP_ERR_ARG if it is on without "domains" = 1 or without "search_structures" > 0.
 * With it 0 nothing is launched, read, written or allocated and every offset is what it was.  With it on, THE d_conf ARGUMENT
 * MUST HOLD (400 + 2L) K MORE FLOATS AT THE END OF THE DOMAIN BLOCK (D0 + 32 + 2L + 256): there sits the DOMAIN-SEARCH BLOCK,
 * all of it outputs, its size a matter of (L, K) alone, and A0 and B0 move behind it.  Offsets relative to its start:
 *   [0, 16K)                      rank[d][r] at K d + r: the entry with the r-th largest tm_model of domain d
 *   [16K, 400K)                   pair (d, k)'s header at 16K + 24 (K d + k): the 24 floats of an align block's offsets 1 .. 24
 *   [400K, 400K + 2LK)            entry k's ali[L] then deviation[L] at 400K + 2Lk
 * THE DEFINITION, the only one.  Let D be the model's domain count and label_model its labels, as the domain block of the
 * same call holds them.  The trace of domain d is the C-alpha rows i with label_model[i] == d, in rising i; it has n_d rows.
 * The result of pair (d, k), d < D, is EXACTLY WHAT "align_structure" GIVES FOR A MODEL CONSISTING OF THAT TRACE AND THE
 * STRUCTURE OF ENTRY k: the same 24 header floats with the same meaning - tm_model normalised by n_d, d0_model = d0(n_d),
 * seeds counted from n_d - and its ali and deviation scattered back to the residues of the domain.  The domains partition the
 * chain, so entry k needs one ali[L] and one deviation[L] for all of them: residue i carries the structure's row and the
 * deviation under the alignment and the superposition OF ITS OWN DOMAIN's pair with entry k (-1 and NaN where that alignment
 * leaves it out).  rank[d] follows the rule of search_rank: falling tm_model, ties to the lower index, NaN entries last in
 * index order.  Rows d >= D - ranks and headers - are NaN.  "search_refine" = R, 0 < R < K, applies to every domain
 * separately by the rule above: every entry is screened against domain d, the R entries that screen best for d are refined,
 * the others keep the screen's numbers and 1 at header offset 21; R = 0 or R >= K is the full sweep, bit for bit.
 * If any m_k is invalid, or the prediction latched a device-side fault, every float of the block is NaN (the block lies
 * inside what the fault latch covers).  A NaN among entry k's coordinates makes the headers of its 16 pairs and its 2L
 * floats NaN.  The structure, the domain block, the search block and every other block keep their bits.
 * THE ONE-DOMAIN SHORTCUT: with D = 1 the domain is the chain and the answer is the whole search's by definition; the sweep's
 * workgroups return at once and the last launch copies the search block's ranks, headers, ali and deviation into row 0.
 * Value 2 never takes the shortcut, so that a test can hold the gather path to the whole search bit for bit.
 * THIS IS TM-ALIGN'S KIND OF SEARCH, a lower bound of the best TM-score per pair, not that program's bits, and nobody has
 * compared its recall with another program's (see "align_structure"); the parse it searches with is "domains"', with every
 * caveat stated there.
 * Launches (csrc/align.hip), behind "search_structures" on the same stream and IN ITS SLOTS - the whole-model search has
 * finished with them, and its table of the entries stays: domsearch_prep (one workgroup: NaN into the block; D and the labels
 * read from the domain block and validated; the residue list sorted by (label, index) and its 17 offsets by a counting sort -
 * integers only); then the stages of "search_structures" over the virtual entries p = K d + k, domain-major, in the same
 * chunks of C slots (a chunk may straddle domains): align_prep - its structure half unchanged, its model half gathering the
 * domain's rows through the list, n_d and what follows from it in the slot header -, align_thread, align_refine (with R:
 * align_screen over all, search_select per domain, then the three stages over the R chosen); search_rank (one workgroup
 * per domain); domsearch_finish (one per entry) - the kernels of "search_structures" themselves, instantiated for the
 * domain query instead of the whole chain.  The bodies that compute are the ones "align_structure" runs: they read the
 * model's row count from the slot header, and L only sizes strides, LDS and grids.  A pair's ali and deviation are written
 * compactly at the domain's offset in the sorted list, inside entry k's 2L floats of the block - the slots are reused chunk
 * after chunk, the block is not - and domsearch_finish permutes them into residue order through LDS.  Nothing comes back from
 * the device: the grids are sized for Dmax = max(1, min(16, L / "domains_min_size")) domains - a split never leaves a part
 * below min_size, so D <= Dmax - and the workgroups of d >= D return before they touch a slot; dmp_predict_end stays
 * asynchronous.  Scratch of its own beside the search's: the screen and select tables per domain (2 x 16 x 4 DMP_SEARCH_MAX
 * bytes), 128 bytes of counts and offsets, the list (4 max_L bytes) - 0.5 MiB, allocated when the option first becomes
 * positive on a context and counted in "device_mib".
 * Measured cost (profiles/search_domains.txt; L = 300, made-up libraries): a model that stays whole pays 0.05 to 2.3 ms beside
 * a search of 3 to 116 ms (1 to 5 %: the copy and the launches that return at once); a model split in 2 (150 + 150) pays 0.8
 * to 2.7 times the whole search again, in 3 (78 + 144 + 78, grids for 4) 1.0 to 3.7 times, in 16 (18 .. 27 residues) 2.1 to
 * 9.2 times - a pair of a small domain costs about half a whole-model pair, because align_refine's dynamic programme pays one
 * barrier per anti-diagonal and an entry of m rows has at least m of them whatever n_d is.
 * "score_domains" (0 or 1, default 0; any other value: DMP_ERR_ARG): score EVERY DOMAIN of the model against the native ON ITS
 * OWN SUPERPOSITION - on a multi-domain target the whole-chain TM-score of "score_native" mostly measures how the domains sit
 * relative to each other, and its lDDT hides a wrong arrangement because few inter-domain pairs lie inside 15 Angstrom.  Read
 * when a prediction begins and held for it; dmp_predict_begin_units answers DMP_ERR_ARG if it is on without "domains" = 1 or
 * without "score_native" = 1.  With it 0 nothing is launched, read, written or allocated and every offset is what it was.  With it
 * 1 THE d_conf ARGUMENT MUST HOLD 1040 + 4L MORE FLOATS AT THE END OF THE DOMAIN-SEARCH BLOCK (of the domain block, D0 + 32 + 2L +
 * 256, with "search_domains" off): there sits the DOMAIN-SCORE BLOCK, all of it outputs, and A0 and B0 move behind it; nothing in
 * front of it moves.  Offsets relative to its start:
 *   0                    D of the model's leg
 *   1                    D of the native's leg, 0 without that leg
 *   2                    rows present: residues with a native row
 *   3 .. 15              zero
 *   16 + 32 (16 e + d) + c   row (e, d), leg e = 0, 1, domain d = 0 .. 15, of 32 floats:
 *     c = 0 n   1 .. 23 the 23 floats of the score block's header behind lnorm (n_pairs, rmsd, tm, gdt_ts, gdt_ha, lddt, the five
 *     counts, R, t)   24, 25 preserved and pairs inside the domain   26, 27 outer_preserved, outer_pairs   28 the domain's size
 *     29 .. 31 zero.  Rows d >= D are NaN; all of leg 1 is NaN without the native's leg.
 *   [1040, 1040 + L)     leg 0: per-residue lDDT inside the residue's own domain
 *   [1040 + L, 1040 + 2L)  leg 0: deviation under its own domain's superposition
 *   [1040 + 2L, 1040 + 4L) the same two arrays of leg 1; NaN without that leg
 * THE DEFINITION, the only one.  Leg 0 uses the model's labels (label_model of the domain block of the same call), leg 1 the
 * native's (label_native): it exists only when the domain block has the native's leg, i.e. when every native row is present.
 * For leg e and domain d let P(e, d) be the residues that carry label d in that leg and have a native row (x not NaN), in
 * sequence order.  ROW (e, d) IS EXACTLY WHAT "score_native" RETURNS FOR THE SAME MODEL TRACE AND A NATIVE IN WHICH EVERY ROW
 * OUTSIDE P(e, d) IS NaN, WITH lnorm = 0: n = |P|, TM and GDT normalised by n with d0 from n, the same seeds, the same 20
 * iterations, the same tie rules, an lDDT that counts only pairs inside the domain - the same device functions compute it, so the
 * agreement is in the bits - and the two arrays are that call's lddt_res and deviation on the residues of P, NaN where the native
 * row is absent.  A domain with n < 3 has NaN in floats 2 .. 23 and in the arrays, as that call has; its counts are still given.
 * Two further integer counts per row, which the masked call cannot give: over the ordered pairs (i, j) with i in P(e, d), j
 * present but OUTSIDE the domain and native distance below 15 Angstrom, outer_pairs counts them and outer_preserved the
 * thresholds 0.5, 1, 2 and 4 Angstrom they preserve, with the distance function and the comparisons of the lDDT above.  The
 * host forms from them the inter-domain lDDT, sum of outer_preserved / (4 x sum of outer_pairs) over the domains of a leg - the
 * figure that shows a wrong arrangement - and from floats 24, 25 the lDDT inside the domains.  Every count is below 2^24 at
 * L = 2048 (4 x 2048 x 2047), so the integers are exact as floats.  If D or a label of either leg present is no integer in
 * range (as "search_domains" validates them), or the prediction latched a device-side fault, every float of the block is NaN.
 * THE TM-SCORE PROGRAM'S KIND OF SEARCH PER DOMAIN, A LOWER BOUND, NOT ITS BITS; THE DOMAINS ARE THE CONTACT-DENSITY BISECTION OF
 * "domains", WITH NO VALIDATION ON REAL DOMAINS; NOBODY HAS COMPARED THE FIGURES WITH AN ASSESSOR'S.  There is no one-domain
 * shortcut: a whole chain is scored once more with lnorm = n.
 * Launches (csrc/score.hip), in dmp_predict_end behind "domains", reading the native from the score block, the model from
 * d_coords and the labels from the domain block - nothing that "score_native" left in its scratch: domscore_prep (one workgroup
 * per leg: validation, the leg's part of the block, the present rows packed in (domain, column) order, per domain its header and
 * the prefix sums of the <= 16 row counts and seed counts); domscore_lddt (the body of score_lddt, (row group, domain, leg), the
 * partner loop over every present row with the domain test an index compare; integer atomics only); domscore_search (the body of
 * score_search on a FLAT grid of Dmax + 5L workgroups per leg, Dmax = max(1, min(16, L / "domains_min_size")): score_seeds(n) <= 1
 * + 5n and the domains partition the chain, so a leg never has more seeds; a workgroup finds its (domain, seed) in the prefix
 * sums, each domain has its own ticket and its stretch of the leg's Dmax + 5 max_L records; 6L floats + L flags of LDS);
 * domscore_counts (floats 24 .. 27).  The same bits on every run; dmp_predict_end stays asynchronous.  Scratch of its own: per leg
 * 16 + 5 max_L records of 20 doubles, the packed traces and columns (28 max_L bytes) and 2 KiB of headers, counters and offsets -
 * 0.5 MiB at max_L = 300, 3.2 MiB at 2048 - allocated when the option first becomes 1 on a context and counted in "device_mib";
 * an allocation failure is an error of dmp_ctx_set_option and leaves the option as it was.
 * Measured cost of dmp_predict_end with the option on (profiles/score_domains.txt; the collapsed model of profiles/exposure.txt, a
 * whole folded-like native, both legs): 0.24 ms at L = 96, 0.60 ms at 300, 2.55 ms at 1000, 5.63 ms at 2048 where the model stays
 * one domain - 1.9 to 2.6 times "score_native" alone in the same run - and 0.20, 0.40, 1.71 and 4.46 ms forced through all four
 * levels (1.3 to 2.1 times).
 * "flex" (0 or 1, default 0; any other value: DMP_ERR_ARG) with "flex_cut_mA" (4000 .. 20000, default 7300; anything else:
 * DMP_ERR_ARG): THE SLOW MODES AND THE RESIDUE FLEXIBILITY OF THE MODEL by the Gaussian network model (GNM: Bahar, Atilgan & Erman,
 * Fold. Des. 2, 173, 1997; Haliloglu, Bahar & Erman, Phys. Rev. Lett. 79, 3090, 1997) of its final C-alpha trace - which parts
 * move together, about which hinge, and how floppy each residue is - without a native or a second program.  Both are read when a
 * prediction begins and held for it.  With "flex" 0 nothing is launched, read, written or allocated and every offset is what it
 * was.  With it 1 THE d_conf ARGUMENT MUST HOLD 48 + 20L MORE FLOATS AT THE END OF THE DOMAIN-SCORE BLOCK (of whatever block lies
 * last in front of the align block, with those behind it off): there sits the FLEX BLOCK, all of it outputs, and A0 and B0 move
 * behind it; nothing in front of it moves.  Offsets relative to its start:
 *   0                    L
 *   1                    the cutoff, "flex_cut_mA"
 *   2                    has_native: 1 where the native's leg was computed, else 0
 *   3 .. 15              zero
 *   16 + 16 e + c        the header of leg e (0 the model, 1 the native): c = 0 contacts   1 sigma   2 components   3 used
 *                        4 .. 7 zero   8 + k lambda_k, k = 0 .. 7
 *   48 + 10 L e          degree [L] of leg e
 *   48 + 10 L e + L      msf [L]
 *   48 + 10 L e + 2L + k L   mode k [L], k = 0 .. 7
 * The integers are exact as floats (contacts <= 2.1 million at L = 2048, below 2^24).  Without the native's leg its header is zero
 * and its 10 L floats are NaN.
 * THE DEFINITION, the only one.  c = "flex_cut_mA" / 1000.0 in double.  For a leg's C-alpha trace x (float32, L rows):
 *   contacts    residues i != j are in contact iff d2 < c c, d2 formed in float64 from the float32 coordinates as
 *               (dx*dx + dy*dy) + dz*dz (the expression of "domains"; a NaN coordinate makes no contact).  NO MINIMUM SEQUENCE
 *               SEPARATION: chain neighbours are springs.  `contacts` counts the pairs i < j, degree_i the contacts of i.
 *   Gamma       the Kirchhoff matrix D - A of the contact matrix A and its degrees D; sigma = 2 x the largest degree, an integer
 *               that bounds Gamma's spectrum (Gershgorin).
 *   eigenpairs  the eight lowest (lambda_k, v_k) of Gamma, ascending in lambda, k = 0 .. 7, computed as the eight largest
 *               (mu, v) of M = sigma I - Gamma - whose entries are integers below 4096, exact in float32 - by the float64 solver
 *               of the MDS step (dmp_eigh_top8's factorisation); lambda_k = sigma - mu_k in double, rounded once to float32; v_k
 *               the unit eigenvector under that solver's sign rule - the component of largest magnitude positive, first index on
 *               ties - each component rounded once to float32.
 *   zero modes  mode k is a zero mode iff lambda_k <= 1e-7, absolute.  Gamma has integer entries; the solver's eigenvalue error is
 *               n 2^-53 sigma <= 9.3e-10 at n = 2048; the smallest non-zero eigenvalue of a connected graph is at least
 *               4 / (n diameter) >= 9.5e-7: 1e-7 sits 100 times above the first and about 10 times below the second.
 *               components = the zero modes among the eight (1 for a connected network), used = 8 - components.
 *   msf         msf_i = sum over the non-zero modes k, ascending, of v_k[i]^2 / lambda_k - the slow-mode mean-square fluctuation
 *               in units of kT / spring constant - accumulated in float64 FROM THE FLOAT64 v OF THE BACK-TRANSFORMATION, not
 *               from the float32 modes of the block, and rounded once to float32; 0 where used = 0.
 * The model's leg is always computed, from the CA rows of d_coords: it sees the minimised and, with "restrain_milli", restrained
 * model, as "assign_ss" and "exposure" do.  The native's leg is computed with "score_native" on and a native trace without a
 * NaN coordinate (whole_xyz of the native entity above, as "domains"); a native with a missing row has no leg.  A prediction that
 * latched a device-side fault has NaN in every float of the block.
 * THIS IS THE GNM OF A C-ALPHA TRACE WITH ONE UNIFORM SPRING CONSTANT, NOT ProDy's BITS; SEVEN MODES AT MOST, NOT THE WHOLE
 * SPECTRUM, SO msf IS THE SLOW-MODE FLUCTUATION, NOT THE FULL PSEUDO-INVERSE DIAGONAL; NOBODY HAS COMPARED THE FIGURES WITH
 * EXPERIMENTAL B-FACTORS OR ANOTHER PROGRAM'S; INSIDE A CLUSTER OF EQUAL EIGENVALUES ANY ORTHONORMAL BASIS IS A RIGHT ANSWER, AND
 * msf DEPENDS ON THE BASIS WHERE A CLUSTER STRADDLES THE 8TH / 9TH EIGENVALUE.
 * Launches (csrc/flex.hip), in dmp_predict_end behind "score_domains" and in front of "align_structure", per leg: a memset of the
 * degrees; flex_kirchhoff_kernel (tiles of 16 rows x 256 columns, the rows' coordinates through LDS: the off-diagonal of M and
 * the degrees, one integer atomic per row and tile); flex_sigma_kernel (one workgroup: largest degree, contact total, sigma, the
 * diagonal of M); the solver exactly as a recycling pass runs it (eig_load_kernel, the tridiagonalisation in the context's current
 * form, tri_eig_kernel) with the second epilogue of backtransform_kernel, which writes the modes into the block and their float64
 * sources into the solver's scratch; flex_finish_kernel (eigenvalues, components, used, msf, degrees, the header).  The solver's
 * scratch and graphs are the passes' own - the last pass is behind these launches on the same stream - but M lies in a scratch of
 * the option's: what dmp_debug_fetch hands out as "gram" and "mds" after a prediction is untouched.  With a score block whose trace
 * is not whole the native's launches still run (nothing is read back to decide) and flex_finish_kernel overwrites what they
 * left.  Integer atomics only: the same bits on every run; dmp_predict_end stays asynchronous.  Scratch of its own: max_L^2 + max_L
 * floats (0.34 MiB at max_L = 300, 16 MiB at 2048) beside the native entity's, allocated when the option first becomes 1 on a
 * context and counted in "device_mib"; an allocation failure is an error of dmp_ctx_set_option and leaves the option as it was.
 * Measured cost of dmp_predict_end with the option on (profiles/flex.txt; the collapsed model of profiles/exposure.txt, a whole
 * folded-like native): the model's leg adds 0.45 ms at L = 96, 1.56 ms at 300, 9.4 ms at 1000 and 41.2 ms at 2048, the native's leg
 * 0.45, 1.50, 9.3 and 41.0 ms more; one dmp_eigh_top8 of the same order takes 0.45, 1.53, 9.2 and 41.1 ms in the same run: a leg is
 * 0.98 to 1.01 of it.
 * "msa_report" (0, 1 or 2, default 0; any other value: DMP_ERR_ARG): A REPORT ON THE ALIGNMENT THE PREDICTION RAN ON - how deep it
 * was, how conserved each column is, and what the raw DCA contact map says - the third leg beside "score_native" (the model) and
 * "score_map" (the network's map): did the alignment carry the signal at all?  Read when a prediction begins and held for it.  With
 * it 0 nothing is launched, read, written or allocated and every offset is what it was.  With it 1 THE d_conf ARGUMENT MUST HOLD
 * 128 + 8L MORE FLOATS AT THE END OF THE FLEX BLOCK (of whatever block lies last in front of the align block, with those behind it
 * off), WITH IT 2 128 + 8L + L*L: there sits the REPORT BLOCK at Q0, all of it outputs, and A0 and B0 move behind it; nothing in
 * front of it moves.  It needs no other option; the DCA precisions need "score_native".
 * A "gap" below is a clamped code of 20: UNKNOWN RESIDUES (20, 21) AND GAPS MERGE, exactly as the network and the reweighting see
 * them.  a_nl is the clamped code of row n, column l; cnt[n,m] = #{l : a_nl == a_ml}, the reference's count (predict.py:32-37),
 * GAPS MATCHING GAPS.  Every integer is stored as a float; all are below 2^24 (N L <= 3000 x 2048).  Offsets relative to Q0:
 *   0, 1        N, L
 *   2, 3, 4     neff_62, neff_80, neff_90: neff_t = sum_n 1 / #{m : float(cnt[n,m]) > float32((double)L * t)}, a float64 sum in
 *               a fixed order, rounded once.  neff_80 uses the very expression of the sequence weights, so its neighbour counts
 *               are the weights' own and neff_80 is the sum of the weights.
 *   5           gap cells in the whole alignment
 *   6           rows that are an exact copy of another row (max over m != n of cnt[n,m] == L)
 *   7           gap columns of row 0 (the query)
 *   8 .. 15     zero
 *   16 .. 35    hist_idq[20]: rows by identity to the query, idq_n = #{l : a_nl == a_0l < 20} over #{l : a_0l < 20} - HERE GAPS DO
 *               NOT MATCH - bin = min(19, 20 num / den) in integer division; row 0 included; den == 0: bin 0
 *   36 .. 55    hist_cov[20]: rows by coverage #{l : a_nl < 20} / L, the same binning
 *   56 .. 75    hist_nn[20]: rows by nearest neighbour, max over m != n of cnt[n,m] / L, the same binning; N == 1: all zero
 *   76 + 12c    c = 0 .. 3, the classes of "score_map": N_c | native contacts | h_{c,1}, h_{c,2}, h_{c,5} | t_{c,1}, t_{c,2}, t_{c,5}
 *               | four zeros
 *   124, 125    n (present native rows), ln
 *   126         has_dca: 1 where N > 1 (a single sequence has no covariance features and no contact map)
 *   127         has_native: 1 where "score_native" is on
 *   128 + kL    k = 0 .. 7, per column l:
 *     0  gaps[l]         #{n : a_nl == 20}
 *     1  neff_col[l]     sum_n w_n [a_nl < 20], w the float32 sequence weights, a float64 sum in a fixed order, rounded once
 *     2  entropy[l]      -sum_a p_a ln p_a over the 20 letters, p_a = the weighted frequency among the non-gap rows, float64,
 *                        rounded once; 0 where neff_col is 0
 *     3  cons[l]         the letter with the largest RAW count, ties to the lowest code; NaN in an all-gap column
 *     4  cons_freq[l]    p of that letter (NaN likewise)
 *     5  query_freq[l]   p of the query's letter; NaN where the query has a gap
 *     6  dca_max[l]      the strongest coupling of the column: the entry contacts[l][j], |j - l| >= 6, that comes first in the
 *                        order of the ranked lists below - its bits
 *     7  dca_partner[l]  the lowest j that attains it
 *                        6 and 7 are NaN where has_dca is 0 or no such j exists
 *   128 + 8L    with value 2: contacts[L][L], the DCA contact map the stem was given (channel 441 of fast_dca, network.py:10), bit
 *               for bit; all zeros when N == 1.
 * DCA against the native.  Rows and pairs, the candidates, the classes, the native-contact test, k_d, t_{c,d} and ln are those of
 * "score_map" above, word for word ("Rows and pairs", "Contacts", "Ranked lists"), with the predicted map replaced by the DCA
 * contact map and the order inverted: the candidates of a class are ordered by the key (r(contacts[i][j]), i, j) ascending, r an
 * order-preserving map of the float's bit pattern to an unsigned integer, INVERTED - the strongest coupling first, +0 in front of
 * -0, every NaN last, ties to the lower (i, j) - and h_{c,d} = the native contacts among the first t_{c,d}.  Only contacts[i][j]
 * with i < j is read.  "score_map" and "emit_distmap" are not needed.  Without "score_native", or with N == 1, offsets 76 .. 125
 * are zero and the two flags say why.  The precisions h / t and their enrichment over native contacts / N_c are formed on the host.
 * A prediction that latched a device-side fault has NaN in every float of the block.
 * THE REFERENCE HAS NO SUCH REPORT.  THE IDENTITY COUNTS ARE THE REFERENCE'S, GAPS MATCHING GAPS, EXCEPT idq.  NOBODY HAS COMPARED
 * Neff WITH ANOTHER PROGRAM'S (hhblits, CCMpred and plmDCA count identity over aligned letters and weight differently) OR THE
 * DCA PRECISIONS WITH ANOTHER EVALUATOR'S; the definition above is the only one (tests/msa_report_ref.py restates it in NumPy).
 * Launches (csrc/msareport.hip), all in dmp_predict_end behind "flex" and in front of "align_structure", from what the front end
 * left on the device - the packed clamped alignment, the weights and the contact map are buffers of the context alone that nothing
 * writes between the front end and the end (the passes read the features from the stem's output; a group's vertical-GRU chain and
 * its riders work in buffers of their own): a memset of the counters; the weights' pair kernel once more with a second, compile-
 * time epilogue (msa_count_kernel<true, MsaReportCut>: 64 x 64 row pairs, packed words through LDS; per row the three neighbour counts and the
 * largest count over the other rows, integer atomics) - with the option off the weights' own instantiation and launch are what they
 * were; msareport_row_kernel (one wave per row, histograms in LDS, one integer atomic per bin and workgroup); msareport_col_kernel
 * (one workgroup per column: raw and weighted 21-bin counts, every thread its own float64 LDS column, then a fixed tree);
 * msareport_dca_kernel (one workgroup per row of the map); with a native msareport_pairs_kernel and msareport_classes_kernel (N_c,
 * native contacts, n, ln) and "score_map"'s radix select instantiated with the coupling key (mapscore_select_kernel<MsByCoupling>;
 * "score_map"'s own instantiation is instruction for instruction what it was); msareport_finish_kernel (one workgroup: the Neff
 * sums through the fixed tree, the header); with value 2 one device-to-device copy of the map.  No float atomics: the same bits on
 * every run; dmp_predict_end stays asynchronous.  Scratch of its own: 320 + 16 max_N bytes, allocated when the option first becomes
 * non-zero on a context and counted in "device_mib"; an allocation failure is an error of dmp_ctx_set_option and leaves the option
 * as it was.  Measured cost: profiles/msa_report.txt. */
int dmp_ctx_set_option(dmp_ctx* ctx, const char* name, int value);
/* Current value of an option of dmp_ctx_set_option ("conv_f32_exact" reads as conv_mode == 1). */
int dmp_ctx_get_option(const dmp_ctx* ctx, const char* name, int* h_value);

/* ---- weights (the reference's state_dict ABI, network.py:182-215) ---------------------
 * dmp_weights_set: hand over one tensor of GRUResNet(512,128).state_dict() by key, host
 * float32, contiguous, with its shape (replaces load_state_dict, predict.py:98).
 * dmp_weights_finalize: checks that all 184 tensors arrived and builds the packed device
 * layouts the kernels read (transposed GRU matrices, K-major conv slabs, the cSE gate
 * sigma(W2 relu(W1 beta)) of every block).  A rejected tensor (unknown key, wrong shape) or an
 * incomplete set drops everything staged so far: the next state_dict starts from nothing. */
int dmp_weights_set(dmp_ctx* ctx, const char* key, const float* h_data, const int64_t* shape,
                    int ndim);
int dmp_weights_finalize(dmp_ctx* ctx);
/* Several contexts on one GPU with the same weights (the engines of a throughput scheduler): `dst` uses the packed
 * device buffers of `src` instead of packing its own (0.6 s of host work and 0.5 GB per context at the reference's
 * model size).  The buffers are reference counted: either context may be destroyed or re-loaded first. */
int dmp_weights_share(dmp_ctx* dst, const dmp_ctx* src);

/* ---- host-side text -> residue codes (predict.py:124-128) -----------------------------
 * Translates nbytes alignment characters to codes: ARNDCQEGHILKMFPSTWYV -> 0..19,
 * BJOUXZ -> 20, '-' '.' -> 21, any other byte b -> (b - 65) mod 256.  Pure host code. */
int dmp_msa_encode(const uint8_t* h_text, int64_t nbytes, uint8_t* h_codes);

/* ---- feature builder ----------------------------------------------------------------- */
/* reweight(), predict.py:32-37.  d_msa: N x L codes (uint8, 0..21). d_w: N floats.
 * Integer exact: w[n] = 1 / #{m : #{l : min(a_nl,20)==min(a_ml,20)} > float32(L*0.8)}. */
int dmp_msa_weights(dmp_ctx* ctx, const uint8_t* d_msa, int N, int L, float* d_w, void* stream);
/* fast_dca() first half, predict.py:45-51: cov_reg (21L x 21L). */
int dmp_cov_build(dmp_ctx* ctx, const uint8_t* d_msa, const float* d_w, int N, int L,
                  float* d_cov, void* stream);
/* torch.inverse, predict.py:53: in-place inverse of a symmetric positive definite D x D
 * matrix (blocked Gauss-Jordan, fp32 MFMA trailing updates). */
int dmp_spd_inverse(dmp_ctx* ctx, float* d_A, int D, void* stream);
/* predict.py:58-60: APC-corrected contact channel (L x L) from the inverse covariance.
 * The 441 coupling channels are never materialised: the stem reads d_inv in place. */
int dmp_dca_contacts(dmp_ctx* ctx, const float* d_inv, int L, float* d_contacts, void* stream);

/* reweight() + fast_dca() in one call, with fast_dca's return value laid out as the reference returns it
 * (predict.py:41-61; train.py:175-190 computes the same tensor in its data loader): d_out (L x L x 442),
 * d_out[i][j][21a+b] = inv_cov[21i+a][21j+b], d_out[i][j][441] = APC-corrected contacts.  N = 1 gives zeros
 * (the glue of predict.py:139).  The prediction path itself never builds this tensor (the stem reads the
 * inverse in place); this export is for consumers that want the features themselves.  Uses the context's
 * covariance workspace: not to be interleaved with a prediction on the same context. */
int dmp_dca_features(dmp_ctx* ctx, const uint8_t* d_msa, int N, int L, float* d_out, void* stream);

/* ---- sequence trunk ------------------------------------------------------------------- */
/* embed + vgru, network.py:223-224: 2-layer GRU down the alignment (time = N, batch = L);
 * d_out: L x 512, top-layer state after the last row. */
int dmp_gru_vertical(dmp_ctx* ctx, const uint8_t* d_msa, int N, int L, float* d_out,
                     void* stream);
/* The same for n <= 8 alignments at once (contexts of one GPU holding the same weights, their alignments may
 * differ in N and L): ONE launch per alignment row serves the columns of all members, and the weight
 * fragments a workgroup fetches are shared by its column tiles - the independent targets of a throughput job are
 * the batch axis the reference's GRU call (batch = L, network.py:224) does not have.  Each member's result is
 * bit-identical to dmp_gru_vertical on it alone.  Everything is enqueued on `stream`; ctxs[0] leads (its
 * record buffers are used). */
int dmp_gru_vertical_group(dmp_ctx* const* ctxs, int n, const uint8_t* const* d_msas, const int* Ns,
                           const int* Ls, float* const* d_outs, void* stream);
/* hgru (which = 0; network.py:225, in T x 512) or coord_gru (which = 1; network.py:253,
 * in T x 520): multi-layer bidirectional GRU along the sequence, batch 1.
 * d_out: T x 512 (forward | reverse halves). */
int dmp_gru_bidir(dmp_ctx* ctx, int which, const float* d_in, int T, float* d_out, void* stream);

/* ---- pair trunk ------------------------------------------------------------------------ */
/* network.py:227-229 + the input-independent part of the stem 1x1 convolution
 * (network.py:25-27, 194): Z0[o,i,j] = b_o + sum_c W[o,c] m[c,i] m[c,j]
 *   + sum_ab W[o,512+21a+b] inv[21i+a,21j+b] + W[o,953] contacts[i,j]   (o < 384).
 * d_mat1d: 512 x L.  d_inv / d_contacts may both be NULL (single-sequence MSA: zero
 * features, predict.py:139).  d_z0: 384 x L x L. */
int dmp_stem_static(dmp_ctx* ctx, const float* d_mat1d, const float* d_inv,
                    const float* d_contacts, int L, float* d_z0, void* stream);
/* Rest of the stem for one trunk pass: + W[o,954]*dmap, max over channel triples,
 * InstanceNorm (network.py:28-32).  d_dmap: L x L.  d_x: 128 x L x L. */
int dmp_stem_update(dmp_ctx* ctx, const float* d_z0, const float* d_dmap, int L, float* d_x,
                    void* stream);
/* ResNet block `block` (1..16), network.py:94-103, as its two kernels:
 * conv 5x5 (128->512) + bias + max over channel quadruples -> d_u (128 x L x L) and the
 * per-channel sum / sum of squares (d_stats: 128 x 2 doubles) ... */
int dmp_block_conv5x5_maxout(dmp_ctx* ctx, int block, const float* d_x, int L, float* d_u,
                             double* d_stats, void* stream);
/* ... then InstanceNorm, scSE gates and the residual add: d_out = d_x + y*(cSE + sSE). */
int dmp_block_norm_scse_residual(dmp_ctx* ctx, int block, const float* d_u,
                                 const double* d_stats, const float* d_x, int L, float* d_out,
                                 void* stream);
/* Training-side slice: backward of the first half of ResNet block `block` - Maxout2d's convolution and
 * max (network.py:25-31 with kernel 5), the piece of autograd train.py:318-344 runs through ResNet_Block
 * (network.py:85-103).  d_x: the block's input (128 x L x L), d_du: gradient w.r.t. the maxout output (128 x L x L).
 * Outputs: d_dx (128 x L x L) gradient w.r.t. the input, d_dw (512 x 128 x 5 x 5) and d_db (512) gradients of
 * layer1.lin.weight / .bias (overwritten, not accumulated).  Implicit GEMMs on the float32 matrix cores (round 5: no
 * patch matrix): the forward is run again in float32 for the winner of every quadruple (ties go to the first maximal
 * channel, as torch.max), the routed gradient travels as d_du + one winner byte per maxout channel and pixel and is
 * expanded only in LDS; dgrad = the forward's tile structure with flipped taps, wgrad = a pixel-K GEMM over 8 x 16
 * pixel tiles reduced in fixed order (deterministic).  EVALUATION MODE ONLY: the dropouts of network.py:96-97 are
 * identities here; a training-mode block (Dropout / Dropout2d masks ahead of layer1) is not representable.
 * Workspace: one allocation per context at the first call of either backward entry point, sized for the context's
 * max_L (2.6 activation tensors: padded input, winners, flipped weight pack, wgrad partial sums) - L may change between
 * calls without reallocation.  Uses the context's maxout scratch plane (not to be interleaved with a prediction in
 * flight on the same context). */
int dmp_block_conv5x5_maxout_bwd(dmp_ctx* ctx, int block, const float* d_x, const float* d_du, const uint8_t* d_idx, int L,
                                 float* d_dx, float* d_dw, float* d_db, void* stream);
/* The forward a training step runs for that block: convolution + maxout in float32, d_u (128 x L x L), and what autograd
 * saves for the backward of torch.max (network.py:31) - d_idx (128 x L x L bytes): which channel of each quadruple won,
 * 0..3, the FIRST maximal one.  Handed to dmp_block_conv5x5_maxout_bwd as d_idx it saves the backward its own forward
 * (a third of its matrix-core work); with d_idx = NULL the backward runs the forward again.  (Two implementations of the
 * convolution can resolve a near-tie - two channels within float32 rounding of each other - differently, about one
 * decision in a million; both are valid subgradients.  The parity tests substitute the reference's winners at the
 * near-ties their fixtures list.) */
int dmp_block_conv5x5_maxout_winners(dmp_ctx* ctx, int block, const float* d_x, int L, float* d_u, uint8_t* d_idx,
                                     void* stream);
/* ... and of its second half - InstanceNorm (network.py:32), scSE (network.py:36-83) and the residual add
 * (network.py:99-101).  d_u: the maxout output the forward normalised (128 x L x L; its statistics are recomputed),
 * d_dout: gradient w.r.t. the block's output.  Outputs: d_du (128 x L x L) = gradient w.r.t. the maxout output (the
 * d_du argument of the entry point above) and d_dparams (2433 floats, overwritten): layer1.norm.weight 128,
 * layer1.norm.bias 128, scSE.cSE.fc.0.weight 8 x 128, scSE.cSE.fc.2.weight 128 x 8, scSE.sSE.conv.weight 128,
 * scSE.sSE.conv.bias 1.  The residual branch is the identity: the gradient w.r.t. the block's input is d_dx of the
 * first half plus d_dout (the caller's add).  Evaluation-mode block (the dropouts of network.py:96-97 are identities). */
int dmp_block_norm_scse_residual_bwd(dmp_ctx* ctx, int block, const float* d_u, const float* d_dout, int L,
                                     float* d_du, float* d_dparams, void* stream);
/* ... and of the 1x1 head convolution (network.py:207, Conv2d(128 -> 2)): d_x its input (128 x L x L), d_g the gradient
 * w.r.t. its two output planes (2 x L x L).  Outputs: d_dx (128 x L x L) and d_dparams (258 floats: weight 2 x 128,
 * bias 2).  With the two entry points above a caller chains the sixteen blocks and the head of net.resnet
 * (tests/test_gpu_train.py). */
int dmp_head_conv_bwd(dmp_ctx* ctx, const float* d_x, const float* d_g, int L, float* d_dx, float* d_dparams, void* stream);
/* ... and of the stem, resnet[0] = Maxout2d(955 -> 128, pool 3, kernel 1) + InstanceNorm (network.py:194, 12-34).  Its
 * 955-channel input is never materialised: channels 0..511 are the outer product of d_mat1d (512 x L, network.py:226-227),
 * 512..953 the covariance planes the context holds after dmp_stem_static for this target, 954 the distance channel.
 * dmp_stem_maxout_winners: from d_z0 (dmp_stem_static) and d_dmap the maxout output d_u (128 x L x L, before the
 * InstanceNorm) and the winner of every triple, d_idx (128 x L x L bytes, 0..2).  dmp_stem_bwd: d_dy = gradient w.r.t. the
 * stem's output; outputs d_dw (384 x 955 = resnet.0.lin.weight.grad), d_dparams (640 floats: lin.bias.grad 384,
 * norm.weight.grad 128, norm.bias.grad 128) and d_dmat1d (512 x L: what flows on into the sequence trunk).  The context
 * remembers what its last dmp_stem_static (or prediction) left in the planes: dmp_stem_bwd returns DMP_ERR_ARG, with nothing
 * enqueued, when that target's length was not L (or none ran yet), and after a dmp_stem_static without features (d_inv =
 * d_contacts = NULL) columns 512 .. 953 of d_dw are exactly 0 - the planes are not read.  With these and
 * the block / head entry points above a caller runs autograd's backward through the whole of net.resnet
 * (tests/test_gpu_train.py). */
int dmp_stem_maxout_winners(dmp_ctx* ctx, const float* d_z0, const float* d_dmap, int L, float* d_u, uint8_t* d_idx, void* stream);
int dmp_stem_bwd(dmp_ctx* ctx, const float* d_u, const uint8_t* d_idx, const float* d_dy, const float* d_mat1d,
                 const float* d_dmap, int L, float* d_dw, float* d_dparams, float* d_dmat1d, void* stream);
/* Head 1x1 conv (network.py:207) + network.py:237-246: d_conf (L) = row means of channel 1,
 * d_M (L x L) = Gram matrix 0.5*(dm_0j^2 + dm_i0^2 - dm_ij^2) of dm = |sym(channel 0)|. */
int dmp_head_gram(dmp_ctx* ctx, const float* d_x, int L, float* d_conf, float* d_M,
                  void* stream);
/* One whole trunk pass on internal buffers: stem_update + 16 blocks + head_gram. */
int dmp_trunk_pass(dmp_ctx* ctx, const float* d_z0, const float* d_dmap, int L, float* d_conf,
                   float* d_M, void* stream);

/* ---- coordinates ----------------------------------------------------------------------- */
/* torch.symeig + scaling, network.py:247-250: the 8 algebraically largest eigenpairs of the
 * symmetric d_M (upper triangle used), eigenvalues clamped to >= 1e-8, d_mds (L x 8) =
 * V*sqrt(lambda) in ascending order.  Solved on the device in float64.  Sign rule: each
 * eigenvector's largest-magnitude component is positive. */
int dmp_eigh_top8(dmp_ctx* ctx, const float* d_M, int L, float* d_mds, void* stream);
/* network.py:251-255: coord_gru on [mat1d^T | mds] then coord_fc -> d_ca (L x 3). */
int dmp_coords_from_mds(dmp_ctx* ctx, const float* d_mat1d, const float* d_mds, int L,
                        float* d_ca, void* stream);
/* network.py:272: d_dmap[i,j] = sqrt(max(|ca_i - ca_j|^2, 1e-8)); clamp = 0 gives the
 * template form of predict.py:143 (no clamp, zero diagonal). */
int dmp_pair_distances(dmp_ctx* ctx, const float* d_ca, int L, int clamp, float* d_dmap,
                       void* stream);
/* refine_coords(), network.py:106-137, all steps in one launch; in place on d_ca (L x 3). */
int dmp_refine_coords(dmp_ctx* ctx, float* d_ca, int L, int steps, void* stream);
/* calpha_to_main_chain() + sigmoid, network.py:141-177, 311-312.
 * d_coords: L x 5 x 3 (N, CA, C, O, CB); d_conf_out: L. */
int dmp_ca_to_backbone(dmp_ctx* ctx, const float* d_ca, const float* d_conf_logit, int L,
                       float* d_coords, float* d_conf_out, void* stream);

/* ---- the whole path -------------------------------------------------------------------- */
/* GRUResNet.forward + the feature glue of aln_to_coords (predict.py:134-153,
 * network.py:218-314).  d_msa: N x L codes (N already capped).  d_template_ca: Lt x 3 or NULL
 * (seed distance channel = -1).  nloops = recycling iterations, refine_steps = minimiser
 * steps.  Outputs d_coords (L x 5 x 3) and d_conf (L).  No host synchronisation - unless option "recycle_tol_mA" is
 * set: the call then waits for the tail of every pass p >= 1 that has a successor (one event synchronisation per pass)
 * to learn whether to go on, and returns with the remaining work enqueued as always.
 * WITH OPTION "emit_distmap" = 1 d_conf MUST HOLD L + L*L + 3 FLOATS (layout: dmp_ctx_set_option).
 * WITH OPTION "score_native" = 1 d_conf MUST HOLD 5L + 24 FLOATS MORE, THE NATIVE TRACE AND lnorm WRITTEN INTO THEM
 * (layout: dmp_ctx_set_option); WITH OPTION "score_map" = 1 64 + L MORE BEHIND THOSE (all outputs);
 * WITH OPTION "assign_ss" = 1 32 + 8L MORE BEHIND THOSE AND THE PASS BLOCK (all outputs);
 * WITH OPTION "align_structure" = 1 25 + 2L + 3m MORE BEHIND THOSE, m AND THE STRUCTURE'S
 * TRACE WRITTEN INTO THEM; WITH OPTION "search_structures" = K THE SEARCH BLOCK (26K + 2LK + 3M FLOATS) BEHIND ALL OF THEM. */
int dmp_predict(dmp_ctx* ctx, const uint8_t* d_msa, int N, int L, const float* d_template_ca,
                int Lt, int nloops, int refine_steps, float* d_coords, float* d_conf,
                void* stream);

/* The same prediction issued unit by unit, so that one host thread can interleave several contexts (different
 * streams).  dmp_predict_begin_units validates and records the arguments without enqueueing anything; the
 * prediction is then a sequence of units handed out by dmp_predict_issue_unit: first the front end in chunks of about 2 ms of GPU work
 * (sequence weights + covariance; the inverse, 6 block steps at a time, then contacts; the
 * vertical GRU, 128 alignment rows at a time; sequence GRU + static stem), then 18 units per pass:
 * unit 0 = recycled distance map + stem update, units 1..16 = residual block k (its conv5x5 takes
 * the lane), unit 17 = head + Gram matrix + MDS + coordinate GRU + best-of update.
 * dmp_predict = begin_units + every unit + dmp_predict_end.  dmp_predict_next_unit tells what the next dmp_predict_issue_unit would
 * enqueue; dmp_ctx_pending returns how many issued units have not completed on the GPU (0, 1, or 2
 * for "two or more"; negative on error), so a scheduler can hand the lane only to contexts whose
 * next convolution can start at once and keep its own issue loop from running far ahead. */
#define DMP_UNIT_NONE 0   /* every pass of this prediction was issued: call dmp_predict_end */
#define DMP_UNIT_LIGHT 1  /* no convolution in the unit */
#define DMP_UNIT_CONV 2   /* residual block: one lane turn */
#define DMP_UNIT_WAIT 3   /* nothing to issue now: the unit waits for another context's units (dmp_predict_group_vgru), or -
                             with option "recycle_tol_mA" - for this prediction's own pass tail: at the boundary in front of
                             every pass >= 2 dmp_predict_next_unit queries that unit's event (it never blocks) and answers
                             WAIT until it has completed, then DMP_UNIT_NONE (converged) or the next unit.  A caller that
                             issues without asking (dmp_predict_issue_unit at such a boundary) is made to wait there, and
                             on a stop the call enqueues nothing and returns DMP_OK. */
int dmp_predict_begin_units(dmp_ctx* ctx, const uint8_t* d_msa, int N, int L,
                            const float* d_template_ca, int Lt, int nloops, int refine_steps);
int dmp_predict_next_unit(const dmp_ctx* ctx);
/* Vertical GRUs of n <= 8 predictions as ONE launch chain (dmp_gru_vertical_group inside the unit machinery): call
 * right after dmp_predict_begin_units on every member, before any of their units is issued.  ctxs[0] leads: its
 * vertical-GRU units serve all members on the stream its units are issued on (which must be ordered behind the
 * producers of every member's alignment), the other members have no vertical-GRU units; their last front-end unit
 * waits (event) for the leader's last vertical-GRU unit, and dmp_predict_next_unit answers DMP_UNIT_WAIT for it
 * until that unit has been issued.  Results are bit-identical to ungrouped predictions.  The members must hold
 * the same weights; the leader cannot begin another prediction before every member has issued that unit. */
int dmp_predict_group_vgru(dmp_ctx* const* ctxs, int n);
/* Riders: the vertical GRUs of n alignments that are NOT being predicted yet (the scheduler's next targets) are
 * computed in the same launch chain as the group led by `lead` (members + riders <= 8; the chain's fixed cost per
 * alignment row - launch boundary, cold L2s - is shared by twice as many columns), their results (L_i x 512 each)
 * written to d_outs[i].  Call once, right after dmp_predict_group_vgru (a group of one is allowed), before the
 * leader issues a unit.  The leader's read-only option "chain_issued" answers
 * 1 once the chain has been enqueued to its end on the stream of the leader's units: an event recorded on that
 * stream from then on is behind the riders' results, which go to their predictions through
 * dmp_predict_set_vgru_result.  Every result is bit-identical to the alignment's own chain. */
int dmp_predict_group_riders(dmp_ctx* lead, int n, const uint8_t* const* d_msas, const int* Ns, const int* Ls,
                             float* const* d_outs);
/* The vertical GRU of this prediction has been (or is being) computed ahead of time by dmp_gru_vertical /
 * dmp_gru_vertical_group on the same alignment: d_vout (L x 512, device) is its result, `event` (hipEvent_t or
 * NULL) was recorded behind it.  Call right after dmp_predict_begin_units, before any unit is issued: the
 * prediction then has no vertical-GRU units and its last front-end unit waits for the event and reads d_vout -
 * a scheduler can run the launch chains of the NEXT targets beside the trunk passes of the current ones (the
 * chain touches none of the buffers the trunk uses).  d_vout must stay valid until that unit has run. */
int dmp_predict_set_vgru_result(dmp_ctx* ctx, const float* d_vout, void* event);
/* After the last unit: final refinement of the best trace + backbone + confidences into d_coords (L x 5 x 3) and
 * d_conf (L); a prediction during which a device-side fault was recorded returns NaN.
 * IF THE PREDICTION BEGAN WITH OPTION "emit_distmap" = 1 d_conf MUST HOLD L + L*L + 3 FLOATS (layout: dmp_ctx_set_option).
 * IF IT BEGAN WITH OPTION "score_native" = 1 d_conf MUST HOLD 5L + 24 FLOATS MORE; the native trace and lnorm are read
 * from them here; WITH OPTION "score_map" = 1 64 + L MORE BEHIND THOSE;
 * WITH OPTION "assign_ss" = 1 32 + 8L MORE BEHIND THOSE AND THE PASS BLOCK (the secondary structure is assigned here);
 * WITH OPTION "align_structure" = 1 25 + 2L + 3m MORE BEHIND THOSE, m and the structure's trace read here;
 * WITH OPTION "search_structures" = K the search block behind all of them, the m_k and the traces read here. */
int dmp_predict_end(dmp_ctx* ctx, float* d_coords, float* d_conf, void* stream);
int dmp_predict_issue_unit(dmp_ctx* ctx, void* stream);
int dmp_ctx_pending(dmp_ctx* ctx);

/* Throughput mode: contexts of ONE process that run on different streams may share a lane.  The
 * machine-filling conv5x5 launches of all contexts on a lane then take turns (cross-stream events),
 * two in flight at a time (a launch waits for the one before the previous one, so the tail of one
 * launch fills with the head of the next), while every other kernel of one target overlaps the
 * convolutions of another.  dmp_ctx_share_lane(ctx, other): ctx joins the lane of `other` (made on first use; it
 * lives as long as a context refers to it); other = NULL detaches.  All contexts of a lane must be driven by the same
 * host thread. */
int dmp_ctx_share_lane(dmp_ctx* ctx, dmp_ctx* other);

/* ---- throughput mode behind the C ABI (ABI 5, round 6) ------------------------------------------------------------
 * The batch form of the reference's one call per alignment (predict.py:74-158): N independent alignments through one
 * GPU.  A pipeline owns `engines` contexts (1..8; 4 is the measured optimum on one MI355X), each on a HIP stream of its
 * own, sharing one lane, and ONE host thread inside the library that schedules all of them unit by unit
 * (csrc/pipeline.hip: the units above, the lane, group start of the vertical GRUs, riders, tail stagger - nothing of
 * the issue loop runs in the caller's language).  Use:
 *   dmp_pipeline_create(device, max_L, max_N, 4, &p);
 *   dmp_weights_set(dmp_pipeline_ctx(p, 0), ...) x 184; dmp_weights_finalize(dmp_pipeline_ctx(p, 0));
 *   dmp_pipeline_weights_ready(p);                       (the other engines share that ONE packed copy)
 *   dmp_pipeline_set_option(p, "precision", 2);          (any option of dmp_ctx_set_option, on every engine; idle pipeline only)
 *   t = dmp_pipeline_submit(p, d_msa, N, L, d_template_ca | NULL, iterations, minsteps, d_coords, d_conf, ready_event | NULL);
 *   ... dmp_pipeline_poll(p, tickets, cap, &n) / dmp_pipeline_wait(p, 2) ... dmp_pipeline_status(p, t, &state, &fault_bits);
 *   dmp_pipeline_release(p, t);  dmp_pipeline_destroy(p);
 * Ownership: every buffer is the caller's (device memory; d_coords L x 5 x 3, d_conf L) and must stay valid until the
 * ticket is DMP_TICKET_DONE or DMP_TICKET_FAILED.  `ready_event` (hipEvent_t or NULL): recorded by the caller behind
 * whatever produces d_msa / d_template_ca; the engine that takes the target orders its stream behind it.  submit returns
 * the ticket (>= 0) or a negative dmp_status; it never blocks on the GPU and may be called from any thread.
 * dmp_pipeline_wait(p, what): block until every submitted target has 0 = been started on an engine, 1 = been issued to
 * its end (the engines' streams then hold all the work: dmp_pipeline_stream(p, i) can be waited for on another stream),
 * 2 = completed on the GPU.  dmp_pipeline_poll: tickets that completed (or failed) since the last call, each once.
 * dmp_pipeline_status: *h_state = DMP_TICKET_*; for a DONE ticket *h_fault_bits = the DMP_FAULT_* bits recorded during
 * THAT prediction (non-zero: its outputs are NaN; the caller repeats it, e.g. alone through dmp_predict with
 * "vgru_persistent" 0 or "conv_mode" 2 as the bit suggests); a FAILED ticket (a HIP / capacity error while it was being
 * issued) returns that error.  dmp_pipeline_release forgets a finished ticket (its event and fault word are reused).
 * Scheduler knobs are read from the environment at creation (DMP_VGRU_GROUP, DMP_VGRU_RIDERS, DMP_GROUP_PATIENCE,
 * DMP_TAIL_STAGGER: DESIGN.md section 6); results are bit-identical to dmp_predict on a lone context with
 * "tridiag_cluster" = 0, whatever the grouping. */
typedef struct dmp_pipeline dmp_pipeline;
#define DMP_TICKET_QUEUED 0
#define DMP_TICKET_RUNNING 1
#define DMP_TICKET_ISSUED 2
#define DMP_TICKET_DONE 3
#define DMP_TICKET_FAILED 4
int dmp_pipeline_create(int device, int max_L, int max_N, int engines, dmp_pipeline** out);
/* the same on `engines` streams of the caller's (hipStream_t[engines], non-blocking streams, used by nothing else while the
 * pipeline lives; not destroyed with it) - a host whose memory allocator tracks streams (PyTorch) passes its own */
int dmp_pipeline_create_on(int device, int max_L, int max_N, int engines, void* const* streams, dmp_pipeline** out);
void dmp_pipeline_destroy(dmp_pipeline* p);
int dmp_pipeline_engines(const dmp_pipeline* p);
dmp_ctx* dmp_pipeline_ctx(dmp_pipeline* p, int i);
void* dmp_pipeline_stream(dmp_pipeline* p, int i);
int dmp_pipeline_weights_ready(dmp_pipeline* p);
int dmp_pipeline_set_option(dmp_pipeline* p, const char* name, int value);
/* d_coords: L x 5 x 3 floats, d_conf: L floats.  WITH OPTION "emit_distmap" = 1 ON THE PIPELINE d_conf MUST HOLD
 * L + L*L + 3 FLOATS (layout: dmp_ctx_set_option); its tail then carries this ticket's own best_pass and passes_run.
 * WITH OPTION "score_native" = 1 ON THE PIPELINE d_conf MUST HOLD 5L + 24 FLOATS MORE, THE NATIVE TRACE AND lnorm WRITTEN
 * INTO THEM BEFORE ready_event; WITH OPTION "score_map" = 1 64 + L MORE BEHIND THOSE (all outputs);
 * WITH OPTION "assign_ss" = 1 32 + 8L MORE BEHIND THOSE AND THE PASS BLOCK (all outputs);
 * WITH OPTION "align_structure" = 1 25 + 2L + 3m MORE BEHIND THOSE, LIKEWISE;
 * WITH OPTION "search_structures" = K THE SEARCH BLOCK BEHIND ALL OF THEM, LIKEWISE. */
int64_t dmp_pipeline_submit(dmp_pipeline* p, const uint8_t* d_msa, int N, int L, const float* d_template_ca, int nloops,
                            int refine_steps, float* d_coords, float* d_conf, void* ready_event);
int dmp_pipeline_wait(dmp_pipeline* p, int what);
int dmp_pipeline_poll(dmp_pipeline* p, int64_t* h_tickets, int capacity, int* h_n);
int dmp_pipeline_status(dmp_pipeline* p, int64_t ticket, int* h_state, int* h_fault_bits);
int dmp_pipeline_release(dmp_pipeline* p, int64_t ticket);
int dmp_pipeline_backlog(dmp_pipeline* p, int* h_queued, int* h_running);
/* dmp_pipeline_pause(p, 1): no NEW target is started until (p, 0) - a caller that submits a batch in a loop pauses around
 * it so that the first vertical-GRU group is formed from the whole batch and not from whatever had arrived when the
 * scheduler looked (results do not depend on it, the first chain's width does). */
int dmp_pipeline_pause(dmp_pipeline* p, int on);
/* counters since creation: [0] vertical-GRU groups formed, [1] largest group, [2] chains that carried riders, [3] most
 * riders in one chain, [4] rider results not yet consumed (0 on an idle pipeline), [5] scheduling rounds that found nothing
 * to issue, [6] scheduling rounds, [7] CPU microseconds of the scheduler thread; with option "recycle_tol_mA" in mind:
 * [8] trunk passes issued (of the predictions issued to their end), [9] predictions that stopped before their nloops,
 * [10] passes saved that way.  Entries beyond `capacity` are not written (a caller built for 8 counters keeps working). */
int dmp_pipeline_stats(dmp_pipeline* p, long long* h_stats, int capacity);

/* Synchronise `stream` and report the device-side faults recorded since the last report
 * (DMP_FAULT_* bits in *h_bits; 0 = every result handed out since then is valid).  Reporting clears
 * them: one failed prediction does not poison the checks of later ones. */
int dmp_sync_faults(dmp_ctx* ctx, void* stream, int* h_bits);

/* ---- introspection for tests and the benchmark ------------------------------------------- */
/* After dmp_predict: copy an internal tensor to d_dst (device).  Names: "w", "contacts",
 * "mat1d", "conf_means" (P floats), "ca_pass" (P x L x 3), "best_ca" (L x 3, before the final
 * refinement), "inv_cov" (21L x 21L), "mds" (L x 8) and "gram" (L x L) of the last pass, "pass_delta" (P floats: d_p of
 * option "recycle_tol_mA", +inf for pass 0; nothing - 0 floats - if the prediction ran with the option off), "best_dm" (L x L: the
 * chosen pass's distance map of option "emit_distmap" or "restrain_milli"; 0 floats if the prediction ran with both off) and "best_pass"
 * (1 float: the pass the best-of rule kept; always available).  Returns the number of floats written or a negative status. */
int64_t dmp_debug_fetch(dmp_ctx* ctx, const char* name, float* d_dst, int64_t capacity,
                        void* stream);
/* Optional HIP-event timing of every conv5x5 launch inside dmp_predict / dmp_trunk_pass / the unit calls (events
 * are recorded on the caller's stream around each launch; up to max_launches).  dmp_profile_enable(ctx, 1, n) starts a
 * fresh record, (ctx, 0, 0) stops recording.  dmp_profile_conv_intervals: start / end of every recorded launch of ctx
 * in ms after the first recorded launch of ref (streams synchronised by the caller); the record is kept. */
int dmp_profile_enable(dmp_ctx* ctx, int on, int max_launches);
int dmp_profile_conv_intervals(dmp_ctx* ctx, dmp_ctx* ref, float* h_start_ms, float* h_end_ms, int capacity,
                               int* h_launches);

#ifdef __cplusplus
}
#endif
#endif /* DMPFOLD_HIP_H */
