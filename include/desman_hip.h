/*
 * desman_hip.h -- C ABI of libdesman_hip.so, the MI355X (gfx950) implementation
 * of DESMAN's haplotype-inference hot path.
 *
 * Two layers:
 *
 *  (1) LEGACY SHIM -- the four entry points the reference's Cython module
 *      `sampletau` binds (sampletau/sampletau.pyx:13-19), with identical
 *      argument meaning: borrowed host pointers, tau mutated in place, one
 *      process-global MT19937 stream.  Differences: explicit int64_t, and
 *      errors come back as negative return codes instead of exit(1)
 *      (c_sample_tau.c:200-203).
 *
 *  (2) CONTEXT API -- the device-resident fast path.  One `dsm_ctx` owns the
 *      count tensor, the chain state (tau, gamma, eta) and all traces in HBM;
 *      the host never touches V-sized arrays per iteration.  It covers the
 *      Python-level hot loops of the reference as well
 *      (desman/HaploSNP_Sampler.py:263-365,431-461; desman/Init_NMFT.py:98-205).
 *
 * Plain pointers and sizes only; no torch / numpy types.  All functions return
 * DSM_OK (0) or a negative DSM_ERR_* code; dsm_last_error() gives the message.
 * All arrays are C-contiguous.  Layouts follow the reference:
 *   tau      [V][G][4] int64 one-hot          (HaploSNP_Sampler.py:68)
 *   gamma/pi [S][G]    f64                    (HaploSNP_Sampler.py:63)
 *   eta      [4][4]    f64, rows = true base, cols = observed base
 *   variants [V][S][4] int64 counts           (HaploSNP_Sampler.py:52)
 */
#ifndef DESMAN_HIP_H
#define DESMAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_OK               0
#define DSM_ERR_HIP         -1   /* a HIP runtime call failed                 */
#define DSM_ERR_ARG         -2   /* bad argument / shape                      */
#define DSM_ERR_STATE       -3   /* call order (no counts / no state / no RNG)*/
#define DSM_ERR_UNSUPPORTED -4   /* size outside the compiled kernel range    */
#define DSM_ERR_NOMEM       -5
#define DSM_ERR_NODEVICE    -6   /* no gfx950 device visible                  */
#define DSM_ERR_COMM        -7   /* an RCCL call failed (dsm_comm_*)           */

#define DSM_MAX_G  32            /* haplotypes: tau is packed 2 bits each     */
#define DSM_MAX_S  512           /* samples per variant row                   */

/* tau-sweep uniform source */
#define DSM_RNG_MT19937 0        /* GSL-compatible serial stream (replay)     */
#define DSM_RNG_PHILOX  1        /* counter-based, keyed by (seed, iter, v,g) */

const char *dsm_last_error(void);
int dsm_device_count(void);
const char *dsm_version(void);

/* ---------------------------------------------------------------- (1) ---- */
/* replaces c_initRNG  (sampletau/c_sample_tau.c:26-34)                       */
int dsm_initRNG(void);
/* replaces c_setRNG   (sampletau/c_sample_tau.c:36-40); seed 0 -> 4357 (GSL) */
int dsm_setRNG(unsigned long seed);
/* replaces c_freeRNG  (sampletau/c_sample_tau.c:42-45)                       */
int dsm_freeRNG(void);
/* replaces c_sample_tau (sampletau/c_sample_tau.c:95-204).  Returns the number
 * of (v,g) whose base changed (>= 0) or a negative DSM_ERR_* code.           */
int dsm_sample_tau(int64_t *tau, const double *pi, const double *eta,
                   const int64_t *variants, int nV, int nG, int nS);
/* the same four entry points under the reference's own names and prototypes (what the four bare `cdef extern`
 * declarations of sampletau/sampletau.pyx:13-19 bind -- there is no header in the reference; c_sample_tau.c:26,36,42,95),
 * so the unmodified .pyx links against libdesman_hip.so.  Errors go to stderr; c_sample_tau then returns -1.        */
void c_initRNG(void);
void c_setRNG(unsigned long seed);
void c_freeRNG(void);
int c_sample_tau(long *tau, double *pi, double *eta, long *variants, int nV, int nG, int nS);
/* read / write the process-global MT19937 stream of the shim (624 words +
 * position): lets a device-resident context continue the same logical stream. */
int dsm_getRNG_state(uint32_t *state625);
int dsm_setRNG_state(const uint32_t *state625);

/* ---------------------------------------------------------------- (2) ---- */
typedef struct dsm_ctx dsm_ctx;

int dsm_ctx_create(dsm_ctx **out, int device);
int dsm_ctx_destroy(dsm_ctx *ctx);
int dsm_ctx_sync(dsm_ctx *ctx);

/* upload the count tensor (HaploSNP_Sampler.py:52); builds the int32 HBM
 * layouts and the data-only log-likelihood constant.                         */
int dsm_ctx_set_counts(dsm_ctx *ctx, const int64_t *variants, int V, int S);

/* chain state in / out.  set_state also (re)defines G.                       */
int dsm_ctx_set_state(dsm_ctx *ctx, const int64_t *tau, const double *gamma,
                      const double *eta, int G);
int dsm_ctx_get_state(dsm_ctx *ctx, int64_t *tau, double *gamma, double *eta);
int dsm_ctx_set_gamma_eta(dsm_ctx *ctx, const double *gamma, const double *eta);

/* priors / clamp of the sampler (HaploSNP_Sampler.py:31: alpha_constant,
 * delta_constant, epsilon); defaults 0.1, 0.1, 1e-6.                          */
int dsm_ctx_set_priors(dsm_ctx *ctx, double alpha, double delta, double epsilon);

/* RNG: mt_seed feeds the GSL-compatible tau stream (bin/desman:131-132),
 * ctr_seed keys every counter-based draw (mu/E, gamma, eta).                 */
int dsm_ctx_seed(dsm_ctx *ctx, unsigned long mt_seed, uint64_t ctr_seed);
int dsm_ctx_set_tau_rng(dsm_ctx *ctx, int mode /* DSM_RNG_* */);
/* export / import the MT19937 stream (624 state words + position), so that one
 * logical GSL stream can continue across contexts, as the reference's single
 * global generator does across sampler objects (bin/desman:131,149-153,199-201). */
int dsm_ctx_get_mt_state(dsm_ctx *ctx, uint32_t *state625);
int dsm_ctx_set_mt_state(dsm_ctx *ctx, const uint32_t *state625);
/* test hook: the next n raw 32-bit words of the context's MT19937 stream (advances it), host buffer.  */
int dsm_ctx_debug_mt_fill(dsm_ctx *ctx, size_t n, uint32_t *out);
/* fill `state625` from a seed exactly as gsl_rng_set(mt19937, seed) would. */
int dsm_mt_seed_state(unsigned long seed, uint32_t *state625);

/* A1: one tau sweep on the resident state (c_sample_tau.c:95-204) with the
 * resident gamma / eta (see dsm_ctx_set_gamma_eta).  logp_out (optional, host,
 * [V][G][4]) receives the un-normalised conditional log-probabilities.       */
int dsm_ctx_sample_tau(dsm_ctx *ctx, int *nchange, double *logp_out);

/* A2: one draw of the auxiliary-count sums (HaploSNP_Sampler.py:284-309 via
 * :266,:276): sum_mu [S][G], esum [4][4] = [observed][true].                 */
int dsm_ctx_sample_stats(dsm_ctx *ctx, uint32_t iter, uint64_t *sum_mu, uint64_t *esum);
/* which counter-based specification dsm_ctx_sample_stats / dsm_ctx_gibbs_update follow for the resident shape:
 * 2 = aggregated sampler (oracle/stats_agg.c, spec 2; needs G <= 16, a subset table of at most 64 MB and every sample's
 * depth < 2^32), 3 = a variant of it (same law; the start of the inversion search from a table exp / log instead of
 * repeated squaring, item streams two Philox rounds off the cell's block instead of three -- selectable, not the default:
 * measured no faster), 4 = spec 2's samplers over tau WORDS: positions whose packed tau words are equal pool their counts in the
 * lowest such position and stage 1 draws once per (word, sample) -- the same law (a sum of multinomials with one probability vector),
 * restated by oracle/cbind.py: stats_agg(spec=4); G <= 8, not for chains sharded by positions (they run spec 2); by rule on large tables
 * (G <= 2 from half a million cells, G = 3 from a million, G = 4 ... 8 from 2.5 million cells with 64 x 2^G <= V) --,
 * 1 = per-read draws (oracle/desman_oracle.c: orc_stats_counter).  Where the aggregated pass applies
 * the cheaper of it and the per-read pass runs, by a cost model over the read total, the cells V x S (padded to the
 * kernel's lane groups) and the atomics per subset counter (kernels_stats.hip: stats_spec) -- a function of the shape and
 * the read totals only, the same on every run.  dsm_ctx_force_stats_spec: 0 = that rule, 1 = always spec 1, 2 / 3 / 4 = that
 * version of the aggregated sampler wherever it applies, small problems too (environment: DESMAN_HIP_STATS_SPEC=1|2|3|4 for
 * contexts without a choice of their own).  A batch (dsm_batch_gibbs_update) runs what its chains would run alone (one
 * specification per batch: chains that differ in it are refused); a chain sharded by positions runs spec 2, so it is the
 * unsharded chain under dsm_ctx_force_stats_spec(ctx, 2).  */
int dsm_ctx_stats_spec(dsm_ctx *ctx);
int dsm_ctx_force_stats_spec(dsm_ctx *ctx, int spec);
/* test hooks of the aggregated sampler: stage 1 only (subset counts ntab [S][2^G] u32 and esum), and nsamp variates of one
 * sampler (kind 0 binom_small, 1 binom_big: out [nsamp]; 2 mult4 with weights w[0..3]: out [nsamp][4]) of version
 * spec (2 / 3) exactly as oracle/stats_agg.c: orc_binom_test / orc_mult4_test draw them.                          */
int dsm_ctx_debug_stage1(dsm_ctx *ctx, uint32_t iter, uint32_t *ntab, uint64_t *esum);
int dsm_ctx_debug_binom(dsm_ctx *ctx, int kind, uint32_t n, const double *w4, uint64_t seed, int nsamp,
                        uint32_t *out, int spec);

/* A3+A4: gamma ~ Dir(alpha + sum_mu[s,:]) clamped/renormalised, eta[a,:] ~
 * Dir(delta + esum[:,a]) (HaploSNP_Sampler.py:263-281) from given sums.      */
int dsm_ctx_draw_gamma_eta(dsm_ctx *ctx, uint32_t iter, const uint64_t *sum_mu,
                           const uint64_t *esum, double *gamma_out, double *eta_out);

/* A5: logLikelihood / logPosterior of the resident state
 * (HaploSNP_Sampler.py:431-461).                                             */
int dsm_ctx_loglik(dsm_ctx *ctx, double *ll, double *lp);

/* A6: HaploSNP_Sampler.update (HaploSNP_Sampler.py:334-365): n_iter full Gibbs
 * iterations with MAP tracking and traces, all on the device.                */
int dsm_ctx_gibbs_update(dsm_ctx *ctx, int n_iter);
/* The same for n_ctx (1..8) chains of one shape -- same device, V, S, G, tau RNG; typically the replicate chains of one
 * G value (scripts/runDesman.sh:15-21) -- with one kernel launch per step of the iteration for all of them.  On tables
 * that leave most of the GPU idle the batch costs little more than one chain.  The mu/E pass of a batch is always the
 * aggregated sampler (dsm_ctx_stats_spec 2; needs G <= 16): every chain ends in the state dsm_ctx_gibbs_update leaves
 * it in after dsm_ctx_force_stats_spec(ctx, 2).                                                                        */
int dsm_batch_gibbs_update(dsm_ctx *const *ctxs, int n_ctx, int n_iter);
/* HaploSNP_Sampler.updateTau (HaploSNP_Sampler.py:383-407): tau-only sweeps
 * driven by host traces gamma_store [n][S][G], eta_store [n][4][4].          */
int dsm_ctx_update_tau(dsm_ctx *ctx, int n_iter, const double *gamma_store,
                       const double *eta_store);
/* ... and for n_ctx (1..8) chains of one shape at once (the -r path of replicate chains): one launch per sweep for all of
 * them; gamma_stores[k] / eta_stores[k] are chain k's traces.                                                          */
int dsm_batch_update_tau(dsm_ctx *const *ctxs, int n_ctx, int n_iter, const double *const *gamma_stores,
                         const double *const *eta_stores);

/* HaploSNP_Sampler.update_fixed_tau (HaploSNP_Sampler.py:409-428): n_iter iterations of the chain with the haplotypes HELD -- per
 * iteration the mu/E pass at (tau, gamma, eta) under the context's own specification (dsm_ctx_stats_spec, dsm_ctx_force_stats_spec), the
 * gamma and eta draws, and ll / lp of the new state; the entry state is evaluated and recorded first, as by dsm_ctx_gibbs_update.
 * Results as after dsm_ctx_gibbs_update: gamma / eta / ll / lp traces, the MAP record (dsm_ctx_get_star), the state; nchange is 0 in every
 * iteration, dsm_ctx_get_tau_at gives the held tau for every iteration and dsm_ctx_get_tau_sum n_iter times it (one row is stored, not
 * n_iter).  The MT19937 stream is not touched (dsm_ctx_get_mt_state is the same before and after), the stream key stays, the iteration
 * counter advances by n_iter; a call of 2 n iterations is two calls of n, bit for bit.
 *   fix_eta != 0: eta is held too.  The E sums and the eta draw are still made (so the gamma draws of iteration 0 are those of
 *     fix_eta = 0), but the chain's eta, every row of the eta trace and the MAP record's eta are the entry matrix bit for bit, and ll / lp
 *     are evaluated at it.
 *   pool: 0 = the chain runs on the table as it is.  1 = on the POOLED table: positions whose packed tau words are equal have the same
 *     cell probabilities, so their counts are added once per call (a sum of multinomials with one probability vector is the multinomial
 *     of the summed count) and the chain runs on W <= min(V, 4^G) rows, one per distinct word in ascending order of the word
 *     (bit 2g.. of the word = base of haplotype g).  Counter-based streams are keyed by the pooled cell indices: the pooled chain is NOT
 *     the unpooled chain draw for draw; it is, bit for bit, the chain this call with pool = 0 runs on the pooled table with the same
 *     gamma, eta, priors, stream key and counter -- the same law.  ll and lp (traces, MAP record) are reported for the CALLER's table: the
 *     multinomial coefficients of the two tables differ by a constant, which is added (fp64; equal to pool = 0 to ~1e-12 relative to the
 *     summed terms).  The caller's counts and tau are only read.  DSM_ERR_UNSUPPORTED, before anything is launched, if a pooled count --
 *     a cell, or the four cells of one (word, sample) together, the depth dsm_ctx_set_counts bounds -- would pass 2^31-1.
 *     -1 = auto: pooled iff W < V and nothing overflows (pooling costs one pass over the table, less than one iteration's mu/E pass;
 *     where it stops paying has not been measured; at V = 10 000 and 200 iterations the pooled call was the slower one, DESIGN.md
 *     sec. 8c -- its set-up is paid per call), else as pool = 0.
 * Degenerate operands: V = 1 and G = 1 run like any other shape (W = 1 at V = 1); a sample without reads draws its gamma row from the
 * prior Dir(alpha) every iteration and adds 0 to ll.  n_iter = 0 evaluates and records the entry state only.
 * DSM_ERR_STATE without counts or state, DSM_ERR_ARG for n_iter < 0 or pool outside -1..1.  No batched or sharded form.              */
int dsm_ctx_gibbs_update_fixed_tau(dsm_ctx *ctx, int n_iter, int fix_eta, int pool);
/* test hooks of the pooled form, for the resident state (nothing of the context changes): the pooled table itself -- *W distinct words,
 * pooled [W][S][4] int32 (give room for [V][S][4]), words [W] ascending (room for V), row [V] = the row of each position's word; any
 * pointer may be NULL -- and one dsm_ctx_sample_stats draw made ON the pooled state.  DSM_ERR_UNSUPPORTED on overflow as above.        */
int dsm_ctx_debug_fixtau_pool(dsm_ctx *ctx, int *W, int32_t *pooled, uint64_t *words, int32_t *row);
int dsm_ctx_debug_fixtau_sample_stats(dsm_ctx *ctx, uint32_t iter, uint64_t *sum_mu, uint64_t *esum);

/* The chain with the LAST n_held haplotypes held and haplotypes 0 .. F-1, F = G - n_held, sampled: a haplotype known
 * from an isolate anchors the fit of the rest, or the haplotypes of a finished run are held while further ones are fitted to new samples
 * (`desman-abund --novel`).  Callers order their haplotypes so that the held ones come last; there is no mask.
 *   dsm_ctx_sample_tau_held: one sweep over the free haplotypes of the resident state with the resident gamma / eta, the counterpart of
 *     dsm_ctx_sample_tau: every step is that sweep's step (the rest mixture runs over all other haplotypes, held ones included), in plain
 *     fp64; the held digits are only read.  *nchange = changed (position, free haplotype) pairs.  The iteration counter advances by one.
 *     DSM_RNG_MT19937: the sweep consumes exactly V F words of the context's stream, position-major, free haplotype ascending (word
 *     v F + g decides step (v, g)); DSM_RNG_PHILOX: step (v, g) is keyed as the full sweep keys it, so the free digits are those
 *     dsm_ctx_sample_tau draws at the same counter.  n_held = 0 is dsm_ctx_sample_tau(ctx, nchange, NULL); n_held = G changes nothing
 *     but the counter and consumes no word.
 *   dsm_ctx_gibbs_update_held_tau: n_iter iterations of dsm_ctx_gibbs_update with the sweep replaced by the held sweep -- the mu/E pass
 *     under the context's own specification, the gamma and eta draws, the held sweep with (new gamma, previous eta), ll / lp of the new
 *     state; the entry state is evaluated and recorded first.  Results as after dsm_ctx_gibbs_update: all traces (dsm_ctx_get_tau_at,
 *     dsm_ctx_get_tau_sum and the dsm_ctx_trace_* reductions read one stored tau per iteration), the MAP record, the state.  fix_eta != 0
 *     holds eta exactly as dsm_ctx_gibbs_update_fixed_tau does: the draw is made, the chain's eta, the trace rows and the MAP record's eta
 *     stay the entry matrix, and the sweep and ll / lp read it.  The MT19937 stream advances by n_iter V F words; the iteration counter
 *     by n_iter; a call of 2 n iterations is two calls of n, bit for bit.
 *     n_held = 0: the call IS dsm_ctx_gibbs_update(ctx, n_iter) (fix_eta is not looked at); n_held = G: it IS
 *     dsm_ctx_gibbs_update_fixed_tau(ctx, n_iter, fix_eta, 0).
 * Limits: those of dsm_ctx_gibbs_update for a single chain.  DSM_ERR_ARG for n_iter < 0 or n_held outside 0..G, DSM_ERR_STATE without
 * counts or state (or, MT19937, without a seeded stream).  No batched or sharded form.                                              */
int dsm_ctx_sample_tau_held(dsm_ctx *ctx, int n_held, int *nchange);
int dsm_ctx_gibbs_update_held_tau(dsm_ctx *ctx, int n_iter, int n_held, int fix_eta);

/* Pair moves of the main chain: an opt-in block-Gibbs step that redraws two haplotypes of a position jointly, so that
 * two haplotypes carrying each other's bases can swap them without passing through the state in which both carry the same base.
 *   dsm_ctx_set_pair_moves: every = 0 (the default) is off; E > 0 = in dsm_ctx_gibbs_update a pair pass follows the single-site sweep of
 *     every iteration whose counter satisfies (iter_ctr + 1) mod E == 0, iter_ctr being the value the iteration takes (it persists across
 *     calls and through dsm_ctx_get_counters / dsm_ctx_set_counters: a chain is the same whether its iterations come in one call or
 *     several, and after a checkpoint).  On such an iteration the sweep runs as always, the pair pass runs with the gamma and the eta the
 *     sweep conditioned on, and a likelihood-only pass at (tau after the pairs, new gamma, new eta) stores tau in the iteration's trace
 *     slot and gives ll, lp and the MAP record; the iteration's nchange is the sweep's count plus the pass's.  Every other iteration
 *     launches what it launches without the setting.  every < 0: DSM_ERR_ARG.  With E > 0 dsm_batch_gibbs_update, the partly held chain
 *     (0 < n_held < G) and both sharded forms return DSM_ERR_UNSUPPORTED; the fixed-tau chain has no tau step and ignores the setting;
 *     dsm_ctx_update_tau keeps the single-site sweep.
 *   dsm_ctx_sample_tau_pairs: one pair pass on the resident state with the resident gamma / eta, keyed by `iter`; the counterpart of
 *     dsm_ctx_sample_tau_held.  The pass visits the pairs (g, h), g < h, of every position in lexicographic order; a step is the pair
 *     step of dsm_assign_tau_sampled_pairs (sixteen totals L_k, k = 4 a + a', q_k = exp(L_k - max) / (e_0 + ... + e_15), inverse CDF over
 *     ascending k with the last edge forced; all sixteen -inf: the pair stays).  The uniform of step (v, g, h) is word 0 / 2^32 of
 *     Philox4x32-10(key = the context's counter seed (lo32, hi32); counter = (lo32 j, hi32 j, iter, 'TPAR')), j = v G^2 + g G + h, in
 *     every tau RNG mode: the MT19937 stream and the iteration counter are not touched.  *nchange = haplotype digits that differ from
 *     their value before their step (0, 1 or 2 per step).  G < 2: nothing to do.
 *   dsm_pairtau_debug_path: test hook, out = {lanes per position, sample slots per lane} of the kernel instantiation for S samples. */
int dsm_ctx_set_pair_moves(dsm_ctx *ctx, int every);
int dsm_ctx_get_pair_moves(dsm_ctx *ctx, int *every);
int dsm_ctx_sample_tau_pairs(dsm_ctx *ctx, uint32_t iter, int *nchange);
int dsm_pairtau_debug_path(int S, int G, int out[2]);

/* results of the last update call.  Any pointer may be NULL.                 */
int dsm_ctx_get_trace(dsm_ctx *ctx, double *ll, double *lp, int32_t *nchange,
                      double *gamma_store, double *eta_store);
int dsm_ctx_get_star(dsm_ctx *ctx, int64_t *tau_star, double *gamma_star,
                     double *eta_star, double *lp_star, int *iter_star);
/* sum over the stored iterations of the one-hot tau ([V][G][4] int64):
 * tauMean = tau_sum / n_iter (HaploSNP_Sampler.py:479-483).                  */
int dsm_ctx_get_tau_sum(dsm_ctx *ctx, int64_t *tau_sum);
/* tau as stored after iteration `it` of the last update ([V][G][4] int64).   */
int dsm_ctx_get_tau_at(dsm_ctx *ctx, int it, int64_t *tau);

/* Reductions of the resident tau trace of the last update call, for posterior summaries that survive label switching (DESIGN.md
 * sec. 8d; desman_amd/relabel.py).  The trace stays on the device: one pass over its packed words (8 B per position and iteration),
 * integer results, the same bits from run to run.  Iteration `it` is what dsm_ctx_get_tau_at(it) returns; after
 * dsm_ctx_gibbs_update_fixed_tau every iteration is the held tau.
 *   dsm_ctx_trace_snd: for the stored iterations it0 .. it0 + n_it - 1 and a reference of Gr haplotypes
 *       snd[t][g][h] = #{ v : tau_t[v][g] != ref_t[v][h] }                              int32 [n_it][G][Gr]
 *     mode DSM_SND_STAR   ref = the tau of the MAP record (what dsm_ctx_get_star returns); Gr = G (pass 0 or G), ref_tau ignored
 *          DSM_SND_SELF   ref_t = tau_t: the pairwise distances within each iteration (calculateSND, HaploSNP_Sampler.py:712-730:
 *                         symmetric, zero diagonal); Gr = G (pass 0 or G), ref_tau ignored
 *          DSM_SND_GIVEN  ref = ref_tau [V][Gr] DIGITS 0..3 (the format dsm_fit_gamma takes), 1 <= Gr <= DSM_MAX_G
 *   dsm_ctx_get_tau_sum_perm: dsm_ctx_get_tau_sum over the same kind of range with the labels of iteration t renamed by row t of perm
 *     (uint8 [n_it][G], each row a permutation of 0..G-1):  tau_sum[v][perm[t][g]][a] += [tau_t[v][g] = a],  int64 [V][G][4].  With
 *     identity rows over the whole trace it is dsm_ctx_get_tau_sum.
 * DSM_ERR_STATE when no update has run (or, DSM_SND_STAR, the MAP record names a slot outside the trace: only after
 * dsm_ctx_debug_set_trace); DSM_ERR_ARG for a range outside 0 .. the trace's length, a bad mode, Gr outside its range, a digit outside
 * 0..3, a perm row that is no permutation.  n_it = 0 succeeds and writes nothing to snd (tau_sum: zeros).  The chain state, both RNG
 * streams, the traces and the MAP record are only read: a chain continues bit for bit after these calls.                          */
#define DSM_SND_STAR  0
#define DSM_SND_SELF  1
#define DSM_SND_GIVEN 2
int dsm_ctx_trace_snd(dsm_ctx *ctx, int mode, const int64_t *ref_tau /*[V][Gr] digits or NULL*/, int Gr, int it0, int n_it,
                      int32_t *snd /*[n_it][G][Gr]*/);
int dsm_ctx_get_tau_sum_perm(dsm_ctx *ctx, const uint8_t *perm /*[n_it][G]*/, int it0, int n_it, int64_t *tau_sum /*[V][G][4]*/);
/* test hook: installs a synthetic tau trace of n iterations, tau_digits [n][V][G] DIGITS 0..3 (DSM_ERR_ARG otherwise): slot 0 (the
 * entry state, dsm_ctx_get_tau_at(-1)) = the resident tau, iteration k = tau_digits[k], the trace's length = n, as after
 * dsm_ctx_gibbs_update (not a fixed-tau trace).  Needs counts and a state (DSM_ERR_STATE).  The state, both RNG streams and the
 * counters are not touched, nor is the MAP record: DSM_SND_STAR then compares against the slot that record names in the PLANTED
 * trace.  A context on which no update has run has no record; it is given the resident state as one (slot 0, lp = -inf).  The
 * ll / lp / nchange / gamma / eta traces keep what they held (zeros where the call had to allocate them).                       */
int dsm_ctx_debug_set_trace(dsm_ctx *ctx, const int64_t *tau_digits /*[n][V][G]*/, int n);

/* Batch sums of the resident tau trace for convergence diagnostics (batch-means MCSE and ESS, split R-hat; DESIGN.md sec. 8f;
 * desman_amd/diagnose.py): one more reduction of the kind above, exact integers, the same bits for any grid.  With L = batch_len,
 * B = 2 * floor(n_it / (2 L)) batches (always even: two halves of equal length) and N = B L, only the LAST N of the iterations
 * it0 .. it0 + n_it - 1 are used; the first n_it - N are skipped.  Iteration numbering is that of dsm_ctx_get_tau_at; row t of perm
 * (uint8 [n_it][G], counted from it0 -- the rows of skipped iterations are passed and validated too; NULL = identity rows) renames
 * iteration t's labels as in dsm_ctx_get_tau_sum_perm.  Write x_t[v][l][a] = [the haplotype carrying label l in iteration t has base
 * a at v]:
 *     sum   [V][G][4] int64   sum of x_t over the N used iterations (= dsm_ctx_get_tau_sum_perm over exactly those)
 *     first [V][G][4] int64   the same over the first B / 2 batches
 *     bsq   [V][G][4] int64   sum over the batches b of (sum_{t in b} x_t)^2
 *     flips [V][G]    int32   the used iterations t, not counting the first, at which label l's base at v differs from its base at
 *                             t - 1, each iteration read under its own perm row
 * Any output pointer may be NULL.  DSM_ERR_STATE when no update has run; DSM_ERR_ARG for a range outside the trace, batch_len < 1,
 * 0 < n_it < 2 batch_len, a perm row that is no permutation.  n_it = 0 succeeds and writes zeros.  After
 * dsm_ctx_gibbs_update_fixed_tau every iteration is the held tau.  The chain is only read, as by the calls above.  Limits as there:
 * one context, 1 <= G <= DSM_MAX_G.                                                                                              */
int dsm_ctx_trace_batch_stats(dsm_ctx *ctx, const uint8_t *perm /*[n_it][G] or NULL*/, int it0, int n_it, int batch_len,
                              int64_t *sum /*[V][G][4]*/, int64_t *first /*[V][G][4]*/, int64_t *bsq /*[V][G][4]*/,
                              int32_t *flips /*[V][G]*/);
/* test hook: the number of parts the call above splits its batches into across workgroups (0 = the library's own choice, the
 * default; more parts than batches: one batch each) */
int dsm_diag_debug_set_parts(int parts);

/* Posterior predictive fit of the chain per sample, per position and per cell (desman_amd/check.py): one device pass
 * over the resident counts and the tau, gamma and eta traces of the iterations it0 .. it0 + n_it - 1 (numbered as by
 * dsm_ctx_get_tau_at).  For a stored iteration t and a cell (v, s) with counts n_b, N = sum_b n_b > 0 (an empty cell adds nothing
 * anywhere), p_b = sum_g gamma_t[s][g] eta_t[tau_t[v][g]][b] -- the likelihood's own probabilities -- and k = #{b : p_b > 0}:
 *     X = sum_{b: p_b > 0} (n_b - N p_b)^2 / (N p_b)       Pearson's discrepancy
 *     D = 2 sum_{b: n_b > 0} n_b ln(n_b / (N p_b))          the deviance against the saturated model
 *     E = k - 1                                             the exact mean of X under multinomial(N, p)
 *     W = 2 (k - 1) + (sum_{b: p_b > 0} 1 / p_b - k^2 - 2 k + 2) / N      its exact variance
 * A base with p_b = 0 < n_b makes X and D of its cell +inf; one with p_b = 0 = n_b adds 0; nothing is ever NaN.  Outputs, sums over the
 * iterations (the caller divides by n_it):
 *     sample   [S][4] double   sum over t and v of (X, D, E, W)
 *     position [V][4] double   sum over t and s of (X, D, E, W)
 *     cell     [V][S] double   sum over t of X
 * Any output pointer may be NULL (cell = NULL also saves its device buffers).  Plain fp64 sums in a fixed order, no floating-point
 * atomics: two calls with the same split of the iteration range give the same bits; another split moves the last bits.  n_it = 0
 * succeeds and writes zeros.  DSM_ERR_STATE when no update has run, DSM_ERR_ARG for a range outside the trace.  After
 * dsm_ctx_gibbs_update_fixed_tau every iteration is the held tau.  The chain, both RNG streams, the traces and the MAP record are only
 * read.  Limits: one context, 1 <= G <= DSM_MAX_G, S <= DSM_MAX_S.                                                                 */
int dsm_ctx_trace_fit_stats(dsm_ctx *ctx, int it0, int n_it, double *sample /*[S][4]*/, double *position /*[V][4]*/,
                            double *cell /*[V][S]*/);
/* test hook: the number of parts the call above splits its iterations into across workgroups (0 = the library's own choice, the
 * default; never more parts than iterations) */
int dsm_fit_debug_set_parts(int parts);
/* test hook: what a dsm_ctx_trace_fit_stats call over n_it >= 1 iterations would launch on this context's table: out = {sample slots
 * per lane (the kernel's instantiation: 1, 2, 4 or 8), lanes per position, haplotypes per staged chunk of gamma, workgroups per part,
 * parts}.  Nothing is launched.  Needs counts and a state.                                                                          */
int dsm_fit_debug_path(dsm_ctx *ctx, int n_it, int out[5]);
/* test hook, the companion of dsm_ctx_debug_set_trace: overwrites the first n rows of the gamma and eta traces.  DSM_ERR_ARG when n
 * exceeds the trace's length (0 before any update or dsm_ctx_debug_set_trace).                                                      */
int dsm_ctx_debug_set_param_trace(dsm_ctx *ctx, const double *gamma /*[n][S][G]*/, const double *eta /*[n][16]*/, int n);

/* Posterior predictive p-values of the chain per sample and per position from replicate tables (desman_amd/check.py):
 * the realised-discrepancy check of Gelman, Meng and Stern (1996) with Pearson's X of dsm_ctx_trace_fit_stats as the discrepancy.
 *
 * Iterations.  The used iterations are t = it0, it0 + stride, ... below it0 + n_it: n_used = ceil(n_it / stride) of them.  Numbering, and
 * the (tau_t, gamma_t, eta_t) that belongs to t, are those of dsm_ctx_trace_fit_stats.
 * Cells.  For a used iteration t, a replicate r = 0 .. R - 1 and a cell (v, s) with counts x_b, N = sum_b x_b (an empty cell adds nothing
 * anywhere) and p_b as dsm_ctx_trace_fit_stats forms it (one shared device function):
 *     x_rep ~ Multinomial(N, p / sum_b p_b), by conditional binomials over the bases with p_b > 0 in ascending b, the last such base
 *             taking the remainder (a base with p_b = 0 is never drawn; a cell without any such base has X_rep = 0)
 *     X_obs = sum_{b: p_b > 0} (x_b - N p_b)^2 / (N p_b), +inf where some p_b = 0 < x_b;  X_rep the same formula on x_rep (finite)
 * Discrepancies.  T_s(t) = sum_v X and T_v(t) = sum_s X, of the observed table and of every replicate, plain fp64 sums in ONE order that
 * depends on S alone (not on parts, chunks or the grid), the same for T_obs and T_rep: with L = min(64, the power of two >= S) lanes per
 * position, lane l adds its samples l, l + L, l + 2 L, ... in ascending order from 0, then the L lane sums meet by a butterfly
 * (a_l += a_{l xor o} for o = L/2, L/4, ... 1); over positions, the 256 / L positions of a tile in ascending order from 0, then the tiles
 * in ascending order from 0.  Sums over (t, r) are nested: over r ascending from 0 inside an iteration, then over t ascending from 0.
 * Outputs (host pointers, any may be NULL):
 *     ge_sample [S], ge_position [V]        int64    the number of (t, r) with T_rep >= T_obs(t); T_obs = +inf counts 0
 *     rep_sample [S][2], rep_position [V][2] double  sum_{t,r} T_rep and sum_{t,r} T_rep^2
 *     obs_sample [S], obs_position [V]       double  sum_t T_obs (column X of dsm_ctx_trace_fit_stats over the same iterations, up to the
 *                                                    order of summation)
 * The posterior predictive p-value is ge / (n_used R).
 * Uniforms.  Counter based, from no stream the chain uses: the generator of (v, s, t, r) is xoshiro128+ seeded with the four words of
 * Philox4x32-10(key = the chain's counter seed xor salt, as (lo32, hi32); counter = (lo32 j, hi32 j, t * DSM_PPC_MAX_R + r, 'PPCR')),
 * j = v S + s (a block of all zeros: word 0 = 1), t the stored iteration's own number.  A cell's draw depends on (seed, salt, v, s, t, r)
 * alone -- not on the tiling, the grid, parts, chunks, R, or which other iterations are used.  salt = 0: the chain's seed alone.
 * Two draw paths, one law.  N <= DSM_PPC_READS: read by read, one 32-bit word w per read against integer thresholds by the rule of the
 * mu/E pass's read loop: c_b = p_0 + .. + p_b added in ascending b from 0, th_b = sat_u32(floor(c_b * (2^32 / c_3))) for b = 0, 1, 2,
 * n_b = #{w < th_b}, n_b = N for every b >= the last base with p_b > 0, and x_rep = (n_0, n_1 - n_0, n_2 - n_1, N - n_2).
 * N > DSM_PPC_READS: three conditional binomials (rem, p_b : p_{b+1} + (.. + p_3)) by the sampler of the mu/E pass (inversion while the
 * rarer outcome's mean is <= 128, BTRS above), the tails added from p_3 downwards.
 * The chain, both RNG streams, every trace and the MAP record are only read.  n_it = 0 succeeds and writes zeros.  DSM_ERR_STATE when no
 * update has run; DSM_ERR_ARG for a range outside the trace, stride < 1 or R < 1.  After dsm_ctx_gibbs_update_fixed_tau every iteration
 * is the held tau.  Limits: one context, 1 <= G <= DSM_MAX_G, S <= DSM_MAX_S, R <= DSM_PPC_MAX_R, iterations below 2^32 / DSM_PPC_MAX_R
 * (DSM_ERR_UNSUPPORTED beyond).  Scratch: at most DSM_PPC_SCRATCH_MB MiB for the per-tile sample sums of a launch (the iterations are
 * cut into chunks, one iteration's replicates too where a single iteration exceeds it) + 40 bytes per position and chunk iteration. */
#define DSM_PPC_MAX_R 1024
#define DSM_PPC_READS 128
#define DSM_PPC_SCRATCH_MB 256
int dsm_ctx_trace_ppc(dsm_ctx *ctx, int it0, int n_it, int stride, int R, uint64_t salt,
                      int64_t *ge_sample /*[S]*/, int64_t *ge_position /*[V]*/,
                      double *rep_sample /*[S][2]*/, double *rep_position /*[V][2]*/,
                      double *obs_sample /*[S]*/, double *obs_position /*[V]*/);
/* test hooks: the parts a launch of the call above splits its iterations into across workgroups, and the iterations / replicates per
 * launch (0 = the library's own choice, the default; fewer replicates than R per launch means one iteration per launch)             */
int dsm_ppc_debug_set_parts(int parts);
int dsm_ppc_debug_set_chunk(int iterations, int replicates);
/* test hook: what the call above over n_used >= 1 used iterations and R replicates would launch on this context's table: out = {sample
 * slots per lane (the kernel's instantiation: 1, 2, 4 or 8), lanes per position, haplotypes per staged chunk of gamma, tiles of
 * positions, parts, iterations per launch, replicates per launch, DSM_PPC_READS}.  Nothing is launched.  Needs counts and a state.    */
int dsm_ppc_debug_path(dsm_ctx *ctx, int n_used, int R, int out[8]);

/* Rao-Blackwellised marginals of tau for the positions of the fit (desman_amd/marginals.py): one device pass over
 * the resident counts and the tau, gamma and eta traces.  Iteration numbering, and which (tau_t, gamma_t, eta_t) belongs to iteration t,
 * are those of dsm_ctx_trace_fit_stats.  For a stored iteration t, a position v and a haplotype g
 *     rest[s][b] = fma chain from 0 over h != g, h ascending, of eta_t[tau_t[v][h]][b] * gamma_t[s][h]          (G = 1: 0)
 *     L_a        = sum over s, b with x[v][s][b] > 0 of x ln(rest[s][b] + eta_t[a][b] gamma_t[s][g]),  a = 0..3   (x exact in fp64; a zero
 *                  count adds 0; p = 0 under a positive count makes L_a = -inf)
 *     q_a        = exp(L_a - max) / (((e_0 + e_1) + e_2) + e_3)
 * is the exact full conditional of tau_vg; where all four L_a are -inf, q is the one-hot of the current base tau_t[v][g] and the
 * cell-iteration is counted in *dead.  Nothing is ever NaN for a finite, non-negative trace.  No random number is drawn.
 * Range, perm (validation of skipped rows included) and the batch rule are those of dsm_ctx_trace_batch_stats: L = batch_len,
 * B = 2 floor(n_it / (2 L)) batches, only the LAST B L iterations are used.  With l = perm[t][g]:
 *     sum  [V][G][4] double   sum over the batches, ascending, of the batch sums; a batch sum is the sum of q from 0 over the batch's
 *                             iterations, t ascending
 *     bsq  [V][G][4] double   sum over the batches, ascending, of (batch sum)^2
 *     dead [1]                cell-iterations without a live base
 * One order of summation per cell, no floating-point atomics: the same bits from call to call and for any grid.  Any output pointer may
 * be NULL.  n_it = 0 succeeds and writes zeros.  DSM_ERR_STATE when no update has run; DSM_ERR_ARG for a range outside the trace,
 * batch_len < 1, 0 < n_it < 2 batch_len, a perm row that is no permutation.  After dsm_ctx_gibbs_update_fixed_tau every iteration is
 * the held tau.  The chain state, both RNG streams, every trace and the MAP record are only read.  Limits: one context,
 * 1 <= G <= DSM_MAX_G, S <= DSM_MAX_S (DSM_ERR_UNSUPPORTED beyond).
 *   dsm_rbtau_debug_path: test hook, out = {lanes per position, sample slots per lane} of the kernel instantiation for S samples.   */
int dsm_ctx_trace_rb_marginals(dsm_ctx *ctx, const uint8_t *perm /*[n_it][G] or NULL*/, int it0, int n_it, int batch_len,
                               double *sum /*[V][G][4]*/, double *bsq /*[V][G][4]*/, long long *dead /*[1]*/);
int dsm_rbtau_debug_path(int S, int G, int out[2]);

/* Rao-Blackwellised JOINT posterior of the bases of two haplotypes at the positions of the fit (DESIGN.md sec. 8l;
 * desman_amd/marginals.py): one device pass over the resident counts and the tau, gamma and eta traces.  Iteration numbering, and which
 * (tau_t, gamma_t, eta_t) belongs to iteration t, are those of dsm_ctx_trace_fit_stats.  P = G (G - 1) / 2 pairs (g, h), g < h, pair
 * p at the index of its place in lexicographic order.  For a used iteration t, a position v and a pair (g, h), with the other G - 2
 * bases at their values in tau_t (the arithmetic of the pair pass, dsm_ctx_sample_tau_pairs, without its draw and without writing tau):
 *     m_a[s]     = sum over k != g, h with tau_t[v][k] = a of gamma_t[s][k]                       (k ascending)
 *     rest[s][b] = ((m_0 eta_t[0][b] + m_1 eta_t[1][b]) + m_2 eta_t[2][b]) + m_3 eta_t[3][b]
 *     L_k        = sum over s, b with x[v][s][b] > 0 of x ln((rest[s][b] + eta_t[a][b] gamma_t[s][g]) + eta_t[a'][b] gamma_t[s][h]),
 *                  k = 4 a + a'  (x exact in fp64; a zero count adds 0; p = 0 under a positive count makes L_k = -inf)
 *     q_k        = exp(L_k - max) / (e_0 + e_1 + ... + e_15, added in this order)
 * is the exact full conditional of (tau_vg, tau_vh); where all sixteen L_k are -inf, q is the one-hot of the current pair and the
 * (position, pair, iteration) is counted in *dead.  Nothing is ever NaN for a finite, non-negative trace.  No random number is drawn.
 * Range and perm validation (all n_it rows) are those of dsm_ctx_trace_batch_stats; stride >= 1 takes the iterations it0, it0 + stride,
 * ... below it0 + n_it, n_used = ceil(n_it / stride) of them, as dsm_ctx_trace_predictive does; the batch rule applies to the taken
 * ones: L = batch_len, B = 2 floor(n_used / (2 L)) batches, only the LAST B L of them are used.  With l = perm[t][g], l' = perm[t][h]
 * (NULL: l = g, l' = h) the pair is accumulated as pair (min(l, l'), max(l, l')), and with l > l' the 4 x 4 matrix q is transposed first:
 *     joint      [V][P][16] double   the sum of q_k over the used iterations, t ascending from 0
 *     same_batch [B][P]     double   per batch the sum over the positions, ascending from 0, of the position's sum over the batch's
 *                                    iterations, t ascending from 0, of ((q_0 + q_5) + q_10) + q_15 = P(both carry the same base)
 *     dead       [1]                 (position, pair, iteration)s without a live state
 * One order of summation per cell, no floating-point atomics: the same bits from call to call, for any grid and for any cut of the
 * positions into chunks.  The positions go through the device in chunks so that the call's device scratch -- per position of a chunk
 * P (16 [joint asked for] + B [same_batch asked for]) doubles -- stays within 128 MiB (a chunk has at least one position: at most
 * P (16 + B) doubles where that is more), plus the B P results and the n_used P two-byte pair indices; at G = 32, P = 496, that is
 * 2114 positions per launch with joint alone.  dsm_rbpair_debug_set_chunk(positions): test hook, positions per launch (0 = by the
 * bound); results do not depend on it.
 * Any output pointer may be NULL.  n_it = 0 succeeds and writes zeros (same_batch has no batch then).  G = 1 (P = 0) succeeds and
 * writes nothing, *dead included.  DSM_ERR_STATE when no update has run; DSM_ERR_ARG for a range outside the trace, stride < 1,
 * batch_len < 1, 0 < n_used < 2 batch_len, a perm row that is no permutation (nothing is written then).  After
 * dsm_ctx_gibbs_update_fixed_tau every iteration is the held tau.  The chain state, both RNG streams, every trace and the MAP record
 * are only read.  Limits: one context, G <= DSM_MAX_G, S <= DSM_MAX_S (DSM_ERR_UNSUPPORTED beyond).
 *   dsm_rbpair_debug_path: test hook, out = {lanes per position, sample slots per lane} of the kernel instantiation for S samples.  */
int dsm_ctx_trace_rb_pairs(dsm_ctx *ctx, const uint8_t *perm /*[n_it][G] or NULL*/, int it0, int n_it, int stride, int batch_len,
                           double *joint /*[V][P][16]*/, double *same_batch /*[B][P]*/, long long *dead /*[1]*/);
int dsm_rbpair_debug_path(int S, int G, int out[2]);
int dsm_rbpair_debug_set_chunk(int positions);

/* A8-A12: Init_NMFT (desman/Init_NMFT.py).  F is derived from the resident
 * counts (:49-60).  tau [4V][G] row v + a*V, gamma [G][S] as in the reference.
 * Every shape up to S = DSM_MAX_S, G = DSM_MAX_G has a kernel (tests/test_gpu_nmft_forms.py
 * walks the dispatch, both limits together included).                        */
int dsm_nmft_set(dsm_ctx *ctx, const double *tau, const double *gamma, int G);
int dsm_nmft_get(dsm_ctx *ctx, double *tau, double *gamma);
/* factorize (:98-115) incl. _adjustment; fix_gamma != 0 -> factorize_tau
 * (:134-149, no _adjustment).  div_trace (optional, max_iter+1) gets the
 * objective before the first and after every update; *n_done = updates run.  */
int dsm_nmft_factorize(dsm_ctx *ctx, int max_iter, double min_change, int fix_gamma,
                       int *n_done, double *div_trace);
/* The same for n_ctx (1..8) chains of one shape at once (replicate chains: one launch of each kernel of an update for all
 * of them; the stop test stays per chain).  One-pass kernels only (families 1 and 2 of dsm_nmft_debug_path; DSM_ERR_UNSUPPORTED otherwise).
 * n_done [n_ctx]; div_traces [n_ctx][max_iter + 1] or NULL.                                                          */
int dsm_batch_nmft_factorize(dsm_ctx *const *ctxs, int n_ctx, int max_iter, double min_change, int fix_gamma,
                             int *n_done, double *div_traces);
int dsm_nmft_objective(dsm_ctx *ctx, double *div);
/* test hook (read only; launches nothing, allocates nothing): the kernels dsm_nmft_factorize (fix_gamma as there) takes for this
 * context as it is set up now -- dsm_nmft_set's shape, dsm_ctx_set_nmft_persist, dsm_ctx_set_nmft_fused, timing -- answered by the
 * functions the launchers ask.  DSM_ERR_STATE before dsm_nmft_set.
 *   out[0] family: 0 two-pass (nmft_pass_a_kernel + nmft_pass_b_kernel), 1 nmft_mfma_kernel (gamma fixed: nmft_mfma_fix_kernel),
 *          2 nmft_split_kernel, 3 nmft_persist_kernel (the shape gate and the residency test of the launch both passed)
 *   out[1] NT, sample tiles of 16 (per column block for family 2);  family 0: the padded sample lanes of pass A (32..256)
 *   out[2] KB, haplotype blocks of 4;                               family 0: the accumulators GM of pass A (4, 8, 16, 32)
 *   out[3] NCB, column blocks (family 2, else 0)       out[4] wavefronts per workgroup (family 3, else 0)
 *   out[5] workgroups of the update launch (family 0: of pass B)    out[6] its dynamic LDS in bytes
 *   out[7] flags: bit 0 nmft_split_kernel runs with two exchange buffers (split_xpar); bit 1 the update kernel begins with the
 *          gamma / control step (see dsm_ctx_set_nmft_fused); bits 8..15 variants per workgroup step of pass B (family 0);
 *          bits 16..30 the device's compute units, which cap the grids and gate family 3
 * Read only for the context; where the shape gate admits family 3 it sets that kernel's maximum dynamic LDS attribute
 * (hipFuncSetAttribute) as the launch would, for the residency test.                                                         */
int dsm_nmft_debug_path(dsm_ctx *ctx, int fix_gamma, int out[8]);
/* get_tau (:230-245) -> one-hot [V][G][4] int64                              */
int dsm_nmft_get_tau(dsm_ctx *ctx, int64_t *tau_onehot);

/* f3 (upstream of the path): one inner step of Variant_Filter.get_filtered_VariantsLogRatio
 * (desman/Variant_Filter.py:348-356) for all V positions: BLL, the bounded-Brent minimiser of
 * mixNLL over p in (0, upperP) when `optimise` (scipy minimize_scalar(method='bounded')
 * semantics), and MLL at p.  Host pointers: ffreq [V][4] f64, maxA/maxB [V] int32, eta [4][4],
 * p_inout/MLL/BLL [V].                                                        */
int dsm_lrt_step(int device, const double *ffreq, const int32_t *maxA, const int32_t *maxB,
                 const double *eta, double upperP, int optimise, int V, double *p_inout,
                 double *MLL, double *BLL);

/* Exact joint haplotype assignment of positions that were not in the fit (desman/HaploSNP_Sampler.py:233-261, assignTau;
 * bin/desman:209-240).  For each of the N positions ALL 4^G joint states t = (a_0 .. a_{G-1}) are evaluated in fp64 under the
 * fitted gamma [S][G] and eta [4][4] with a uniform prior over the states:
 *     L(t) = sum_{s,b} x[s][b] ln sum_g gamma[s][g] eta[a_g][b]     (cells with x = 0 contribute exactly 0),
 * state index idx(t) = sum_g a_g 4^(G-1-g), the order of the reference's tauStates.  Host pointers:
 *     map_state [N][G]    argmax_t L(t), ties to the lowest idx
 *     conf      [N]       posterior of map_state = 1 / sum_t exp(L(t) - L_max)   (the reference's conf)
 *     logz      [N]       ln sum_t exp L(t)
 *     marg      [N][G][4] P(a_g = a | x, gamma, eta)
 *     draw_state[N][G]    (may be NULL) one draw from the posterior: inverse CDF over idx order with one Philox uniform keyed by
 *                         (seed, position index within the call); the reference's assignTau in law
 * A position at which no state has positive probability (exact zeros in eta / gamma that contradict its counts) comes back as
 * map_state = draw_state = 0..0, conf = 0, logz = -inf, marg = 0.  Limits: 1 <= G <= DSM_ASSIGN_MAX_G (4^10 ~ 10^6 states per
 * position; above: DSM_ERR_UNSUPPORTED), S <= DSM_MAX_S, counts as dsm_ctx_set_counts takes them (DSM_ERR_ARG otherwise; gamma and
 * eta must be finite and >= 0).  Positions are processed in chunks, device scratch stays below ~40 MB whatever N is.  The results
 * do not depend on the chunking, on scheduling or on the entry point: dsm_ctx_assign_tau runs the same code on the count tensor
 * resident in the context (N = its V; the chain state is neither needed nor touched).                                        */
#define DSM_ASSIGN_MAX_G 10
int dsm_assign_tau(int device, const int64_t *counts /*[N][S][4]*/, int N, int S, int G, const double *gamma, const double *eta,
                   uint64_t seed, uint8_t *map_state, double *conf, double *logz, double *marg, uint8_t *draw_state);
int dsm_ctx_assign_tau(dsm_ctx *ctx, const double *gamma, const double *eta, int G, uint64_t seed, uint8_t *map_state,
                       double *conf, double *logz, double *marg, uint8_t *draw_state);
/* test hook: positions per launch of the two calls above (0 = by the scratch bound, the default) */
int dsm_assign_debug_set_chunk(int positions);

/* Position-marginal predictive density of a chain (desman_amd/predictive.py): for every used iteration t of the
 * resident gamma and eta traces and every position v of `counts` -- host [N][S][4] int64, or NULL = the count tensor resident in the
 * context, N = its V (the argument N is then ignored) --
 *     logz[t][v] = ln sum over the 4^G joint states of exp L_t(state),
 * L exactly as dsm_assign_tau defines it under (gamma_t, eta_t): cells with a zero count are not evaluated, logarithms by dsm_log,
 * the same sums in the same order (the value is dsm_ctx_assign_tau's logz for that gamma and eta).  The haplotype bases of the
 * position are summed out, so the value does not depend on tau, on the haplotype labels or on whether the position was in the fit;
 * p(x_v | gamma_t, eta_t) = M_v 4^-G exp logz[t][v], M_v the product of the samples' multinomial coefficients (the caller adds
 * ln M_v - G ln 4).  Used iterations: t = it0, it0 + stride, ... below it0 + n_it, numbered as by dsm_ctx_get_tau_at;
 * n_used = ceil(n_it / stride).  Outputs over them, host pointers, any may be NULL:
 *     lppd    [N]          ln((1 / n_used) sum_t exp logz[t][v]), a max-shifted sum in iteration order
 *     mean    [N]          the mean of logz[t][v]
 *     var     [N]          the sample variance, divisor n_used - 1, from a second, centred pass; 0 when n_used = 1
 *     logz_it [n_used][N]  the matrix itself
 * A (t, v) whose every state has L = -inf (exact zeros in eta_t / gamma_t that contradict the counts) has logz = -inf: zero mass in
 * lppd, mean = -inf, var = +inf; every iteration -inf: lppd = -inf.  Nothing is ever NaN for a trace that is finite and >= 0 (what
 * the chain writes; a trace planted by dsm_ctx_debug_set_param_trace is not checked).  n_it = 0 (and N = 0) succeeds and writes
 * nothing.  DSM_ERR_STATE when no update has run; DSM_ERR_ARG for a range outside the trace, stride < 1, N < 0 and counts that
 * dsm_ctx_set_counts would refuse; DSM_ERR_UNSUPPORTED for G > DSM_ASSIGN_MAX_G; S <= DSM_MAX_S.  The work is n_used N 4^G states.
 * Positions are processed in chunks and the iterations of a chunk in launches: device scratch stays below ~100 MB whatever N and n_used
 * are (beyond 4 M used iterations: one position's logz column, 8 n_used bytes).  No floating-point atomics, every sum has one order:
 * the results do not depend on the chunking, on the number of iteration parts or on scheduling, and NULL gives the same bits as a
 * copy of the resident table.  The chain state, both RNG streams, every trace and the MAP record are only read: a chain continues
 * bit for bit after the call.                                                                                                      */
int dsm_ctx_trace_predictive(dsm_ctx *ctx, const int64_t *counts /*[N][S][4] host, or NULL = the resident table, N = its V*/, int N,
                             int it0, int n_it, int stride, double *lppd /*[N]*/, double *mean /*[N]*/, double *var /*[N]*/,
                             double *logz_it /*[n_used][N] or NULL*/);
/* test hooks: positions per chunk of the call above (0 = the library's choice, by the scratch bounds), and the parts a launch cuts
 * its iterations into across workgroups (0 = the library's choice: 1 once positions x partials fill the machine; never more parts
 * than iterations) */
int dsm_pred_debug_set_chunk(int positions);
int dsm_pred_debug_set_parts(int parts);

/* Sampled joint assignment: the model of dsm_assign_tau for every G <= DSM_MAX_G.  Each position runs four
 * private Gibbs chains over its G sites; chain c starts at "every haplotype = base c", runs burn + kept sweeps over g = 0 .. G-1 and
 * keeps the last `kept`.  A step forms the rest mixture afresh, the four candidate totals L_a (the L of the whole state with
 * a_g = a) in fp64, q_a = exp(L_a - max) / sum, and draws by inverse CDF over a = 0..3 with u = word 0 / 2^32 of Philox4x32-10,
 * key = (lo32, hi32) of seed, counter = (lo32 i, hi32 i, sweep, 'ASMP' + c), i = (position index within the call) G + g.  A step whose
 * four candidates are all -inf keeps its base (q = 0) and still spends its uniform.  Host pointers (spread, conf, map_ll and
 * draw_state may be NULL):
 *     map_state [N][G]    digits 0..3 of the best state seen at any step of any chain (ties: lowest chain, earliest step), polished by
 *                         coordinate ascent (arg-max candidate per site; ties keep the base, else the lowest a; at most 64 sweeps)
 *     map_ll    [N]       L of map_state
 *     conf      [N]       share of the 4 * kept end-of-sweep states equal to map_state: a Monte-Carlo estimate of dsm_assign_tau's conf
 *     marg      [N][G][4] mean of q_a over the four chains and the kept sweeps (Rao-Blackwellised marginals)
 *     spread    [N]       max over (g, a) of the largest minus the smallest of the four chains' own means: large where the chains sit
 *                         in different modes (single-site moves do not cross swapped bases of two haplotypes with near-equal gamma)
 *     draw_state[N][G]    chain 0's state after the last sweep
 * A position whose best L is -inf: map_state = draw_state = 0..0, conf = marg = spread = 0, map_ll = -inf.  Nothing is ever NaN.
 * Limits: 1 <= G <= DSM_MAX_G, S <= DSM_MAX_S, burn + kept <= 65536 (DSM_ERR_UNSUPPORTED above); kept >= 1, burn >= 0, counts as
 * dsm_ctx_set_counts takes them, gamma and eta finite and >= 0 (DSM_ERR_ARG otherwise).  Device scratch stays below ~40 MB whatever
 * N is.  The results depend on (seed, position index within the call, counts, gamma, eta, burn, kept) alone -- not on the chunking,
 * on scheduling or on the entry point; two calls give the same bits.                                                             */
int dsm_assign_tau_sampled(int device, const int64_t *counts /*[N][S][4]*/, int N, int S, int G, const double *gamma,
                           const double *eta, uint64_t seed, int burn, int kept, uint8_t *map_state, double *map_ll, double *conf,
                           double *marg, double *spread, uint8_t *draw_state);
int dsm_ctx_assign_tau_sampled(dsm_ctx *ctx, const double *gamma, const double *eta, int G, uint64_t seed, int burn, int kept,
                               uint8_t *map_state, double *map_ll, double *conf, double *marg, double *spread, uint8_t *draw_state);
/* The same call with joint moves of two haplotypes.  pair_every = E >= 0; E = 0 is the call above exactly (the two entry points above
 * are the E = 0 case of the same host code).  With E > 0, sweep t (t = 0 .. burn + kept - 1) is followed by a pair pass when
 * (t + 1) mod E = 0 -- after the sweep's G single-site steps and before its end-of-sweep state is recorded, so conf, draw_state and
 * the kept states see the state after the pass.  The pass visits the pairs (g, h), g < h, in lexicographic order.  A step of (g, h)
 * forms m_a = sum of gamma[s][k] over k not in {g, h} with a_k = a (k in order), the rest mixture as in a single-site step, the
 * sixteen totals L_k, k = 4 a + a' (a the new base of g, a' of h): the L of the whole state, x ln((rest + eta[a][b] gamma[s][g]) +
 * eta[a'][b] gamma[s][h]) over the cells with x > 0, q_k = exp(L_k - max) / (e_0 + ... + e_15 in this order), and draws the pair by
 * inverse CDF over ascending k with u = word 0 / 2^32 of Philox4x32-10, key = (lo32, hi32) of seed, counter = (lo32 j, hi32 j, sweep,
 * 'APAR' + c), j = (position index within the call) G^2 + g G + h.  All sixteen -inf: the pair keeps its bases (q = 0), its uniform
 * is spent.  Best-state tracking looks at all sixteen totals of a pair step: the largest of them (the lowest k among equals), with
 * the state that has this pair, enters like a single-site step's chosen total (ties: lowest chain, earliest step); marg and spread
 * keep their definition: the q of the single-site steps only.  The polish alternates
 * coordinate ascent to its fixed point with one pass of pair ascent over g < h (arg-max of the sixteen totals; a tie with the
 * current pair keeps it, else the lowest k) and repeats while the pair pass changed something.  The coordinate sweeps and pair passes
 * that changed something number at most 64 together: the polish ends with the 64th, whichever kind it is (totals that tie in the
 * model, as under equal gamma columns, are ordered by rounding differently under each pair, so pair ascent alone need not end).
 * map_ll is the total as the last polish step formed it -- with E > 0 the pair form ((rest + g's term) + h's term) of the last
 * pair, which can differ in the last bits from the single-site form that E = 0 reports for the same state.  G = 1 has no pairs.  Limits as above and 0 <= pair_every <= 65536
 * (DSM_ERR_UNSUPPORTED above, DSM_ERR_ARG below 0); the same device scratch.  The results depend on (seed, position index within the
 * call, counts, gamma, eta, burn, kept, pair_every) alone -- not on the chunking, on scheduling or on the entry point.             */
int dsm_assign_tau_sampled_pairs(int device, const int64_t *counts /*[N][S][4]*/, int N, int S, int G, const double *gamma,
                                 const double *eta, uint64_t seed, int burn, int kept, int pair_every, uint8_t *map_state,
                                 double *map_ll, double *conf, double *marg, double *spread, uint8_t *draw_state);
int dsm_ctx_assign_tau_sampled_pairs(dsm_ctx *ctx, const double *gamma, const double *eta, int G, uint64_t seed, int burn, int kept,
                                     int pair_every, uint8_t *map_state, double *map_ll, double *conf, double *marg, double *spread,
                                     uint8_t *draw_state);
/* test hooks: positions per launch of the four calls above (0 = by the scratch bound); the path of a shape, nothing launched --
 * out[5] = instantiation (2 log2 NSL + 1 where gamma is staged in chunks), lanes per (position, chain), sample slots per lane,
 * haplotypes per staged chunk of gamma, positions per workgroup */
int dsm_assign_sampled_debug_set_chunk(int positions);
int dsm_assign_sampled_debug_path(int S, int G, int *out);

/* Abundances of the fitted haplotypes in samples that were not in the fit: tau and eta are held fixed, every
 * sample's gamma row is the maximiser of its own log-likelihood
 *     L(gamma) = sum_{v,b} x_vb ln sum_g gamma_g eta[tau_vg][b]        (cells with x = 0 contribute exactly 0, as in dsm_assign_tau),
 * found by EM from the uniform row: gamma'_g = gamma_g / N sum_{v,b: x > 0} x_vb eta[tau_vg][b] / p_vb, N = the sample's reads.  L is
 * concave in gamma, so the iteration ends in the global maximum; it stops after the step with max_g |gamma' - gamma| < tol or after
 * max_iter steps (tol = 0: exactly max_iter steps).  The whole loop runs on the device, in fp64.  Host pointers:
 *     counts    [V][S][4] int64, as dsm_ctx_set_counts takes them (DSM_ERR_ARG otherwise)
 *     tau       [V][G] int64 DIGITS 0..3 (not the one-hot form; DSM_ERR_ARG on any other value)
 *     gamma     [S][G]   the estimate
 *     loglik    [S]      L(gamma) at the estimate
 *     deviance  [S]      2 (L_sat - L(gamma)),  L_sat = sum x_vb ln(x_vb / n_v),  n_v = sum_b x_vb
 *     iters     [S]      EM steps taken;  converged [S]  1 if the stop test was met, 0 if max_iter ended the loop
 *     lr_absent [S][G]   (may be NULL; computed when presence != 0) 2 (L(gamma) - max L with gamma_g forced to 0): the likelihood-ratio
 *                        statistic of "haplotype g is absent", from G further fits per sample with the same max_iter and tol, each
 *                        started uniform over the other haplotypes.  >= 0; a negative value (rounding, or a restricted fit ahead of
 *                        an unconverged full one) is returned as 0.  G = 1: +inf (no haplotype is left).  A restricted model that
 *                        gives some read probability 0: +inf.  `converged` speaks of the full fit only; a restricted fit that runs
 *                        into max_iter understates its maximum and so overstates the statistic.
 * Degenerate operands: a sample without reads (N = 0) -> the uniform row, loglik 0, deviance 0, iters 0, converged 1, lr_absent 0.
 * A cell with x > 0 whose p is 0 (exact zeros in eta that contradict the counts) -> gamma row 0, loglik -inf, deviance +inf,
 * iters = the steps taken before it was met, converged 0, lr_absent NaN; the other samples are not affected.  As a rule that is at
 * the uniform start (iters 0); it can also come later, when under such an eta a gamma_g underflows to 0 (iters > 0).
 * Limits: 1 <= G <= DSM_MAX_G, V >= 1, max_iter >= 0, tol >= 0 and finite, eta finite and >= 0 (DSM_ERR_ARG otherwise); any S >= 0:
 * the samples are processed in chunks whose device copy of the counts stays below 64 MB (one sample's V x 16 B at the least).  A
 * sample's results are the same bits from run to run, for any chunking, with and without `presence`, and from both entry points:
 * dsm_ctx_fit_gamma fits the S samples of the count tensor resident in the context with the given tau, or -- tau = NULL -- with the
 * context's resident tau (DSM_ERR_STATE without a resident state of G haplotypes); the chain state is not touched.               */
int dsm_fit_gamma(int device, const int64_t *counts /*[V][S][4]*/, int V, int S, int G, const int64_t *tau /*[V][G] digits*/,
                  const double *eta, int max_iter, double tol, int presence, double *gamma, double *loglik, double *deviance,
                  int32_t *iters, int32_t *converged, double *lr_absent);
int dsm_ctx_fit_gamma(dsm_ctx *ctx, int G, const int64_t *tau /*[V][G] digits or NULL*/, const double *eta, int max_iter, double tol,
                      int presence, double *gamma, double *loglik, double *deviance, int32_t *iters, int32_t *converged,
                      double *lr_absent);
/* test hook: samples per launch of the two calls above and of the two interval calls below (0 = by the scratch bound, the default) */
int dsm_abund_debug_set_chunk(int samples);

/* Profile-likelihood intervals of the abundances: tau and eta fixed, gamma_hat [S][G] the fitted rows (input: what
 * dsm_fit_gamma returned).  For haplotype g of a sample the profile log-likelihood is
 *     l_g(c) = max { L(gamma) : gamma_g = c, gamma_h >= 0, sum_h gamma_h = 1 }          (L as above: zero cells contribute 0),
 * concave in c, and the interval is { c in [0, 1] : 2 (Lhat - l_g(c)) <= q }, Lhat = L(gamma_hat) evaluated by the call in the summation
 * order of dsm_fit_gamma's final pass, q the chi-square (1 d.o.f.) quantile of the level (3.841... for 0.95).  Deterministic: no prior, no RNG.
 *   Inner fit at c.  gamma_g is held at c on every pass and never updated; EM over the others: r_h = gamma_h sum_{v,b: x > 0} x_vb
 *     eta[tau_vh][b] / p_vb as in the fit, R = sum_{h != g} r_h added in index order, gamma'_h = (1 - c) r_h / R.  (EM with one component of
 *     known weight: L does not decrease.)  Stop rule of the fit: the step with max_h |gamma' - gamma| < tol, or max_iter steps; then one pass
 *     evaluates l.  R = 0 (the free haplotypes explain no read): the fit ends where it is, as converged.  G = 2 or c = 1: the free part is
 *     determined (gamma_h = 1 - c, resp. 0), l is one evaluation and counts as converged.
 *   Start of an inner fit.  w = the free part (h != g) of the row at which the search's previous inner fit ended, of gamma_hat for the first
 *     one and whenever that part sums to 0 (after c = 1), uniform if gamma_hat's free part sums to 0 too; normalised by its sum F added in
 *     index order; gamma_h = (1 - c) (0.999 (w_h / F) + 0.001 / (G - 1)): a warm start that cannot be trapped at an underflowed zero.
 *   Outer search, one per (haplotype, side).  The bracket is [0, gamma_hat_g] for lo, [gamma_hat_g, 1] for hi; gamma_hat_g is its inside end
 *     (not evaluated).  gamma_hat_g = 0: lo = 0, bit 1, no fit; gamma_hat_g = 1: hi = 1, bit 2, no fit.  Otherwise the far end (c = 0, c = 1)
 *     is tried first: inside the threshold -> lo = 0 (hi = 1) exactly, bit 1 (2).  Else bisection: c = (inside end + outside end) / 2, an
 *     inside c replaces the inside end, any other c the outside end, until |outside - inside| <= ctol (or c equals one of the ends: ctol
 *     below the spacing of doubles); the reported end is the INSIDE end -- itself inside the threshold, and short of the true end by at
 *     most ctol.  The sequence of c depends on nothing but the outcomes, so a search is ~log2(bracket / ctol) + 1 inner fits.
 *   Outside: 2 (Lhat - l) > q; an inner fit that meets p = 0 at a cell with reads (in an EM pass or in the evaluation).
 *     lo, hi  [S][G]   the ends;   flags [S][G]   bit 1: lo is the boundary 0; bit 2: hi is the boundary 1; bit 4: some inner fit of this
 *                      haplotype ended at max_iter (it understates l, the interval comes out too narrow).
 * Degenerate operands: G = 1 -> [1, 1], flags 2.  A sample without reads (N = 0, G > 1) -> [0, 1], flags 3.  A gamma_hat row that is all 0
 * (the fit's result for a sample that eta contradicts) or whose L is -inf -> lo = hi = NaN, flags 0; the other samples are not affected.
 * Limits: those of dsm_fit_gamma, and q > 0 and finite, 0 < ctol < 1, every gamma_hat entry in [0, 1], every row summing to 1 within 1e-9
 * or all 0 (DSM_ERR_ARG otherwise).  Chunks as in dsm_fit_gamma.  A sample's lo, hi and flags are the same bits from run to run, for any
 * chunking and from both entry points (dsm_ctx_fit_gamma_interval: the resident counts, tau given or -- NULL -- resident).              */
int dsm_fit_gamma_interval(int device, const int64_t *counts /*[V][S][4]*/, int V, int S, int G, const int64_t *tau /*[V][G] digits*/,
                           const double *eta, const double *gamma_hat /*[S][G]*/, double q, int max_iter, double tol, double ctol,
                           double *lo, double *hi, int32_t *flags);
int dsm_ctx_fit_gamma_interval(dsm_ctx *ctx, int G, const int64_t *tau /*[V][G] digits or NULL*/, const double *eta,
                               const double *gamma_hat, double q, int max_iter, double tol, double ctol, double *lo, double *hi,
                               int32_t *flags);

/* The error matrix of samples that were not in the fit, estimated with their abundances: tau is held fixed; the call
 * fits gamma [S][G], one row per sample, and ONE eta [4][4] ([true][observed], rows summing to 1) shared by all samples of the call, by
 * plain EM on
 *     L(gamma, eta) = sum_s sum_{v,b: x > 0} x_svb ln p_svb,   p_svb = sum_a c_sva eta[a][b],   c_sva = sum_{g: tau_vg = a} gamma_sg
 * (cells with x = 0 contribute exactly 0).  One step, from a single E-step at the current (gamma, eta):
 *     q_svb = x_svb / p_svb where x > 0, else 0;        w_sva = sum_b q_svb eta[a][b];
 *     gamma'_sg = gamma_sg / N_s sum_v w_{s,v,tau_vg}                                  (the step of dsm_fit_gamma),
 *     M[a][b] = eta[a][b] sum_s sum_v c_sva q_svb   (the samples added in index order),  eta'[a][b] = M[a][b] / sum_b M[a][b]  (b in order).
 *   A row a with sum_b M[a][b] = 0 (no haplotype of positive abundance carries base a anywhere) keeps its previous values; bit a of
 *   dead_rows is set if that happened in any step of the call.
 *   Start: every gamma row uniform, eta = eta0 (the run's Eta_star.csv).  Stop: the step with max(max |gamma' - gamma|, max |eta' - eta|) < tol,
 *   or max_iter steps (tol = 0: exactly max_iter steps; max_iter = 0: eta0 and the uniform rows).  After the stop one pass evaluates L
 *   per sample at the returned (gamma, eta), in the summation order of dsm_fit_gamma's final pass.  L does not decrease along the steps.
 *     gamma [S][G], eta [16]   the estimate;     loglik [S], deviance [S]   as in dsm_fit_gamma, at the estimate
 *     loglik0 [S]   the log-likelihood of the fit with eta held at eta0: what dsm_fit_gamma returns in loglik for the same counts, tau,
 *                   eta = eta0, max_iter and tol (it is that call, the same bits)
 *     iters, converged, dead_rows   one value each per call: steps taken; 1 if the stop test was met; the bit mask above
 *     lr_eta        2 (sum_s loglik - sum_s loglik0), a negative value returned as 0: how much better the re-estimated eta explains the
 *                   samples.  A likelihood-ratio statistic of "eta0 holds for these samples" on at most 12 free parameters, with a
 *                   NOMINAL chi-square(12) reference: exact zeros in eta0 (EM keeps them) and dead rows lower the degrees of freedom,
 *                   and gamma is re-fitted under both hypotheses.  A fit that max_iter ended early understates it.
 * Degenerate operands: a sample without reads contributes nothing to M, keeps the start row and has loglik 0, deviance 0.  A cell with
 * reads and p = 0 in any pass (exact zeros in eta0 that the counts contradict; at the uniform start as a rule, later when a gamma_sg
 * underflows to 0) kills the whole call's fit, because eta is shared: every gamma row 0, every loglik -inf, every deviance +inf, converged
 * 0, iters = the steps completed before, eta returned as eta0, lr_eta NaN; loglik0 is still returned per sample.  G = 1 is valid: the
 * gamma step leaves 1 (to rounding, as in dsm_fit_gamma) and only eta moves.
 * Limits: those of dsm_fit_gamma, S >= 1, and every row of eta0 sums to 1 within 1e-9 (DSM_ERR_ARG otherwise).  Every step reads every
 * sample, so -- unlike dsm_fit_gamma -- the sample-major copy of ALL the counts is staged at once: V x S x 16 B above 1 GiB is
 * DSM_ERR_UNSUPPORTED (checked before anything is allocated); dsm_abund_debug_set_chunk does not apply to the joint fit (it does to the
 * loglik0 fit, whose results do not depend on it).  The host enqueues the steps in batches of 32 and reads the device's stop word
 * between batches; a step launched after the stop changes nothing, so the results do not depend on the batch size.  No atomics, every
 * sum has one order: the results are the same bits from run to run and from both entry points (dsm_ctx_fit_gamma_eta: the resident
 * counts, tau given or -- NULL -- resident; the chain state is not touched).                                                          */
int dsm_fit_gamma_eta(int device, const int64_t *counts /*[V][S][4]*/, int V, int S, int G, const int64_t *tau /*[V][G] digits*/,
                      const double *eta0, int max_iter, double tol, double *gamma, double *eta, double *loglik, double *loglik0,
                      double *deviance, int32_t *iters, int32_t *converged, int32_t *dead_rows, double *lr_eta);
int dsm_ctx_fit_gamma_eta(dsm_ctx *ctx, int G, const int64_t *tau /*[V][G] digits or NULL*/, const double *eta0, int max_iter, double tol,
                          double *gamma, double *eta, double *loglik, double *loglik0, double *deviance, int32_t *iters,
                          int32_t *converged, int32_t *dead_rows, double *lr_eta);
/* test hooks: steps per batch of the two calls above (0 = the default, 32); the bound of their sample-major copy in bytes (0 = 1 GiB) */
int dsm_abund_debug_set_eta_batch(int steps);
int dsm_abund_debug_set_eta_stage_max(long long bytes);

/* ------------------------------------------------------------------------ */
/* f4: accessory-gene assignment (desman/Eta_Sampler.py, desman/GeneAssign.py) */
/* C genes, gene c owns the rows gene_off[c]..gene_off[c+1]-1 of one           */
/* concatenated [Vtot][S][4] count tensor; eta[c][g] in {0..max_eta-1} is the  */
/* copy number of gene c in haplotype g.  All tau sweeps are the A1 sweep with */
/* the gene's masked, re-normalised gamma (Eta_Sampler.maskGamma :147-157).    */
/* ------------------------------------------------------------------------ */
typedef struct dsm_genes dsm_genes;
#define DSM_MAX_ETA 8

int dsm_genes_create(dsm_genes **out, int device);
int dsm_genes_destroy(dsm_genes *gs);
/* variants may be NULL when Vtot == 0 (GeneAssign without -v).  cov [C][S].   */
int dsm_genes_set_data(dsm_genes *gs, const int64_t *variants, int Vtot, int S, int C,
                       const int32_t *gene_off /*[C+1]*/, const double *cov);
/* gamma [S][G] (unmasked), epsilon [4][4], delta [G][S] (Eta_Sampler.__init__:47),
 * eta_log_prior [max_eta] (:139-145); cov_const[c] = -sum_s lgamma(cov+1) and
 * mult_const[c] = sum_{v,s} (lgamma(n+1) - sum_b lgamma(x_b+1)) are the data-only
 * constants of log_Poisson (:34-39) and log_multinomial_pdf (:27-32).         */
int dsm_genes_set_model(dsm_genes *gs, const double *gamma, const double *epsilon,
                        const double *delta, int G, int max_eta, const double *eta_log_prior,
                        const double *cov_const, const double *mult_const);
/* eta [C][G]; tau one-hot [Vtot][G][4] (either may be NULL = keep)            */
int dsm_genes_set_state(dsm_genes *gs, const int32_t *eta, const int64_t *tau);
int dsm_genes_get_state(dsm_genes *gs, int32_t *eta, int64_t *tau);
/* GSL-compatible MT19937 stream of the tau draws (shared semantics with dsm_setRNG) and the
 * Philox key of the batched sampler                                           */
int dsm_genes_seed(dsm_genes *gs, unsigned long mt_seed, uint64_t ctr_seed);
/* this object holds genes gene_base.. of a larger set sharded over several objects / ranks: the counter-based
 * draws are keyed by (global gene index, row within the gene), so results do not depend on the sharding   */
int dsm_genes_set_gene_base(dsm_genes *gs, int gene_base);
int dsm_genes_get_mt_state(dsm_genes *gs, uint32_t *state625);
int dsm_genes_set_mt_state(dsm_genes *gs, const uint32_t *state625);

/* Init_NMFT.factorize_tau per gene with the masked gamma (Eta_Sampler.__init__:128-134,
 * calcTauStar:419-426): tau_init [Vtot][4][G] f64 holds each gene's random start
 * (Init_NMFT.random_initialize_tau), genes without variants or with an all-zero mask row are
 * skipped; the arg-max (get_tau) becomes the resident tau.  n_iter [C] (optional).           */
int dsm_genes_nmft_tau(dsm_genes *gs, const int32_t *eta_mask /*[C][G] or NULL = resident*/,
                       const double *tau_init, int max_iter, double min_change, int32_t *n_iter);
/* Eta_Sampler.sampleTauC over all genes with variants and a non-empty mask, in gene order on
 * the GSL stream (:135, calcTauStar:437): nchange [C], logvar [C] = sum x log p after the
 * sweep, v_ll [Vtot] the same per variant (any may be NULL).  sweep = 0: evaluate only; 1: the GSL
 * stream; 2: counter-based draws (sharding-invariant).                                        */
int dsm_genes_sweep_all(dsm_genes *gs, const int32_t *eta_mask, int sweep, int32_t *nchange,
                        double *logvar, double *v_ll);
/* reference-order single step (Eta_Sampler.update:226-262): the two candidate sweeps
 * eta[c][g] = 0 / 1 of gene c (GSL stream: candidate 0 first, only if it keeps a haplotype),
 * logvar[2], swept[2]; then dsm_genes_step_choose commits the value drawn by the caller.      */
int dsm_genes_step_candidates(dsm_genes *gs, int c, int g, double *logvar, int *swept);
int dsm_genes_step_choose(dsm_genes *gs, int c, int g, int eta_value);
/* batched Gibbs: n_iter iterations of Eta_Sampler.update for all genes at once with
 * counter-based draws; eta_store [n_iter][C][G], gene_ll_trace [n_iter][C] (optional).
 * u_tau_ext [n_iter][G][2][Vtot*G] raw 32-bit words and u_eta_ext [n_iter][C][G] uniforms
 * replace the Philox draws when given (parity tests).  reset_star != 0: star := entry state
 * (update:216-219).                                                                          */
int dsm_genes_update(dsm_genes *gs, int n_iter, int reset_star, int32_t *eta_store,
                     double *gene_ll_trace, const uint32_t *u_tau_ext, const double *u_eta_ext);
/* Eta_Sampler.logLikelihood (:182-202) per gene for the resident state                        */
int dsm_genes_loglik(dsm_genes *gs, double *gene_ll);
int dsm_genes_get_star(dsm_genes *gs, int32_t *eta_star, double *gene_llstar);
int dsm_genes_set_star(dsm_genes *gs, const int32_t *eta_star, const double *gene_llstar);
/* test hook (read only): the sweep tiling chosen for the resident data and model -- lanes per variant row, samples
 * per lane, lane groups per workgroup, dynamic LDS of a sweep launch.  Valid after set_data and set_model, DSM_ERR_ARG
 * otherwise; any pointer may be NULL.                                                                                */
int dsm_genes_debug_tile(const dsm_genes *gs, int *lpv, int *nsl, int *groups_per_block, size_t *lds_bytes);

/* GeneAssign.KLAssign.factorize (GeneAssign.py:85-120): eta [C][G] in/out (start values drawn by
 * the caller), cov [C][S], delta [S][G]; *n_done updates, *div final divergence.               */
int dsm_kl_assign(int device, const double *cov, const double *delta, double *eta, int C, int S,
                  int G, int max_iter, double min_change, int *n_done, double *div);

/* per-kernel HIP-event timing on the context's stream (bench/roofline).      */
#define DSM_K_STATS    0
#define DSM_K_DIRICH   1
#define DSM_K_TAU      2
#define DSM_K_FINAL    3
#define DSM_K_MT       4
#define DSM_K_NMFT_A   5
#define DSM_K_NMFT_G   6
#define DSM_K_NMFT_B   7
#define DSM_K_STATS2   8         /* stage 2 of the aggregated mu/E pass       */
#define DSM_K_STATSBIG 9         /* deferred stage-1 items (stats_big_kernel) */
#define DSM_K_STATSPAT 10        /* spec 4: word table + per-word count sums ahead of stage 1 (pat_rep_kernel, pat_agg_kernel) */
#define DSM_K_COUNT    11
/* evidence for the screening pass of the tau sweep: wavefront-steps run / left to the fp64 code, over the sweeps
   of dsm_ctx_gibbs_update and dsm_ctx_update_tau so far.  mode 1 = read and zero, 0 = read */
int dsm_ctx_sweep_stats(dsm_ctx *ctx, uint64_t *steps, uint64_t *exact_steps, int mode);
/* test hook: out[i] = the hardware log2 (v_log_f32) of in[i], the logarithm of the screening pass */
int dsm_ctx_debug_log2f(dsm_ctx *ctx, const float *in, float *out, size_t n);
/* Frees what the library keeps per process and device beyond the life of a context: the MT19937 jump tables of the parallel generator
   (2 x 50 MB per device, built by the first fill of >= 6 x 131 040 words: 2 x 2.2 ms).  For long-lived processes and for several rank processes sharing one GPU; nothing may be in flight.  Returns 0. */
int dsm_release_device_caches(void);
/* test hook: out[i] = a[i] / b[i] as the NMFT update divides (kernels_nmft.hip): kind 0 = fdiv_ext (any a, b >= 0: operands brought to
   within 2^+-512 of one by exact powers of two), 1 = fdiv_lo (a in (0, 1]), 2 = fdiv (operands far from the ends of the exponent range).
   Runs on the current device's default stream. */
int dsm_debug_fdiv(int kind, const double *a, const double *b, double *out, int n);
/* gamma / control step of an NMFT update (Init_NMFT.py:163-168 and the stop test :106): -1 = by size (default): one launch together
   with the reduction while the update kernel leaves <= 128 workgroup partials; above that at the start of the update kernel itself on
   the matrix-core path (S <= 128, G <= 16: an update is two launches), else a launch of its own (three); 0 = always a launch of its own;
   1 = always with the reduction; 3 = in the update kernel wherever that path runs.  The factors, update counts and objective traces do
   not depend on it (tests/test_gpu_fullsize.py asserts bit-equality). */
int dsm_ctx_set_nmft_fused(dsm_ctx *ctx, int mode);
/* dsm_nmft_factorize as ONE persistent launch (resident workgroups, in-kernel grid barriers, tau rows kept in LDS) where the
   table fits the machine (S <= 64, G <= 12, V <= 48 x compute units; factorize_tau also S <= 96 with V <= 16 x compute units): -1 / 1 = wherever it applies (default), 0 = never (the
   three-launch loop).  Same stopping rule, update counts, objective trace and factors, bit for bit: every path sums the workgroup
   partials in one canonical order (kernels_nmft.hip: nmft_sum_partials; tests/test_gpu_fullsize.py asserts the equality). */
int dsm_ctx_set_nmft_persist(dsm_ctx *ctx, int mode);
/* on = 0: every step of the tau sweep in fp64 (A/B switch).  Same law, and the same draws except in near-ties: after a screened
   step the current base's log-probability is evaluated afresh, an all-fp64 sweep re-uses the previous step's value (equal up to
   the last bits; a different draw needs the uniform within ~1e-13 of a CDF edge -- none in the ~1e7 draws of the parity tests) */
int dsm_ctx_set_tau_screen(dsm_ctx *ctx, int on);
/* the tau sweep of dsm_ctx_gibbs_update has a second instantiation with one more screen, for the steps of haplotypes that are rare in
   every sample (max_s gamma_sg <= 0.01: the spare haplotypes of a chain with more haplotypes than the table has strains -- their steps
   are near-ties that only the DIFFERENCES of the candidates can settle short of fp64).  mode -1 (default): a call runs it while the
   chain's abundances hold such a haplotype (as set by dsm_ctx_set_state / left by the previous call, and looked at every 64 iterations); 0 = never; 1 = always.  The draws are those of the fp64 code
   either way (tests/test_gpu_parity.py); not used for batches and sharded chains. */
int dsm_ctx_set_tau_neartie(dsm_ctx *ctx, int mode);
/* stage 1 of the aggregated mu/E pass hands a few items (deep cells, burn-in states, chains that fit badly) to lists; a launch of its
   own (stats_big_kernel) draws them, and where it was left out the launch that runs stage 2 does, the same draws bit for bit.  For
   the full chain with G < 10 under specification 2 / 3, not sharded, the launch is a choice: mode -1 (default) = launched while the
   lists were last seen non-empty (looked at when a Gibbs call ends and every 64 iterations inside one; the first call after
   dsm_ctx_set_state / dsm_ctx_set_counts launches), 0 = never, 1 = always.  DESMAN_HIP_BIG_LAUNCH=0|1 chooses for every context
   that has no mode of its own.  Everywhere else the launch is unconditional. */
int dsm_ctx_set_big_launch(dsm_ctx *ctx, int mode);
/* test hook: how many words of the deferred lists' counters are non-zero now (0 between passes), and the device's running count of
   lists found non-empty */
int dsm_ctx_debug_big_lists(dsm_ctx *ctx, int *nonzero, uint32_t *seen);
/* workgroups one tau sweep of the resident shape launches, and how many of them the device holds at once (occupancy of the
   kernel x compute units): launched / resident = rounds of the launch, the partly filled last one being its tail */
int dsm_ctx_tau_launch_info(dsm_ctx *ctx, int *launched, int *resident);
/* ---- one chain over several GPUs, sharded by positions (only worthwhile when there are fewer chains than
 * GPUs, V >~ 50k).  Each process / GPU holds a contiguous slice of the positions in its own context (dsm_ctx_set_counts with the
 * slice, dsm_ctx_set_state with the slice of tau and the shared gamma / eta, the same dsm_ctx_seed ctr_seed everywhere,
 * dsm_ctx_set_tau_rng(DSM_RNG_PHILOX)) and calls dsm_ctx_gibbs_update_sharded with its offset.  Once per iteration the library
 * hands `exchange` its subset table (uint32, to be SUMMED element-wise over the shards, in place) and an 18-double vector
 * (likewise); n_tab = 0 means the vector only.  The callback is the caller's all-reduce (RCCL: desman_amd/vshard.py); it is
 * called with the context's stream drained and must return 0 once the sums are in place, non-zero to abort.  Afterwards
 * gamma / eta / every trace are identical on all shards and equal the unsharded chain's (ll / lp to rounding), and each
 * shard's tau is the unsharded chain's slice: the counter-based streams are keyed by global indices.                       */
/* checkpoint / resume: besides (tau, gamma, eta) and the MT19937 state (dsm_ctx_get_state / dsm_ctx_get_mt_state)
 * a chain's position in its counter-based streams is the stream key and the number of iterations drawn so far.  A fresh context
 * given the same counts, state, MT19937 state, priors, tau RNG and these two words continues the chain bit for bit.          */
int dsm_ctx_get_counters(dsm_ctx *ctx, uint64_t *ctr_seed, uint32_t *iter_ctr);
int dsm_ctx_set_counters(dsm_ctx *ctx, uint64_t ctr_seed, uint32_t iter_ctr);
/* ... and the tau sweep's screening state: two words (one per launch parity) = sweeps still to run without the fp32 screening pass.
 * Which steps are screened cannot change a draw outside a ~1e-13 near-tie; carrying the words makes the resumed
 * chain take the same screening decisions as the uninterrupted one, so "bit for bit" holds without that caveat.                  */
int dsm_ctx_get_screen_state(dsm_ctx *ctx, uint32_t *out2);
int dsm_ctx_set_screen_state(dsm_ctx *ctx, const uint32_t *in2);
typedef int (*dsm_exchange_fn)(void *user, uint32_t *dev_tab, size_t n_tab, double *dev_vec, size_t n_vec);
int dsm_ctx_gibbs_update_sharded(dsm_ctx *ctx, int n_iter, int v_offset, int v_total, dsm_exchange_fn exchange, void *user);
/* ---- RCCL (xGMI) inside the library: one communicator per process / GPU, no torch.  librccl is dlopen()ed on first use
 * (DESMAN_HIP_RCCL names another copy).  Replaces the reference's "gather" -- `cat *\/fit.txt` over per-chain directories,
 * complete_example/README.md:626-627 after scripts/runDesman.sh:15-21 -- and carries the per-iteration exchange of a sharded
 * chain.  Bootstrap: rank 0 calls dsm_comm_unique_id and hands the 128 bytes to the other ranks by any
 * means (desman_amd/comm.py: a TCP socket on MASTER_ADDR); then EVERY rank calls dsm_comm_create (collective).              */
typedef struct dsm_comm dsm_comm;
int dsm_comm_unique_id(void *id128);
int dsm_comm_create(dsm_comm **out, const void *id128, int rank, int world, int device);
int dsm_comm_destroy(dsm_comm *comm);
int dsm_comm_rank(const dsm_comm *comm);
int dsm_comm_world(const dsm_comm *comm);
/* recv[world][n] <- every rank's send[n] (host buffers): the chain scheduler's one exchange, a fit record per chain */
int dsm_comm_allgather_f64(dsm_comm *comm, const double *send, double *recv, size_t n);
/* data[n] <- sum (op 0) or maximum (op 1) over the ranks, in place (host buffer); dsm_comm_barrier = the same with n = 0 */
int dsm_comm_allreduce_f64(dsm_comm *comm, double *data, size_t n, int op);
int dsm_comm_barrier(dsm_comm *comm);
/* dsm_ctx_gibbs_update_sharded with the exchange done by the library itself: the two all-reduces are ENQUEUED on the context's
 * stream between stage 1 and the Dirichlet launch (one grouped RCCL call), no host synchronisation, no callback.  The
 * communicator must live on the context's device; every rank of it must make the call (same n_iter, same v_total).          */
int dsm_ctx_gibbs_update_sharded_comm(dsm_ctx *ctx, int n_iter, int v_offset, int v_total, dsm_comm *comm);
/* plain device <-> host copies of the exchange buffers (host-side reductions, tests) */
int dsm_device_read(int device, const void *dev, void *host, size_t bytes);
int dsm_device_write(int device, void *dev, const void *host, size_t bytes);
int dsm_ctx_set_timing(dsm_ctx *ctx, int on);
int dsm_ctx_get_timing(dsm_ctx *ctx, double *ms_total /*[DSM_K_COUNT]*/,
                       int64_t *launches /*[DSM_K_COUNT]*/);
const char *dsm_kernel_name(int k);

#ifdef __cplusplus
}
#endif
#endif /* DESMAN_HIP_H */
