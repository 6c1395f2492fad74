/*
 * beer_hip.h -- C ABI of the MI355X (gfx950) implementation of beer's
 * variational-Bayes hot path.
 *
 * The reference (beer-asr/beer) is pure Python on torch and has no FFI of its
 * own; the seam is its Python `Model` protocol.  Every
 * entry point below names the reference function it replaces (paths relative
 * to the reference root).  The Python host layer `beer_amd` binds these with
 * ctypes (beer_amd/_hip.py); INTEGRATION.md shows the stub a maintainer of
 * the reference would add to call them from beer itself.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch is only
 *     the allocator) unless the name ends in `_h` (host);
 *   - `dtype`: BEER_F32 / BEER_F64 is the element type of every `void*`
 *     floating-point buffer of the call; `double*` buffers are always fp64
 *     (cross-frame accumulators are fp64 whatever the model dtype is);
 *   - matrices are row-major and dense, no padding;
 *   - `stream` is a hipStream_t (0 = default stream); calls are asynchronous,
 *     never synchronise, never allocate device memory, keep no state between
 *     calls and are re-entrant per stream;
 *   - return value: 0 on success, BEER_EINVAL for a bad argument, or
 *     -(hipError_t) if a launch failed.  Nothing throws.
 *   - `cov`: BEER_FULL / BEER_DIAG / BEER_ISO selects the layout of the
 *     sufficient statistics, Q = D*D+D+2 | 2D+2 | D+3
 *     (beer/dists/normalwishart.py:30-38, normalgamma.py:20-27,
 *     isonormalgamma.py:21-30).
 */
#ifndef BEER_HIP_H
#define BEER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEER_F32 0
#define BEER_F64 1
#define BEER_I16 2   /* audio samples only (beer_features_*) */

#define BEER_FULL 0
#define BEER_DIAG 1
#define BEER_ISO 2

#define BEER_OK 0
#define BEER_EINVAL (-100000)

/* Library / device probes (no reference counterpart). */
int beer_hip_version(void);
int beer_hip_device_count(void);

/* Tuning options (no reference counterpart): process-wide launch parameters of the
 * matrix-core kernels, for measurements and for the tests that pin the defaults.
 * They change how the work is cut into launches and chains, never what is computed;
 * the defaults are what the parity suite validates.  A value outside the range is
 * refused with BEER_EINVAL and leaves the option as it was. */
#define BEER_OPT_AX_MAXFRAMES 0  /* frames a workgroup of beer_normal_accumulate_packed sums in
                                  * float32 before its partial sums meet in fp64 (the matrix
                                  * core truncates its accumulator: bias ~ 8e-11 per frame of
                                  * chain on same-sign sums).  Default 4096, range 64 .. 2^20. */
#define BEER_OPT_ACCF_ROUNDS 1   /* workgroup rounds per CU of beer_mixtureset_accumulate_fused.
                                  * Default 6, range 1 .. 64. */
#define BEER_OPT_ACCFI_WAVES 2   /* waves per workgroup of the fused accumulation over a frame
                                  * image: 4 (two workgroups per CU: one flushes its partial
                                  * sums while the other multiplies) or 8.  Default 4. */
#define BEER_OPT_LNFI 3          /* 1: beer_mixtureset_lognorm_image keeps a chunk's packed
                                  * parameters in LDS and walks blocks of frames (lnfi_kernel);
                                  * 0: one tile per wave, parameters streamed from L2.  Default 1. */
#define BEER_OPT_FB_LOG 4        /* 1: the one-wave-per-utterance forward-backward runs EVERY
                                  * utterance in log space (the kernel that otherwise only
                                  * redoes utterances whose dynamic range exceeds the
                                  * scaled-probability recursion; beer/graph.py:270-326 is
                                  * log-space throughout).  Default 0. */
#define BEER_OPT_K1_LDS 5        /* 1: the packed full-covariance E-step stages the packed
                                  * parameters of a k-step through LDS once per workgroup (DMA,
                                  * ring of two half k-steps) instead of streaming them from L2
                                  * per wave; 0: per wave.  Same products in the same order:
                                  * bit-identical results.  Default 1. */
#define BEER_OPT_COUNT 6
int beer_hip_set_option(int option, int value);
int beer_hip_get_option(int option);   /* the value, or BEER_EINVAL for an unknown option */

/* How float32 models multiply on the matrix cores is chosen PER CALL (float64
 * models always use the exact fp64 MFMA): the `dtype` argument of
 * beer_mixtureset_estep is BEER_F32 for the default arithmetic, "bf16x3" -- every
 * fp32 operand is held EXACTLY as three bf16 pieces (3 x 8 significand bits = the
 * 24 of fp32, fp32's exponent range: no scaling, no range restrictions) and every
 * product is the six leading partial products on v_mfma_f32_16x16x32_bf16, fp32
 * accumulation: operands and accumulation are fp32's own, what a product drops is
 * <= 2^-23 of it (2^-25 typically, no systematic sign), at 2.7x the rate of the
 * fp32 pipe -- or BEER_F32 | BEER_EXACT for v_mfma_f32_16x16x4_f32, bitwise an
 * fmaf chain.  The packed hand-over calls below (beer_mixture_estep_packed, ...)
 * are bf16x3 by construction.  The library keeps no mode. */
#define BEER_EXACT 0x10

/* ------------------------------------------------------------------------
 * Exponential-family parameter kernels (once per VB iteration, K = number of
 * distributions in the set, D = feature dimension).
 * ---------------------------------------------------------------------- */

/* E_q[T(theta)], the "natural form" every E-step consumes.
 * Replaces NormalWishart.expected_sufficient_statistics
 * (beer/dists/normalwishart.py:170-210) reached through
 * ConjugateBayesianParameter.natural_form (beer/models/parameters.py:131-132).
 * mean [K,D], scale [K], scale_matrix [K,D,D], dof [K] -> out [K, D*D+D+2]. */
int beer_nw_expected_stats(int dtype, int K, int D, const void* mean,
                           const void* scale, const void* scale_matrix,
                           const void* dof, void* out, void* stream);
/* The two calls around this comment in one launch (they share the
 * factorisation of the scale matrix, and a VB iteration needs both: E[T] for
 * the E-step, the log-normaliser for the KL term): out [K, D*D+D+2],
 * log_norm [K]. */
int beer_nw_expected_stats_log_norm(int dtype, int K, int D, const void* mean,
                                    const void* scale, const void* scale_matrix,
                                    const void* dof, void* out, void* log_norm,
                                    void* stream);
/* NormalWishart.log_norm (normalwishart.py:219-236) -> out [K]. */
int beer_nw_log_norm(int dtype, int K, int D, const void* mean,
                     const void* scale, const void* scale_matrix,
                     const void* dof, void* out, void* stream);
/* NormalWishart.natural_parameters (normalwishart.py:242-269) -> [K,Q]. */
int beer_nw_natural(int dtype, int K, int D, const void* mean,
                    const void* scale, const void* scale_matrix,
                    const void* dof, void* out, void* stream);
/* NormalWishartStdParams.from_natural_parameters (normalwishart.py:110-141). */
int beer_nw_from_natural(int dtype, int K, int D, const void* eta, void* mean,
                         void* scale, void* scale_matrix, void* dof,
                         void* stream);

/* The M-step of a Normal-Wishart posterior in one launch:
 * from_natural_parameters (normalwishart.py:110-141) and, from the same
 * elimination, what the next iteration asks of the new posterior: `exp_stats`
 * [K, D*D+D+2] (expected_sufficient_statistics, normalwishart.py:170-210),
 * `log_norm` [K] (normalwishart.py:219-236) and, when `moments` is not NULL, the
 * moments of its expected Gaussian, [K, D + D*D] = (mean, E[Lambda]^-1 = W^-1 / nu).
 * One factorisation where the three separate calls make two and an inverse. */
int beer_nw_update(int dtype, int K, int D, const void* eta, void* mean, void* scale,
                   void* scale_matrix, void* dof, void* exp_stats, void* log_norm,
                   void* moments, void* stream);

/* NormalGamma (diagonal covariance), beer/dists/normalgamma.py:118-146,
 * 151-157, 163-180, 77-94.  mean [K,D], scale [K], shape [K], rates [K,D]. */
int beer_ng_expected_stats(int dtype, int K, int D, const void* mean,
                           const void* scale, const void* shape,
                           const void* rates, void* out, void* stream);
int beer_ng_log_norm(int dtype, int K, int D, const void* mean,
                     const void* scale, const void* shape, const void* rates,
                     void* out, void* stream);
int beer_ng_natural(int dtype, int K, int D, const void* mean,
                    const void* scale, const void* shape, const void* rates,
                    void* out, void* stream);
int beer_ng_from_natural(int dtype, int K, int D, const void* eta, void* mean,
                         void* scale, void* shape, void* rates, void* stream);

/* IsotropicNormalGamma, beer/dists/isonormalgamma.py:119-157, 163-168,
 * 174-192, 78-95.  mean [K,D], scale [K], shape [K], rate [K]. */
int beer_ing_expected_stats(int dtype, int K, int D, const void* mean,
                            const void* scale, const void* shape,
                            const void* rate, void* out, void* stream);
int beer_ing_log_norm(int dtype, int K, int D, const void* mean,
                      const void* scale, const void* shape, const void* rate,
                      void* out, void* stream);
int beer_ing_natural(int dtype, int K, int D, const void* mean,
                     const void* scale, const void* shape, const void* rate,
                     void* out, void* stream);
int beer_ing_from_natural(int dtype, int K, int D, const void* eta, void* mean,
                          void* scale, void* shape, void* rate, void* stream);

/* Dirichlet (set of S pdfs over G categories), beer/dists/dirichlet.py:
 * 106-128 (E[T]), 135-138 (log_norm), 144-159 (natural), 71-81 (from). */
int beer_dirichlet_expected_stats(int dtype, int S, int G, const void* conc,
                                  void* out, void* stream);
int beer_dirichlet_log_norm(int dtype, int S, int G, const void* conc,
                            void* out, void* stream);
int beer_dirichlet_natural(int dtype, int S, int G, const void* conc,
                           void* out, void* stream);
int beer_dirichlet_from_natural(int dtype, int S, int G, const void* eta,
                                void* conc, void* stream);
/* Truncated stick-breaking categorical (any truncation P; device, one workgroup: up to
 * 1024 sticks ranked in LDS, beyond that on the global arrays).
 * beer_sb_transform_stats: SBCategorical._transform_stats
 * (beer/models/categorical.py:106-118) -- the sticks are ordered by decreasing
 * count (stable), `ordering[r]` = category of stick r, and the counts [P] become
 * the Dirichlet statistics of the sticks [P,2] = (count_i, count_i + sum of the
 * counts ordered after i), stored in the categories' own order.
 * beer_sb_log_weights: SBCategorical._log_prob + the re-ordering of
 * expected_log_likelihood (categorical.py:120-131, 157-159) -- E[ln pi_i] =
 * E[ln v_i] + sum over the sticks before i of E[ln(1 - v)], [P] in the categories'
 * order; `log_1_v_sum` (nullable) = sum_i E[ln(1 - v_i)], the statistic of the
 * Gamma hyper-prior (categorical.py:203-209). */
int beer_sb_transform_stats(int dtype, int P, const void* counts, int64_t* ordering,
                            void* stats, void* stream);
int beer_sb_log_weights(int dtype, int P, const void* conc, const int64_t* ordering,
                        void* log_w, void* log_1_v_sum, void* stream);
/* n stick-breaking rows of K sticks that share ONE ordering: the rows of a hierarchical
 * Dirichlet process (SBCategoricalSet, beer/models/categoricalset.py:167-307), which follow
 * their root's ordering and are never re-sorted.  K <= 1024; one workgroup per row.
 * beer_sb_set_log_weights: conc [n K, 2] -> log_w [n, K], E[ln pi] of every row in the
 * categories' order (categoricalset.py:264-281).
 * beer_sb_set_transform_stats: counts [n, K] -> stats [n K, 2] = (count_i, count_i + the
 * counts of the sticks after i), categories' order (categoricalset.py:215-224). */
int beer_sb_set_log_weights(int dtype, int n, int K, const void* conc, const int64_t* ordering,
                            void* log_w, void* stream);
int beer_sb_set_transform_stats(int dtype, int n, int K, const void* counts,
                                const int64_t* ordering, void* stats, void* stream);
/* E[ln pi] of S categoricals: the `eye -> sufficient_statistics -> stats @
 * E[T]` sequence of Mixture._log_weights (beer/models/mixture.py:45-48) and
 * MixtureSet._log_weights (mixtureset.py:64-67) -> out [S,G]. */
int beer_dirichlet_log_weights(int dtype, int S, int G, const void* conc,
                               void* out, void* stream);

/* Gamma (n independent pdfs), beer/dists/gamma.py:112-124, 129-131,
 * 137-140, 68-77.  shape [n], rate [n]; E[T] / natural are [2n]. */
int beer_gamma_expected_stats(int dtype, int n, const void* shape,
                              const void* rate, void* out, void* stream);
int beer_gamma_log_norm(int dtype, int n, const void* shape, const void* rate,
                        void* out /*[1]*/, void* stream);
int beer_gamma_natural(int dtype, int n, const void* shape, const void* rate,
                       void* out, void* stream);
int beer_gamma_from_natural(int dtype, int n, const void* eta, void* shape,
                            void* rate, void* stream);

/* KL(q || p) of K same-family members from their expected statistics,
 * natural parameters and log-normalisers: beer/dists/basedist.py:243-263.
 * out [K]. */
int beer_kl_div(int dtype, int K, int Q, const void* exp_stats_q,
                const void* eta_q, const void* eta_p, const void* lnorm_q,
                const void* lnorm_p, void* out, void* stream);

/* eta <- eta_q + lrate * (eta_p + stats - eta_q): the body of
 * ConjugateBayesianParameter.natural_grad_update
 * (beer/models/parameters.py:134-141).  n elements. */
int beer_natural_grad_step(int dtype, int64_t n, const void* eta_prior,
                           const void* eta_post, const void* stats,
                           double lrate, void* out, void* stream);

/* Dense statistics phi(X) [T,Q] exactly as the reference materialises them
 * (normalwishart.py:30-38 etc.).  Only for callers that ask for the tensor
 * (Model.sufficient_statistics(...).dense()); the E-step never forms it. */
int beer_suffstats_expand(int dtype, int cov, int64_t T, int D, const void* X,
                          void* out, void* stream);

/* ------------------------------------------------------------------------
 * E-step: expected log-likelihoods and responsibilities
 * ---------------------------------------------------------------------- */

/* Per-component expected log-likelihood + per-state mixture normaliser +
 * component responsibilities for S states of G Gaussians each (K = S*G):
 *   l[t,s,g]  = stat_scale * phi(x_t) . E[T]_{s,g} - D/2 ln 2pi
 *   w         = l + log_weights[s,g]
 *   log_norm[t,s]     = logsumexp_g w            (nullable)
 *   comp_resps[t,s,g] = exp(w - log_norm[t,s])   (nullable)
 *   pc_llh[t,s,g]     = l                         (nullable)
 * Replaces NormalLikelihood.__call__ (normalwishart.py:88-92; diag
 * normalgamma.py:55-59; iso isonormalgamma.py:56-60) through
 * NormalSet.expected_log_likelihood (beer/models/normalset.py:117-119),
 * Mixture.expected_log_likelihood (mixture.py:70-93: S = 1) and
 * MixtureSet.expected_log_likelihood (mixtureset.py:85-98).  With
 * `labels` (int64 [T], S must be 1) responsibilities are one-hot and
 * log_norm[t] = l[t, label] (mixture.py:85-87).  `log_weights` nullable
 * (= 0).  `stat_scale` reproduces HMM.posteriors' scaling of the statistics
 * (beer/models/hmm.py:119); pass 1.  `llh_sum` (nullable) += sum_t,s log_norm
 * in fp64.  With G > 1 the generic kernels need `comp_resps` as their work
 * buffer; the matrix-core path (workspace given, shape supported) keeps the
 * responsibilities in registers and accepts log_norm / llh_sum alone. */
int beer_mixtureset_estep(int dtype, int cov, int64_t T, int D, int S, int G,
                          const void* X, const void* exp_stats,
                          const void* log_weights, const int64_t* labels,
                          double stat_scale, void* pc_llh, void* log_norm,
                          void* comp_resps, double* llh_sum, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Scratch the matrix-core (MFMA) implementations of the two calls around
 * this comment need (packed parameter / partial-sum images).  0 = the shape
 * has no MFMA implementation.  With `workspace` NULL or too small the calls
 * run the generic kernels -- same results, slower.  The workspace holds no
 * state between calls.  For float32 the size covers both arithmetic variants
 * (BEER_EXACT). */
size_t beer_estep_workspace_bytes(int dtype, int cov, int D, int S, int G);
size_t beer_accumulate_workspace_bytes(int dtype, int cov, int D, int S, int G);
/* ... the same for a call over T frames: never smaller; for float32 diagonal / isotropic
 * Gaussians accumulated without state posteriors (T >= 16384, D <= 64: acc_diag.hip) it also
 * holds the partial sums of every 2048-frame chain, which a second small kernel adds up in
 * fp64 -- with the smaller workspace that call adds them with fp64 atomics (same sums). */
size_t beer_accumulate_frames_workspace_bytes(int dtype, int cov, int64_t T, int D, int S, int G);

/* gamma-weighted sufficient statistics (N_k, sum r x, sum r xx^T) packed as
 * the reference packs them, [K,Q] = resps^T @ phi(X), accumulated (+=) in
 * fp64:  acc[k,:] += sum_t comp_resps[t,k] * state_resps[t, k / G] * phi(x_t).
 * Replaces NormalSet.accumulate (beer/models/normalset.py:121-123) with the
 * joint responsibilities of MixtureSet.accumulate (mixtureset.py:100-112);
 * `state_resps` [T,S] nullable (= 1), `comp_resps` [T,K] nullable (= 1).
 * float32 without BEER_EXACT, diagonal / isotropic, comp_resps given and no state_resps,
 * T >= 16384, D <= 64, 16 <= K <= 65536: the bf16x3 arithmetic of the E-step (acc_diag.hip:
 * three bf16 pieces per operand, six MFMAs per product, 512-frame sums on the matrix cores,
 * float32 to 2048 frames, fp64 beyond); everything else float32: the exact fp32 kernels. */
int beer_normal_accumulate(int dtype, int cov, int64_t T, int D, int S, int G,
                           const void* X, const void* comp_resps,
                           const void* state_resps, double* acc, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The E-step -> accumulate hand-over of a single mixture (S = 1, float32, bf16x3
 * arithmetic) without the float32 responsibilities in between.  `packed_resps`
 * (beer_packed_resps_bytes(T, D, K) bytes: 6 bytes per element with T rounded up
 * to 64 and K to 128, then, for 129..256 components, the transposed frames the
 * E-step kernel leaves behind for the accumulation) receives each responsibility
 * already split into the three bf16 pieces the accumulation kernel multiplies
 * with (r = p0 + p1 + p2 exactly), laid out as that kernel's LDS tiles: per
 * (64 frames, 128 components) 48 KB = three planes of 16 KB, plane q = the pieces
 * p_q as rows [component][64 frames] whose 16-byte chunks sit at position
 * chunk ^ (component & 7); frames >= T and components >= K are 0.  The
 * accumulation kernel copies the tiles to LDS as they are (LDS-DMA).  Same
 * reference functions as the two calls above (mixture.py:86-101 for the
 * responsibilities, normalset.py:121-123 for the statistics).  beer_unpack_resps
 * restores the [T,K] float32 matrix exactly.  The accumulation workspace also
 * holds the frames transposed into 64-frame tiles, hence its own size query with T.
 * EINVAL: shape without a matrix-core path, workspace NULL / too small (sizes
 * from beer_estep_workspace_bytes(BEER_F32, ...) and
 * beer_accumulate_packed_workspace_bytes). */
size_t beer_packed_resps_bytes(int64_t T, int D, int K);
size_t beer_accumulate_packed_workspace_bytes(int cov, int64_t T, int D, int K);
int beer_mixture_estep_packed(int cov, int64_t T, int D, int K, const float* X,
                              const float* exp_stats, const float* log_weights,
                              float* log_norm, void* packed_resps, double* llh_sum,
                              void* workspace, size_t workspace_bytes, void* stream);
int beer_normal_accumulate_packed(int cov, int64_t T, int D, int K, const float* X,
                                  const void* packed_resps, double* acc,
                                  void* workspace, size_t workspace_bytes,
                                  void* stream);
/* The same hand-over for a mixture SET around the forward-backward pass (float32,
 * bf16x3 arithmetic, full covariance; S states of G components, G a power of two
 * in 8..128): beer_mixtureset_estep_packed leaves `log_norm` [T, S] and
 * the responsibilities WITHIN each state's mixture as packed tiles (layout above,
 * K = S * G; no frame tiles behind them); after the forward-backward pass
 * beer_mixtureset_accumulate_packed multiplies the state posteriors
 * `state_resps` [T, S] in while a tile sits in LDS -- (p0 + p1 + p2) * gamma in
 * fp32, split again, each element once per workgroup -- and accumulates
 *     acc[k,:] += sum_t r[t,k] state_resps[t, k / G] phi(x_t)           (fp64, +=)
 * MixtureSet.expected_log_likelihood / accumulate (beer/models/mixtureset.py:85-112)
 * around HMM.expected_log_likelihood (beer/models/hmm.py:73-92): neither the
 * [T, K] float32 responsibilities nor their product with the state posteriors is
 * ever stored.  beer_mixtureset_packed_supported: 1 where both calls have a
 * kernel; EINVAL elsewhere (callers then use beer_mixtureset_estep +
 * beer_normal_accumulate).  Workspaces: beer_estep_workspace_bytes(BEER_F32, ...)
 * and beer_mixtureset_accumulate_packed_workspace_bytes (grows with T: the
 * transposed frames and state posteriors). */
int beer_mixtureset_packed_supported(int cov, int D, int S, int G);
size_t beer_mixtureset_accumulate_packed_workspace_bytes(int cov, int64_t T, int D, int S,
                                                         int G);
int beer_mixtureset_estep_packed(int cov, int64_t T, int D, int S, int G, const float* X,
                                 const float* exp_stats, const float* log_weights,
                                 float* log_norm, void* packed_resps, double* llh_sum,
                                 void* workspace, size_t workspace_bytes, void* stream);
int beer_mixtureset_accumulate_packed(int cov, int64_t T, int D, int S, int G,
                                      const float* X, const void* packed_resps,
                                      const float* state_resps, double* acc,
                                      void* workspace, size_t workspace_bytes,
                                      void* stream);
/* The packed buffer from float32 responsibilities: comp_resps [T, S*G], times
 * state_resps[t, k / G] when given (the joint responsibilities of
 * MixtureSet.accumulate, mixtureset.py:100-112), split and tiled as above;
 * (S*G) % 4 == 0.  This is how float32 responsibilities that exist in memory
 * (labels, generic E-step) reach the bf16x3 accumulation kernel. */
int beer_pack_resps(int64_t T, int D, int S, int G, const float* X,
                    const float* comp_resps, const float* state_resps,
                    void* packed_resps, void* stream);
int beer_unpack_resps(int64_t T, int K, const void* packed_resps, float* resps,
                      void* stream);

/* The accumulation of a mixture set WITHOUT its responsibilities in memory
 * (float32, bf16x3 arithmetic; diagonal / isotropic covariances, D <= 64: few
 * statistics per Gaussian).  beer_mixtureset_estep is then called with
 * comp_resps = NULL and leaves only the per-state log-normalisers `log_norm`
 * [T, S]; after the forward-backward pass this call recomputes the component
 * logits on the matrix cores, forms
 *     r[t,k] * state_resps[t, k / G] = exp(l[t,k] - log_norm[t, k / G]) * state_resps[t, k / G]
 * in registers and multiplies them with the statistics of the frames at once:
 *     acc[k,:] += sum_t r[t,k] state_resps[t, k / G] phi(x_t)            (fp64, +=)
 * -- MixtureSet.accumulate (beer/models/mixtureset.py:100-112) over
 * NormalSet.accumulate (normalset.py:121-123) with the responsibilities of
 * mixtureset.py:85-98 recomputed instead of cached.  `exp_stats`, `log_weights`
 * ([S,G], nullable) as given to beer_mixtureset_estep; `state_resps` [T,S]
 * nullable (= 1).  At K = 1920 Gaussians this removes 15.4 GB of traffic per
 * million frames (the [T, K] matrix written and read back).
 * EINVAL: full covariance, D > 64, workspace NULL / too small. */
size_t beer_accumulate_fused_workspace_bytes(int cov, int D, int S, int G);
int beer_mixtureset_accumulate_fused(int cov, int64_t T, int D, int S, int G,
                                     const float* X, const float* exp_stats,
                                     const float* log_weights, const float* log_norm,
                                     const float* state_resps, const void* frame_image,
                                     double* acc, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* `frame_image` above (nullable): the operands of that kernel that depend on the
 * frames only -- phi(x_t) = [x^2, x, 1] of every 32-frame tile as bf16x3 pieces, once in
 * the layout of the logits' A fragments and once in that of the statistics' B
 * fragments, 1056 bytes per frame at D = 40 (the statistics' data columns: the counts are
 * summed on the vector ALU).  The kernel is bound by vector
 * instruction issue and two thirds of its vector instructions rebuild these for each
 * of the K / 64 component chunks; the frames do not change between the VB iterations
 * of a training run, so a caller that keeps X resident builds the image once per block
 * of frames (beer_frame_image; the same T, D, cov as the accumulation call it is handed
 * to) and the accumulation loads every fragment with 16-byte loads.  Same results bit
 * for bit.  beer_frame_image_bytes = 0: no image for this shape (full covariance, D not a
 * multiple of 4 or > 40); the accumulation ignores an image it cannot use. */
size_t beer_frame_image_bytes(int cov, int64_t T, int D);
/* beer_mixtureset_estep(BEER_F32, ..., comp_resps = NULL) -- the per-state
 * log-normalisers of a mixture set (mixtureset.py:85-98), all that a forward-backward
 * pass needs -- with the A fragments of the logits taken from the same frame image:
 * no staging of the frames, no fragment arithmetic.  Same log_norm bit for bit.
 * Workspace as beer_estep_workspace_bytes(BEER_F32, cov, D, S, G).  EINVAL where the
 * image does not exist or G < 4. */
int beer_mixtureset_lognorm_image(int cov, int64_t T, int D, int S, int G, const float* X,
                                  const float* exp_stats, const float* log_weights,
                                  const void* frame_image, float* log_norm, double* llh_sum,
                                  void* workspace, size_t workspace_bytes, void* stream);
int beer_frame_image(int cov, int64_t T, int D, const float* X, void* image,
                     size_t image_bytes, void* stream);

/* The kernel family and launch form an E-step entry point picks for a call (host only: it
 * launches nothing and touches no device), built from the launchers' own decisions
 * (estep.hip: estep_plan; estep_mfma.hip: llh_form; estep_bf16.hip: llhx_form); it reads
 * BEER_OPT_K1_LDS and BEER_OPT_LNFI from the option table as they do.
 *   entry            BEER_ESTEP_PLAIN: beer_mixtureset_estep; BEER_ESTEP_PACKED:
 *                    beer_mixture_estep_packed (S == 1, K = G) / beer_mixtureset_estep_packed
 *                    (S > 1); BEER_ESTEP_IMAGE: beer_mixtureset_lognorm_image
 *   dtype            BEER_F32 / BEER_F64, | BEER_EXACT
 *   args             which arguments are non-NULL (BEER_ARG_RESPS: comp_resps / packed_resps),
 *                    BEER_ARG_SCALED: stat_scale != 1
 *   workspace_bytes  0: no workspace
 * BEER_EINVAL exactly where the entry point refuses the call (T >= 0 and the frames given);
 * else family | form:
 *   BEER_ESTEP_GENERIC   | BEER_ESTEP_GENERIC_PASS1 / _FUSED / _NORMALISE / _LABELS
 *   BEER_ESTEP_EXACT_F32 / _F64 (llh_kernel<T, NT, MT, GQ>)
 *                        | NT (4 / 8 / 16) | GQ (1 / 2 / 4) << 5 | jw << 8 | chunks << 16
 *   BEER_ESTEP_LLHX (llhx_kernel<NT, MT, GQ, PACKED, SQ, LNO, IMG, BL>; SQ = not full)
 *                        | NT | GQ << 5 | BEER_ESTEP_X_* | chunks << 16
 *   BEER_ESTEP_LNFI (lnfi_kernel<NKU, G, NT>)
 *                        | NT (16 / 8) | NKU (1 .. 4) << 5 | G (4 / 8 / 16) << 8 | chunks << 16
 * chunks: component chunks of 16 NT slots (capped at 4095 in the value).  Every form is held
 * against the oracle in tests/test_gpu_estep_routes.py. */
#define BEER_ESTEP_PLAIN 0
#define BEER_ESTEP_PACKED 1
#define BEER_ESTEP_IMAGE 2
#define BEER_ARG_PC_LLH 1u
#define BEER_ARG_LOG_NORM 2u
#define BEER_ARG_RESPS 4u
#define BEER_ARG_LLH_SUM 8u
#define BEER_ARG_LABELS 16u
#define BEER_ARG_SCALED 32u
#define BEER_ARG_LOG_WEIGHTS 64u
#define BEER_ESTEP_GENERIC 0x10000000
#define BEER_ESTEP_EXACT_F32 0x20000000
#define BEER_ESTEP_EXACT_F64 0x30000000
#define BEER_ESTEP_LLHX 0x40000000
#define BEER_ESTEP_LNFI 0x50000000
#define BEER_ESTEP_FAMILY(route) ((route) & 0x70000000)
#define BEER_ESTEP_GENERIC_PASS1 1      /* llh_kernel alone (pc_llh, or G == 1 log_norm) */
#define BEER_ESTEP_GENERIC_FUSED 2      /* llh_kernel with the normalisation inside */
#define BEER_ESTEP_GENERIC_NORMALISE 3  /* llh_kernel + normalise_kernel */
#define BEER_ESTEP_GENERIC_LABELS 4     /* llh_kernel + labels_kernel */
#define BEER_ESTEP_X_PACKED 0x100       /* responsibilities as packed tiles */
#define BEER_ESTEP_X_LNO 0x200          /* log-normalisers only */
#define BEER_ESTEP_X_IMG 0x400          /* A fragments from the frame image */
#define BEER_ESTEP_X_BL 0x800           /* packed parameters staged in LDS (BEER_OPT_K1_LDS) */
#define BEER_ESTEP_X_NARROW 0x1000      /* <= 128 single Gaussians: one chunk of 4 / 8 tiles */
#define BEER_ESTEP_X_LANE_MAJOR 0x2000  /* groups of 4 / 8 / 16 inside a lane */
#define BEER_ESTEP_X_PADDED 0x4000      /* groups padded to a power of two */
#define BEER_ESTEP_X_XT 0x8000          /* 129 .. 256 packed components: X^T left behind */
int beer_estep_route(int entry, int dtype, int cov, int D, int S, int G, unsigned args,
                     size_t workspace_bytes);

/* The same for the accumulation entry points (host only), built from the launchers' own
 * decisions (estep.hip: accumulate_plan; estep_mfma.hip: acc_form; estep_bf16.hip: accx_form,
 * accf_form; acc_diag.hip: accd_form); it reads BEER_OPT_ACCFI_WAVES as accf_form does.
 *   entry            BEER_ACC_PLAIN: beer_normal_accumulate; BEER_ACC_PACKED:
 *                    beer_normal_accumulate_packed (K = S G), with BEER_ARG_STATE_RESPS
 *                    beer_mixtureset_accumulate_packed; BEER_ACC_FUSED:
 *                    beer_mixtureset_accumulate_fused
 *   dtype            BEER_F32 / BEER_F64, | BEER_EXACT (PLAIN only: the others are float32)
 *   args             BEER_ARG_RESPS: comp_resps / packed_resps; BEER_ARG_STATE_RESPS;
 *                    BEER_ARG_IMAGE: the frame image of the fused entry point
 *   workspace_bytes  0: no workspace
 * BEER_EINVAL exactly where the entry point refuses the call (its other pointers given), an
 * empty batch included; else family | form:
 *   BEER_ACC_GENERIC     accumulate_kernel<T, COV>
 *   BEER_ACC_EXACT_F32 / _F64 (acc_kernel<T, NQ, HAS_SR>)   | NQ (1 / 2 / 4) | BEER_ACC_SR
 *   BEER_ACC_DIAG  (accd_kernel<NJ2, NC>)   | NJ2 (1 .. 4) | NC (1 / 2) << 4 | BEER_ACC_D_PARTIAL
 *   BEER_ACC_ACCX  (accx_kernel<SR, NQ>)    | NQ (6 / 7 / 8) | BEER_ACC_SR | BEER_ACC_X_*
 *   BEER_ACC_ACCF  (accf_kernel<4, NQT, true, W, XP, BLK>)
 *                        | NQT (6 / 9 / 10) | BEER_ACC_F_BLK | W (8 / 4) << 21
 *   BEER_ACC_ACCF | BEER_ACC_F_IMAGE (accfi_kernel<NKU, W, NS>)
 *                        | NKU (1 .. 4) << 4 | NS (4 / 16) << 16 | W << 21 */
#define BEER_ACC_PLAIN 0
#define BEER_ACC_PACKED 1
#define BEER_ACC_FUSED 2
#define BEER_ARG_STATE_RESPS 128u
#define BEER_ARG_IMAGE 256u
#define BEER_ACC_GENERIC 0x10000000
#define BEER_ACC_EXACT_F32 0x20000000
#define BEER_ACC_EXACT_F64 0x30000000
#define BEER_ACC_DIAG 0x40000000
#define BEER_ACC_ACCX 0x50000000
#define BEER_ACC_ACCF 0x60000000
#define BEER_ACC_FAMILY(route) ((route) & 0x70000000)
#define BEER_ACC_SR 0x100               /* state posteriors multiplied in by the kernel */
#define BEER_ACC_D_PARTIAL 0x200        /* partial sums per chain + accd_reduce_kernel */
#define BEER_ACC_X_SX 0x200             /* D > 118 (sets: > 103): one X^T tile in LDS */
#define BEER_ACC_X_XT_REUSED 0x400      /* X^T image read from behind the packed tiles */
#define BEER_ACC_F_BLK 0x200            /* the states of every chunk: 4 consecutive ones */
#define BEER_ACC_F_IMAGE 0x400          /* accfi_kernel: fragments from the frame image */
int beer_accumulate_route(int entry, int dtype, int cov, int64_t T, int D, int S, int G,
                          unsigned args, size_t workspace_bytes);

/* Mixture-weight statistics from the accumulated Gaussian statistics: the
 * zero-order count is N_k = -2 * acc[k, Q-2]; out[s,g] = N_{s,g} for
 * g < G-1 and out[s,G-1] = sum_g N_{s,g} -- the "last column <- row sum"
 * convention of CategoricalLikelihood.sufficient_statistics
 * (beer/dists/dirichlet.py:18-21) summed over frames as in
 * Categorical.accumulate (categorical.py:78-79) and
 * CategoricalSet.accumulate_from_jointresps (categoricalset.py:57-58). */
int beer_weights_from_acc(int S, int G, int Q, const double* acc,
                          double* out /*[S,G] +=*/, void* stream);

/* Tied-mixture (semi-continuous) emissions: S mixtures over ONE pool of K Gaussians that
 * differ in their weights only (no reference counterpart: the reference's MixtureSet,
 * beer/models/mixtureset.py:22-133, gives every mixture its own components; what is
 * replaced is its cat / logsumexp / exp sequence, mixtureset.py:84-103, for weights of
 * shape [S, K] over shared components).  `l` [T,K] are the pool's expected
 * log-likelihoods (beer_mixtureset_estep with S = K, G = 1), `lw` [S,K] the E[ln pi] in
 * fp64 whatever `dtype` is (float32 holds the -130 of an unused component to 8e-6 only, an
 * error the responsibilities would inherit).
 *   pc [T,S]   = logsumexp_k(l[t,k] + lw[s,k])
 *   m  [T]     = max_k l[t,k] (0 for a row without a finite entry)
 * computed as m + ln(E W^T), e = exp(l - m), w = exp(lw), on the matrix cores (exact fp32
 * / fp64 MFMA).  An entry whose linear-domain sum p = sum_k e w is below 2^-94 (float32) /
 * 2^-970 (float64) -- where terms lost to underflow could cost more than 2^-20 / 2^-40 of
 * it; derivation in csrc/tied.hip -- is redone in log space; `log_count` (nullable,
 * device, +=) receives the number of such entries.  K <= 4096, else BEER_EINVAL. */
int beer_tied_lognorm(int dtype, int64_t T, int K, int S, const void* l, const double* lw,
                      void* pc, void* m, int64_t* log_count, void* stream);
/* The statistics of the same model from the state posteriors `g` [T,S] (times the
 * acoustic scale, as MixtureSet.accumulate receives them, mixtureset.py:105-117), with
 * j[t,s,k] = g[t,s] exp(l[t,k] + lw[s,k] - pc[t,s]) never stored:
 *   r [T,K] (of dtype, stored)  = sum_s j   responsibilities of the pool, for
 *                                 beer_normal_accumulate
 *   C [S,K] (fp64, +=)          = sum_t j   counts of the weights' Dirichlet rows
 * as E o (Q W) and W o (Q^T E), q = g / p, p = exp(pc - m); E is recomputed from `l` and
 * `m` (beer_tied_lognorm's outputs).  q of an entry with g = 0 is 0; an entry below the
 * threshold above has q = 0 in the products and its j added in log space afterwards
 * (normalised by its own fp64 logsumexp, not by the stored pc).
 * Workgroups sum at most 4096 frames in dtype before their partial C meet in fp64. */
int beer_tied_accumulate(int dtype, int64_t T, int K, int S, const void* l, const void* m,
                         const void* pc, const double* lw, const void* g, void* r, double* C,
                         void* stream);

/* ------------------------------------------------------------------------
 * Posterior-predictive densities (no reference counterpart: the reference and every
 * entry point above compute exp(E_q[ln p(x | theta)]), which is not a density)
 * ----------------------------------------------------------------------
 * ln p(x | posterior) = ln of the integral of p(x | theta) q(theta): for the three Gaussian
 * families a Student-t in closed form.  With kappa' = kappa / (kappa + 1):
 *   diagonal   l = D [lnG(a + 1/2) - lnG(a)] + 1/2 sum_d ln(kappa' / (2 pi b_d))
 *                  - (a + 1/2) sum_d log1p(kappa' (x_d - m_d)^2 / (2 b_d))
 *   isotropic  l = lnG(a + D/2) - lnG(a) + D/2 ln(kappa' / (2 pi b))
 *                  - (a + D/2) log1p(kappa' |x - m|^2 / (2 b))
 *   full       l = lnG((nu + 1)/2) - lnG((nu + 1 - D)/2) + 1/2 ln|W| + D/2 ln(kappa' / pi)
 *                  - ((nu + 1)/2) log1p(kappa' (x - m)^T W (x - m))
 * each of the form l = c - h L(x), L >= 0, and l = c exactly at x = m.
 *
 * beer_*_predictive_table: what the frame kernels need per pdf, computed in fp64 and stored
 * in `dtype`; standard parameters as for beer_*_expected_stats; `table` [K, Q], Q the
 * family's statistics dimension (2 D + 2, D + 3, D^2 + D + 2), row k:
 *   diagonal   [ m (D) | kappa' / (2 b_d) (D)                          | c | h ]
 *   isotropic  [ m (D) | kappa' / (2 b)                                | c | h ]
 *   full       [ m (D) | R (D x D row-major, upper triangular, zeros   | c | h ]
 *                        below the diagonal), R^T R = kappa' W
 * (R: the quadratic form is |R (x - m)|^2, a sum of squares of the centred frame.)  The
 * differences of ln Gamma are formed without cancellation (shape and dof up to 1e6 and
 * beyond keep c to fp64 rounding of its terms).  Full covariance: D <= 128. */
int beer_ng_predictive_table(int dtype, int K, int D, const void* mean, const void* scale,
                             const void* shape, const void* rates, void* table, void* stream);
int beer_ing_predictive_table(int dtype, int K, int D, const void* mean, const void* scale,
                              const void* shape, const void* rate, void* table, void* stream);
int beer_nw_predictive_table(int dtype, int K, int D, const void* mean, const void* scale,
                             const void* scale_matrix, const void* dof, void* table,
                             void* stream);

/* out[t,k] = l_k(x_t) from the raw frames X [T,D] and a table of K rows (no [T,Q]
 * statistics).  BEER_F32 / BEER_F64; log1p is evaluated accurately relative to its argument
 * (a trained Gaussian has arguments ~1e-5 multiplied by h ~ 1e4..1e6).  One kernel form.
 * BEER_EINVAL where a tile of 64 frames and a chunk of table rows exceed a CU's LDS:
 * 4 (65 D + 32 D + 48) bytes > 160 KiB diagonal float32, i.e. D > ~420 (half that in
 * float64); full covariance D > 128 in float32, D > ~100 in float64. */
int beer_predictive_llh(int dtype, int cov, int64_t T, int D, int K, const void* X,
                        const void* table, void* out, void* stream);

/* log_norm[t,s] = ln sum_g exp(log_mean_weights[s,g] + l_{s,g}(x_t)): the predictive
 * density of S mixtures of G components (table row s G + g) by an online log-sum-exp
 * inside the kernel -- the [T, S G] matrix is never written.  `log_mean_weights` [S,G]
 * are ln E[pi] (NOT E[ln pi]); nullable (= 0).  Any G >= 1.  Same kernel and limits as
 * beer_predictive_llh, which is this call with G = 1 and no weights. */
int beer_mixtureset_predictive(int dtype, int cov, int64_t T, int D, int S, int G,
                               const void* X, const void* table,
                               const void* log_mean_weights, void* log_norm, void* stream);

/* ------------------------------------------------------------------------
 * Speaker-adaptive affine feature transforms (CMLLR / fMLLR), cmllr.hip
 * ---------------------------------------------------------------------- */
/* y = A_s x + b_s per speaker, W_s = [A_s | b_s] [D, D+1], estimated by maximum likelihood
 * under a model of diagonal or isotropic Gaussians.  With r_tk the
 * component responsibilities of frame t, xi_t = [x_t; 1] and E = D + 1:
 *   omega_ti = sum_k r_tk E[lambda]_ki       [T, P]   P = D diagonal, 1 isotropic
 *   nu_ti    = sum_k r_tk E[lambda mu]_ki    [T, D]
 *   c_t      = sum_k r_tk
 *   G_{s,i}  = sum_t omega_ti xi_t xi_t^T    symmetric E x E, i < P (packed lower triangle,
 *                                            entry (a, b), b <= a, at a (a + 1) / 2 + b)
 *   k_{s,i}  = sum_t nu_ti xi_t              E entries, i < D
 *   beta_s   = sum_t c_t
 * the sums over the frames of speaker s.  D <= BEER_CMLLR_MAX_DIM everywhere below. */
#define BEER_CMLLR_MAX_DIM 63

/* out[t, :] += [omega_t | nu_t | c_t], float64 [T, P + D + 1], with
 * r_tk = comp_resps[t, k] * state_resps[t, k / G] -- the contract of beer_normal_accumulate,
 * transposed: `comp_resps` [T, S G] nullable when G == 1 (= 1), `state_resps` [T, S] nullable
 * (= 1), both in `dtype` like E [S G, Q], the natural_form() of the Gaussians (BEER_DIAG:
 * Q = 2 D + 2, BEER_ISO: Q = D + 3; its first D columns are E[lambda mu], the next P
 * E[lambda]).  Products and sums in float64 on the matrix cores; it ADDS, so that the groups
 * of a joint emission set accumulate into one buffer.  BEER_EINVAL for BEER_FULL. */
int beer_cmllr_frame_params(int dtype, int cov, int64_t T, int D, int S, int G,
                            const void* comp_resps, const void* state_resps, const void* E,
                            double* out, void* stream);

/* HOST: the table beer_cmllr_accumulate walks, from the utterances' lengths and speakers
 * (host arrays; speaker -1: the utterance is left out).  The frames of a speaker, in
 * utterance order, are cut into items of `chunk_frames` frames (0: the default, 1024); an
 * item lists its runs of frames inside utterances.  With `table` NULL *n_ints receives the
 * number of int32 the table takes; else *n_ints is the room in `table` on entry and what
 * was written on return:
 *   [n_items, n_segs, n_spk, nutt | spk_ptr [n_spk + 1] | item_spk [n_items] |
 *    item_ptr [n_items + 1] | seg [n_segs][3] = (utterance, first frame in it, frames)]
 * BEER_EINVAL for a speaker outside -1 .. n_spk - 1 or an utterance of 2^31 frames. */
int beer_cmllr_table(int32_t nutt, int32_t n_spk, const int64_t* lengths,
                     const int32_t* utt_spk, int32_t chunk_frames, int32_t* table,
                     size_t* n_ints);

/* Bytes of workspace beer_cmllr_accumulate needs for a table of n_items items (a slab of
 * P E (E + 1) / 2 + D E + 1 doubles each); 0 for a shape it refuses. */
size_t beer_cmllr_workspace_bytes(int D, int P, int64_t n_items);

/* G [n_spk, P, E (E + 1) / 2], k [n_spk, D, E], beta [n_spk] (float64) += the statistics
 * above of the frames X [T, D] (`dtype`) with params [T, P + D + 1] = [omega | nu | c] of
 * beer_cmllr_frame_params, over the ragged batch `frame_off` [nutt + 1] (device).  `table`:
 * the device copy of `table_host` (beer_cmllr_table with the same chunk_frames), whose
 * structure is checked on the host before anything is launched.  Every item is summed on
 * the matrix cores by one workgroup per eight dimensions i into a slab of the workspace,
 * four frames per step in frame order; a second kernel adds a speaker's slabs in chunk
 * order.  No atomics: the result depends on the inputs and chunk_frames only, bit for bit.
 * BEER_EINVAL: D > BEER_CMLLR_MAX_DIM, P neither 1 nor D, a table that does not fit
 * (n_spk, nutt, chunk_frames) or names a speaker or utterance out of range, a workspace
 * smaller than beer_cmllr_workspace_bytes. */
int beer_cmllr_accumulate(int dtype, int64_t T, int D, int P, int32_t nutt, int32_t n_spk,
                          const void* X, const double* params, const int64_t* frame_off,
                          const int32_t* table_host, const int32_t* table, size_t table_ints,
                          int32_t chunk_frames, double* G, double* k, double* beta,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Y[t] = A_s x_t + b_s, s = utt_spk[utterance of t], W [n_spk, D, D + 1] float64: the sum
 * in float64 (a fused multiply-add chain over the dimensions, then + b), rounded once to
 * `dtype`.  A speaker of -1 (and a frame outside every utterance) copies the frame.
 * `utt_spk` [nutt] on the device; `utt_spk_host` (nullable): its host copy, checked before
 * the launch -- BEER_EINVAL for an entry outside -1 .. n_spk - 1 (an entry the kernel meets
 * out of range copies the frame).  Y must not be X. */
int beer_cmllr_apply(int dtype, int64_t T, int D, int32_t nutt, int32_t n_spk, const void* X,
                     const double* W, const int64_t* frame_off, const int32_t* utt_spk,
                     const int32_t* utt_spk_host, void* Y, void* stream);

/* ------------------------------------------------------------------------
 * HMM inference over a ragged batch of utterances
 * ---------------------------------------------------------------------- */

/* Inference graph in device memory (CompiledGraph, beer/graph.py:243-268):
 * dense init/final log-probabilities plus the finite transitions in two
 * CSR forms (by destination for the forward / Viterbi recursions, by source
 * for the backward recursion).  Arcs inside a row are sorted by the other
 * end's index (ascending) -- Viterbi's first-index tie-break relies on it.
 * Built on the host by beer_amd.graph.CompiledGraph; -inf transitions are
 * simply absent.  Rows are additionally cut into segments of at most
 * BEER_SEG arcs so that the log-sum-exp of a high-degree state (a phone
 * start in a phone loop has one incoming arc per phone) is reduced by
 * several lanes instead of one. */
#define BEER_SEG 8
typedef struct {
    int32_t n_states;
    int32_t n_arcs;
    int32_t n_in_seg;          /* segments (<= BEER_SEG arcs of one row) by destination */
    int32_t n_out_seg;         /* ... by source */
    const void* init;          /* [S]  */
    const void* final;         /* [S]  */
    const int32_t* in_ptr;     /* [S+1] arcs grouped by destination */
    const int32_t* in_src;     /* [nnz] source state               */
    const int32_t* in_dst;     /* [nnz] destination state (row id)  */
    const void* in_w;          /* [nnz] log-probability             */
    const int32_t* in_seg;     /* [n_in_seg+1] arc offsets of the segments  */
    const int32_t* in_row_seg; /* [S+1] segment range of every destination  */
    const int32_t* out_ptr;    /* [S+1] arcs grouped by source      */
    const int32_t* out_dst;    /* [nnz] destination state           */
    const int32_t* out_src;    /* [nnz] source state (row id)       */
    const void* out_w;         /* [nnz] */
    const int32_t* out_seg;    /* [n_out_seg+1] */
    const int32_t* out_row_seg;/* [S+1] */
    const struct beer_graph_lowdeg* lowdeg;   /* optional factorised image, see below */
} beer_graph;

/* Optional low-degree image of the same graph, used by the fast
 * forward-backward variant.  compile() of the reference eliminates
 * non-emitting states, which turns a phone loop's pivot state into a dense
 * P x P block of arcs (every phone end -> every phone start) whose
 * log-weights are rank one: A[e, s] = src_w[e] + dst_w[s].  Such a block is
 * kept here as a "hub" (one log-sum-exp over its sources per frame) and removed
 * from the CSR, which leaves every state with a handful of arcs.  Present only
 * when every remaining row has <= BEER_SEG arcs.  */
typedef struct beer_graph_lowdeg {
    int32_t n_arcs;            /* arcs left after removing the hub blocks */
    int32_t n_hubs;
    const int32_t* in_ptr;     /* [S+1] */
    const int32_t* in_src;     /* [n_arcs] */
    const void* in_w;          /* [n_arcs] */
    const int32_t* out_ptr;    /* [S+1] */
    const int32_t* out_dst;    /* [n_arcs] */
    const void* out_w;         /* [n_arcs] */
    const int32_t* hub_src_id; /* [S] hub fed by the state, -1: none */
    const void* hub_src_w;     /* [S] */
    const int32_t* hub_dst_id; /* [S] hub feeding the state, -1: none */
    const void* hub_dst_w;     /* [S] */
    const int32_t* src_ptr;    /* [n_hubs+1] source states of every hub ... */
    const int32_t* src_list;
    const int32_t* dst_ptr;    /* [n_hubs+1] ... and its destination states */
    const int32_t* dst_list;
} beer_graph_lowdeg;

/* Ragged batch: utterance u owns frames [frame_off[u], frame_off[u+1]) of the
 * packed feature matrix and rows [llh_off[u], ...) (in elements) of the
 * packed per-state buffers, whose row length is graphs[graph_id[u]].n_states.
 * All arrays are device arrays of length nutt (+1 for frame_off). */
typedef struct {
    int32_t nutt;
    int32_t max_states;        /* max n_states over the batch's graphs (LDS sizing) */
    int32_t max_arcs;          /* max n_arcs over the batch's graphs   (LDS sizing) */
    int32_t max_segs;          /* max(n_in_seg, n_out_seg) over the graphs          */
    int32_t all_lowdeg;        /* != 0: every graph has a `lowdeg` image            */
    int32_t n_graphs;
    const int64_t* frame_off;  /* [nutt+1] */
    const int64_t* llh_off;    /* [nutt]   element offsets */
    const int32_t* graph_id;   /* [nutt]   */
    const beer_graph* graphs;  /* device array of graph descriptors */
    const int32_t* pdf_off;    /* [n_graphs+1] offsets into pdf_ids */
    const int32_t* pdf_ids;    /* concatenated pdf_id_mapping of every graph */
    /* what the host knows about the `lowdeg` images (0 = unknown: the
     * one-wave-per-utterance recursion is then not used) */
    int32_t max_degree;        /* largest in / out degree of their CSRs (>= 1) */
    int32_t max_hubs;          /* largest n_hubs */
    int32_t max_hub_members;   /* largest number of sources / destinations of a hub */
    int32_t reserved;
    /* (nullable) [nutt]: the order in which the one-wave-per-utterance kernels hand the
     * utterances to their waves -- longest first, so that the four waves of a workgroup
     * finish together and the launch ends with its shortest utterances (the reference
     * loops over utterances in file order, accumulate.py:39-59; the sums do not care).
     * NULL: 0, 1, 2, ... */
    const int32_t* order;
} beer_batch;

/* pc_llhs[u][t,s] = scale * pc_all[frame_off[u]+t, pdf_id[s]]: the gather of
 * DynamicallyOrderedModelSet.expected_log_likelihood
 * (beer/models/modelset.py:140-146) and the acoustic scale of
 * HMM.expected_log_likelihood (beer/models/hmm.py:79). */
int beer_hmm_gather(int dtype, const beer_batch* batch_h, int S_total,
                    const void* pc_all, double scale, void* pc_llhs,
                    void* stream);

/* Log-space forward-backward, per-frame-normalised state posteriors and
 * (optional) summed transition posteriors:
 * CompiledGraph._baum_welch_forward/_backward/posteriors
 * (beer/graph.py:270-326).  gamma has the layout of pc_llhs.  `alpha_ws` is
 * caller-provided fp64 scratch with as many elements.  `xi_sum` (nullable, [S,S]
 * fp64, +=) receives sum_u sum_t xi_t -- every utterance must then use
 * graph 0; `gamma0_sum` (nullable, [S] fp64, +=) receives sum_u gamma_0.
 * `lognorm_mean` (nullable, [nutt]) receives mean_t lognorm_t
 * (graph.py:326).  When every graph of the batch carries a `lowdeg` image
 * the factorised recursion runs; transition posteriors through a hub are
 * then reported per destination state, summed over the hub's sources, in
 * `hub_flow` ([S] fp64, +=; required whenever xi_sum is given) instead of as
 * individual xi_sum entries.  `hub_ws` (nullable; fp64 scratch, 4 per frame of
 * the batch) lets low-degree graphs of at most 256 states run one WAVE per
 * utterance (no workgroup barrier in the recursion: about 4x faster). */
int beer_hmm_forward_backward(int dtype, const beer_batch* batch_h,
                              const void* pc_llhs, double* alpha_ws, double* hub_ws,
                              void* gamma, double* xi_sum, double* gamma0_sum,
                              double* hub_flow, void* lognorm_mean, void* stream);
/* How many utterances of the batch the last beer_hmm_forward_backward /
 * beer_hmm_posteriors_fused call on `hub_ws` ran in LOG SPACE (no reference counterpart:
 * beer/graph.py:270-326 is log-space throughout; the one-wave kernels run on scaled
 * probabilities and hand an utterance over to their log-space twin when a column or a
 * frame's normaliser falls below 2^-800 of its scale, or a log-likelihood is NaN).
 * `count` (device, int64) += that number.  EINVAL unless the batch is of the kind the
 * one-wave kernels take (other kernels are log-space: nothing to count). */
int beer_hmm_fb_log_count(const beer_batch* batch_h, const double* hub_ws, int64_t* count,
                          void* stream);

/* Which kernel family beer_hmm_forward_backward launches for this descriptor (host only: it
 * reads the scalar fields of the batch and launches nothing), given a `hub_ws` workspace as
 * above, transition posteriors asked for or not (`want_xi`: xi_sum != NULL) and, with them,
 * `hub_flow` given or not.  The launcher decides with the same predicates.
 *   BEER_FB_WAVE | SPL << 4 | DEG   one wave per utterance (linear domain, log-space twin):
 *                                   SPL in {1, 2, 4} states per lane for at most 64 / 128 / 256
 *                                   states, DEG in {2, 4, 8} arcs per state unrolled
 *   BEER_FB_LOWDEG | threads        one thread per state, 128 / 256 / 512 threads: low-degree
 *                                   images of up to 512 states, hubs of any size
 *   BEER_FB_GENERAL                 the segment kernel, arc lists in LDS
 *   BEER_FB_GENERAL_BIG             the segment kernel, per-arc scratch in `hub_ws`
 *                                   (beer_hmm_fb_scratch_doubles > 0)
 * BEER_EINVAL where beer_hmm_forward_backward refuses the batch.  BEER_FB_FAMILY(route) is
 * the family alone.  The families other than BEER_FB_WAVE leave logarithms in `alpha_ws`. */
#define BEER_FB_WAVE 0x1000
#define BEER_FB_LOWDEG 0x2000
#define BEER_FB_GENERAL 0x3000
#define BEER_FB_GENERAL_BIG 0x4000
#define BEER_FB_FAMILY(route) ((route) & 0xF000)
int beer_hmm_fb_route(int dtype, const beer_batch* batch_h, int want_xi, int have_hub_flow);

/* Doubles `hub_ws` of beer_hmm_forward_backward must hold BESIDES the hub values
 * (BEER_MAX_HUBS per frame) for this batch: 0 while the arc lists of its largest
 * graph fit a CU's LDS (about 4000 arcs with transition posteriors in float32);
 * beyond that the general kernel keeps its per-arc scratch there -- 2 max_arcs +
 * max_segs doubles for each of at most 512 workgroups -- and reads the topology
 * from the graph image, so that graphs of any density run (the reference's dense
 * recursion, graph.py:270-326, has no size limit); only the per-state arrays
 * stay in LDS (up to ~4000 states). */
size_t beer_hmm_fb_scratch_doubles(int dtype, const beer_batch* batch_h, int want_xi);

/* The HMM inference step of a whole shard in ONE launch, for batches whose
 * graphs all carry a `lowdeg` image with at most one hub of at most 64 sources /
 * destinations and have at most 256 states (phone loops with their pivot declared
 * as a hub, alignment chains): the gather of
 * beer_hmm_gather, the recursions of beer_hmm_forward_backward (one wave per
 * utterance) and the scatter of beer_hmm_scatter without the packed pc_llhs /
 * gamma arrays in between.
 *   pc_all       [n_frames, S_total] per-pdf log-likelihoods (read through the
 *                pdf ids, times `scale`: modelset.py:140-146, hmm.py:79)
 *   state_resps  [n_frames, S_total]: scale * gamma at the pdf ids
 *                (modelset.py:148-154, hmm.py:95).  atomic_out = 0: plain stores --
 *                every graph's pdf ids are distinct; the caller zero-fills the
 *                array unless they also cover 0 .. S_total-1.  atomic_out = 1:
 *                added atomically into the zero-filled array (repeated ids).
 *                atomic_out = 2 (S_total <= 512, else BEER_EINVAL): whole rows -- a
 *                wave adds its states' posteriors into a zero row in LDS (repeated
 *                ids add up there) and stores all S_total entries of the frame,
 *                zeros included: the array needs no initialisation and sees no
 *                atomic.  What alignment-graph training uses (accumulate.py:39-59
 *                with --alis: a transcription names a phone more than once).
 *   utt_llh      (nullable, [nutt] fp64, +=) sum_t sum_s gamma * scale * pc
 *                (hmm.py:87);  gamma0_sum, hub_flow: as above (graph 0 for all).
 *   frame_llh    (nullable, [n_frames] of dtype, stored) the per-frame value
 *                sum_s gamma_ts * scale * pc_ts that HMM.expected_log_likelihood returns
 *                (hmm.py:87), reduced over the wave while both factors are in registers --
 *                what beer_rowdot(state_resps, pc_all) computes from the two [T, S] arrays.
 *   alpha_ws     fp64 scratch, sum_u T_u * S_u;  hub_ws: fp64 scratch, n_frames.
 * EINVAL when the batch is not of that kind (use the three calls instead). */
int beer_hmm_posteriors_fused(int dtype, const beer_batch* batch_h, int S_total,
                              const void* pc_all, double scale, double* alpha_ws,
                              double* hub_ws, void* state_resps, int atomic_out,
                              double* gamma0_sum, double* hub_flow, double* utt_llh,
                              void* frame_llh, void* stream);

/* Transition counts for LEARNED transition probabilities (HMM / PhoneLoop created with
 * train_transitions=True; an extension: the reference's transition probabilities are constants
 * copied from conf/hmm.yml, beer/cli/subcommands/hmm/mkphones.py:12-43, and only the phone weights
 * are re-estimated, beer/models/phoneloop.py:53-65).  Batches whose utterances all use ONE graph
 * (n_graphs == 1) of the kind the one-wave kernels take (see above); the recursions, and every
 * other output, are those of beer_hmm_posteriors_fused / beer_hmm_forward_backward, bit for bit,
 * and the log-space twin gives the same counts for the utterances it takes over.
 *   arc_counts  [n_arcs of the graph's lowdeg image] fp64, +=: sum over utterances and frames of
 *               the transition posteriors xi_t(i, j) of every arc of the low-degree image, in its
 *               out-CSR order (by source, destinations ascending; hub arcs are not in it):
 *               graph.py:308-323 summed over t, restricted to those arcs.
 *   src_flow    [S] fp64, +=: the expected exits of every state -- its transition posteriors
 *               into the hub summed over the hub's destinations (phoneloop.py:88-95 counts the
 *               same arcs by destination), plus its posterior at the last frame of every
 *               utterance (the utterance ends by leaving it; 0 where the final weight is 0).
 * EINVAL when the batch is not of that kind or an output is NULL. */
int beer_hmm_posteriors_fused_counts(int dtype, const beer_batch* batch_h, int S_total,
                                     const void* pc_all, double scale, double* alpha_ws,
                                     double* hub_ws, void* state_resps, int atomic_out,
                                     double* gamma0_sum, double* hub_flow, double* utt_llh,
                                     void* frame_llh, double* arc_counts, double* src_flow,
                                     void* stream);
/* The same two outputs from beer_hmm_forward_backward's one-wave path (packed pc_llhs / gamma,
 * graph.py:270-326): the dense xi_sum is replaced by `arc_counts` / `src_flow`. */
int beer_hmm_forward_backward_counts(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                                     double* alpha_ws, double* hub_ws, void* gamma,
                                     double* gamma0_sum, double* hub_flow, double* arc_counts,
                                     double* src_flow, void* lognorm_mean, void* stream);

/* The general path of the same counts, for every graph beer_hmm_forward_backward takes (more
 * than 256 states, hubs of more than 64 phones): its dense xi_sum with the hub arcs in the matrix
 * (the batch's lowdeg flag cleared) gives the arcs and, row by row, the exits; what it lacks is
 * the end-of-utterance exit, the posteriors of every utterance's last frame:
 * out [S] fp64 (+=) = sum_u gamma_u[T_u - 1, :] (gamma packed as beer_hmm_forward_backward
 * leaves it; graph.py:304-307 at t = T - 1).  n_graphs must be 1. */
int beer_hmm_last_frame_sum(int dtype, const beer_batch* batch_h, const void* gamma, double* out,
                            void* stream);

/* Learned transition probabilities trained against ALIGNMENT GRAPHS (accumulate.py:39-59 with
 * --alis; an extension like the counts above): every utterance has a graph of its own, and every
 * arc of every graph is bound to a category of the model's transitions.  The maps are device
 * arrays over the graphs of the batch, graph g of `beer_batch.graphs` at its own offsets:
 *   arc_cat   category of every arc, in the graph's out-CSR order (by source, destinations
 *             ascending: `out_ptr` / `out_dst`, which for these graphs is the low-degree
 *             image's order too): arc a of graph g at arc_cat[arc_off[g] + a]
 *   last_cat  per state, the category that receives its posterior at the LAST frame of an
 *             utterance (the exit of the unit the state ends; the convention of `src_flow`
 *             above), or -1: state j of graph g at last_cat[state_off[g] + j] */
typedef struct {
    const int32_t* arc_cat;
    const int32_t* last_cat;
    const int64_t* arc_off;    /* [n_graphs] */
    const int64_t* state_off;  /* [n_graphs] */
} beer_cat_map;

/* w[pos[i]] = log_a[cat[i]] for i < n: every weight array of a bound image (in_w, out_w -- the
 * low-degree image of an alignment graph reads the same two arrays) rewritten with E[ln a] of its
 * arcs' categories.  `image` is the image's blob seen as an array of dtype, `pos` element
 * positions in it, `log_a` [n_categories] of dtype.  Reads nothing on the host. */
int beer_hmm_refresh_weights(int dtype, int64_t n, const int64_t* pos, const int32_t* cat,
                             const void* log_a, void* image, void* stream);

/* beer_hmm_posteriors_fused / beer_hmm_forward_backward with the transition counts BY CATEGORY
 * of a batch of different graphs: cat_counts [n_categories] fp64, += the transition posteriors
 * of every arc summed over frames and utterances, at the arc's category, and the last-frame
 * posteriors at `last_cat`.  The recursions and every other output are those of the un-mapped
 * calls on the same image, bit for bit.  beer_hmm_posteriors_fused_cat takes what
 * beer_hmm_posteriors_fused takes (one-wave kernels); beer_hmm_forward_backward_cat every batch
 * beer_hmm_forward_backward takes (beyond 256 states: the workgroup kernels).  `hub_ws` as for
 * beer_hmm_forward_backward with transition posteriors (beer_hmm_fb_scratch_doubles). */
int beer_hmm_posteriors_fused_cat(int dtype, const beer_batch* batch_h, int S_total,
                                  const void* pc_all, double scale, double* alpha_ws,
                                  double* hub_ws, void* state_resps, int atomic_out,
                                  double* gamma0_sum, double* utt_llh, void* frame_llh,
                                  const beer_cat_map* map, double* cat_counts, void* stream);
int beer_hmm_forward_backward_cat(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                                  double* alpha_ws, double* hub_ws, void* gamma,
                                  double* gamma0_sum, const beer_cat_map* map,
                                  double* cat_counts, void* lognorm_mean, void* stream);
/* The hard counts of a state path (viterbi=True / state_path=): cat_counts += 1 at the category
 * of every arc (p_t, p_t+1) and at last_cat of every utterance's last state.  An arc is looked
 * up in its source's out-row.  A pair of states that is not an arc counts nothing. */
int beer_hmm_path_counts_cat(const beer_batch* batch_h, const int64_t* path,
                             const beer_cat_map* map, double* cat_counts, void* stream);

/* A phone loop with a BIGRAM language model (beer/models/phoneloop.py:104-191):
 * its end -> start block trans[src[i], dst[j]] = ln(1 - loop_i) + E[ln w][i, j] is a
 * full P x P matrix, kept apart from the rest of the graph (a low-degree CSR: the
 * arcs of the block removed, every row <= BEER_SEG arcs).  Device arrays; weights in
 * the model's dtype. */
#define BEER_BIGRAM_MAX_PHONES 128
#define BEER_BIGRAM_MAX_STATES 512
typedef struct {
    int32_t n_states;          /* S <= BEER_BIGRAM_MAX_STATES */
    int32_t n_phones;          /* P <= BEER_BIGRAM_MAX_PHONES */
    int32_t max_degree;        /* largest in / out degree of the residual CSR */
    int32_t reserved;
    const void* init;          /* [S] */
    const void* final;         /* [S] */
    const int32_t* in_ptr;     /* [S+1] residual arcs by destination */
    const int32_t* in_src;
    const void* in_w;
    const int32_t* out_ptr;    /* [S+1] residual arcs by source */
    const int32_t* out_dst;
    const void* out_w;
    const int32_t* src;        /* [P] the block's source states (phone ends) */
    const int32_t* dst;        /* [P] its destination states (phone starts) */
    const void* block_w;       /* [P, P] trans[src[i], dst[j]] */
    const int32_t* src_slot;   /* [S] i of a source state, -1: none */
    const int32_t* dst_slot;   /* [S] j of a destination state, -1: none */
    const int32_t* pdf_ids;    /* [S] */
} beer_bigram;

/* The HMM inference step of a free bigram loop over a ragged batch of utterances,
 * in ONE launch (graph.py:270-326, hmm.py:73-95): the pdf-id gather with the acoustic
 * scale, forward-backward (scaled linear domain, fp64 trellis, the block as a
 * matrix-vector product per frame from LDS), the scatter of scale * gamma to pdf ids
 * and sum_t sum_s gamma * scale * pc per utterance.
 *   frame_off     [nutt+1] device, frames of the batch (0-based), n_frames in all
 *   order         [nutt] device, nullable: the order utterances are handed to waves
 *   pc_all        [n_frames, S_total] per-pdf log-likelihoods
 *   alpha_ws      [n_frames, S] fp64 scratch
 *   uv_ws         [2, n_frames, P] fp64: U[f] = a_t(src) / n_t and V[f] = b_{t+1}
 *                 beta_{t+1}(dst) of frame f = frame_off[u] + t (0 for the last frame
 *                 of an utterance); the block's summed transition posteriors are
 *                 C = exp(block) o (U^T V) (phoneloop.py:174-186)
 *   state_resps   [n_frames, S_total]; atomic_out != 0: added into a zero-filled array
 *                 (repeated pdf ids), else plain stores (distinct ids covering S_total)
 *   utt_llh       [nutt] fp64, written (not added)
 *   flags         [nutt] int32: 1 where an utterance left fp64's range (it then
 *                 contributes nothing valid: redo the batch in log space)
 * EINVAL beyond BEER_BIGRAM_MAX_PHONES / _STATES or BEER_SEG residual arcs. */
int beer_hmm_posteriors_bigram(int dtype, const beer_bigram* graph, int32_t nutt,
                               int64_t n_frames, const int64_t* frame_off,
                               const int32_t* order, int S_total, const void* pc_all,
                               double scale, double* alpha_ws, double* uv_ws,
                               void* state_resps, int atomic_out, double* utt_llh,
                               int32_t* flags, void* stream);

/* The launch shape beer_hmm_posteriors_bigram picks for this descriptor and batch size
 * (host only: it reads n_states, n_phones and max_degree, and launches nothing), built from
 * the launcher's own expressions:
 *   SPL | DEG << 8 | waves << 16
 * SPL in {1, 2, 4, 5, 8} states per lane for at most 64 / 128 / 256 / 320 / 512 states, DEG in
 * {2, 4, 8} residual arcs per state unrolled, waves (= utterances) per workgroup:
 * min(8, what the LDS holds behind W, ceil(nutt / n_cu)), at least 1.  `n_cu` <= 0: the
 * current device's compute units as the launcher asks for them, 256 if that fails.
 * BEER_EINVAL exactly where beer_hmm_posteriors_bigram refuses the descriptor. */
int beer_hmm_bigram_route(int dtype, const beer_bigram* graph, int32_t nutt, int32_t n_cu);

/* Per-frame transition posteriors in the reference's own layout, xi [T-1, S, S]
 * (beer/graph.py:308-323: normalised per frame, NaN -> 0), for ONE utterance,
 * from what beer_hmm_forward_backward left behind: `alpha` (its fp64 workspace
 * [T,S]), `gamma` [T,S], the emission log-likelihoods `llhs` [T,S] it was given
 * and the dense transition log-probabilities `trans` [S,S].  The batched path
 * never forms this tensor (8 S^2 bytes per frame); it exists for callers that
 * switch the reference layout on (beer_amd.reference_layout). */
int beer_hmm_trans_posteriors(int dtype, int64_t T, int S, const double* alpha,
                              const void* llhs, const void* gamma, const void* trans,
                              void* xi, void* stream);

/* Viterbi + backtrack, CompiledGraph.best_path (beer/graph.py:329-344):
 * first-index tie-break, -inf safe, int64 state path per frame (packed like
 * the frames).  `bt_ws` is int32 scratch with the layout of pc_llhs.  With `map_pdf` != 0 the path is mapped through pdf_id_mapping as
 * HMM.decode does (beer/models/hmm.py:105-114). */
int beer_hmm_viterbi(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                     int32_t* bt_ws, int64_t* path, int map_pdf, void* stream);

/* N-best Viterbi: the k best state paths of every utterance, with their scores.
 *   pc_llhs    packed per-state log-likelihoods, as for beer_hmm_viterbi (read only)
 *   k          1 <= k <= BEER_NBEST_MAX
 *   bt_ws      caller-provided int32 scratch, k * n_elems of them (n_elems: the elements of
 *              pc_llhs); its content is opaque
 *   paths      [k, n_frames] int64, frame index as in frame_off: row r holds the r-th best path of
 *              every utterance -- state indices, or with `map_pdf` != 0 pdf ids
 *   scores     [nutt, k] fp64 whatever the dtype: the value computed in the dtype, widened exactly
 * Definition.  For an utterance of T frames on a graph of S states a path is p_0 .. p_{T-1}.  All
 * arithmetic is done in the dtype of pc_llhs, in exactly the order beer_hmm_viterbi uses:
 *   omega_0[j] = llh[0,j] + init[j]
 *   candidate c = omega_{t-1}[i][r] + w_ij,  then omega_t[j][q] = llh[t,j] + c
 *   final candidate omega_{T-1}[j][r] + final[j]
 * At every cell (t, j) the k best candidates over (source i, rank r) are kept, at the end the k
 * best over (state j, rank r).  Order of the candidates: the larger score first; on equal scores
 * the smaller source (or final) state first, then the smaller rank.  Should a row of the in-CSR
 * hold parallel arcs i -> j, the arc's position in the row decides before the rank (rows are
 * sorted by source, so the position refines the source order).  In exact arithmetic this orders
 * the paths by (score descending, then the lexicographic order of the REVERSED path); the k
 * results are pairwise distinct paths by construction.
 * A candidate of score -inf is not a path.  Where fewer than k paths of finite score exist the
 * remaining ranks get the score -inf and path rows filled with -1, under `map_pdf` too.  An
 * utterance of no frames gets k scores of -inf.
 * Whenever the best score is finite, rank 0 is the path beer_hmm_viterbi returns, element for
 * element.  When no path is finite the two differ: beer_hmm_viterbi returns the path of its
 * default arguments (source 0 wherever nothing is reachable), this entry only -inf and -1.  NaN
 * inputs are undefined, as for beer_hmm_viterbi.
 * EINVAL, checked before anything is launched: k outside 1 .. BEER_NBEST_MAX, a dtype other than
 * BEER_F32 / BEER_F64, a NULL batch, more than 32767 states (a back-pointer packs
 * source << 4 | rank), an LDS need (below) beyond a CU's 160 KiB; a NULL pointer argument with a
 * batch that has utterances. */
#define BEER_NBEST_MAX 16
int beer_hmm_viterbi_nbest(int dtype, const beer_batch* batch_h, const void* pc_llhs, int32_t k,
                           int32_t* bt_ws, int64_t* paths, double* scores, int map_pdf,
                           void* stream);

/* The form beer_hmm_viterbi_nbest picks for this batch and k (host only: it reads max_states and
 * max_arcs and launches nothing), built from the launcher's own plan:
 *   chunk | BEER_NBEST_ARCS_LDS
 * One workgroup per utterance, a thread per state (min(256, S rounded up to 64) threads, strided
 * beyond 256 states); a thread keeps BEER_NBEST_LIST(k) list entries in registers.  With
 * S = max_states, A = max_arcs, w = 4 / 8 bytes of the dtype and row = 4 S k bytes (the
 * back-pointers of one frame):
 *   chunk   frames of back-pointers the back-trace stages into LDS at a time: 32 when 32 rows
 *           take at most 16 KiB (S k <= 128), else 8 when 8 rows do (S k <= 512), else 2
 *   base  = 2 S k w + 64 + chunk * row    two score columns [S][k], the k walks, the chunk
 *   BEER_NBEST_ARCS_LDS  the arc lists are kept in LDS: base + 4 (S + 2 + A) + w A <= 64 KiB;
 *           else they are read from global memory
 * BEER_EINVAL exactly where beer_hmm_viterbi_nbest refuses: the argument errors above, and
 * base > 160 KiB.  BEER_NBEST_CHUNK(route) is the chunk alone. */
#define BEER_NBEST_ARCS_LDS 0x100
#define BEER_NBEST_CHUNK(route) ((route) & 0xFF)
#define BEER_NBEST_LIST(k) ((k) <= 1 ? 1 : ((k) <= 2 ? 2 : ((k) <= 4 ? 4 : ((k) <= 8 ? 8 : 16))))
int beer_hmm_nbest_route(int dtype, const beer_batch* batch_h, int32_t k);

/* State paths drawn from the posterior p(s_0..s_{T-1} | x) of every utterance: forward
 * filtering, backward sampling, `nsamples` >= 1 independent paths per utterance from one
 * forward pass (two launches).
 *   pc_llhs    packed per-state log-likelihoods, as for beer_hmm_viterbi
 *   uniforms   [nsamples, n_frames] fp64 in [0, 1), frame index as in frame_off
 *   alpha_ws   caller-provided, n_elems doubles with the layout of pc_llhs; on return the
 *              normalised forward values in log space,
 *                alpha_ws[llh_off[u] + t*S + j] = ln alpha_t(j) - ln sum_i alpha_t(i)
 *              (-inf for unreachable states); arithmetic is fp64 whatever the dtype
 *   path       [nsamples, n_frames] int64: the state index, or with `map_pdf` != 0 the pdf id
 * The rule of a draw.  Last frame: weights w_j = exp(alpha_{T-1}(j) + final_j) over the states
 * j = 0..S-1.  Frame t < T-1, given the drawn s_{t+1}: w_e = exp(alpha_t(src_e) + in_w_e) over
 * the in-arcs e of s_{t+1} in CSR order (source ascending).  The chosen term is the first whose
 * inclusive running sum exceeds u * total; if rounding leaves none, the last term of non-zero
 * weight.  A term of weight 0 is never chosen, not even at u = 0.  Where total is 0 or not
 * finite (an utterance the graph cannot explain) the row's first arc is taken -- state 0 at the
 * last frame or where a row has no arc: deterministic, no NaN, no index out of range.
 * EINVAL: nsamples < 1 or more than 4 * 65535, a dtype other than BEER_F32 / BEER_F64, more
 * than 32767 states, or a graph whose two trellis rows do not fit a CU's LDS (about 10000
 * states); checked before anything is launched. */
int beer_hmm_sample_paths(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                          const double* uniforms, int32_t nsamples, double* alpha_ws,
                          int64_t* path, int map_pdf, void* stream);

/* The forms beer_hmm_sample_paths picks for this batch (host only: it reads max_states and
 * max_arcs and launches nothing), built from the launcher's own expressions:
 *   chunk | BEER_SAMPLE_ARCS_LDS | BEER_SAMPLE_QUAD | waves << 12
 * With S = max_states, A = max_arcs, w = 4 / 8 bytes of the dtype, row = 8 S + 32 bytes (a
 * trellis row and the uniforms of its frame):
 *   chunk   frames of the trellis the draw stages into LDS at a time: 32 when 32 rows take at
 *           most 32 KiB, else 8 when 8 rows do, else 2
 *   BEER_SAMPLE_ARCS_LDS  both kernels keep the arc lists in LDS:
 *           max(chunk * row, 16 S + 128) + 4 (S + 2 + A) + w A <= 64 KiB; else they are read
 *           from global memory
 *   BEER_SAMPLE_QUAD      the forward pass runs four lanes per state on 512 threads
 *           (4 S <= 512); else one thread per state on 256 threads, strided beyond
 *   waves   samples of one utterance per workgroup of the draw, one wave each: 1 when
 *           nsamples == 1, else 4
 * BEER_SAMPLE_CHUNK(route) and BEER_SAMPLE_WAVES(route) are the two numbers alone.  Whether a
 * row is scanned by one lane (at most BEER_SEG terms) or by the wave is decided per row inside
 * the kernel.  BEER_EINVAL exactly where beer_hmm_sample_paths refuses the batch. */
#define BEER_SAMPLE_ARCS_LDS 0x100
#define BEER_SAMPLE_QUAD 0x200
#define BEER_SAMPLE_CHUNK(route) ((route) & 0xFF)
#define BEER_SAMPLE_WAVES(route) (((route) >> 12) & 0xF)
int beer_hmm_sample_route(int dtype, const beer_batch* batch_h, int32_t nsamples);

/* The log-evidence ln p(x_0 .. x_{T-1}) of every utterance under its graph, summed over all
 * state paths: the forward pass alone, one launch, no trellis and no workspace.
 *   pc_llhs         packed per-state log-likelihoods, as for beer_hmm_viterbi (read only)
 *   utt_evidence    [nutt] fp64 whatever the dtype, written (=)
 *   frame_evidence  nullable, [n_frames] fp64, written (=), frame index as in frame_off; with
 *                   or without it `utt_evidence` is the same, bit for bit
 * Definition, over the full in-CSR (hub and bigram arcs included, as beer_hmm_viterbi and
 * beer_hmm_sample_paths read it), l_t(j) the log-likelihoods, w_ij the arcs' log-weights:
 *   a_0(j) = init_j + l_0(j)
 *   a_t(j) = l_t(j) + ln sum_i exp(â_{t-1}(i) + w_ij)
 *   c_t    = ln sum_j exp(a_t(j)),    â_t = a_t - c_t
 *   frame_evidence[frame_off[u] + t] = c_t            = ln p(x_t | x_0 .. x_{t-1}), no final term
 *   utt_evidence[u] = sum_t c_t + ln sum_j exp(â_{T-1}(j) + final_j)
 * which is the reference's `lognorm` (graph.py:289-326) and the logarithm of the sum, over all
 * S^T state paths, of exp(path score).  Log space: maxima, differences, running sums and the
 * per-utterance sum are fp64, exp / log of a difference to the maximum are in the model's
 * precision; no range flags, no redo path.  (The one-wave form below works on scaled fp64
 * probabilities and owns the hand-over: inside the kernel, an utterance in which a frame has no
 * reachable state or a normaliser below 2^-800, or whose graph has an arc weight exp(w) the
 * dtype cannot hold, is started again in log space; a state whose mass falls below 2^-1022 of
 * its frame's total without that showing is lost, as in beer_hmm_forward_backward.)
 * Edges.  -inf log-likelihoods and unreachable states are legal.  From the first frame at which
 * no state is reachable, frame_evidence is -inf for the rest of the utterance and utt_evidence[u]
 * is -inf.  When only the final term is unreachable the frames stay finite and utt_evidence[u] is
 * -inf.  Inputs without NaN give no NaN, and no utterance sees another's values (NaN inputs are
 * outside the contract).  T = 1 is legal; an utterance of no frames gets utt_evidence[u] = 0.
 * EINVAL exactly where beer_hmm_sample_paths refuses the batch: a dtype other than BEER_F32 /
 * BEER_F64, more than 32767 states, or a graph whose two fp64 rows (plus 128 bytes) do not fit a
 * CU's 160 KiB of LDS (more than 10232 states); also a NULL pc_llhs or utt_evidence.  Everything
 * is checked before anything is launched. */
int beer_hmm_log_evidence(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                          double* utt_evidence, double* frame_evidence, void* stream);

/* The form beer_hmm_log_evidence picks for this batch (host only: it reads max_states and
 * max_arcs and launches nothing), built from the launcher's own expressions.  With
 * S = max_states, A = max_arcs, w = 4 / 8 bytes of the dtype and
 * arcs = 4 (S + 2 + A) + w A bytes (the in-CSR of the largest graph):
 *   BEER_EVIDENCE_WAVE | SPL    one wave per utterance, four utterances per workgroup, SPL
 *           states per lane -- 1 (S <= 64), 2 (S <= 128) or 4 (S <= 256) -- the normalised row
 *           and the utterance's own arc lists in the wave's slice of LDS, no workgroup barrier
 *           in the frame loop, utterances handed to waves longest first (batch->order); the wave
 *           runs on scaled probabilities (one exponential per state and frame, none on an arc)
 *           and starts an utterance that leaves fp64's range again in log space:
 *           S <= 256 and 512 SPL + arcs <= 16 KiB
 *   BEER_EVIDENCE_BLOCK | BEER_EVIDENCE_ARCS_LDS | BEER_EVIDENCE_QUAD    else: one workgroup per
 *           utterance;
 *           BEER_EVIDENCE_ARCS_LDS  the arc lists are kept in LDS: 16 S + 128 + arcs <= 64 KiB;
 *                                   else they are read from global memory
 *           BEER_EVIDENCE_QUAD      four lanes per state on 512 threads (4 S <= 512); else one
 *                                   thread per state on 256 threads, strided beyond
 * BEER_EVIDENCE_FAMILY(route) is the family alone, BEER_EVIDENCE_SPL(route) the states per lane
 * of the wave form.  BEER_EINVAL exactly where beer_hmm_log_evidence refuses the batch. */
#define BEER_EVIDENCE_WAVE 0x1000
#define BEER_EVIDENCE_BLOCK 0x2000
#define BEER_EVIDENCE_ARCS_LDS 0x100
#define BEER_EVIDENCE_QUAD 0x200
#define BEER_EVIDENCE_FAMILY(route) ((route) & 0xF000)
#define BEER_EVIDENCE_SPL(route) ((route) & 0xF)
int beer_hmm_evidence_route(int dtype, const beer_batch* batch_h);

/* The categories of beer_hmm_arc_posteriors: device arrays over the graphs of the batch, graph g
 * of `beer_batch.graphs` at its own offsets:
 *   arc_cat    category of every arc in the graph's out-CSR order over the FULL CSR (by source,
 *              destinations ascending: `out_ptr` / `out_dst`; hub and bigram arcs are explicit in
 *              it, as beer_hmm_sample_paths and beer_hmm_log_evidence read them): arc a of graph g
 *              at arc_cat[arc_off[g] + a]
 *   init_cat   category of every state's posterior at the FIRST frame: state j of graph g at
 *              init_cat[state_off[g] + j]
 * Every entry lies in [0, n_cat) or is -1, "count nothing"; the caller answers for that range
 * (an entry >= n_cat writes out of bounds).  Not beer_cat_map, which describes the low-degree
 * image and counts the LAST frame. */
typedef struct {
    const int32_t* arc_cat;
    const int32_t* init_cat;
    const int64_t* arc_off;    /* [n_graphs] */
    const int64_t* state_off;  /* [n_graphs] */
} beer_arc_map;

/* Arc posteriors by category: forward-backward over a ragged batch, every arc's posterior at
 * every frame folded into the caller's categories and kept per frame, summed per utterance, or
 * both.  One launch, one workgroup per utterance.
 *   pc_llhs    packed per-state log-likelihoods, as for beer_hmm_viterbi (read only)
 *   map        the categories (above); n_cat >= 1 their number
 *   ws         caller-provided fp64 scratch of n_frames + n_elems +
 *              beer_hmm_arcs_scratch_doubles() doubles (n_elems: the elements of pc_llhs).  On
 *              return ws[frame_off[u] + t] = c_t, the normalisers of beer_hmm_log_evidence, and
 *              ws[n_frames + llh_off[u] + t*S + j] = â_t(j), its normalised forward values in
 *              log space (-inf: unreachable), up to the frame at which an utterance died
 *   frame_out  nullable, [n_frames, n_cat] of dtype, written (=), frame index as in frame_off
 *   utt_out    nullable, [nutt, n_cat] fp64 whatever the dtype, written (=)
 * Definition.  For utterance u of T frames, gamma and xi the exact posteriors under pc_llhs and
 * the graph's init / arc / final weights (the recursion beer_hmm_log_evidence documents, and its
 * backward counterpart):
 *   frame_out[frame_off[u], c]     = sum over the states j with init_cat[j] = c of gamma_0(j)
 *   frame_out[frame_off[u] + t, c] = sum over the arcs e = (i -> j) with arc_cat[e] = c of
 *                                    P(s_{t-1} = i, s_t = j | x),              t = 1 .. T - 1
 *   utt_out[u, c] = sum_t of those rows
 * Row t says how frame t was entered: a row sums to 1 when no category is -1.  With
 * arc_cat[e] = dst(e), init_cat[j] = j, n_cat = S the rows are gamma; with one category per arc
 * and init_cat = -1 they are the sparse per-frame xi.
 * Arithmetic.  Maxima, differences, sums, the trellis and the bins are fp64; exp / log are in
 * the model's precision.  The backward pass walks the out-row of every source once per frame:
 * an arc's posterior is exp(â_{t-1}(i) + w_ij + l_t(j) + b_t(j) - c_t), one exponential per arc
 * and frame, the sum over the row is gamma_{t-1}(i) and b_{t-1}(i) = ln gamma_{t-1}(i) -
 * â_{t-1}(i) after the row sums have been normalised to 1 (they are 1 but for rounding).  Bins
 * are summed with atomic adds, whose order is not fixed: the last bits can differ between runs.
 * Edges.  -inf log-likelihoods and unreachable states are legal.  An utterance whose evidence is
 * -inf (a frame with nothing reachable, an unreachable final) gets zeros in all its rows and in
 * utt_out.  Inputs without NaN give no NaN.  T = 1 is legal (the init row alone); an utterance of
 * no frames writes nothing to frame_out and zeros to utt_out.  pc_llhs is not modified.
 * EINVAL, checked before anything is launched: where beer_hmm_sample_paths refuses the batch (a
 * dtype other than BEER_F32 / BEER_F64, more than 32767 states, a graph whose two fp64 rows plus
 * 128 bytes do not fit a CU's 160 KiB of LDS); n_cat < 1; a NULL map or map member; frame_out
 * and utt_out both NULL; with utterances in the batch a NULL pc_llhs or ws.  n_cat has no upper
 * limit: bins that do not fit LDS are the output rows themselves. */
int beer_hmm_arc_posteriors(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                            const beer_arc_map* map, int n_cat, double* ws, void* frame_out,
                            double* utt_out, void* stream);

/* Doubles `ws` of beer_hmm_arc_posteriors must hold BESIDES one per frame (the normalisers) and
 * one per element of pc_llhs (the trellis), which the host-side descriptor does not know: 0 for
 * the one form there is, and for a batch the launch refuses. */
size_t beer_hmm_arcs_scratch_doubles(int dtype, const beer_batch* batch_h);

/* The form beer_hmm_arc_posteriors picks (host only: it reads max_states and max_arcs and
 * launches nothing), built from the launcher's own plan; `want_frames` != 0: frame_out is
 * given.  With S = max_states, A = max_arcs, w = 4 / 8 bytes of the dtype, rows = 16 S + 128
 * bytes (two fp64 rows and the reduction scratch), arcs = 4 (S + 2 + 2 A) + w (A + 1) bytes (the
 * out-CSR of the largest graph with its categories; the in-CSR of the forward pass is staged in
 * the same place first); a bin is 8 bytes:
 *   BEER_ARCS_BLOCK        one workgroup of 256 threads per utterance, a thread per state,
 *                          strided beyond (the only family)
 *   BEER_ARCS_ARCS_LDS     the arc lists and categories are kept in LDS: rows + arcs <= 64 KiB;
 *                          else they are read from global memory
 *   BEER_ARCS_FRAME_LDS    a frame's bins are fp64 in LDS, summed with LDS atomic adds and
 *                          written as a row once per frame: want_frames, n_cat <= 1024 and
 *                          rows <= 96 KiB (6136 states); else (with want_frames) the rows of
 *                          frame_out are zeroed and take global atomic adds in the dtype
 *   BEER_ARCS_UTT_LDS      the utterance's bins, when utt_out is given, are fp64 in LDS:
 *                          n_cat <= 4096 and rows <= 96 KiB; else the row of utt_out is zeroed
 *                          and added to in place.  With BEER_ARCS_FRAME_LDS the thread that
 *                          writes bin c of a row adds it to bin c of the utterance; without it
 *                          every arc's posterior is a second atomic add
 * (the launch takes at most 64 + 8 + 32 KiB of LDS with the arcs in it, 96 + 8 + 32 KiB without).
 * BEER_ARCS_FAMILY(route) is the family alone.  BEER_EINVAL exactly where
 * beer_hmm_arc_posteriors refuses the batch and n_cat. */
#define BEER_ARCS_BLOCK 0x1000
#define BEER_ARCS_ARCS_LDS 0x100
#define BEER_ARCS_FRAME_LDS 0x200
#define BEER_ARCS_UTT_LDS 0x400
#define BEER_ARCS_FAMILY(route) ((route) & 0xF000)
int beer_hmm_arcs_route(int dtype, const beer_batch* batch_h, int n_cat, int want_frames);

/* Viterbi max-marginals: for every frame and state, and for every arc folded into the caller's
 * categories, the score of the best path forced through it minus the score of the best path.
 * The max-product twin of beer_hmm_arc_posteriors: 0 on the Viterbi path, negative off it,
 * -inf where no path passes.  One launch, one workgroup per utterance, no exponential.
 *   pc_llhs    packed per-state log-likelihoods, as for beer_hmm_viterbi (read only)
 *   map        nullable, the categories as beer_hmm_arc_posteriors reads them (beer_arc_map);
 *              n_cat >= 1 their number.  NULL is legal when frame_out and utt_out are NULL
 *   ws         caller-provided fp64 scratch of n_elems + beer_hmm_maxmarg_scratch_doubles()
 *              doubles (n_elems: the elements of pc_llhs); its content on return is unspecified
 *   state_out  nullable, [n_elems] of dtype, packed like pc_llhs, written (=): mm
 *   frame_out  nullable, [n_frames, n_cat] of dtype, written (=), frame index as in frame_off
 *   utt_out    nullable, [nutt, n_cat] fp64 whatever the dtype, written (=)
 *   best       [nutt] fp64, written (=): the Viterbi score
 * Definition, over the full CSR (hub and bigram arcs included), l = pc_llhs, init / w / final
 * the graph's weights, for utterance u of T frames:
 *   d_0(j)     = l_0(j) + init_j
 *   d_t(j)     = max_i (d_{t-1}(i) + w_ij) + l_t(j)                      t = 1 .. T-1
 *   e_{T-1}(j) = final_j
 *   e_t(i)     = max_j (w_ij + (l_{t+1}(j) + e_{t+1}(j)))                t = T-2 .. 0
 *   best[u]    = max_j (d_{T-1}(j) + final_j)
 *   mm_t(j)    = (d_t(j) + e_t(j)) - best[u]                              -> state_out
 *   am_t(i->j) = (((d_{t-1}(i) + w_ij) + l_t(j)) + e_t(j)) - best[u]     t >= 1
 *   frame_out[frame_off[u], c]     = max over the states j with init_cat[j] = c of mm_0(j)
 *   frame_out[frame_off[u] + t, c] = max over the arcs e with arc_cat[e] = c of am_t(e)
 *   utt_out[u, c] = max over t of those rows: the relative score of the best path that uses
 *                   category c anywhere
 * A category with no member at a frame holds -inf.  Arithmetic is fp64 whatever the dtype
 * (float32 inputs are upcast on load) and the additions are made in exactly the bracketed
 * order: rounding is monotone, so max_i am_t(i->j) == mm_t(j) bit for bit.  Folding is by
 * maximum (integer atomic max on order-preserving keys): the outputs are the same bits on every
 * run.  best and d + e associate the same sums differently: where the sums are not exact, mm on
 * the best path is 0 only up to that rounding and can be a few ulps of the score ABOVE 0.
 * Edges.  -inf log-likelihoods and unreachable states are legal and give -inf.  An utterance
 * with best = -inf gets -inf in all its outputs, never NaN; inputs without NaN give no NaN.
 * T = 1 is legal.  An utterance of no frames gets best = -inf and utt_out = -inf ("no frame, no
 * path", as beer_hmm_viterbi_nbest has it) and nothing in the per-frame outputs.  pc_llhs is
 * not modified; no utterance sees another's values.
 * EINVAL, checked before anything is launched: where beer_hmm_sample_paths refuses the batch (a
 * dtype other than BEER_F32 / BEER_F64, more than 32767 states, a graph whose two fp64 rows plus
 * 128 bytes do not fit a CU's 160 KiB of LDS); n_cat < 1 with a map; a NULL map member;
 * frame_out or utt_out without a map; all three outputs NULL; with utterances in the batch a
 * NULL best, pc_llhs or ws.  n_cat has no upper limit. */
int beer_hmm_max_marginals(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                           const beer_arc_map* map, int n_cat, double* ws, void* state_out,
                           void* frame_out, double* utt_out, double* best, void* stream);

/* Doubles `ws` of beer_hmm_max_marginals must hold BESIDES one per element of pc_llhs (the
 * trellis): 0 for the one form there is -- what a thread holds between two frames lives in a
 * register or in the trellis itself -- and for a batch the launch refuses. */
size_t beer_hmm_maxmarg_scratch_doubles(int dtype, const beer_batch* batch_h);

/* The form beer_hmm_max_marginals picks (host only: it reads max_states and max_arcs and
 * launches nothing), built from the launcher's own plan; want_state / want_frames / want_utt
 * != 0: that output is given.  With S = max_states, A = max_arcs, w = 4 / 8 bytes of the dtype,
 * cats = want_frames or want_utt, rows = 16 S + 128 bytes (two fp64 rows and the reduction
 * scratch), arcs = 4 (S + 2 + A) + w (A + 1) bytes, plus 4 A with cats (the out-CSR of the
 * largest graph, with its categories when they are read; the in-CSR of the forward pass is
 * staged in the same place first); a bin is 8 bytes:
 *   BEER_MAXMARG_BLOCK     one workgroup of 256 threads per utterance, a thread per state,
 *                          strided beyond (the only family)
 *   BEER_MAXMARG_ARCS_LDS  the arc lists (and categories) are kept in LDS:
 *                          rows + arcs <= 64 KiB; else they are read from global memory
 *   BEER_MAXMARG_BINS_LDS  the bins of a frame (with want_frames) and of the utterance (with
 *                          want_utt) are 64-bit keys in LDS under LDS integer atomic max, a
 *                          frame's written as a row once per frame by the threads that also
 *                          own the utterance's: cats, n_cat <= 2048 and rows <= 96 KiB (6136
 *                          states); else (with cats) the output rows themselves hold keys of
 *                          their dtype, take global integer atomic max and are decoded in
 *                          place at the end
 * (the launch takes at most 64 + 32 KiB of LDS with the arcs in it, 96 + 32 KiB without).
 * BEER_MAXMARG_FAMILY(route) is the family alone.  BEER_EINVAL where beer_hmm_max_marginals
 * refuses the batch, all three wants 0, or cats with n_cat < 1. */
#define BEER_MAXMARG_BLOCK 0x1000
#define BEER_MAXMARG_ARCS_LDS 0x100
#define BEER_MAXMARG_BINS_LDS 0x200
#define BEER_MAXMARG_FAMILY(route) ((route) & 0xF000)
int beer_hmm_maxmarg_route(int dtype, const beer_batch* batch_h, int n_cat, int want_state,
                           int want_frames, int want_utt);

/* The closures of beer_hmm_segment_margins: device arrays built on the host once per distinct
 * graph (hmm_kernels.segment_map).  The closure of category c in graph g is the set of states
 * reachable from the category's entry states -- the destinations of the arcs with arc_cat == c
 * and the states with init_cat == c -- through arcs with arc_cat == -1; only these can carry r
 * (below).  Closure k = g * n_cat + c holds the members mem_ptr[k] .. mem_ptr[k + 1] - 1, a
 * member's LOCAL index is its position in its closure:
 *   members    the member's state in its graph
 *   mem_init   1 when init_cat of that state == c, else 0
 *   in_ptr     [n_members + 1] the member's in-arcs with arc_cat == -1 (their sources are
 *              members of the same closure): in_src the source's LOCAL index, in_arc the arc's
 *              index in the graph's out-CSR (where its weight is read)
 *   ent_ptr    [n_members + 1] the member's in-arcs with arc_cat == c: ent_src the source STATE
 *              (any state of the graph), ent_arc the arc's index in the out-CSR
 *   max_closure the largest number of members of a closure (0: no category has a member) */
typedef struct {
    const int32_t* mem_ptr;    /* [n_graphs * n_cat + 1] */
    const int32_t* members;
    const int32_t* mem_init;
    const int32_t* in_ptr;
    const int32_t* in_src;
    const int32_t* in_arc;
    const int32_t* ent_ptr;
    const int32_t* ent_src;
    const int32_t* ent_arc;
    int32_t max_closure;
    int32_t reserved;
} beer_seg_map;

/* Unit segment lattices: the max-marginal of a whole segment.  With the categories of
 * beer_hmm_arc_posteriors / beer_hmm_max_marginals (beer_arc_map), for a path z_0 .. z_{T-1}:
 * frame 0 is a boundary with label init_cat[z_0]; frame t >= 1 is a boundary with label
 * arc_cat(z_{t-1} -> z_t) when that label is >= 0.  The path HAS THE SEGMENT (c, s, e) when s is a
 * boundary with label c, no frame in s+1 .. e is a boundary, and e + 1 is a boundary or
 * e = T - 1.  seg(c, s, e) is the maximum score over the paths that have the segment, minus
 * best; -inf when there is none.  With d, e and best as in beer_hmm_max_marginals:
 *   X_{T-1}(i) = final_i
 *   X_t(i)     = max over arcs i->j with arc_cat >= 0 of (w_ij + (l_{t+1}(j) + e_{t+1}(j)))   t < T-1
 *   r_s(j)     = d_0(j) if init_cat[j] == c else -inf                                         s = 0
 *   r_s(j)     = max over arcs i->j with arc_cat == c of ((d_{s-1}(i) + w_ij) + l_s(j))       s >= 1
 *   r_t(j)     = max over arcs i->j with arc_cat == -1 of ((r_{t-1}(i) + w_ij) + l_t(j))      t = s+1 ..
 *   seg(c,s,e) = max_i (r_e(i) + X_e(i)) - best
 * All of it fp64 whatever the dtype (float32 inputs are upcast on load), the additions in
 * exactly the bracketed order, every fold a maximum: the same bits on every run.  On inputs
 * whose sums are exact, max_e seg(c, s, e) is the start margin frame_out[s, c].
 *
 * beer_hmm_segment_trellis: one launch, one workgroup per utterance, the shape of
 * beer_hmm_max_marginals.
 *   map, n_cat the categories, n_cat >= 1
 *   d, x       [n_elems] fp64 each, packed like pc_llhs, written (=): d_t(j) and X_t(i); an
 *              utterance with best = -inf gets X = -inf
 *   ws         fp64 scratch of beer_hmm_segments_scratch_doubles() doubles (NULL when that is 0)
 *   frame_out  [n_frames, n_cat] of dtype, written (=): the start margins, with exactly the
 *              meaning and the bits of beer_hmm_max_marginals' frame_out
 *   best       [nutt] fp64, written (=); -inf for an utterance of no frames
 * EINVAL where beer_hmm_max_marginals refuses the batch with frame_out given; a NULL map or map
 * member; n_cat < 1; with utterances in the batch a NULL pc_llhs, d, x, frame_out or best, or a
 * NULL ws where the scratch is not 0. */
int beer_hmm_segment_trellis(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                             const beer_arc_map* map, int n_cat, double* d, double* x, double* ws,
                             void* frame_out, double* best, void* stream);

/* beer_hmm_segment_margins: expands a list of entries (frame, category) into their segment
 * margins, from the trellises and best that beer_hmm_segment_trellis wrote for the same batch,
 * pc_llhs and categories.
 *   entry_frame [n_entries] the frame of the entry, indexed as in frame_off
 *   entry_cat   [n_entries] its category
 *   entry_off   [nutt + 1] the entries are sorted by utterance: those of utterance u are
 *               entry_off[u] .. entry_off[u + 1] - 1
 *   out         [n_entries, max_dur] of dtype, written (=): column k holds
 *               seg(c, s, s + k); -inf where the segment is impossible or runs past the utterance
 * A team of L lanes handles an entry (L: the smallest power of two in 4 .. 256 that is
 * >= max_closure; lanes stride over larger closures), a workgroup of 256 threads holds 256 / L
 * teams, each with two fp64 rows of max_closure (at least 1) doubles and two 8-byte key slots in
 * LDS.  An entry whose category is outside [0, n_cat), whose frame is outside its utterance or
 * whose utterance has best = -inf gets -inf in its row.
 * EINVAL where beer_hmm_segment_trellis refuses the batch; a NULL seg map; max_closure < 0 or
 * above max_states; (256 / L) (16 max(max_closure, 1) + 16) bytes above 64 KiB (max_closure >
 * 4095); n_entries < 0; max_dur < 1; with entries and utterances a NULL member or argument. */
int beer_hmm_segment_margins(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                             const beer_seg_map* seg_map, int n_cat, const double* d,
                             const double* x, const double* best, const int64_t* entry_frame,
                             const int32_t* entry_cat, const int64_t* entry_off,
                             int64_t n_entries, int max_dur, void* out, void* stream);

/* Doubles `ws` of beer_hmm_segment_trellis must hold: nutt * max_states where a thread owns
 * several states (max_states > 256: e_{t-1} waits in the utterance's row, the d trellis being
 * kept), else 0; 0 for a batch the launch refuses. */
size_t beer_hmm_segments_scratch_doubles(int dtype, const beer_batch* batch_h);

/* The form the two launches pick (host only), built from the launchers' own plan.  With rows,
 * arcs (with the categories) and the thresholds of beer_hmm_maxmarg_route at want_frames:
 *   BEER_SEGMENTS_BLOCK     the trellis kernel: one workgroup of 256 threads per utterance
 *   BEER_SEGMENTS_ARCS_LDS  its arc lists and categories are kept in LDS: rows + arcs <= 64 KiB
 *   BEER_SEGMENTS_BINS_LDS  its bins are 64-bit keys in LDS: n_cat <= 2048 and rows <= 96 KiB;
 *                           else the rows of frame_out hold keys and are decoded at the end
 *   BEER_SEGMENTS_TEAM(route)  the lanes L of a team of the expand kernel, 4 .. 256
 * BEER_EINVAL exactly where beer_hmm_segment_trellis or, with this max_closure,
 * beer_hmm_segment_margins refuses the batch and n_cat. */
#define BEER_SEGMENTS_BLOCK 0x1000
#define BEER_SEGMENTS_ARCS_LDS 0x100
#define BEER_SEGMENTS_BINS_LDS 0x200
#define BEER_SEGMENTS_FAMILY(route) ((route) & 0xF000)
#define BEER_SEGMENTS_TEAM(route) (1 << ((route) & 0xF))
int beer_hmm_segments_route(int dtype, const beer_batch* batch_h, int n_cat, int max_closure);

/* Segment posteriors: the sum-product twin of the unit segment lattice.  Categories, boundaries
 * and "the path HAS THE SEGMENT (c, s, e)" are exactly those of beer_hmm_segment_trellis above:
 * frame 0 is a boundary labelled init_cat[z_0], frame t >= 1 one labelled arc_cat(z_{t-1} -> z_t)
 * when that is >= 0; the segment runs from boundary s with label c through frames without a
 * boundary to e, where e + 1 is a boundary or e = T - 1.
 *   post(c, s, e) = P(the path has the segment (c, s, e) | x_0 .. x_{T-1})
 * under pc_llhs and the graph's init / arc / final weights.  With â_t, c_t as
 * beer_hmm_log_evidence documents them, f = ln sum_j exp(â_{T-1}(j) + final_j) and the normalised
 * backward values of beer_hmm_arc_posteriors:
 *   b_{T-1}(j) = final_j - f
 *   b_{t-1}(i) = ln sum over arcs i->j of exp(w_ij + l_t(j) + b_t(j)) - c_t
 *   Y_{T-1}(i) = final_i - f
 *   Y_t(i)     = ln sum over arcs i->j with arc_cat >= 0 of exp(w_ij + l_{t+1}(j) + b_{t+1}(j))
 *                - c_{t+1}                                                              t < T-1
 *   r_s(j)     = â_0(j) if init_cat[j] == c else -inf                                   s = 0
 *   r_s(j)     = ln sum over arcs i->j with arc_cat == c of exp(â_{s-1}(i) + w_ij)
 *                + l_s(j) - c_s                                                         s >= 1
 *   r_t(j)     = ln sum over arcs i->j with arc_cat == -1 of exp(r_{t-1}(i) + w_ij)
 *                + l_t(j) - c_t                                                         t = s+1 ..
 *   post(c,s,e) = sum_i exp(r_e(i) + Y_e(i))
 * sum_e post(c, s, e) is the start posterior frame_out[s, c] of beer_hmm_arc_posteriors, and
 * ln p(x) = sum_t c_t + f.  Only members of the closure of c (beer_seg_map) can carry r, and
 * r_t(j) <= â_t(j): the expand kernel carries the ratio rho_t(j) = exp(r_t(j) - â_t(j)) in [0, 1],
 *   rho_t(j) = sum over arcs i->j of category -1 of
 *              rho_{t-1}(i) exp((â_{t-1}(i) + w_ij) + ((l_t(j) - c_t) - â_t(j)))
 *   post(c,s,e) = sum_j rho_e(j) exp(â_e(j) + Y_e(j))
 * one exponential of a log-probability per arc and step, no logarithm; an underflow is 0.
 * Arithmetic.  Differences, sums, the trellises, the rows and the folds are fp64; exp / log are in
 * the model's precision, as in beer_hmm_arc_posteriors.
 *
 * beer_hmm_segpost_trellis: one launch, one workgroup of 256 threads per utterance, the shape of
 * beer_hmm_arc_posteriors.
 *   map, n_cat the categories, n_cat >= 1
 *   alpha, y   [n_elems] fp64 each, packed like pc_llhs, written (=): â_t(j) and Y_t(i) (-inf:
 *              unreachable, or nothing goes on); of an utterance whose evidence is -inf their
 *              content is unspecified
 *   norm       [n_frames] fp64, written (=): c_t, up to the frame at which an utterance died
 *   frame_out  [n_frames, n_cat] of dtype, written (=): the start posteriors, with the meaning of
 *              beer_hmm_arc_posteriors' frame_out
 *   evidence   [nutt] fp64, written (=): ln p(x); 0 for an utterance of no frames, as
 *              beer_hmm_log_evidence has it
 * Every value of alpha and y is written by the thread that owns its state, every sum of a row in
 * the row's order: the two trellises, norm and evidence are the same bits on every run.  The bins
 * of frame_out take atomic adds, whose order is not fixed.
 * Edges.  -inf log-likelihoods and unreachable states are legal.  An utterance whose evidence is
 * -inf gets zeros in frame_out; T = 1 and an utterance of no frames are legal; inputs without NaN
 * give no NaN; pc_llhs is not modified.
 * EINVAL, checked before anything is launched: where beer_hmm_arc_posteriors refuses the batch
 * with frame_out given; a NULL map or map member; n_cat < 1; with utterances in the batch a NULL
 * pc_llhs, alpha, y, norm, frame_out or evidence. */
int beer_hmm_segpost_trellis(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                             const beer_arc_map* map, int n_cat, double* alpha, double* y,
                             double* norm, void* frame_out, double* evidence, void* stream);

/* beer_hmm_segment_posteriors: expands a list of entries (frame, category) into their segment
 * posteriors, from the trellises, norm and evidence that beer_hmm_segpost_trellis wrote for the
 * same batch, pc_llhs and categories.  entry_frame, entry_cat, entry_off as
 * beer_hmm_segment_margins takes them.
 *   out         [n_entries, max_dur] of dtype, written (=): column k holds post(c, s, s + k); 0
 *               where the segment is impossible or runs past the utterance
 * A team of L lanes handles an entry (L: the smallest power of two in 4 .. 256 that is
 * >= max_closure; lanes stride over larger closures), a workgroup of 256 threads holds 256 / L
 * teams, each with four fp64 rows of max_closure (at least 1) doubles (rho and â of the closure,
 * ping-pong) and eight 8-byte slots in LDS.  The fold over a team is a sum in a fixed order
 * (cross-lane moves within a wave, then the waves' partial sums in order), no atomic add: given
 * the same trellises and entries, `out` is the same bits on every run.  An entry whose category is
 * outside [0, n_cat), whose frame is outside its utterance or whose utterance has evidence -inf
 * gets zeros in its row.
 * EINVAL where beer_hmm_segpost_trellis refuses the batch; a NULL seg map or member;
 * max_closure < 0 or above max_states; (256 / L) (32 max(max_closure, 1) + 64) bytes above 64 KiB
 * (max_closure > 2046); n_entries < 0; max_dur < 1; with entries and utterances a NULL argument. */
int beer_hmm_segment_posteriors(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                                const beer_seg_map* seg_map, int n_cat, const double* alpha,
                                const double* y, const double* norm, const double* evidence,
                                const int64_t* entry_frame, const int32_t* entry_cat,
                                const int64_t* entry_off, int64_t n_entries, int max_dur,
                                void* out, void* stream);

/* The form the two launches pick (host only), built from the launchers' own plan.  With S =
 * max_states, A = max_arcs, w = 4 / 8 bytes of the dtype, rows = 16 S + 128 bytes and arcs =
 * 4 (S + 2 + 2 A) + w (A + 1) bytes as beer_hmm_arcs_route has them:
 *   BEER_SEGPOSTS_BLOCK     the trellis kernel: one workgroup of 256 threads per utterance
 *   BEER_SEGPOSTS_ARCS_LDS  its arc lists and categories are kept in LDS: rows + arcs <= 64 KiB
 *   BEER_SEGPOSTS_BINS_LDS  a frame's bins are fp64 in LDS and written as a row once per frame:
 *                           n_cat <= 1024 and rows <= 96 KiB; else the rows of frame_out are
 *                           zeroed and take global atomic adds in the dtype
 *   BEER_SEGPOSTS_TEAM(route)  the lanes L of a team of the expand kernel, 4 .. 256
 * BEER_EINVAL exactly where beer_hmm_segpost_trellis or, with this max_closure,
 * beer_hmm_segment_posteriors refuses the batch and n_cat.  The trellis kernel keeps nothing
 * besides the two trellises and norm: there is no scratch to size. */
#define BEER_SEGPOSTS_BLOCK 0x1000
#define BEER_SEGPOSTS_ARCS_LDS 0x100
#define BEER_SEGPOSTS_BINS_LDS 0x200
#define BEER_SEGPOSTS_FAMILY(route) ((route) & 0xF000)
#define BEER_SEGPOSTS_TEAM(route) (1 << ((route) & 0xF))
int beer_hmm_segposts_route(int dtype, const beer_batch* batch_h, int n_cat, int max_closure);

/* One-hot posteriors of a given state path (hmm.py:42-58: viterbi=True /
 * state_path= branches): gamma one-hot, xi_sum[p_t, p_t+1] += 1,
 * gamma0_sum[p_0] += 1. */
int beer_hmm_path_posteriors(int dtype, const beer_batch* batch_h,
                             const int64_t* path, void* gamma, double* xi_sum,
                             double* gamma0_sum, void* stream);

/* ---- explicit state durations (hidden semi-Markov model, Ferguson 1980) ------------------
 * Every emitting state owns a law over how long ONE stay lasts, 1 .. D frames; the self-loop
 * of the graph is not used.  No reference counterpart: the definitions below are the contract.
 * For utterance u of T frames on graph g with S states:
 *   id(j)    the pdf id of state j (the batch's pdf_ids)
 *   l_t(j)   the packed pc_llhs
 *   lam_j(d) = log_dur[id(j)][d-1], d = 1 .. D; `log_dur` is a device table [S_total, D] fp64;
 *            -inf entries are legal (a minimum duration is a row that starts with -inf); a state
 *            whose id is outside 0 .. S_total-1 has lam = -inf throughout
 *   w_ij     = trans_ij + leave_w[id(i)] for every arc with i != j; `leave_w` [S_total] fp64,
 *            nullable (NULL: 0), the renormalisation of a state's other arcs once its self-loop
 *            is gone
 * Arcs with src == dst are skipped wherever they are stored, in either CSR or in a hub block (a
 * stay is the duration law's business); `final` gets no leave_w.  With lse the log-sum-exp over
 * the finite terms (-inf when there are none):
 *   beg_0(j)  = init_j                      beg_t(j) = lse_{i != j} end_{t-1}(i) + w_ij
 *   end_t(j)  = lse_{d=1..min(D,t+1)}  beg_{t-d+1}(j) + lam_j(d) + sum_{tau=t-d+1..t} l_tau(j)
 *   Z         = lse_j end_{T-1}(j) + final_j     (the last segment ends ON the last frame)
 *   bend_{T-1}(j) = final_j                 bend_t(j) = lse_{k != j} w_jk + bbeg_{t+1}(k)
 *   bbeg_t(j) = lse_{d=1..min(D,T-t)}  lam_j(d) + sum_{tau=t..t+d-1} l_tau(j) + bend_{t+d-1}(j)
 *   q(j,s,d)  = exp(beg_s(j) + lam_j(d) + sum_{tau=s..s+d-1} l_tau(j) + bend_{s+d-1}(j) - Z)
 * Outputs of beer_hsmm_forward_backward (all nullable but `gamma`; every += array is fp64):
 *   gamma        packed like pc_llhs, in the batch's dtype, written (=):
 *                gamma_t(j) = sum over (s, d) with s <= t < s + d of q(j,s,d); rows sum to 1
 *   utt_evidence [nutt] fp64, written (=): Z
 *   dur_counts   [S_total, D], += sum_s q(j,s,d) at [id(j)][d-1] (ids may repeat within a graph
 *                and across utterances: fp64 atomic adds)
 *   entry_sum    [S], += sum_{s>=1,d} q(j,s,d); the batch must share one graph
 *   gamma0_sum   [S], += sum_d q(j,0,d); the batch must share one graph
 * An utterance with no finite segmentation (Z = -inf) gets the evidence -inf, gamma rows all 0
 * and nothing added to the three count arrays; an utterance of no frames the evidence 0.
 * Numerics: the recursions run in fp64 log space whatever the dtype (exp and log in fp64 too);
 * float32 differs only in the type of pc_llhs, gamma and the graph's weights.  Running segment
 * scores sit in a ring indexed by start (backward: end) mod D: a frame adds l_t(j) - c_t - n to
 * every live slot and takes one lse over the slots with the rotated lam_j -- no differences of
 * prefix sums.  c_t is max_j l_t(j) rounded to an integer and n the previous frame's largest
 * end (backward: begin) value rounded to a multiple of 1/256, so that their running sums are
 * exact; gamma follows from gamma_t = gamma_{t+1} - B_{t+1} + E_t (B, E the begin and end
 * posteriors), clamped at 0.  gamma, the evidence and the Viterbi path are the same bits on
 * every run.  NaN and +inf inputs are outside the contract.
 * `ws`: fp64 workspace of 2 doubles per element of pc_llhs (the beg and end trellises) plus
 * 2 per frame of the batch plus beer_hsmm_scratch_doubles(dtype, batch, D).
 * BEER_EINVAL (everything is checked before anything is launched): a dtype other than
 * BEER_F32 / BEER_F64, D outside 1 .. BEER_HSMM_MAX_DUR, a graph of more than
 * BEER_HSMM_MAX_STATES states, S_total < 1, a NULL pc_llhs, log_dur, ws or gamma. */
#define BEER_HSMM_MAX_DUR 128
#define BEER_HSMM_MAX_STATES 2048
int beer_hsmm_forward_backward(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                               const double* log_dur, const double* leave_w, int D, int S_total,
                               double* ws, void* gamma, double* utt_evidence,
                               double* dur_counts, double* entry_sum, double* gamma0_sum,
                               void* stream);

/* The same recursion with max for lse: `path` [n_frames] int64 receives the state of every
 * frame (graph state indices as beer_hmm_viterbi gives them, pdf ids with `map_pdf`), `score`
 * [nutt] fp64 the score of the best segmentation.  Back-pointers are (source state, duration).
 * Ties: the shorter duration first, then the smaller source state, then at the end the smaller
 * final state.  An utterance without a finite path gets the score -inf and the path -1, one
 * of no frames the score 0.  Reads the graph's full in-CSR, as beer_hmm_viterbi does (a hub's
 * arcs are in it).  `ws` and BEER_EINVAL as above (path and score must not be NULL). */
int beer_hsmm_viterbi(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                      const double* log_dur, const double* leave_w, int D, int S_total,
                      double* ws, int64_t* path, double* score, int map_pdf, void* stream);

/* Doubles `ws` must hold BESIDES the two trellises and the two values per frame: 0 while the
 * rings fit LDS (BEER_HSMM_RING_LDS below), else 2 max_states D for each of the
 * min(nutt, 512) workgroups of the launch.  0 where the entry points refuse the batch. */
size_t beer_hsmm_scratch_doubles(int dtype, const beer_batch* batch_h, int D);

/* The form the two entry points take for this batch and D (host only: it reads the scalar
 * fields of the batch and launches nothing; the launcher decides with the same predicates).
 * One workgroup of 256 threads per utterance, at most 512 workgroups striding over the batch
 * (batch->order: longest first); with S = max_states:
 *   BEER_HSMM_BLOCK | BEER_HSMM_RING_LDS | BEER_HSMM_LOWDEG | LOG2TEAM
 *     LOG2TEAM            log2 of the lanes that share one state's D ring slots: the largest
 *                         power of two `team` <= 64 with team / 2 < D and team S <= 256
 *                         (1 when S > 128); 256 / team states are worked on at a time
 *     BEER_HSMM_RING_LDS  the ring and the duration counts of the utterance, 2 S D doubles,
 *                         sit in LDS beside the 8 S + 32 doubles of per-state rows:
 *                         8 (8 S + 32 + 2 S D) <= 160 KiB; else in `ws`
 *     BEER_HSMM_LOWDEG    forward-backward walks the low-degree images and their hubs:
 *                         all_lowdeg != 0, max_degree > 0 (the host knows the images) and
 *                         max_hubs <= 4; else the full CSR
 * BEER_HSMM_TEAM(route) is the team.  BEER_EINVAL exactly where the entry points refuse the
 * batch for its shape (dtype, D, max_states). */
#define BEER_HSMM_BLOCK 0x1000
#define BEER_HSMM_RING_LDS 0x100
#define BEER_HSMM_LOWDEG 0x200
#define BEER_HSMM_FAMILY(route) ((route) & 0xF000)
#define BEER_HSMM_TEAM(route) (1 << ((route) & 0xF))
int beer_hsmm_route(int dtype, const beer_batch* batch_h, int D);

/* Arc posteriors by category under explicit durations: beer_hsmm_forward_backward -- the same
 * inputs, the same outputs (all nullable but `gamma`), the same arithmetic -- which also folds
 * WHICH ARC every segment was entered by into the caller's categories (beer_arc_map, as
 * beer_hmm_arc_posteriors reads it: `arc_cat` over the full out-CSR, hub and bigram arcs
 * explicit in it; entries in [0, n_cat) or -1, the caller answers for the range).  With the
 * symbols above:
 *   frame_out  nullable, [n_frames, n_cat] of dtype, written (=):
 *                row frame_off[u], category c:  sum over the states j with init_cat[j] = c of
 *                                               sum_d q(j,0,d)
 *                row frame_off[u] + t, t = 1 .. T-1:  sum over the arcs e = (i -> j), i != j,
 *                     with arc_cat[e] = c of exp(end_{t-1}(i) + w_ij + bbeg_t(j) - Z)
 *   utt_out    nullable, [nutt, n_cat] fp64, written (=): the sum of the utterance's rows
 *   total_out  nullable, [n_cat] fp64, accumulated (+=): the sum over the whole batch (what a
 *              model with n_cat = P^2 bigram categories reads: utt_out would be nutt P^2)
 * A row does NOT sum to 1: with no category -1 it sums to B_t = sum_j sum_d q(j,t,d), the
 * posterior that a segment begins at frame t (1 at t = 0).  An arc with src == dst contributes
 * nothing whatever category it carries.
 * The kernel always walks the full CSR, in both directions (the low-degree image hides the arcs
 * behind its hubs).  An arc's posterior is formed in the backward pass where bend_t(i) is: its
 * exponent is (end_t(i) - O_t) + w_ik + (bbeg_{t+1}(k) - Q_{t+1}) + ((N_{t-1} + N'_{t+2}) - Z),
 * the stored values and the exact offset that E_t(i) itself uses, so nothing cancels; one more
 * fp64 exp per arc and frame.  The arc terms of a state sum to its end posterior E_t(i) up to
 * rounding; neither is renormalised by the other.
 * Bins.  With used = 8 (8 S + 32) bytes of rows, plus 16 S D of ring when BEER_HSMM_RING_LDS,
 * S = max_states: a frame's bins are fp64 in LDS, summed with LDS atomic adds and written as a
 * row once per frame, when frame_out is given, n_cat <= 1024 and used + 8 n_cat <= 160 KiB
 * (BEER_HSMM_ARCS_FRAME_LDS); else the rows of frame_out are zeroed and take global atomic adds
 * in the dtype.  The utterance's bins are fp64 in LDS when n_cat <= 4096 and they fit behind
 * that: used [+ 8 n_cat] + 8 n_cat <= 160 KiB (BEER_HSMM_ARCS_UTT_LDS); else its row of utt_out
 * (without utt_out: total_out itself) takes the adds.  The order of atomic adds is not fixed: the
 * last bits of frame_out, utt_out and total_out may differ between runs.  gamma and the evidence
 * are the same bits on every run, and the bits beer_hsmm_forward_backward gives on its full-CSR
 * route.
 * Edges.  An utterance with Z = -inf: its rows and its utt_out row are zeros, nothing is added
 * to total_out, and the shared outputs are as beer_hsmm_forward_backward documents.  T = 1: the
 * init row alone.  No frames: nothing written to frame_out, zeros to utt_out.  -inf inputs are
 * legal; inputs without NaN give no NaN.
 * `ws` as for beer_hsmm_forward_backward, with beer_hsmm_arcs_scratch_doubles for its rings.
 * BEER_EINVAL (everything is checked before anything is launched): where
 * beer_hsmm_forward_backward refuses; n_cat < 1; a NULL map or map member; frame_out, utt_out
 * and total_out all NULL. */
int beer_hsmm_arc_posteriors(int dtype, const beer_batch* batch_h, const void* pc_llhs,
                             const double* log_dur, const double* leave_w, int D, int S_total,
                             const beer_arc_map* map, int n_cat, double* ws, void* gamma,
                             double* utt_evidence, double* dur_counts, double* entry_sum,
                             double* gamma0_sum, void* frame_out, double* utt_out,
                             double* total_out, void* stream);

/* Doubles `ws` of beer_hsmm_arc_posteriors must hold besides the two trellises and the two
 * values per frame: beer_hsmm_scratch_doubles' value (the bins never live in `ws`). */
size_t beer_hsmm_arcs_scratch_doubles(int dtype, const beer_batch* batch_h, int D);

/* The form beer_hsmm_arc_posteriors takes (host only, from the launcher's own plan;
 * `want_frames` != 0: frame_out is given):
 *   BEER_HSMM_BLOCK | BEER_HSMM_RING_LDS | BEER_HSMM_ARCS_FRAME_LDS | BEER_HSMM_ARCS_UTT_LDS |
 *   LOG2TEAM
 * team and ring as beer_hsmm_route has them, never BEER_HSMM_LOWDEG, the two bin bits as
 * defined above.  BEER_EINVAL exactly where beer_hsmm_arc_posteriors refuses the batch, D and
 * n_cat. */
#define BEER_HSMM_ARCS_FRAME_LDS 0x400
#define BEER_HSMM_ARCS_UTT_LDS 0x800
int beer_hsmm_arcs_route(int dtype, const beer_batch* batch_h, int D, int n_cat, int want_frames);

/* Scatter the (scaled) state posteriors back to pdf ids, repeated ids add
 * (DynamicallyOrderedModelSet.accumulate, beer/models/modelset.py:148-154,
 * with the scale of HMM.accumulate, hmm.py:95), and the per-frame expected
 * log-likelihood exp_llh[t] = sum_s gamma[t,s] * pc_llhs[t,s] (hmm.py:87).
 * state_resps [Ttot, S_total] must be zeroed by the caller; `exp_llh`
 * nullable [Ttot]; `utt_llh` nullable fp64 [nutt] (+= sum_t exp_llh). */
int beer_hmm_scatter(int dtype, const beer_batch* batch_h, int S_total,
                     const void* pc_llhs, const void* gamma, double scale,
                     void* state_resps, void* exp_llh, double* utt_llh,
                     void* stream);

/* Per-utterance sums of a per-frame quantity: out[u] += sum_t v[t]
 * (the `exp_llh.sum()` of evidence_lower_bound,
 * beer/inference/objectives.py:184, for every utterance of a batch). */
int beer_segment_sum(int dtype, int32_t nutt, const int64_t* frame_off,
                     const void* v, double* out, void* stream);

/* ---- "statistics-in" E-step (VAE models, beer/models/vae.py:63-89) ---------
 * The prior of a VAE receives dense sufficient statistics [T, Q] (averages of
 * phi(z) over the samples of the latent variable) instead of frames, and its
 * expected log-likelihood is differentiated w.r.t. them. */

/* float32 products with Q >= 512 and T >= 8192 (full-covariance latent) run on
 * the matrix cores in the E-step's bf16x3 arithmetic (float32 operands held
 * exactly as three bf16 pieces, float32 accumulation; sums over frames in chains
 * of 4096 frames, fp64 between workgroups); everything else, and fp64, on an
 * LDS-tiled kernel that accumulates in fp64.  No library underneath.  These entry
 * points take BEER_F32 / BEER_F64 only: BEER_EXACT (the fp32 MFMA of the frame
 * kernels) has no counterpart here -- large float32 shapes are bf16x3, as
 * accurate as a float32 product, in either mode of the host layer. */

/* out[t,k] = sum_q stats[t,q] * exp_stats[k,q] + base   -> [T, K]
 * (ConjugateLikelihood.__call__, beer/dists/normalgamma.py:55-59; base is the
 * log base measure -D/2 ln 2pi). */
int beer_dense_llh(int dtype, int64_t T, int Q, int K, const void* stats,
                   const void* exp_stats, double base, void* out, void* stream);

/* Gradient of sum_t grad[t] * sum_k weights[t,k] * llh[t,k] w.r.t. stats:
 * out[t,q] = grad[t] * sum_k weights[t,k] * exp_stats[k,q]   -> [T, Q].
 * This is what autograd gives the reference for `(pc_llh * resps).sum(-1)`
 * with detached responsibilities (mixture.py:79,92; hmm.py:81-87).
 * `grad` nullable (= 1). */
int beer_dense_llh_backward(int dtype, int64_t T, int K, int Q,
                            const void* weights, const void* grad,
                            const void* exp_stats, void* out, void* stream);

/* acc[k,q] += sum_t weights[t,k] * state_resps[t, k / G] * stats[t,q], fp64
 * [K, Q] (NormalSet.accumulate, normalset.py:121-123, with the joint
 * responsibilities of MixtureSet.accumulate, mixtureset.py:103-106).
 * `state_resps` nullable [T, K / G]. */
int beer_dense_accumulate(int dtype, int64_t T, int K, int Q, int G,
                          const void* weights, const void* state_resps,
                          const void* stats, double* acc, void* stream);

/* Which kernel the three entry points above run for a shape (host only: no pointer, no
 * stream, nothing launched), from the launchers' own decision (dense.hip: dense_form).
 *   op      BEER_DENSE_LLH: beer_dense_llh; BEER_DENSE_BACKWARD: beer_dense_llh_backward;
 *           BEER_DENSE_ACCUMULATE: beer_dense_accumulate (K = S G; any G)
 *   dtype   BEER_F32 / BEER_F64
 * BEER_EINVAL for another op or dtype, T < 0, Q < 1 or K < 1; else family | form:
 *   BEER_DENSE_PLAIN   gemm_kernel<T, TC, ATOMIC> (float64 accumulation)
 *   BEER_DENSE_GEMM3   gemm3_kernel<.., AK, BK, ATOMIC> | BEER_DENSE_T64x128 / _T128x64 /
 *                      _T128x128 | BEER_DENSE_AK | BEER_DENSE_BK; BEER_DENSE_ACCUMULATE:
 *                      | (frames a workgroup sums in float32) / 32 << 8, BEER_DENSE_CHAIN
 * Every form is held against the oracle in tests/test_gpu_vae_prior_routes.py. */
#define BEER_DENSE_LLH 0
#define BEER_DENSE_BACKWARD 1
#define BEER_DENSE_ACCUMULATE 2
#define BEER_DENSE_PLAIN 0x10000000
#define BEER_DENSE_GEMM3 0x20000000
#define BEER_DENSE_FAMILY(route) ((route) & 0x70000000)
#define BEER_DENSE_T64x128 1
#define BEER_DENSE_T128x64 2
#define BEER_DENSE_T128x128 3
#define BEER_DENSE_AK 0x10              /* A contiguous along the inner dimension */
#define BEER_DENSE_BK 0x20              /* B contiguous along the inner dimension */
#define BEER_DENSE_CHAIN(route) (((route) >> 8 & 0xFF) * 32)
int beer_dense_route(int op, int dtype, int64_t T, int Q, int K);

/* out[t] = sum_k a[t,k] * b[t,k]  (exp_llh = (pc_llhs * resps).sum(-1)). */
int beer_rowdot(int dtype, int64_t T, int K, const void* a, const void* b,
                void* out, void* stream);

/* Per (frame, mixture) softmax over G components of pc_llh[T, S*G] +
 * log_weights[S, G] (nullable): log_norm [T, S] and resps [T, S*G], both
 * nullable (mixture.py:78-82, mixtureset.py:92-95). */
int beer_softmax_groups(int dtype, int64_t T, int S, int G, const void* pc_llh,
                        const void* log_weights, void* log_norm, void* resps,
                        void* stream);

/* out[t,:] = (1/ns) sum_s phi(X[t*ns + s]) -> [T, Q]: the sample-averaged
 * statistics a VAE hands to its prior (vae.py:73-74: sufficient_statistics of
 * the [T*ns, D] samples, reshape, mean over the samples) without the
 * [T*ns, Q] intermediate.  ns = 1 is beer_suffstats_expand. */
int beer_suffstats_mean(int dtype, int cov, int64_t T, int ns, int D,
                        const void* X, void* out, void* stream);

/* Backward of beer_suffstats_mean: grad_X[t*ns + s, :] =
 * (1/ns) J_phi(x_ts)^T grad_stats[t, :] -> [T*ns, D]
 * (normalwishart.py:30-38 / normalgamma.py:22-31 / isotropicnormalgamma.py
 * sufficient_statistics differentiated by autograd in the reference). */
int beer_suffstats_backward(int dtype, int cov, int64_t T, int ns, int D,
                            const void* X, const void* grad_stats,
                            void* grad_X, void* stream);

/* ---- one sample per frame: the prior of a VAE on the frame kernels -----------
 * With ONE sample z_t per frame (vae.py:63-86, nsamples = 1) the statistics the
 * prior receives are phi(z_t): its E-step and accumulation are the frame entry
 * points above (beer_mixtureset_estep, beer_normal_accumulate ...) on the samples,
 * and the gradient the reference's autograd carries from `(pc_llhs * resps).sum(-1)`
 * through the statistics to the samples (mixture.py:79,92; hmm.py:81-87;
 * normalwishart.py:30-38) is one product, with no [T, Q] tensor in between:
 *
 *   out[t,:] = grad[t] * sum_k weights[t,k] * d(phi(x_t) . exp_stats[k]) / d x_t  -> [T, D]
 *
 * = beer_suffstats_backward(beer_dense_llh_backward(weights, grad, exp_stats)) at
 * ns = 1.  `grad` nullable (= 1); `weights` [T, K]; `exp_stats` [K, Q] as for
 * beer_dense_llh.  BEER_F32 / BEER_F64.  Full covariance, float32, 8 <= D <= 64,
 * T >= 4096 with a workspace of beer_frames_llh_backward_workspace_bytes (the
 * parameters as bf16x3 MFMA fragments): matrix cores, bf16x3 arithmetic, float32
 * accumulation over the components; diagonal / isotropic, float32, D <= 128: one
 * [T, K] x [K, 2 D] product in the same arithmetic, combined with the frames in
 * its epilogue (HBM-bound).  Other shapes with T >= 4096 and that workspace
 * (<= 256 MiB): the two calls above over chunks of frames whose [frames, Q]
 * gradient fits it.  T < 4096 (the query returns 0), or workspace
 * NULL: one thread per output, float64 accumulation. */
size_t beer_frames_llh_backward_workspace_bytes(int dtype, int cov, int64_t T, int D, int K);
/* Which kernels beer_frames_llh_backward runs (host only), from its own decision
 * (sample_grad.hip: sg_route).  workspace_bytes: 0 = no workspace.  BEER_EINVAL where the
 * entry point refuses the call; else family | form:
 *   BEER_SGRAD_GENERIC   sgrad_generic_kernel<T>
 *   BEER_SGRAD_FULL      sgrad_kernel<NKB>          | NKB (1 / 2)
 *   BEER_SGRAD_DIAG      sgrad_diag_kernel<NJ2>     | NJ2 (2 / 3 / 4 / 8)
 *   BEER_SGRAD_CHUNKED   beer_dense_llh_backward + beer_suffstats_backward per chunk
 *                                                   | frames per chunk (BEER_SGRAD_FORM)
 * Every form is held against the oracle in tests/test_gpu_vae_prior_routes.py. */
#define BEER_SGRAD_GENERIC 0x10000000
#define BEER_SGRAD_FULL 0x20000000
#define BEER_SGRAD_DIAG 0x30000000
#define BEER_SGRAD_CHUNKED 0x40000000
#define BEER_SGRAD_FAMILY(route) ((route) & 0x70000000)
#define BEER_SGRAD_FORM(route) ((route) & 0x0FFFFFFF)
int beer_frames_llh_backward_route(int dtype, int cov, int64_t T, int D, int K,
                                   size_t workspace_bytes);
int beer_frames_llh_backward(int dtype, int cov, int64_t T, int D, int K, const void* X,
                             const void* weights, const void* grad, const void* exp_stats,
                             void* out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- feature front-end (beer/features.py, `beer features extract`) ----------
 * Ragged batch of utterances: `signal` holds the samples of all utterances
 * back to back, utterance u owns samples [sample_off[u], sample_off[u+1]) and
 * output rows [frame_off[u], frame_off[u+1]), with
 * frames_u = (samples_u - flen) / fstep + 1 (features.py:131,178).  Offsets
 * are DEVICE arrays of nutt + 1 int64.  All arithmetic is float64 as in the
 * reference (numpy), except the float32 pre-emphasis of `fbank()`. */

typedef struct {
    int32_t flen;        /* frame length in samples, int(srate * flen) */
    int32_t fstep;       /* frame shift in samples, int(srate * frate) */
    int32_t fft_len;     /* 2^(floor(log2(flen)) + 1), 64 .. 2048 */
    int32_t mode;        /* 0: features.fbank() -- float32 pre-emphasis over the
                            whole signal (features.py:182-184);
                            1: features.short_term_mspec() -- DC removal and
                            pre-emphasis inside each frame (features.py:124-139) */
    int32_t nfilters;    /* rows of `filters`; 0 = keep the fft_len/2 magnitudes */
    int32_t apply_log;   /* log(x + log_offset) after the filter bank */
    int32_t n_dct;       /* columns of `dct`; 0 = no cosine transform */
    int32_t add_energy;  /* prepend sum_f log-mel * norm (extract.py:148-151) */
    double preemph;
    double log_offset;   /* 1 in fbank() (features.py:204), 1e-6 in the CLI */
    double norm;         /* sqrt(2 / nfilters) (extract.py:131) */
    const double* window;   /* device [flen] */
    const double* filters;  /* device [nfilters, fft_len/2] (create_fbank) */
    const int32_t* filt_lo; /* device [nfilters] first non-zero bin, nullable */
    const int32_t* filt_hi; /* device [nfilters] last non-zero bin, nullable */
    const double* dct;      /* device [nfilters, n_dct] (extract.py:36-40) */
    const double* lifter;   /* device [n_dct], nullable (extract.py:141-145) */
} beer_feaconf;

/* mean[u] = mean of the samples of utterance u (the DC offset removed by
 * short_term_mspec, features.py:124).  in_dtype: BEER_I16 / BEER_F32 / BEER_F64. */
int beer_features_signal_mean(int in_dtype, int32_t nutt, const int64_t* sample_off,
                              const void* signal, double* mean, void* stream);

/* Framing -> pre-emphasis -> window -> |FFT| -> filter bank -> log ->
 * cosine transform * norm * lifter, with the optional energy column first.
 * out [total_frames, out_ld] float64, the features occupy the first
 * add_energy + (n_dct ? n_dct : nfilters ? nfilters : fft_len/2) columns of a
 * row (room for the deltas after them).  `utt_mean` nullable (mode 1 only). */
int beer_features_extract(int in_dtype, int32_t nutt, const int64_t* sample_off,
                          const int64_t* frame_off, int64_t total_frames,
                          const void* signal, const double* utt_mean,
                          const beer_feaconf* conf, double* out, int32_t out_ld,
                          void* stream);

/* One order of derivatives (features.add_deltas, features.py:95-105):
 * out[t,d] = sum_{j=-wlen..wlen} j / (2 sum j^2) * in[clamp(t+j), d], t clamped
 * inside its utterance.  `in` / `out` point at the first of D columns of rows
 * with stride ld (they may be column blocks of the same buffer). */
int beer_features_deltas(int32_t nutt, const int64_t* frame_off, int64_t total_frames,
                         int32_t D, int32_t ld, int32_t wlen, const double* in,
                         double* out, void* stream);

/* Per-utterance mean normalisation in place (extract.py:160-162). */
int beer_features_cmn(int32_t nutt, const int64_t* frame_off, int32_t D, int32_t ld,
                      double* x, void* stream);

/* ---- token sequences: unit sequences of paths, edit distances (csrc/editdist.hip) ----
 * Integer arithmetic only: every output is exact and the same bits in every run. */

/* Pdf-id paths collapsed into unit sequences (`phones_of_path` of the command line, without the
 * names), one wave per sequence.
 *   sym          packed int64 symbols (pdf ids) of all the sequences (read only)
 *   start, len   [n_seq] int64 / int32: sequence q is sym[start[q] .. start[q] + len[q])
 *   unit_of_pdf  [n_pdf] int32: the index of the unit whose FIRST pdf this is, else -1
 *   units        int32, as large as sym: the units of sequence q are written compactly at
 *                units[start[q] ..]; a sequence never has more units than symbols
 *   n_units      [n_seq] int32
 *   frame_unit   NULL, or int32 as large as sym: for every symbol the unit (the value written to
 *                `units`) that is running at that frame -- the per-frame form of the sequence
 * Position 0 starts a unit; position t > 0 starts one iff sym[t] != sym[t-1] and
 * unit_of_pdf[sym[t]] >= 0.  n_units[q] is the number of starts, except:
 *   len[q] <= 0                          0, nothing written
 *   sym[start[q]] < 0                   -1, nothing written (an n-best rank without a path)
 *   a pdf outside [0, n_pdf), or a first pdf that is no unit's first
 *                                       -2; what `units` / `frame_unit` hold for q is unspecified
 *                                       (nothing is written outside q's own range)
 * EINVAL, checked before anything is launched: n_seq < 0, n_pdf < 1, a NULL pointer (but
 * frame_unit) with n_seq > 0. */
int beer_unit_sequences(const int64_t* sym, const int64_t* start, const int32_t* len,
                        int64_t n_seq, const int32_t* unit_of_pdf, int32_t n_pdf, int32_t* units,
                        int32_t* n_units, int32_t* frame_unit, void* stream);

/* Levenshtein distances of a ragged batch of sequence pairs.
 *   sym          packed int32 symbols of all the sequences (read only)
 *   start, len   [n_seq] int64 / int32, as above
 *   pair_a/b     [n_pair] int32 sequence indices; repeats and a == b are allowed
 *   max_short    >= min(len[a], len[b]) of every pair     } the caller's: the launcher reads no
 *   max_long     >= max(len[a], len[b]) of every pair     } device memory
 *   dist         [n_pair] int32: the smallest number of substitutions, deletions and insertions
 *                that turn sequence a into sequence b
 *   ops          NULL, or [n_pair, 3] int32: (substitutions, deletions, insertions) of the
 *                alignment that is, among ALL alignments of that smallest cost, the one with the
 *                lexicographically smallest (sub, del, ins).  A deletion consumes a symbol of a
 *                alone, an insertion a symbol of b alone; ops(b, a) is ops(a, b) with the two
 *                swapped.  Computed with no back-trace: the recursion runs on cells
 *                cost << 42 | sub << 21 | del, whose integer order is that lexicographic order
 *   workspace    device scratch of beer_edit_distance_scratch_bytes(n_pair, max_short, max_long,
 *                ops != NULL) bytes (0: none needed, NULL will do); its content is opaque
 * Length limits, from the field widths: BEER_EDIT_MAX_LEN_OPS = 2^21 - 1 symbols with `ops`
 * (sub, del <= 2^21 - 1; cost <= 2^22 - 2 in 22 bits), BEER_EDIT_MAX_LEN = 2^30 without (the
 * cost, at most twice that inside the table, in a uint32).
 * EINVAL, checked before anything is launched: max_short < 0, max_long < max_short, max_long
 * beyond the limit, n_seq or n_pair < 0, a NULL pointer (but ops / workspace) or n_seq = 0 with
 * n_pair > 0, a workspace smaller than the query says.  The pair indices live on the device: the
 * launcher cannot read them, so a pair that names a sequence outside [0, n_seq), a sequence of
 * negative length, or one longer than max_short / max_long admit, reads nothing and gets dist
 * (and ops) -1 -- the caller checks its indices on the host first. */
#define BEER_EDIT_MAX_LEN (1 << 30)
#define BEER_EDIT_MAX_LEN_OPS ((1 << 21) - 1)
int beer_edit_distance(const int32_t* sym, const int64_t* start, const int32_t* len, int64_t n_seq,
                       const int32_t* pair_a, const int32_t* pair_b, int64_t n_pair,
                       int32_t max_short, int32_t max_long, int32_t* dist, int32_t* ops,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t beer_edit_distance_scratch_bytes(int64_t n_pair, int32_t max_short, int32_t max_long,
                                        int want_ops);

/* The form beer_edit_distance picks for these maxima (host only: it launches nothing), built
 * from the launcher's own plan:
 *   team | BEER_EDIT_OPS | BEER_EDIT_ROW_LDS or BEER_EDIT_ROW_WS
 *   team   lanes that share a pair, the shorter sequence on them: 8 / 16 / 32 / 64, the smallest
 *          that covers max_short (64 beyond); a wave holds 64 / team pairs, a workgroup 4 waves
 *   BEER_EDIT_OPS      cells are uint64 (cost, sub, del) instead of uint32: `ops` is asked for
 *   max_short <= 64    one strip of rows, nothing is kept between strips: neither ROW bit
 *   BEER_EDIT_ROW_LDS  strips of 64 rows; the strip's last row, max_long + 1 cells of 4 (8 with
 *                      ops) bytes, waits in a wave's 16 KiB of LDS: max_long <= 4095 (2047)
 *   BEER_EDIT_ROW_WS   ... beyond that in the workspace, one row per wave of the grid
 * BEER_EINVAL exactly where beer_edit_distance refuses these three arguments. */
#define BEER_EDIT_OPS 0x100
#define BEER_EDIT_ROW_LDS 0x1000
#define BEER_EDIT_ROW_WS 0x2000
#define BEER_EDIT_TEAM(route) ((route) & 0xFF)
int beer_edit_distance_route(int32_t max_short, int32_t max_long, int want_ops);

/* Copy `nbytes` (a multiple of 16, both pointers 16-byte aligned) from PINNED
 * host memory to device memory with a kernel on `stream`.  Used for the small
 * batch / graph descriptors: a copy-engine transfer queued behind running
 * kernels was measured to stall the stream for tens of ms on this platform; a
 * kernel that reads the pinned pages directly does not. */
int beer_copy_pinned(void* dst_device, const void* src_pinned_host, size_t nbytes,
                     void* stream);

/* Measurement aid (bench.py's `clock`): one wave sleeps through `sleeps` x s_sleep 127 and
 * writes the elapsed ticks of the shader clock (s_memtime) and of the fixed 100 MHz reference
 * clock (s_memrealtime) to `ticks_out[0..1]` (device).  Launched on a side stream while the
 * kernels of an iteration run, their ratio x 100 MHz is the clock those kernels really ran at
 * -- what a roofline fraction measured on one box needs to be compared with another box's.
 * Replaces nothing of the reference (beer has no device clock to read). */
int beer_clock_probe(int64_t* ticks_out, int32_t sleeps, void* stream);

/* ---- graph compilation (HOST functions: host pointers, no stream) -----------
 * Graph.compile (beer/graph.py:185-240) and create_graph_from_seq
 * (beer/cli/subcommands/hmm/mkaligraph.py:18-39) in O(states + arcs), for one
 * graph or for a whole corpus of transcriptions at once.  The result lives in
 * an opaque host object; beer_graphset_image lays every graph out as the
 * beer_graph CSR image above inside ONE blob, for a single host-to-device
 * copy. */
typedef struct beer_graphset beer_graphset;

/* Compile one topology.  States 0..n_states-1 in insertion order, pdf_ids[s]
 * < 0 for a non-emitting state; arcs in insertion order, weights are
 * probabilities (already normalised by the caller, Graph.normalize). */
int beer_graph_compile(int32_t n_states, const int32_t* pdf_ids, int64_t n_arcs,
                       const int32_t* arc_src, const int32_t* arc_dst,
                       const double* arc_w, int32_t start_state,
                       int32_t end_state, beer_graphset** out);

/* Alignment graphs of n_utts transcriptions: utterance u is the sequence of
 * unit ids seq_units[seq_off[u] .. seq_off[u+1]), each unit a small HMM given
 * by its states (unit_pdf_ids, < 0: non-emitting), start / end state and arcs
 * (local state ids), all concatenated with *_off offsets.  Equals
 * create_graph_from_seq(seq, units) for every utterance: chain of unit
 * copies, Graph.normalize, Graph.compile. */
int beer_aligraphs_compile(int32_t n_units, const int32_t* unit_state_off,
                           const int32_t* unit_pdf_ids, const int32_t* unit_start,
                           const int32_t* unit_end, const int32_t* unit_arc_off,
                           const int32_t* unit_arc_src, const int32_t* unit_arc_dst,
                           const double* unit_arc_w, int64_t n_utts,
                           const int64_t* seq_off, const int32_t* seq_units,
                           beer_graphset** out);

int beer_graphset_free(beer_graphset* set);

/* A set from the tables beer_graphset_export gives (host arrays; offsets [n_graphs + 1]):
 * how graphs that were compiled elsewhere -- dense CompiledGraph objects of an `alis.npz` --
 * get an arena image, and how a set is copied so that the copy owns its image.  EINVAL
 * unless every graph's arcs are sorted by (source, destination), distinct and in range. */
int beer_graphset_from_csr(int64_t n_graphs, const int64_t* state_off, const int64_t* arc_off,
                           const float* init, const float* fin, const int32_t* pdf_ids,
                           const int32_t* arc_src, const int32_t* arc_dst,
                           const float* arc_prob, beer_graphset** out);

/* Number of graphs and (nullable) cumulative state / arc offsets [n+1]. */
int beer_graphset_sizes(const beer_graphset* set, int64_t* n_graphs,
                        int64_t* state_off, int64_t* arc_off);

/* Concatenated contents (every pointer nullable): initial / final
 * probabilities and pdf ids per state, arcs sorted by (source, destination)
 * with local state ids and float32 probabilities, as the reference's tables
 * before `.log()`. */
int beer_graphset_export(const beer_graphset* set, float* init, float* fin,
                         int32_t* pdf_ids, int32_t* arc_src, int32_t* arc_dst,
                         float* arc_prob);

/* Size of, and the blob holding, the device image of every graph in `dtype`
 * (log-probabilities: float32 log of the float32 tables, as the reference).
 * `graphs[i]` receives the beer_graph descriptor of graph i whose pointers
 * are device_base + offset, i.e. valid once the blob has been copied to
 * device_base.  Graphs whose states all have <= BEER_SEG arcs get the
 * `lowdeg` image (no hubs). */
int beer_graphset_image_bytes(const beer_graphset* set, int dtype, size_t* bytes);
int beer_graphset_image(const beer_graphset* set, int dtype, void* host_blob,
                        uint64_t device_base, beer_graph* graphs);

#ifdef __cplusplus
}
#endif
#endif /* BEER_HIP_H */
