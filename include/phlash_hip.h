/* libphlash_hip.so -- C ABI of the MI355X (gfx950) PSMC likelihood engine.
 *
 * Drop-in boundary for the *kernel plugin* of jthlab/phlash (v1.0.6).  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo):
 *
 *   phk_create / phk_destroy   <->  _PSMCKernelBase.__init__ / __del__      src/phlash/gpu.py:101-174
 *                                   (validate + upload the int8 het matrix once, own it for life)
 *   phk_loglik                 <->  _PSMCKernelBase.__call__ + the two CUDA entry points
 *                                   `loglik` / `loglik_grad`                 src/phlash/gpu.py:182-325,
 *                                                                           529-538, 575-586
 *   phk_device_count           <->  PSMCKernel._initialize_devices           src/phlash/gpu.py:369-384
 *   phk_last_error             <->  CudaError / ASSERT_DRV                   src/phlash/gpu.py:23-46
 *
 * Conventions
 *   - plain C, no exceptions: every call returns PHK_OK (0) or a PHK_E* code; the message of the
 *     last failure on the calling thread is phk_last_error().
 *   - `params`, `inds`, `ll`, `grad` are DEVICE pointers (e.g. torch tensors' data_ptr()): nothing
 *     bounces through the host.  `data` of phk_create may be host or device memory.
 *   - calls on one handle are stream-ordered on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and return without synchronising.  A handle is not re-entrant (it owns
 *     scratch buffers), exactly like a reference kernel object (gpu.py:222-237).
 *   - parameter block layout [B, S or 1, 7, K], rows b,d,u,v,emis0,emis1,pi (gpu.py:189, 496-501),
 *     element type float (double_precision = 0) or double (1) (gpu.py:133-136).
 */
#ifndef PHLASH_HIP_H
#define PHLASH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHK_OK 0
#define PHK_EINVAL 1   /* bad argument (the reference raises AssertionError: gpu.py:106-113,197-214) */
#define PHK_ENOMEM 2   /* device allocation failed (the reference raises MemoryError: gpu.py:117-124) */
#define PHK_EHIP 3     /* HIP runtime error (the reference raises CudaError/RuntimeError) */
#define PHK_EUNSUPPORTED 4 /* K / variant not compiled in */
#define PHK_EOVERRUN 5 /* a kernel loop ran out of the iteration budget the host derived from the row length: the kernel
                          returned early, the evaluation is invalid; phk_last_error() names kernel, sequence and block.
                          (No counterpart in the reference, whose kernels loop over ``L`` alone: gpu.py:541, 617.) */

typedef struct phk_handle phk_handle;

/* ABI version of this library (major*1000 + minor). */
int phk_version(void);

/* Message of the last failure on this thread ("" if none).  Never NULL. */
const char* phk_last_error(void);

/* Number of visible HIP devices. */
int phk_device_count(int* n);

/* Create a kernel object for K hidden states over the observation matrix data[N][L]
 * (int8, values -1 missing / 0 hom / >=1 het; values above 1 are clipped to 1 and values below -1
 * rejected, as gpu.py:106-110; rows that are entirely missing are rejected as gpu.py:111-113).
 * The matrix is re-packed on the device to a private 2-bit layout; `data` is not referenced after
 * the call returns.  K in {4,8,16,32,64}. */
int phk_create(phk_handle** out, int K, const int8_t* data, int64_t N, int64_t L,
               int data_on_device, int double_precision, int device);

int phk_destroy(phk_handle* h);

/* One evaluation over B particles x S chunks.
 *   params     device, [B, S, 7, K] with element strides (pstride_b, pstride_s); pstride_s = 0
 *              broadcasts one [7,K] block of a particle over all S chunks.
 *   inds       device int64 [S]: row of `data` for each chunk.  0 <= inds[s] < N (gpu.py:197-199) is
 *              checked on the device: an index outside the range is clamped to row 0 and raises
 *              bit 1 of the flag word; the next phk_underflow_risk then returns PHK_EINVAL.
 *   W          number of leading sites of every row that are run but NOT scored (the reference's
 *              warm-up prefix, model.py:52-55).  W = 0 reproduces `loglik`/`loglik_grad` exactly:
 *              pi is the state law one transition before site 0.
 *   ll         device double [B, S]: log-likelihood of sites W..L-1 of chunk s under particle b
 *   grad       device [B, S, 7, K] (float or double as the handle) or NULL for the no-gradient
 *              kernel.  grad_dlog = 0: d ll / d theta.  grad_dlog = 1: theta * d ll / d theta, the
 *              quantity the reference kernel returns (gpu.py:647-653,686-691), every row in natural
 *              index order (i.e. after the reference's np.roll of the v row, gpu.py:307-309).
 */
int phk_loglik(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s,
               const int64_t* inds, int64_t B, int64_t S, int64_t W, double* ll, void* grad,
               int grad_dlog, void* stream);

/* float64 parameter blocks -> what a float32 kernel object runs on, one launch.  The reference rounds its float64
 * PSMCParams to the kernel's float type field by field on the host (src/phlash/gpu.py:200-214, ``astype(float_type)``);
 * the float32 kernels here additionally run on the model written with hom emission 1 ("folded"):
 *   params       device double [nblocks, 7, K]  rows b,d,u,v,emis0,emis1,pi (gpu.py:189)
 *   params_f32   device float  [nblocks, 7, K]  the same block rounded to float32
 *   prefold_f32  device float  [nblocks, 5, K]  rows fl(emis0 b), fl(emis0 d), fl(emis0 v), fl(emis1 / emis0), fl(1 / emis0),
 *                each formed in float64 and rounded ONCE.  Handed to phk_loglik_prefolded beside params_f32 the kernels
 *                take these factors as they are; without them (phk_loglik) they fold the float32 rows themselves, which
 *                rounds every folded factor three times -- an error that is the same at every site of a row and adds up
 *                along it.
 *   crel         device double [nblocks, 7, K] or NULL: coefficients of the first-order correction phk_ll_first_order applies */
int phk_prefold(int device, int K, const double* params, int64_t nblocks, float* params_f32, float* prefold_f32, double* crel,
                void* stream);

/* First-order correction of a float32 gradient call's log-likelihoods for the rounding of the model to float32:
 *     ll[b, s] += sum_j theta[b, s, j] * (d ll / d theta)[b, s, j] * crel[b, s, j]
 * with the gradient that call returned (grad_dlog as it was passed to phk_loglik*), the float64 blocks and the coefficients
 * of phk_prefold (params and crel share the element strides pstride_b, pstride_s; 0 broadcasts over the chunks).  The rounding of
 * a float32 model is the same at every site of a row, so its effect on ll grows with the row length (about 1e-8 per site
 * absolute: the reference's own float32 kernels lose the same); it is linear in the rounding residuals
 * to first order, and the derivative it multiplies is the gradient the call has just computed.  What is left is the
 * arithmetic's error, which does not add up coherently.  Not available to a no-gradient call. */
int phk_ll_first_order(int device, int K, double* ll, const float* grad, int grad_dlog, const double* params, const double* crel,
                       int64_t pstride_b, int64_t pstride_s, int64_t B, int64_t S, void* stream);

/* phk_loglik for a float32 kernel object with the blocks' pre-folded factors (phk_prefold): ``prefold`` is laid out like
 * ``params`` with five rows per block instead of seven (element strides pstride_b / 7 * 5, pstride_s / 7 * 5).  Same outputs,
 * same flags; gradients are with respect to the rows of ``params`` as ever. */
int phk_loglik_prefolded(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                         const int64_t* inds, int64_t B, int64_t S, int64_t W, double* ll, void* grad, int grad_dlog,
                         void* stream);

/* Posterior decoding, the quantity of Li & Durbin's `psmc -d` (the reference has no counterpart): the hidden-state
 * posteriors gamma_t(k) = P(z_t = k | o) = alpha_t(k) beta_t(k) / sum_j alpha_t(j) beta_t(j) of every scored site
 * t = W .. L-1 of each sequence (b, s), with alpha_0 = pi, alpha_t = (alpha_{t-1} A) .* e_{o_t}, beta_L = 1,
 * beta_{t-1} = A (e_{o_t} .* beta_t), missing sites e = 1.  The posterior conditions on the whole row, warm-up included;
 * there is no warm-up correction.  Sites are reduced over bins of `bin` >= 1 consecutive scored sites (the last bin may be
 * partial; nbin = ceil((L - W) / bin)):
 *   marginals  [B, S, nbin, K] in the handle's float type, or NULL: the mean of gamma_t over the bin's sites;
 *   mean       [B, S, nbin] in the handle's float type, or NULL: the mean over the bin's sites of sum_k values_k gamma_t(k),
 *              values device double [B, K] (row stride vstride_b; 0: one row [K] for every particle);
 *   ll         [B, S] double, required: log P(o), the forward pass's by-product -- what phk_loglik without a gradient
 *              returns (to the bit where both calls run the same forward variant, e.g. under phk_set_plan).
 * At least one of marginals / mean (with W = L there is no scored site: nbin = 0, ll = 0, both outputs are empty and may be
 * NULL).  params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as
 * phk_loglik).  The call runs the forward leg (and, for a segmented plan, the beta-scan leg) of the plan a gradient call
 * of this shape would use, then the decode sweep; a hybrid plan is run as its serial half.  Stream-ordered; no two calls
 * on one handle may overlap.  The underflow flag (phk_underflow_risk) is raised as by phk_loglik: re-evaluate after
 * phk_set_rescale_interval(h, 1).  PHK_EINVAL, before anything is enqueued, for a NULL handle, bin < 1, both outputs NULL,
 * W outside [0, L], a NULL values with mean. */
int phk_posterior(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                  const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const double* values, int64_t vstride_b,
                  double* ll, void* mean, void* marginals, void* stream);

/* Transition posteriors (the reference has no counterpart): the pair posterior xi_t(i, j) = P(z_prev = i, z_t = j | o) of every
 * scored site t = W .. L-1 of each sequence (b, s), split by how state k at the site was reached.  Conventions of
 * phk_posterior: z_0 ~ pi precedes site 0 (it is z_prev of site 0), site t is step t + 1, alpha_t is the forward vector after
 * site t with alpha_{-1} = pi, beta_L = 1, a missing site has e = 1, the W warm-up sites are conditioned on and not reported,
 * and there is no warm-up correction.  With A[i,j] = b_j (i > j), d_j (i = j), u_i v_j (i < j), w = e_{o_t} .* beta_t and Z_t
 * the sum of all three terms over k:
 *   stay_t(k) = P(z_prev = k, z_t = k | o) = alpha_{t-1}(k) d_k w(k) / Z_t
 *   up_t(k)   = P(z_prev < k, z_t = k | o) = (sum_{i<k} u_i alpha_{t-1}(i)) v_k w(k) / Z_t      (a move to an older state)
 *   down_t(k) = P(z_prev > k, z_t = k | o) = (sum_{i>k} alpha_{t-1}(i)) b_k w(k) / Z_t          (a move to a younger state)
 * so stay + up + down = gamma_t(k), the marginal phk_posterior reports.  d_k contains "recombined and coalesced again in the
 * same interval": up and down count changes of the TMRCA STATE, not recombination events.  Sites are reduced over bins of
 * `bin` >= 1 consecutive scored sites (the last bin may be partial; nbin = ceil((L - W) / bin)):
 *   arrivals   [B, S, nbin, 3, K] in the handle's float type, or NULL: the MEAN over the bin's sites of (stay, up, down), in
 *              that order;
 *   changes    [B, S, nbin, 2] in the handle's float type, or NULL: the SUM over the bin's sites of (sum_k up_t(k),
 *              sum_k down_t(k)) -- the expected number of moves to an older and to a younger state inside the bin; their
 *              total is the expected number of TMRCA changes.  The sum over states is taken in float64;
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N], one own length per data row of the handle (W < lens[i] <= L), or NULL = L for all.  A site
 *              at or past its row's own length adds nothing to a sum and is not counted in a mean; a bin without a site of
 *              the row's own is written as zeros.  The row is still conditioned on as a whole: pad with missing windows,
 *              whose beta is 1 -- the padded sites themselves carry the prior's change rate, which is what the mask keeps out.
 *              An entry out of range raises the bad-index flag on the device (reported by phk_underflow_risk; the length is
 *              clamped).
 * At least one of arrivals / changes (with W = L there is no scored site: nbin = 0, ll = 0, both outputs are empty and may be
 * NULL).  params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs, slabs
 * (phk_set_workspace_limit) and stream ordering are phk_posterior's: the forward leg (and, for a segmented plan, the beta-scan
 * leg) of the plan a gradient call of this shape would use, then the transition sweep; a hybrid plan is run as its serial half;
 * the plan is read, never tuned or recorded.  Every bin is written once, by one unit: the same bits for any slab and any order
 * of the units.  Stream-ordered; no two calls on one handle may overlap.  The underflow flag is raised as by phk_loglik:
 * re-evaluate after phk_set_rescale_interval(h, 1).  PHK_EINVAL, before anything is enqueued, for a NULL handle, NULL params /
 * inds / ll, bin < 1, both outputs NULL, W outside [0, L]. */
int phk_transitions(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                    const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const int64_t* lens, double* ll,
                    void* arrivals, void* changes, void* stream);

/* Leave-one-out predictive decoding (the reference has no counterpart): for every scored site t = W .. L-1 of each sequence
 * (b, s), the probability that the site is het given every OTHER site of the row, P(o_t = het | o_{-t}, o_t observed), and the
 * log of that predictive at the observation the site has.  Conventions of phk_posterior and phk_transitions: z_0 ~ pi precedes
 * site 0, alpha_{t-1} is the forward vector before site t with alpha_{-1} = pi, beta_L = 1 and beta_t includes the emissions of
 * sites t+1 .. L-1 only, a missing site has e = 1, the W warm-up sites are conditioned on and not reported, and there is no
 * warm-up correction.  With A[i,j] = b_j (i > j), d_j (i = j), u_i v_j (i < j):
 *   c_t(k)  = (alpha_{t-1} A)(k) beta_t(k)               the cavity weight: everything but site t's own emission
 *   n0_t    = sum_k c_t(k) emis0(k)       n1_t = sum_k c_t(k) emis1(k)
 *   phet_t  = n1_t / (n0_t + n1_t)
 *   score_t = log(n_{o_t} / (n0_t + n1_t)) at an observed site (o_t = 0 or >= 1), 0 at a missing site.
 * The emission rows need not sum to one (they are clamped upstream): the division by n0 + n1 keeps the definition exact.  Sites
 * are reduced over bins of `bin` >= 1 consecutive scored sites (the last bin may be partial; nbin = ceil((L - W) / bin)):
 *   track      [B, S, nbin, 3] in the handle's float type: the SUM over the bin's sites, accumulated in float64 and rounded once,
 *              of [0] phet_t over the OBSERVED sites (the expected het count where there is an observed count to hold it
 *              against), [1] phet_t over the MISSING sites (the imputed het count under the mask), [2] score_t (the
 *              leave-one-out log score; missing sites add 0);
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N] or NULL, exactly as phk_transitions: a site at or past its row's own length adds nothing, a bin
 *              without a site of the row's own is written as zeros, an entry outside (W, L] is clamped and raises the bad-index
 *              flag.
 * A site whose n0 + n1 is not positive adds nothing and raises the underflow flag (re-evaluate after
 * phk_set_rescale_interval(h, 1)).  With W = L there is no scored site: nbin = 0, ll = 0, track is empty and may be NULL.
 * params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs, slabs
 * (phk_set_workspace_limit) and stream ordering are phk_posterior's, with the predictive sweep in the decode sweep's place; the
 * plan is read, never tuned or recorded.  Every bin is written once, by one unit: the same bits for any slab and any order of the
 * units.  Stream-ordered; no two calls on one handle may overlap.  PHK_EINVAL, before anything is enqueued, for a NULL handle,
 * NULL params / inds / ll, bin < 1, W outside [0, L], NULL track with W < L. */
int phk_predictive(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                   const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const int64_t* lens, double* ll, void* track,
                   void* stream);

/* Tract posteriors (the reference has no counterpart): for every bin of scored sites of each sequence (b, s), the posterior
 * expectation of the product of a per-state weight over the bin's sites -- with the weight an indicator of a state set S, the
 * probability that EVERY site of the bin has its state in S: a joint event of the bin's sites, which the per-site marginals do
 * not determine (their bin mean is only an upper bound).  Conventions of phk_posterior and phk_predictive: z_0 ~ pi precedes
 * site 0, alpha_t is the forward vector after site t with alpha_{-1} = pi, beta_{L-1} = 1 and beta_t holds the emissions of sites
 * t+1 .. L-1 only, a missing site has e = 1, the W warm-up sites are conditioned on and not reported, and there is no warm-up
 * correction.  Let m in [0,1]^K be the particle's weight row.  Bin k holds the scored sites s = W + k bin .. e =
 * min(s + bin, L) - 1 (the last bin may be partial; nbin = ceil((L - W) / bin)), and
 *   q_e     = beta_e
 *   q_{t-1} = A (m .* e_{o_t} .* q_t)            for t = e, e-1, .., s
 *   tract_k = sum_i alpha_{s-1}(i) q_{s-1}(i) / sum_i alpha_{s-1}(i) beta_{s-1}(i)
 *           = E[ prod_{t=s..e} m(z_t) | o ]       ( = P(z_s .. z_e in S | o) for an indicator of S ).
 *   weights    device double [B, K] with row stride wstride_b, or [K] with wstride_b = 0 (one row for all particles, like
 *              `values` of phk_posterior); rounded to the handle's float type; values outside [0, 1] are the caller's error;
 *   tract      [B, S, nbin] in the handle's float type;
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N] or NULL: a site at or past its row's own length is stepped with m replaced by 1, so it restricts
 *              nothing; a bin without a site of the row's own is written as 0; an entry outside (W, L] is clamped and raises
 *              the bad-index flag.
 * q runs on beta's scale and q <= beta holds elementwise in the computed numbers as well, so a tract never exceeds 1 and a
 * smaller set never has the larger tract.  A bin whose denominator is not positive is written as 0 and raises the underflow flag
 * (re-evaluate after phk_set_rescale_interval(h, 1)); a numerator that flushes to 0 is a legitimate answer (q can underflow
 * where beta does not) and raises nothing.  With W = L there is no scored site: nbin = 0, ll = 0, tract is empty and may be NULL.
 * params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs, slabs
 * (phk_set_workspace_limit) and stream ordering are phk_posterior's, with the tract sweep in the decode sweep's place; the plan is
 * read, never tuned or recorded.  Every bin is written once, by one unit: the same bits for any slab and any order of the units.
 * Stream-ordered; no two calls on one handle may overlap.  PHK_EINVAL, before anything is enqueued, for a NULL handle, NULL
 * params / inds / ll / weights, bin < 1, W outside [0, L], NULL tract with W < L. */
int phk_tracts(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
               const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const double* weights,
               int64_t wstride_b, const int64_t* lens, double* ll, void* tract, void* stream);

/* Bin moments (the reference has no counterpart): for every bin of scored sites of each sequence (b, s), the first two raw
 * posterior moments of the bin sum S_k = sum_{t in bin} v(z_t) of a per-state value v -- the posterior mean of the sum and, as
 * m2 - m1^2, its posterior variance, covariances between the bin's sites included: the per-site marginals determine the mean
 * only.  Conventions of phk_tracts: z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t with alpha_{-1} = pi,
 * beta_{L-1} = 1 and beta_t holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1, the W warm-up sites are
 * conditioned on and not reported, and there is no warm-up correction.  Let v in [-1,1]^K be the particle's value row.  Bin k
 * holds the scored sites s = W + k bin .. e = min(s + bin, L) - 1 (the last bin may be partial; nbin = ceil((L - W) / bin)), and
 *   q1_e = 0,  q2_e = 0
 *   w0 = e_{o_t} .* beta_t,   w1 = e_{o_t} .* q1_t,   w2 = e_{o_t} .* q2_t
 *   beta_{t-1} = A w0
 *   q1_{t-1}   = A (w1 + v .* w0)
 *   q2_{t-1}   = A (w2 + 2 v .* w1 + v^2 .* w0)        for t = e, e-1, .., s
 *   m1_k = sum_i alpha_{s-1}(i) q1_{s-1}(i) / sum_i alpha_{s-1}(i) beta_{s-1}(i) = E[ S_k | o ]
 *   m2_k = sum_i alpha_{s-1}(i) q2_{s-1}(i) / (the same denominator)             = E[ S_k^2 | o ].
 * (The third argument is formed as w2 + v .* (w1 + x1) with x1 the second.)
 *   values     device double [B, K] with row stride vstride_b, or [K] with vstride_b = 0 (one row for all particles, like
 *              `values` of phk_posterior); rounded to the handle's float type; values outside [-1, 1] are the caller's error
 *              (|q1| <= n beta and q2 <= n^2 beta for a bin of n sites hold for values inside it only); centre and scale a
 *              general row first and map the moments back (the variance is shift-invariant, and m2 - m1^2 of an uncentred row
 *              cancels digits the float32 recursion does not have);
 *   m1, m2     [B, S, nbin] double for both handle types (a float32 store of m2 would drop the digits m2 - m1^2 needs);
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N] or NULL: a site at or past its row's own length is stepped with v replaced by 0, so it adds
 *              nothing; a bin without a site of the row's own is written as m1 = m2 = 0; an entry outside (W, L] is clamped and
 *              raises the bad-index flag.
 * q1 is signed, q2 is non-negative up to rounding; both run on beta's scale and take every power of two that rescales beta, so
 * they need no exponent of their own.  v = 0 gives m1 = m2 = 0 exactly.  A bin whose denominator is not positive is written as
 * 0 and raises the underflow flag (re-evaluate after phk_set_rescale_interval(h, 1)).  With W = L there is no scored site:
 * nbin = 0, ll = 0, m1 and m2 are empty and may be NULL.
 * params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs, slabs
 * (phk_set_workspace_limit) and stream ordering are phk_posterior's, with the moment sweep in the decode sweep's place; the plan
 * is read, never tuned or recorded; a hybrid plan runs as its serial half.  Every bin is written once, by one unit: the same bits
 * for any slab and any order of the units.  Stream-ordered; no two calls on one handle may overlap.  PHK_EINVAL, before anything
 * is enqueued, for a NULL handle, NULL params / inds / ll / values, bin < 1, W outside [0, L], NULL m1 or m2 with W < L. */
int phk_bin_moments(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                    const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const double* values,
                    int64_t vstride_b, const int64_t* lens, double* ll, double* m1, double* m2, void* stream);

/* Local likelihood-ratio scans (the reference has no counterpart): for every bin of scored sites of each sequence (b, s), the log
 * of the ratio
 *   P(o | the bin's sites are generated by an ALTERNATIVE model, the rest of the row by the fitted one) / P(o | fitted model),
 * which says where along the row the fitted model is wrong and in which direction (an alternative with theta, rho or Ne scaled).
 * phk_tracts is the special case "the same model with emissions multiplied by m"; an alternative with both emission rows set to 1
 * gives the block-out predictive, logratio = -log P(o_bin | o_-bin).  Conventions of phk_posterior and phk_tracts: z_0 ~ pi
 * precedes site 0, alpha_t is the forward vector after site t with alpha_{-1} = pi, beta_{L-1} = 1 and beta_t holds the emissions
 * of sites t+1 .. L-1 only, a missing site has e = 1 in both models, the W warm-up sites are conditioned on and not reported, and
 * there is no warm-up correction.  Let (A, e) be the particle's model and (A', e') its alternative block.  Bin k holds the scored
 * sites s = W + k bin .. e = min(s + bin, L) - 1 (the last bin may be partial; nbin = ceil((L - W) / bin)), and
 *   q_e        = beta_e
 *   q_{t-1}    = A' (e'_{o_t} .* q_t)            for t = e, e-1, .., s
 *   logratio_k = log sum_i alpha_{s-1}(i) q_{s-1}(i)  -  log sum_i alpha_{s-1}(i) beta_{s-1}(i):
 * every site of the bin has the transition INTO it and its emission taken from the alternative; alpha, beta and the rest of the
 * row are the fitted model's.
 *   alt_params  the alternative blocks, laid out like params ([B, S|1, 7, K] in the handle's float type) with element strides
 *               astride_b / astride_s (astride_s = 0: one block per particle; both 0: one block for all).  Their pi row is never
 *               read: pi precedes site 0 and no bin contains it;
 *   alt_prefold the pre-folded factors of the alternative blocks (phk_prefold), laid out like them with five rows, or NULL: as
 *               prefold is to params.  The alternative folds its own hom emission into its own factors, by its own decision: a
 *               block that cannot be folded runs unfolded;
 *   logratio    [B, S, nbin] in the handle's float type, natural log;
 *   ll          [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens        device int64 [N] or NULL: a site at or past its row's own length is stepped with the fitted model; a bin without
 *               a site of the row's own is written as 0; an entry outside (W, L] is clamped and raises the bad-index flag.
 * Unlike a tract, q is not bounded by beta and the ratio may leave the float range in either direction (with the emissions removed
 * over a whole row it is 1 / P(o)).  q therefore carries an integer power-of-two exponent of its own relative to beta: it is
 * renormalised where beta is rescaled, the exponent is folded into the ratio before the log while the product is representable
 * and added in the log domain where it is not, so logratio is right wherever the true value is representable as a log.  An
 * alternative block bit-identical to the fitted one gives exactly 0.  A bin whose denominator is not positive is written as 0 and
 * raises the underflow flag (re-evaluate after phk_set_rescale_interval(h, 1)); a numerator of exactly 0 (an alternative that
 * forbids the data) is a legitimate -inf and raises nothing.  With W = L there is no scored site: nbin = 0, ll = 0, logratio is
 * empty and may be NULL.  params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs,
 * slabs (phk_set_workspace_limit) and stream ordering are phk_posterior's, with the local-ratio sweep in the decode sweep's place
 * (a hybrid plan runs as its serial half); the plan is read, never tuned or recorded.  Every bin is written once, by one unit:
 * the same bits for any slab and any order of the units.  Stream-ordered; no two calls on one handle may overlap.  PHK_EINVAL,
 * before anything is enqueued, for a NULL handle, NULL params / alt_params / inds / ll, bin < 1, W outside [0, L], NULL logratio
 * with W < L. */
int phk_local_ratio(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                    const void* alt_params, int64_t astride_b, int64_t astride_s, const float* alt_prefold,
                    const int64_t* inds, int64_t B, int64_t S, int64_t W, int bin, const int64_t* lens,
                    double* ll, void* logratio, void* stream);

/* Interval tracts (the reference has no counterpart): phk_tracts over intervals with arbitrary ends, each with a state set of its
 * own, as a log -- how sure the data are of a called segment.  For each chunk position s of the call a list of intervals in
 * REPORTED sites (position p is site W + p, as the path of phk_viterbi), disjoint, sorted and half-open, 0 <= start_j < end_j <=
 * len - W; interval j has a state set S_j given as a 64-bit mask, bit k set = state k is inside (bits at or above K are not
 * read).  Conventions of phk_tracts: z_0 ~ pi precedes site 0, alpha_{-1} = pi, beta_t holds the emissions of sites t+1 .. L-1
 * only, a missing site has e = 1 and is restricted to the set all the same.  With s = W + start_j, e = W + end_j - 1:
 *   q_e     = beta_e
 *   q_{t-1} = A (1_{S_j} .* e_{o_t} .* q_t)      for t = e, e-1, .., s
 *   logp_j  = log sum_i alpha_{s-1}(i) q_{s-1}(i)  -  log sum_i alpha_{s-1}(i) beta_{s-1}(i)
 *           = log P(z_s .. z_e in S_j | o)   for sequence (b, s).
 *   iv_off     device int64 [S + 1]: the intervals of chunk position s are iv_off[s] .. iv_off[s + 1] - 1 (CSR; iv_off[0] = 0,
 *              n_iv = iv_off[S]); the lists are shared by the particles;
 *   iv_start, iv_end   device int64 [n_iv];
 *   masks      device uint64 [B, n_iv] with row stride mstride_b, or [n_iv] with mstride_b = 0 (one set per interval for all
 *              particles);
 *   max_len    an upper bound on end - start over the call (>= 1): it sizes the loop budget of a unit of the segmented plan;
 *   logp       device double [B, n_iv] for both handle types, natural log; one writer per entry;
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N] or NULL: the own length of every data row, the bound of its intervals.
 * q carries a power-of-two exponent of its own relative to beta, as in phk_local_ratio: a tract of thousands of sites whose
 * probability is far below the float range is right as a log.  A mask with all K bits set gives exactly 0, an empty mask -inf;
 * an interval's bits do not depend on the other intervals of the call, on slabs or on the order of the units.  One small kernel
 * checks every list before the first sweep: a list that is not sorted and disjoint, holds an empty interval, one outside
 * [0, len - W] or one longer than max_len raises the bad-index flag (phk_underflow_risk) and all its logp are NaN; the other
 * lists are not affected.  An interval whose denominator is not positive is written as 0 and raises the underflow flag.  n_iv = 0
 * computes ll only (masks and logp must still point at one element).  An interval belongs to the unit of the segmented plan
 * that holds its last site; the unit walks left to the interval's first site.  params / prefold / inds / strides as
 * phk_loglik_prefolded; plan legs, slabs and stream ordering are phk_posterior's (a hybrid plan runs as its serial half); the
 * plan is read, never tuned or recorded.  Stream-ordered; no two calls on one handle may overlap.  PHK_EINVAL, before anything is
 * enqueued, for a NULL handle, NULL iv_off / iv_start / iv_end / masks / logp, max_len < 1, mstride_b < 0, NULL params / inds /
 * ll, W outside [0, L]. */
int phk_interval_tracts(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                        const int64_t* inds, int64_t B, int64_t S, int64_t W, int64_t max_len, const int64_t* lens,
                        const int64_t* iv_off, const int64_t* iv_start, const int64_t* iv_end, const uint64_t* masks,
                        int64_t mstride_b, double* ll, double* logp, void* stream);

/* Pair counts (the reference has no counterpart): the full pair posterior summed along the row,
 *   counts[b, s, i, j] = sum over the row's own scored sites t of xi_t(i, j),    xi_t(i, j) = P(z_prev = i, z_t = j | o),
 * the expected number of moves from TMRCA state i (the ORIGIN, first index) to state j: the Baum-Welch transition statistic, the
 * matrix phk_transitions reduces to (stay, up, down) per state reached.  Conventions of phk_transitions: z_0 ~ pi precedes site 0
 * (it is z_prev of site 0), alpha_t is the forward vector after site t with alpha_{-1} = pi, beta_L = 1, a missing site has
 * e = 1, the W warm-up sites are conditioned on and not counted, and there is no warm-up correction.  With A[i,j] = b_j (i > j),
 * d_j (i = j), u_i v_j (i < j) and w = e_{o_t} .* beta_t,
 *   xi_t(i, j) = alpha_{t-1}(i) A[i, j] w_t(j) / Z_t,      Z_t = the sum of the numerator over all (i, j),
 * so every counted site adds exactly 1: counts[b, s] sums to the number of the row's own scored sites, min(lens, L) - W.  Its
 * diagonal is the sum of stay_t, its strict-upper column sums that of up_t and its strict-lower ones that of down_t of
 * phk_transitions; its column sums are the summed marginals of phk_posterior.  d_k contains "recombined and coalesced again in the
 * same interval": the diagonal counts sites whose TMRCA STATE stays, not sites without a recombination.
 *   counts     [B, S, K, K] double for both handle types, required unless W = L.  The sweep sums alpha_{t-1}(i) w_t(j) / Z_t --
 *              float32 handles in float32, added into float64 every 64 sites; float64 handles in float64 -- and A[i, j], formed
 *              in float64 from the parameter block (the factors as the kernels hold them), multiplies the float64 sum once;
 *   ll         [B, S] double, required: bitwise what phk_posterior returns on the same plan;
 *   lens       device int64 [N] or NULL, exactly as phk_transitions: a site at or past its row's own length adds nothing; an
 *              entry outside (W, L] is clamped and raises the bad-index flag.
 * With W = L there is no scored site: ll = 0 and counts, where given, is zeros (it may be NULL).  params / prefold / inds /
 * strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Plan legs, slabs (phk_set_workspace_limit) and stream ordering
 * are phk_posterior's, with the pair-count sweep in the decode sweep's place (a hybrid plan runs as its serial half); the plan is
 * read, never tuned or recorded.  Every unit of the sweep writes a float64 partial of its own in the call's workspace (K * K
 * doubles per unit and sequence: part of the slab arithmetic, a large batch is cut into more slabs) and one kernel sums them in
 * unit order: no atomics, the same bits for any slab size and for repeated calls under one plan; a serial and a segmented plan
 * sum in different orders and may differ in the last bits.  Stream-ordered; no two calls on one handle may overlap.  The underflow
 * flag is raised as by phk_loglik: re-evaluate after phk_set_rescale_interval(h, 1).  PHK_EINVAL, before anything is enqueued,
 * for a NULL handle, NULL params / inds / ll, NULL counts with W < L, W outside [0, L]. */
int phk_pair_counts(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                    const int64_t* inds, int64_t B, int64_t S, int64_t W, const int64_t* lens, double* ll, double* counts,
                    void* stream);

/* Viterbi decoding (the reference has no counterpart): the single most probable hidden path of every sequence (b, s).
 * For a row o_0 .. o_{n-1} (n = the row's own length, see lens) with the convention of the forward recursion (z_0 ~ pi
 * precedes site 0, site t is step t + 1, a missing site has e = 1):
 *   (z*_0, z*_1 .. z*_n) = argmax  pi(z_0) * prod_{t=1..n} A[z_{t-1}, z_t] * e_{o_{t-1}}(z_t)
 *   logp = log of that maximum (natural log).
 * Ties: among equal candidates the lowest predecessor index wins, and the lowest final state.  z*_0 is not reported.
 *   logp         [B, S] double;
 *   path         uint8 [B, S, path_stride], path_stride >= L - W: z*_{W+1} .. z*_n, the states at sites W .. n-1 (the
 *                warm-up sites take part in the maximisation and are not reported; there is no warm-up correction of
 *                logp); every byte past a row's own length is 255;
 *   lens         device int64 [N], one own length per data row of the handle (W < lens[i] <= L), or NULL = L for all.
 *                A short contig padded with missing windows is NOT the same problem: the best continuation through a
 *                missing tail depends on the end state and can bend the last tract.  An entry out of range raises the
 *                bad-index flag on the device (reported by phk_underflow_risk; the length is clamped).
 * params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Two kernels per slab of the
 * checkpoint store (phk_set_workspace_limit applies as to a gradient call): the max-product recursion with delta
 * checkpointed every 16 sites (float64: 8), then the traceback.  No plan is tuned or recorded: the call leaves phk_get_plan and the
 * bits of every later call unchanged.  Stream-ordered; no two calls on one handle may overlap.  The underflow flag is
 * raised as by phk_loglik: re-evaluate after phk_set_rescale_interval(h, 1).  PHK_EINVAL, before anything is enqueued,
 * for a NULL handle, NULL params / inds / logp / path, W outside [0, L), path_stride < L - W. */
int phk_viterbi(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                const int64_t* inds, int64_t B, int64_t S, int64_t W, const int64_t* lens, double* logp, uint8_t* path,
                int64_t path_stride, void* stream);

/* Posterior path sampling (forward-filtering backward-sampling; the reference has no counterpart): n_samples whole hidden
 * paths z ~ P(z | o) of every sequence.  Conventions of phk_posterior: z_0 ~ pi precedes site 0, alpha_t is the forward
 * vector after site t, a missing site has e = 1, the W warm-up sites condition the draw and are not reported.
 * For sequence q = b * S + s -- (b, s) the position in THIS CALL, not in a slab and not the data row -- and sample r:
 *   last site      the state at site L-1 is drawn with weights w_i = alpha_{L-1}(i);
 *   earlier sites  for t = L-2 .. W the state at site t given state j at site t+1 is drawn with weights
 *                    w_i = (u_i alpha_t(i)) v_j  (i < j),   d_j alpha_t(j)  (i = j),   b_j alpha_t(i)  (i > j):
 *                  column j of the transition matrix times alpha_t (the kernels' folded factors of column j multiply every
 *                  candidate alike);
 *   one draw       c_i = inclusive prefix sum of w, theta = U c_{K-1}, state = #{ i <= K-2 : c_i <= theta } (the <= skips
 *                  states of weight zero);
 *   U              for (seed, q, r, site t): Philox4x32-10 with counter (t, r, q mod 2^32, q >> 32), key (seed mod 2^32,
 *                  seed >> 32), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, output words
 *                  x0 .. x3.  float64 kernels: U = (x0 2^21 + (x1 >> 11)) 2^-53; float32 kernels: U = (x0 >> 8) 2^-24,
 *                  the top 24 bits of the same number.
 * The generator is counter-based: sample r does not depend on n_samples, on the slabs (phk_set_workspace_limit) or on how
 * the kernel groups samples, and the same seed gives the same bytes.  There is no lens: a draw over a row padded with
 * missing windows has exactly the right marginal on the row's own sites (pad, then cut).
 *   ll           [B, S] double: the forward kernel's by-product, bitwise what phk_posterior returns;
 *   paths        uint8 [B, S, n_samples, path_stride], path_stride >= L - W: the states at sites W .. L-1.
 * params / prefold / inds / strides as phk_loglik_prefolded (prefold NULL: as phk_loglik).  Per slab of the checkpoint
 * store: the forward kernel of the plan a gradient call of this shape would run, as phk_posterior launches it, then the
 * sampling traceback.  The plan is read, never tuned or recorded: the call leaves phk_get_plan and the bits of every later
 * call unchanged.  Stream-ordered; no two calls on one handle may overlap.  The underflow flag is raised as by phk_loglik,
 * and by a draw whose weights have no mass: re-evaluate after phk_set_rescale_interval(h, 1).  PHK_EINVAL, before anything
 * is enqueued, for a NULL handle, NULL params / inds / ll / paths, W outside [0, L), n_samples outside [1, 65535],
 * path_stride < L - W, and phk_viterbi's prefold rules. */
int phk_sample_paths(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                     const int64_t* inds, int64_t B, int64_t S, int64_t W, int64_t n_samples, uint64_t seed, double* ll,
                     uint8_t* paths, int64_t path_stride, void* stream);

/* Sampled tract spectra (the reference has no counterpart): the paths of phk_sample_paths reduced inside the kernel to what is
 * not additive over sites -- how many tracts a row has, how long they are, which bins lie in a long one -- without a byte of
 * path stored.  Conventions of phk_sample_paths: params / prefold / inds / strides, W, n_samples, seed, and q = b * S + s the
 * position in THIS CALL.
 *   draws        sample r of sequence q is, byte for byte, the path phk_sample_paths returns for (seed, q, r) on the same handle
 *                and plan: the same forward leg and alpha checkpoints, the same draw, the same Philox counters, the same folded
 *                factors and rescale schedule.
 *   the set      masks: device uint64 [B] (mask_stride = 1, one per particle) or [1] (mask_stride = 0); state k is inside iff
 *                bit k is set.  Padded states are never drawn, so their bits do not matter.
 *   own reported sites   W <= t < len, len = lens[data row] (device int64 [N] as phk_tracts; NULL = L for all; an entry outside
 *                (W, L] is clamped and raises the bad-index flag).  Sites at or past len are still drawn -- the chain of draws
 *                needs them -- and count for nothing.
 *   a tract      a maximal run of consecutive own reported sites whose state is inside the set.  A tract that touches site W or
 *                site len - 1 is counted at its VISIBLE length: what lies before W or past the row's end is not looked at.
 *   stats        int32 [B, S, n_samples, 4 + C], C = n_edges + 1:
 *                  0  own reported sites inside the set;
 *                  1  number of tracts;
 *                  2  length of the longest tract (0 if none);
 *                  3  number of adjacent pairs (t - 1, t) of own reported sites, both >= W, whose states differ (the set plays
 *                     no part);
 *                  4 .. 3 + C  histogram of tract lengths: a tract of n sites falls in class #{e : edges[e] <= n}, so a length
 *                     equal to an edge goes to the upper class;
 *   edges        HOST array of n_edges strictly ascending int64 >= 1, 0 <= n_edges <= 15 (NULL allowed with n_edges = 0);
 *   cover        int32 [B, S, nbin] or NULL, nbin = ceil((L - W) / bin), bins over the reported sites as in every other call:
 *                the sum over the samples of the number of own reported sites of the bin that lie in a tract of min_len sites
 *                or more (min_len >= 1).  cover / (n_samples x own sites of the bin) estimates P(the window lies in a tract
 *                at least min_len long | o).  bin and min_len are ignored where cover is NULL;
 *   ll           [B, S] double: bitwise what phk_posterior returns, as for phk_sample_paths.
 * Everything is integer: sample r's row of stats depends on (seed, q, r) alone -- not on n_samples, the slabs or how the kernel
 * groups samples, and on the plan only as far as the paths themselves do -- and cover, a sum of integers added in whatever order
 * the units arrive, is the same for any slab size and any repeat of the call.  Per slab of the checkpoint store: the forward
 * kernel of the plan a gradient call of this shape would run, as phk_sample_paths launches it, the reducing traceback, and where
 * cover is wanted a kernel that adds the bins tracts cover whole (kept as an int32 difference row per sequence of the slab: that
 * workspace is part of the slab arithmetic, phk_set_workspace_limit, and a large batch is cut into more slabs).  stats and cover
 * are zeroed by the call.  The plan is read, never tuned or recorded: the call leaves phk_get_plan and the bits of every later
 * call unchanged.  Stream-ordered; no two calls on one handle may overlap.  The underflow flag is raised as by phk_sample_paths.
 * PHK_EINVAL, before anything is enqueued, for a NULL handle, NULL params / inds / ll / stats / masks, W outside [0, L),
 * n_samples outside [1, 65535], mask_stride other than 0 or 1, n_edges outside [0, 15], edges not strictly ascending or
 * edges[0] < 1, L - W >= 2^31 - 1, a non-NULL cover with bin < 1, min_len < 1 or n_samples x min(bin, L - W) >= 2^31, and
 * phk_viterbi's prefold rules. */
int phk_sample_tracts(phk_handle* h, const void* params, int64_t pstride_b, int64_t pstride_s, const float* prefold,
                      const int64_t* inds, int64_t B, int64_t S, int64_t W, int64_t n_samples, uint64_t seed,
                      const uint64_t* masks, int64_t mask_stride, const int64_t* lens, const int64_t* edges, int n_edges, int bin,
                      int64_t min_len, double* ll, int32_t* stats, int32_t* cover, void* stream);

/* Posterior predictive simulation (the reference has no counterpart): n_rep replicate observation rows of L sites drawn from
 * the HMM of every (particle b, row s), laid under row s's accessibility mask; stored, or reduced on the fly to het counts
 * per bin and a histogram of hom-run lengths, or both.  Device-level like phk_param_map: no handle, no plan, no upload.
 * This comment is the definition; kernel and CPU restatement agree with it exactly, bit for bit.
 *   params       device float64 [B, S or 1, 7, K], rows b,d,u,v,emis0,emis1,pi, element strides pstride_b / pstride_s
 *                (pstride_s = 0: the particle's one block serves its S rows); K any integer in [2, 64], no padding.
 *   arithmetic   IEEE float64, each operation rounded once, in the order written here; no division.
 *   sequences    (b, s, r), r in [0, n_rep), numbered q = seq0 + b S + s: seq0 lets a caller cut a call into slabs over
 *                particles without changing a draw.
 *   uniforms     Philox4x32-10, key (seed mod 2^32, seed >> 32), multipliers, Weyl constants and the 53-bit formula
 *                U(x, y) = (x 2^21 + (y >> 11)) 2^-53 of phk_sample_paths.  The block at counter (t, r, q mod 2^32, q >> 32)
 *                serves site t: U1_t = U(x0, x1) drives the transition into site t, U2_t = U(x2, x3) the emission at site t;
 *                the block at counter (0xFFFFFFFF, r, q lo, q hi) gives U0 = U(x0, x1) for the state before site 0.  Hence
 *                L <= 2^32 - 2.
 *   tables       per block, serial sums in ascending index: cp_j = sum_{k<=j} pi_k, cb_j = sum_{k<=j} b_k, cv_j = sum_{k<=j} v_k.
 *   start        z = #{k <= K-2 : cp_k <= U0 cp_{K-1}}.
 *   transition   from state i into site t: PB = cb_{i-1} (0 for i = 0), SV = cv_{K-1} - cv_i, tot = (PB + d_i) + u_i SV,
 *                theta = U1_t tot.  theta < PB: j = #{k <= i-1 : cb_k <= theta}.  Otherwise phi = theta - PB; phi < d_i: j = i.
 *                Otherwise psi = phi - d_i and j = min(K-1, i + 1 + #{k : i < k <= K-2, u_i (cv_k - cv_i) <= psi}).
 *   emission     at state j the code is 1 (het) iff U2_t (emis0_j + emis1_j) < emis1_j, else 0 (the rows need not sum to one).
 *   mask         device int8 [S, mask_stride] or NULL: where mask[s, t] < 0 the reported code is -1.  The hidden path and
 *                every uniform are what they are without a mask; the mask is laid over the output only.
 *   no mass      a draw whose total is not positive or not finite sets bit 0 of *flags (a plain store of 1) and is replaced:
 *                cp_{K-1}: the start state is 0; tot of state i: the state stays i; emis0_j + emis1_j: the code is 0.  Each
 *                of the three is judged alone, and the call completes normally.
 * Outputs, each may be NULL (at least one is given):
 *   obs          int8 [B, S, n_rep, row_stride]: the reported codes -1 / 0 / 1 at sites 0 .. L-1;
 *   paths        uint8, same shape: the state at each site.  The kernel stores 16 bytes per lane: obs, paths (where given)
 *                and row_stride must be multiples of 16 bytes, row_stride >= L.  Bytes at positions >= L of a row are
 *                never written;
 *   het          int32 [B, S, n_rep, nbin], nbin = ceil(L / bin): the sites of the bin whose reported code is 1;
 *   runs         int32 [B, S, n_rep, 32]: histogram over floor(log2(len)) of the maximal runs of consecutive sites with
 *                reported code 0; a het, a missing site or the end of the row ends a run, and a run is counted when it ends;
 *   flags        one device int32, required; it is only ever set, the caller clears it.
 * Stream-ordered, does not synchronise.  PHK_EINVAL, before anything is enqueued, for K outside [2, 64]; B, S, n_rep or
 * L < 1; n_rep > 65535; L > 2^32 - 2; NULL params or flags; all four outputs NULL; bin < 1 with het given; with obs or
 * paths given, row_stride < L or a violated alignment rule; mask_stride < L with a mask; more workgroups than one launch
 * holds (2^31 - 1 of 64 sequences that share a parameter block). */
int phk_simulate(int device, int K, const double* params, int64_t pstride_b, int64_t pstride_s, int64_t B, int64_t S,
                 int64_t n_rep, int64_t L, uint64_t seed, int64_t seq0, const int8_t* mask, int64_t mask_stride, int8_t* obs,
                 uint8_t* paths, int64_t row_stride, int bin, int32_t* het, int32_t* runs, int32_t* flags, void* stream);

/* Particle -> PSMCParams for a whole population in one launch, float64, with its Jacobian.
 * Replaces, for B particles at once: MCMCParams.to_dm (src/phlash/params.py:94-127),
 * SizeHistory.ect / .pi (src/phlash/size_history.py:123-138,170-193), transition_matrix + _expQ
 * (src/phlash/transition.py:9-85) and PSMCParams.from_dm (src/phlash/params.py:33-55), which the
 * reference evaluates per particle under vmap and differentiates with jax.grad.
 *   K                 hidden states (3..64); P epochs; epoch_of_state[K] (host) maps each state to its
 *                     epoch (the expansion of the PSMC pattern, src/phlash/util.py:35-37)
 *   x        device   [B, P+3] = t_tr(2), c_tr(P), rho_over_theta_tr  (ravel order of params.py:58-66)
 *   params   device   [B, 7, K] rows b,d,u,v,emis0,emis1,pi
 *   jac      device   [B, 7*K, P+3] d params / d x, or NULL */
int phk_param_map(int device, int K, int P, const int32_t* epoch_of_state, double theta, const double* x,
                  int64_t B, double* params, double* jac, void* stream);

/* The same, and the [B, 7, K] block once more rounded to float32 (params_f32, may be NULL): what a float32 kernel
 * object takes in phk_loglik, without a conversion launch in between. */
int phk_param_map_rounded(int device, int K, int P, const int32_t* epoch_of_state, double theta, const double* x,
                      int64_t B, double* params, double* jac, float* params_f32, void* stream);

/* The tail of a sampler step between the likelihood kernels and the SVGD update, two launches.
 * phk_reduce_chunks: the sum over the minibatch that model.py:57 takes (``.sum()``), for value and gradient, and the
 *   hand-over of the kernel object's flags, in the layout that is all-reduced over the ranks:
 *     ll   device double [B, S], grad device [B, S, 7, K] (float or double as the handle): outputs of phk_loglik
 *     buf  device double [B + 1, 1 + 7K]: row b = [sum_s ll, sum_s grad]; row B = [underflow flag, bad-index flag,
 *          0...] as 0.0 / 1.0 (the handle's flag word is cleared, as by phk_take_flags_async)
 * phk_chain_rule: log density of every particle and its gradient in particle space -- what the reference obtains
 *   with jax.grad through log_density (src/phlash/model.py:24-73) and PSMCParams.from_dm(MCMCParams.to_dm()):
 *     logp[b] = c_prior * log_prior(x_b) + c_hmm * buf[b, 0] + c_extra * extra_val[b]
 *     grad[b] = c_prior * d log_prior / d x_b + c_hmm * jac[b]^T buf[b, 1:] + c_extra * extra_grad[b]
 *   x [B, P+3], jac [B, 7K, P+3] (phk_param_map), buf as above after the all-reduce; extra_val [B] / extra_grad
 *   [B, P+3] may be NULL (the AFS term, evaluated elsewhere).  A particle whose logp is not finite gets -inf and a
 *   zero gradient (model.py:73 under jax.grad). */
int phk_reduce_chunks(phk_handle* h, const double* ll, const void* grad, int64_t B, int64_t S, double* buf, void* stream);
int phk_chain_rule(int device, int K, int P, double alpha, double beta, const double* x, const double* buf,
                   const double* jac, int64_t B, double c_prior, double c_hmm, const double* extra_val,
                   const double* extra_grad, double c_extra, double* logp, double* grad, void* stream);

/* The AFS term of the objective with its gradient w.r.t. the particles, one launch.  Replaces, under vmap + jax.grad,
 *   l3 = xlogy(T afs, T esfs).sum(),  esfs = etbl / etbl.sum(),  etbl = W etjj          (src/phlash/model.py:58-68,
 *   size_history.py:212-226: etjj_k = int_0^inf exp(-k(k-1)/2 R(t)) dt, k = 2..n, through JaxPPoly.exp_integral,
 *   jax_ppoly.py:44-84; W = _W_matrix(n), size_history.py:350-369),
 * a function of the particle through t = [0, geomspace(t1, tM, K-1)] and c = softplus(c_tr) by epoch only (params.py:94-127).
 *   x      device [B, P+3];  n: sample size (n - 1 spectrum entries), 3 <= n <= 128 (n = 2: the term is 0, do not call)
 *   tw     device [m, n-1] = T W,  w1 device [n-1] = column sums of W,  y device [m] = T afs   (constants of a run;
 *          T = identity, m = n - 1, when the run has no afs_transform)
 *   value  device [B];  grad device [B, P+3]: the arguments extra_val / extra_grad of phk_chain_rule */
int phk_afs_term(int device, int K, int P, const int32_t* epoch_of_state, const double* x, int64_t B, int n, int m,
                 const double* tw, const double* w1, const double* y, double* value, double* grad, void* stream);

/* log_prior of the whole population with its gradient, one launch.  Replaces log_prior
 * (src/phlash/model.py:11-21) under vmap + jax.grad:
 *   value[b] = logN(log(rho/theta); 0, 1) - alpha * sum_i (log c_{i+1} - log c_i)^2 - beta * |x_b|^2
 * with rho/theta = 0.1 + 9.9 sigmoid(x[P+2]) and c = softplus(x[2 .. 2+P)) per epoch (params.py:106-118).
 *   x      device [B, P+3];  value device [B];  grad device [B, P+3] d value / d x, or NULL */
int phk_log_prior(int device, int P, double alpha, double beta, const double* x, int64_t B, double* value,
                  double* grad, void* stream);

/* The SVGD / AMSGrad update of the sampler's inner step for the whole population on the device:
 *   phi_j = (1/B) sum_i [ -k_ij g_i + (2/h)(x_i - x_j) k_ij ],  k_ij = exp(-|x_i - x_j|^2 / h);
 *   AMSGrad (b1, b2, eps, bias correction with `count` = the step number starting at 1, running max of the
 *   corrected second moment), x_out = x - lr mu_hat / (sqrt(nu_max) + eps);
 *   h_out = median(pairwise distances of x_out)^2 / log B  (median as torch.quantile(., 0.5)).
 * Replaces what the reference delegates to blackjax.svgd(..., optax.amsgrad(lr)) per iteration
 * (src/phlash/mcmc.py:178-199, 279; blackjax 1.2.5 / optax 0.2.6).  All arrays device float64:
 *   x, grad_logp, mu, nu, nu_max, x_out [B, D] (mu, nu, nu_max updated in place; x_out must not alias x);
 *   h_in, h_out scalars (may alias); dist_ws workspace of phk_svgd_workspace_doubles(B) doubles, whose first
 *   B (B - 1) / 2 hold the pairwise distances of x_out on return (strict lower triangle).  The median is an exact
 *   bucket select: by one workgroup up to 256 particles, over the whole chip beyond (the reference's default is
 *   500).  h_out = NULL skips it.  B <= 4096, D <= 72. */
int64_t phk_svgd_workspace_doubles(int64_t B);
int phk_svgd_step(int device, int64_t B, int D, const double* x, const double* grad_logp, double* mu, double* nu,
                  double* nu_max, const double* h_in, double* h_out, double* x_out, double* dist_ws, int64_t count,
                  double lr, double b1, double b2, double eps, void* stream);

/* Tuning / introspection (no reference counterpart).
 * R = lanes per sequence (1,2,4,8,16; must divide K, K/R <= 16), T = checkpoint block (8, or 16
 * where K/R <= 4).
 * 0 = choose automatically from B*S. */
int phk_set_variant(phk_handle* h, int R, int T);
int phk_get_variant(phk_handle* h, int64_t B, int64_t S, int* R, int* T);
/* With autotuning on (default; environment PHK_AUTOTUNE=0 turns it off) the first phk_loglik for a
 * new batch shape times every compiled (R, T) on the first 2,048 sites of that batch (scratch
 * outputs, a few tens of ms, synchronises the stream once) and keeps the fastest; otherwise a
 * static rule picks R from the sequence count. */
int phk_set_autotune(phk_handle* h, int on);
/* How the gradient is evaluated: 0 = serial (forward kernel, then one backward sweep per sequence:
 * best when B*S sequences fill the chip), 1 = segmented (forward kernel and an independent
 * beta-recursion kernel run concurrently on two streams, then every 512-site segment of every
 * sequence is swept in parallel, each unit storing its partial sums in a slot of its own that a
 * finalize kernel adds up in unit order: best for small batches such as the reference's 500
 * particles x 5 chunks), -1 = automatic (default; the autotuner times both where the batch is small). */
int phk_set_backward_mode(phk_handle* h, int mode);
/* Force a complete plan (segmented = -1 returns to automatic).  Serial: (R, T).  Segmented: R for
 * the segment sweep, R_forward for the forward kernel, R_scan for the beta scan; T (8 or 16) is
 * shared by the forward kernel and the sweep. */
int phk_set_plan(phk_handle* h, int segmented, int R, int T, int R_forward, int R_scan);
/* The plan the last phk_loglik ran with. */
int phk_get_plan(phk_handle* h, int* segmented, int* R, int* T, int* R_forward, int* R_scan);
/* Hybrid form of the serial plan (chosen by the tuner where the serial sweep would leave wave slots
 * empty): sequences [0, first) of the launch are swept serially, the rest by segments (R_sweep lanes
 * per sequence, seeds from a beta scan with R_scan) at the same time.  first = 0: not hybrid. */
int phk_get_plan_hybrid(phk_handle* h, int64_t* first, int* R_sweep, int* R_scan);
/* Force the hybrid part of a plan forced with phk_set_plan(h, 0, R, T, R_forward, 0) (first = 0: plain serial).
 * Together the two calls reproduce what phk_get_plan + phk_get_plan_hybrid report, so that one rank's tuned
 * plan can be installed on its peers (the reference's GPUs all run the same kernel, gpu.py:386-438). */
int phk_set_plan_hybrid(phk_handle* h, int64_t first, int R_sweep, int R_scan);
/* The scaled forward state is brought back to [0.5,1) by an exact power of two after every nrm-th
 * site (1, 2 or 4; 0 = library default).  nrm = 1 is the reference's per-site normalisation
 * (hmm.py:77-79); larger intervals do the same arithmetic with fewer rescales and are safe while
 * nrm consecutive sites cannot shrink the total mass below the float range. */
int phk_set_rescale_interval(phk_handle* h, int nrm);
/* With nrm > 1 the forward kernel raises a sticky flag when a rescale finds the total mass below
 * 2^-64 (float) / 2^-600 (double), i.e. the parameters are extreme enough that the unscaled sites in
 * between could have lost precision.  Reads (and clears) the flag; synchronises with the work
 * enqueued before.  The Python host re-evaluates such a call with nrm = 1.
 * The same word carries two failure bits: a chunk index outside [0, N) (returns PHK_EINVAL) and, round 6, a kernel
 * loop that ran out of its iteration budget (returns PHK_EOVERRUN; the message names kernel, sequence and block). */
int phk_underflow_risk(phk_handle* h, int* flag);
/* Test hook: scale the iteration budgets the kernels of this handle are given (default 1 / 1; the budget is twice the
 * row's block count, an upper bound on the iterations any loop of a kernel can legitimately make).  kernels: bit 0 forward
 * kernel, bit 1 backward kernel, bit 2 beta scan.  A scale below ~1/2 makes a healthy evaluation overrun, which is how
 * tests/test_plans_and_modes.py exercises the PHK_EOVERRUN path. */
int phk_set_loop_budget_scale(phk_handle* h, int kernels, int num, int den);
/* Test hook (synchronises): of the checkpoint blocks the forward kernel wrote in the last launch of the last gradient call, how
 * many per sequence carry a non-zero exponent, i.e. had a power of two taken out of the state inside them.  counts[i], i < min(n,
 * sequences of that launch), in the launch's storage order; *blocks = checkpoint blocks per sequence.  The forward kernels with
 * several states per lane rescale on demand at the default interval (a sequence only once its mass has fallen below 2^-16), so
 * nearly every block of an ordinary row counts 0 there; tests/test_rescale_on_demand.py reads how often the rescale fired. */
int phk_block_rescale_counts(phk_handle* h, int64_t* counts, int64_t n, int64_t* blocks);
/* The K = 16 float32 sweeps with two lanes per sequence run their hot blocks through a hand-written instruction sequence
 * (csrc/sweep_run_k16r2.inc, generated by scripts/gen_sweep_asm.py: the C++ body's arithmetic, operation for operation, an all-hom
 * block without its per-site tests and with the beta pass's suf(v.*w) kept for the forward pass).  It returns the same bits as the
 * C++ body (tests/test_asm_run_default.py, tests/test_hip_parity.py::test_asm_block_run_equals_the_cxx_body).  A new K = 16
 * float32 handle has it on; on = 0, or PHK_ASM_RUN=0 in the environment when the handle is created, selects the C++ body.  Handles
 * of other kernels have no such sequence: the flag stays 0 whatever is asked.  A library built with -DPHK_ASM_RUN=0 answers
 * on = 1 with PHK_EUNSUPPORTED.  Timings: profiles/ab_asm_run.txt. */
int phk_set_asm_run(phk_handle* h, int on);
/* 1 if the handle's sweeps use that sequence, else 0. */
int phk_get_asm_run(const phk_handle* h);
/* The K = 16 float32 forward kernel with one lane per sequence, writing checkpoints (the forward phase of the headline shape), runs
 * its lean 64-site pieces -- in waves that hold at most two observation rows and whose sequences fold -- through a hand-written
 * instruction sequence (csrc/fwd_run_k16r1.inc, generated by scripts/gen_fwd_asm.py: Lane::fwd_site<false> operation for operation,
 * an all-hom block without its per-site tests, no pairing moves, the checkpoint stores from a wave-uniform base).  It returns the same
 * bits as the C++ body (tests/test_fwd_run.py).  on = 0, or PHK_FWD_RUN=0 in the environment when the handle is created, selects
 * the C++ body.  Handles of other kernels have no such sequence: the flag stays 0 whatever is asked.  A library built with
 * -DPHK_FWD_RUN=0 answers on = 1 with PHK_EUNSUPPORTED.  Default and timings: profiles/ab_fwd_run.txt. */
int phk_set_fwd_run(phk_handle* h, int on);
/* 1 if the handle's forward kernel uses that sequence, else 0. */
int phk_get_fwd_run(const phk_handle* h);
/* The same flag word handed over WITHOUT a host synchronisation: a one-thread kernel on `stream`
 * writes dst[0] = 1.0 if the underflow-risk bit is set (else 0.0), dst[1] = 1.0 if a chunk index was
 * outside [0, N) (else 0.0) -- `dst` is a device array of two doubles -- and clears the word.  The
 * multi-rank host puts `dst` inside the buffer it all-reduces (SUM) anyway, so that every rank sees the same flags and takes the same redo branch
 * (the reference has no counterpart: its kernel objects are driven by threads of one process,
 * gpu.py:386-438). */
int phk_take_flags_async(phk_handle* h, double* dst, void* stream);
/* Deterministic mode (also environment PHK_DETERMINISTIC=1): the plan comes from the static rule,
 * never from a timing, and every reduction runs in a fixed order, so two calls with the same inputs
 * return the same bits.  (Without it the tuner may pick different variants on different runs, and
 * float32 variants differ in their last digits.) */
int phk_set_deterministic(phk_handle* h, int on);
/* Upper bound for the checkpoint workspace; larger problems are run in particle / chunk slabs. */
int phk_set_workspace_limit(phk_handle* h, int64_t bytes);
int64_t phk_workspace_bytes(phk_handle* h);
/* The (particles x chunks) slab the last phk_loglik was cut into (= B x S when it ran as one launch). */
int phk_get_slab(phk_handle* h, int64_t* particles, int64_t* chunks);
/* With profiling on, every phk_loglik records HIP events around its kernels on the call's stream;
 * phk_last_timing waits for them and returns the summed device time of the forward and backward
 * kernels of the last call (ms) and the number of launches of each. */
int phk_set_profiling(phk_handle* h, int on);
int phk_last_timing(phk_handle* h, float* fwd_ms, float* bwd_ms, int* n_launches);
/* Same, summed over every call since the previous phk_timing_totals (or since profiling was
 * switched on); waits once, at query time, so a timed loop needs no per-step synchronisation. */
int phk_timing_totals(phk_handle* h, double* fwd_ms, double* bwd_ms, int* n_launches);

/* Environment variables read by the library (none is needed in normal use):
 *   PHK_AUTOTUNE=0         static plan rule instead of the timing-based tuner
 *   PHK_DETERMINISTIC=1    as phk_set_deterministic(h, 1) for every handle
 *   PHK_TUNE_VERBOSE=1     the tuner's timings and decision on stderr
 *   PHK_HYBRID=R:Rf:first:R3:R2   developer override of the hybrid plan (tests)
 *   PHK_SIDE_PRIO=high     second stream at the highest instead of the lowest priority (A/B runs)
 *   PHK_POISON=<byte>      diagnostic: fill the scratch buffers with that byte before every launch sequence
 *                          (255: NaN patterns); PHK_POISON_MASK selects buffers */

#ifdef __cplusplus
}
#endif
#endif
