/*
 * libvargp_hip — C ABI of the MI355X (gfx950) kernels behind the VAR-GP ELBO hot path.
 *
 * The reference (uber-research/vargp) has no FFI: its hot path is Python on top of ATen call sites
 * (SURVEY.md §2.3).  Each entry point below replaces one group of those call sites; the reference
 * lines are cited per function.  Conventions:
 *   - all tensors are contiguous row-major fp32 DEVICE pointers unless a leading dimension /
 *     stride argument says otherwise; labels are int64; the caller owns every buffer, including
 *     the workspace (size from the matching *_workspace_bytes query);
 *   - every function only enqueues work on `stream` and never synchronises or allocates, so the
 *     caller may capture a sequence of calls into a hipGraph;
 *   - return value: 0 on success, negative VARGP_E* on a bad argument / launch failure
 *     (vargp_last_error() gives the text).  Numerical failure of a Cholesky is reported through the
 *     device-side `info` array (0 = ok, j+1 = first non-positive pivot, LAPACK style); the factor
 *     of a failed matrix is filled with NaN so the failure cannot go unnoticed downstream.
 */
#ifndef VARGP_HIP_H
#define VARGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vargp_stream_t; /* a hipStream_t */

#define VARGP_OK 0
#define VARGP_EINVAL (-1)
#define VARGP_ELAUNCH (-2)
#define VARGP_EWORKSPACE (-3)

int vargp_version(void);
const char* vargp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Batched strided fp32 GEMM on the f32 MFMA (v_mfma_f32_32x32x2_f32):
 *     C[b] = alpha * op(A[b]) * op(B[b]) + beta * D[b]          op(A): M x K, op(B): K x N
 * Replaces the einsum/bmm call sites of var_gp/gp_utils.py:18,94,96,127,131,136,178,184 and the
 * triangular_solve call sites :89,92,124-134,175-182 (solves are products with the explicit
 * inverse factor T = L^-1 produced by vargp_chol_inv_fwd).
 * transX = 0: X stored row-major as op(X) (ldx = row stride); transX = 1: stored as op(X)^T.
 * Batch index b = (i0*nb[1] + i1)*nb[2] + i2, element strides per batch dim (0 = broadcast).
 * triA/triB: structure hint for op(A)/op(B) (0 none, 1 lower-triangular, 2 upper-triangular); the
 * stored zeros must really be zero, the hint only clips the K range.
 * triC: 0 full; 1 compute the lower triangle and write zeros above it; 2 compute and write only
 * tiles that touch the lower triangle (entries above the diagonal are left unspecified / untouched).
 * D may be NULL (beta ignored) and may alias C.
 */
typedef struct vargp_gemm_desc {
  int32_t M, N, K;
  int32_t transA, transB;
  const float* A;
  const float* B;
  float* C;
  const float* D;
  int32_t lda, ldb, ldc, ldd;
  int32_t nb[3];
  int64_t sA[3], sB[3], sC[3], sD[3];
  float alpha, beta;
  int32_t triA, triB, triC;
} vargp_gemm_desc;

int vargp_bgemm(const vargp_gemm_desc* d, vargp_stream_t stream);

/* out[i] = sum_r in[r*inner + i], r < outer   (reduction of broadcast batch dims in backward) */
int vargp_sum_outer(const float* in, float* out, int64_t outer, int64_t inner, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RBF / ARD kernel matrix (reference: RBFKernel.compute, var_gp/kernels.py:24-56).
 *   theta[S, D+1] = [log lengthscale_1..D, log gamma];  X[C, M, D];
 *   Y: NULL (Y = X, symmetric K_uu: the diagonal is exactly gamma^2, kernels.py:47-48,54),
 *      or [C, N, D] (y_shared = 0), or [N, D] shared by every class (y_shared = 1; the reference
 *      expands the minibatch over classes, var_gp/vargp.py:106);
 *   K[S, C, M, N] = gamma_s^2 * exp(-0.5 * (|x/sig|^2 + |y/sig|^2 - 2 (x/sig).(y/sig))), no clamp.
 * Backward (autograd of the same lines): gK[S,C,M,N] -> gX[C,M,D], gY (NULL if not wanted; for
 * Y = NULL both sides are accumulated into gX), gtheta[S, D+1].
 */
size_t vargp_rbf_workspace_bytes(int S, int C, int M, int N, int D, int backward);
int vargp_rbf_gram_fwd(const float* theta, const float* X, const float* Y, float* K, int S, int C, int M,
                       int N, int D, int y_shared, void* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_rbf_gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK,
                       float* gX, float* gY, float* gtheta, int S, int C, int M, int N, int D, int y_shared,
                       int accumulate /* add into gX / gY / gtheta instead of overwriting */, void* ws, size_t ws_bytes,
                       vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Matern / ARD kernel matrix, nu = nu2 / 2 with nu2 = 1, 3 or 5 (anything else is an error).  Arguments, layouts, the three
 * Y cases and `accumulate` exactly as for the RBF entries above.  With d2 the same scaled squared distance, clamped at 0
 * (the inner-product form can come out slightly negative), and r = sqrt(d2):
 *   K / gamma^2 = exp(-r) | (1 + sqrt3 r) exp(-sqrt3 r) | (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r);
 *   for Y = NULL the diagonal is exactly gamma^2.
 * Backward: the derivative of nu = 1/2 with respect to d2, -exp(-r) / (2 r), is DEFINED as 0 where d2 <= 0 (coincident points
 * contribute nothing to gX, gY and the lengthscale part of gtheta); the other two are finite there.  The backward recomputes
 * d2 from X and Y (nothing is carried over from the forward call but K), so its workspace is the larger one.
 */
size_t vargp_matern_workspace_bytes(int S, int C, int M, int N, int D, int backward);
int vargp_matern_gram_fwd(const float* theta, const float* X, const float* Y, float* K, int S, int C, int M, int N, int D,
                          int y_shared, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_matern_gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK, float* gX,
                          float* gY, float* gtheta, int S, int C, int M, int N, int D, int y_shared, int nu2, int accumulate,
                          void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Batched Cholesky with jitter + explicit inverse factor (reference: gp_utils.cholesky,
 * var_gp/gp_utils.py:5-11, and every torch.triangular_solve(., Lz) that consumes it).
 *   A[nbatch, n, n] symmetric (lower triangle read);  L = chol(A + eps I) lower, zeros above;
 *   T = L^-1 (lower; NULL to skip);  logdet[nbatch] = sum_i log L_ii (NULL to skip);
 *   info[nbatch] as described at the top.
 * Backward: gA = d/dA of <gL, L> + <gT, T> (either may be NULL), symmetric like torch's
 * cholesky_backward.
 */
size_t vargp_chol_workspace_bytes(int nbatch, int n, int backward);
int vargp_chol_inv_fwd(const float* A, float eps, float* L, float* T, float* logdet, int32_t* info, int nbatch,
                       int n, void* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_chol_inv_bwd(const float* L, const float* T, const float* gL, const float* gT, float* gA, int nbatch,
                       int n, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* Triangular solve against a factor L whose inverse T = L^-1 came with it from vargp_chol_inv_fwd (reference:
 * torch.triangular_solve(B, L, upper=False), var_gp/gp_utils.py:89,92,124-134,175-182).  By design a solve is a product
 * with T on the MFMA; these entries exist so that the op list of SURVEY.md §8(b) is complete.
 *   fwd: X[nb, n, nrhs] = T B.     bwd: gB = T^T gX,  gL = -tril(gB X^T)  (the adjoint w.r.t. L; either may be NULL;
 *   gB == NULL needs a workspace of nb*n*nrhs floats).
 */
int vargp_trsm_lower_fwd(const float* T, const float* B, float* X, int nbatch, int n, int nrhs, vargp_stream_t stream);
int vargp_trsm_lower_bwd(const float* T, const float* X, const float* gX, float* gB, float* gL, int nbatch, int n, int nrhs,
                         void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Packed lower triangle <-> matrix with softplus on the diagonal (reference: vec2tril /
 * mat2trilvec, var_gp/gp_utils.py:22-65; packing order = torch.tril_indices, row-major).
 */
int vargp_vec2tril_fwd(const float* vec, float* tril, int nbatch, int m, vargp_stream_t stream);
int vargp_vec2tril_bwd(const float* vec, const float* gtril, float* gvec, int nbatch, int m,
                       vargp_stream_t stream);
int vargp_mat2trilvec(const float* mat, float* vec, int nbatch, int m, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Predictive marginal mean / variance reductions (reference: linear_marginal_diag,
 * var_gp/gp_utils.py:178-186):  with P = Lz^-1 Kzx [nb, M, B], W = (Lz^-1 L_S)^T P [nb, M, B],
 * a = Lz^-1 m [nb, M]:   mu_b = sum_m P_mb a_m;  var_b = kdiag - sum_m P_mb^2 + sum_m W_mb^2,
 * kdiag[nb] (= gamma^2 of the sample, kernels.py:58-60).
 * a_stride: element stride between consecutive a_m (1 = contiguous [nb, M]; the fused path reads a as a
 * column of a wider matrix), a_bstride: stride between batches.  ga is always written contiguous [nb, M].
 */
int vargp_predictive_diag_fwd(const float* P, const float* W, const float* a, int64_t a_stride, int64_t a_bstride,
                              const float* kdiag, float* mu, float* var, int nbatch, int M, int B,
                              vargp_stream_t stream);
int vargp_predictive_diag_bwd(const float* P, const float* W, const float* a, int64_t a_stride, int64_t a_bstride,
                              const float* gmu, const float* gvar, float* gP, float* gW, float* ga, float* gkdiag,
                              int nbatch, int M, int B, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Full predictive covariance of one block of B test points (the reference has the formula only in gp_cond; nothing there
 * forms the marginal's off-diagonal).  With P and W [S*C, Mt, B] exactly as for vargp_predictive_diag_fwd, theta [S, D+1] and
 * X [B, D] the block itself, shared by all classes:
 *   Sigma[s, c] = K_theta_s(X, X) - P[s,c]^T P[s,c] + W[s,c]^T W[s,c]        Sigma [S*C, B, B], dense, fp32
 * in ONE pass over the output (a tile stays in the MFMA accumulators from the distance product through the kernel epilogue
 * and the product over the stacked 2 Mt rows to its only store).  nu2: 0 = RBF, 1 | 3 | 5 = Matern, nu = nu2 / 2 (the coding
 * of vargp_elbo_tn_desc.kernel_nu2; anything else is an error).  K follows the gram entries with Y = NULL: exactly gamma^2 on
 * the diagonal, the direct distance form for D <= 32, the inner-product form above (d2 clamped at 0 for the Matern kernels
 * only).  Only the lower triangle is computed and every entry is written to both halves: Sigma is bitwise symmetric, and
 * its diagonal is vargp_predictive_diag_fwd's var up to the order of summation.  Any Mt, B, D >= 1; S*C <= 65535.
 */
size_t vargp_predictive_cov_workspace_bytes(int S, int B, int D);
int vargp_predictive_cov(const float* theta, const float* X, const float* P, const float* W, float* Sigma, int S, int C,
                         int Mt, int B, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Random-Fourier-feature paths (csrc/rff.hip; nothing of this is in the reference): the feature matrix of a point set times a
 * block of weight columns, for every hyper-sample s and output c, without the features ever being written to memory.  With
 * theta [S, D+1] (log lengthscales, log gamma), omega [R, D] the frequencies and coef [S*C, 2R, N]:
 *   p[s, i, r]      = sum_d X[i, d] omega[r, d] / exp(theta[s, d])
 *   Phi_s(X)[i, :]  = exp(theta[s, D]) / sqrt(R) [cos p[s, i, :] | sin p[s, i, :]]
 *   out[s, c, i, k] = sum_j Phi_s(X)[i, j] coef[s, c, j, k]                  out [S*C, n, N], dense, fp32
 * x_shared = 1: X [n, D], one point set for all outputs (the C N columns of a hyper-sample share one set of features);
 * x_shared = 0: X [C, n, D], a point set per output.  One pre-scaling launch (omega / lengthscales into the workspace) and ONE
 * launch for everything else: f32 MFMA phase tiles, sin / cos on the phase reduced to revolutions (accurate at any |p|), the
 * second MFMA product accumulated over all of R by the workgroup that owns the output tile -- no atomics, two calls are bitwise
 * equal.  Any n, D, R, N >= 1; S*C <= 65535; C*N <= 2^22.
 */
size_t vargp_rff_paths_workspace_bytes(int S, int D, int R);
int vargp_rff_paths(const float* theta, const float* X, const float* omega, const float* coef, float* out, int S, int C, int n,
                    int D, int R, int N, int x_shared, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* The backward of vargp_rff_paths in the points, same operand layouts; gout [S*C, n, N] is the gradient of out.  With
 * om[s, r, d] = omega[r, d] / exp(theta[s, d]) and gs[s] = exp(theta[s, D]) / sqrt(R):
 *   h[s, i, r] = sum_(c, k) gout[s, c, i, k] (-sin p[s, i, r] coef[s, c, r, k] + cos p[s, i, r] coef[s, c, R + r, k])
 *   gX[i, d]   = sum_s gs[s] sum_r h[s, i, r] om[s, r, d]                      gX [n, D] (x_shared = 1) | [C, n, D] (0)
 * (x_shared = 0: the sum in h runs over k only, on output c's own points, and gX keeps its c index.)  One pre-scaling launch,
 * ONE fused launch (phase tile, gout coef^T, h and h om per 64 frequencies; neither p, the features nor h reach memory) whose
 * workgroups each own one hyper-sample and one piece of R, and -- when that makes more than one partial sum -- one launch that
 * adds the partial sums from the workspace in ascending order.  No atomics: two calls are bitwise equal.  Any n, D, R, N >= 1;
 * S*C <= 65535; C*N <= 2^22; gX below 2^31 elements.
 */
size_t vargp_rff_paths_bwd_workspace_bytes(int S, int C, int n, int D, int R, int x_shared);
int vargp_rff_paths_bwd(const float* theta, const float* X, const float* omega, const float* coef, const float* gout, float* gX,
                        int S, int C, int n, int D, int R, int N, int x_shared, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Lloyd's two steps for G independent sets of K centres Z [G, K, D] over one data matrix X [N, D] (the model's z [C, M, D]: one
 * set per output).  Data-dependent initialisation of the inducing points; nothing of this is in the reference, whose inducing
 * points start at random data points (var_gp/vargp.py:207).
 *   assign: label[g, n] = argmin_k |x_n - z_gk|^2 in plain squared Euclidean distance, the smallest index on a tie, and
 *           dist2[g, n] = that distance, clamped at 0.  The N x K distances stay in registers (f32 MFMA inner products for
 *           D > 32, compared as |z|^2 - 2 x.z; the direct sum of squared differences for D <= 32, exactly 0 for coincident
 *           points); only the two [G, N] vectors are stored.
 *   update: Z[g, k] = mean of the points with label[g, n] == k (fp64 sums in ascending point order), count[g, k] = their number;
 *           a centre without points keeps its value bit for bit.  Labels outside [0, K) are ignored.
 * Both are deterministic (no atomics): two calls on the same input are bitwise equal.  The workspace holds the squared norms
 * of the rows of X and Z only (4 (N + G K) bytes and padding for D > 32): it never grows with N K.  Any G, K, N, D >= 1;
 * G <= 65535 (update: K <= 65535 too).
 */
size_t vargp_kmeans_workspace_bytes(int G, int K, int N, int D);
int vargp_kmeans_assign(const float* X, const float* Z, int32_t* label, float* dist2, int G, int K, int N, int D, void* ws,
                        size_t ws_bytes, vargp_stream_t stream);
int vargp_kmeans_update(const float* X, const int32_t* label, float* Z, int32_t* count, int G, int K, int N, int D, void* ws,
                        size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Greedy conditional-variance selection of inducing points: a pivoted Cholesky of K(X_cand, X_cand) for G independent candidate
 * sets over one data matrix X [N, D] and ONE hyper vector theta [D + 1] (log lengthscale_1..D, log gamma).  Not in the reference.
 *   k(x, y) = gamma^2 f(r), r^2 = sum_d ((x_d - y_d) / lengthscale_d)^2 formed directly at every D (coincident points give exactly
 *   gamma^2); f by nu2: 0 = RBF, 1 | 3 | 5 = Matern nu = nu2 / 2, as the gram entries define it.
 *   cand [G, Nc]: row numbers into X (numbers outside [0, N) are clamped into it), or NULL = rows 0..Nc-1 for every set (Nc <= N).
 *   LT [G, k0 + M, Nc], k-major: row k is the k-th Cholesky column over the candidates.  d [G, Nc]: residual variances.
 *   k0 == 0: the call sets d = gamma^2.  k0 > 0: rows 0..k0-1 of LT and all of d are the caller's (a factorisation already begun,
 *   e.g. from earlier tasks' inducing points: LT0 = chol(K(z, z) + eps I)^-1 K(z, x_cand), d = gamma^2 - colsum(LT0^2)).  Nothing is
 *   marked selected on entry in either case.
 *   Step k = 0..M-1 per set: the key of an unselected candidate is d_i if d_i > eps, else 0; p = the unselected candidate with the
 *   largest key, the lowest position on a tie (so step 0 of an empty start picks position 0); pick[k] = p (a POSITION in the
 *   candidate list), pivot[k] = d_p before its downdate.  If d_p > eps, for every candidate i:
 *   c_i = k(x_i, x_p) - sum_{j < k0 + k} LT[j, i] LT[j, p], LT[k0 + k, i] = c_i / sqrt(d_p), d_i = max(d_i - LT[k0 + k, i]^2, 0);
 *   otherwise the set is exhausted: row k0 + k is zeros and d stays.  p is marked selected (the mask lives in the workspace).
 * M + 1 launches on `stream` and no host synchronisation; no cooperative launch and no waiting between workgroups: each step's
 * workgroups leave their tile's best in a table that the next launch's workgroups reduce.  Deterministic (no atomics): two calls
 * on the same input are bitwise equal.  The workspace is linear in Nc (a mask, the table, exp(-2 theta)); 0 for G == 0.
 * VARGP_EINVAL before any launch: a null pointer other than cand, a size < 1, k0 < 0, M > Nc, cand == NULL with Nc > N, nu2 not
 * one of the four, G > 65535, a short workspace.  eps: the jitter the Cholesky of K(z, z) will add.
 */
size_t vargp_greedy_workspace_bytes(int G, int Nc, int D, int Mtot);
int vargp_greedy_select(const float* theta, const float* X, const int32_t* cand, float* LT, float* d, int32_t* pick, float* pivot,
                        int G, int Nc, int N, int D, int k0, int M, int nu2, float eps, void* ws, size_t ws_bytes,
                        vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted moments of the cross-kernel over a data set, for G outputs over one data matrix X [N, D] and ONE hyper vector theta
 * [D + 1] (log lengthscale_1..D, log gamma) -- what the closed-form optimal q(u) of a Gaussian likelihood needs of the data
 * (vargp_amd/collapsed.py).  Not in the reference.  With k_n = k_theta(Z_g, x_n), an Mt-vector of the kernel of gram (nu2 = 0: RBF;
 * 1, 3, 5: Matern nu = nu2 / 2; D <= 32: the direct distance form):
 *   Phi[g] = sum_n w[g, n] k_n k_n^T  (Mt x Mt, bitwise symmetric),   c[g] = sum_n w[g, n] y[g, n] k_n,
 *   sums[g] = (sum_n w[g, n], sum_n w[g, n] y[g, n]^2);   w == NULL: every weight is 1.
 * K(Z, X) is never stored: 64-column tiles of it live in LDS and feed an f32-MFMA rank update.  The points are cut into
 * vargp_gram_moments_chunks(G, Mt, N, D) chunks -- a function of the shapes alone, at most 1024 and no more than give the launch
 * about 1024 workgroups -- each accumulated in fp32; a second launch adds the chunks in ascending order in fp64 and rounds once.
 * No atomics: two calls on the same input are bitwise equal.  A zero weight contributes exactly nothing; nothing is read
 * behind row N of X.
 * Workspace: per-chunk partial sums only -- with nt = ceil(Mt / 64) and ntri = nt (nt + 1) / 2, chunks x G x (ntri 16384 + nt 256
 * + 8) bytes and padding, chunks x G x ntri <= 1024 + G ntri: at most (1024 + G ntri) x 16.6 KB, whatever N is.
 * Any G, Mt, N, D >= 1, G <= 65535.  VARGP_EINVAL before any launch: a null pointer other than w, a size < 1, nu2 not one of the
 * four, G > 65535, a short workspace.  The two queries return 0 for a size < 1.
 */
size_t vargp_gram_moments_workspace_bytes(int G, int Mt, int N, int D);
int vargp_gram_moments_chunks(int G, int Mt, int N, int D);
int vargp_gram_moments(const float* theta, const float* Z, const float* X, const float* w, const float* y, float* Phi, float* c,
                       float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* The backward of vargp_gram_moments for theta and Z (X, w and y get no gradient), in one fused pass over the data.  gPhi
 * [G, Mt, Mt] is ANY matrix (it is symmetrised inside: S = gPhi + gPhi^T), gc [G, Mt].  With gK = (S K + gc y^T) diag(w) and
 * V = gK o (-2 dk/dd2) (RBF: gK o K; Matern: matern_w; 0 at a zero distance for nu = 1/2), neither ever stored:
 *   r = V 1, cn = V^T 1, P = V X, wl_d = exp(-2 theta_d),
 *   gZ[g, i]  = -wl o (r_i z_i - P_i)                                                          [G, Mt, D]
 *   gtheta[d] = wl_d sum_g [sum_i z_id (r_i z_id - 2 P_id) + sum_n cn_n x_nd^2]                 d < D.
 * gtheta has D + 1 entries; entry D is LEFT TO THE CALLER: it needs no pass over the data,
 *   gtheta[D] = sum_g 4 <gPhi_g, Phi_g> + 2 <gc_g, c_g>   with the forward's outputs.
 * A workgroup owns (g, a 64-row panel of Z, a chunk of N, a group of at most 448 values of d); the contract of the forward holds:
 * masked columns behind a chunk's end, a zero weight adds exactly nothing, no atomics, the chunks' partials added in ascending
 * order in fp64 by a last launch and rounded once, two calls bitwise equal.  vargp_gram_moments_bwd_chunks(G, Mt, N, D): the
 * chunk count, a function of the shapes alone -- as the forward's (about 1024 workgroups, >= 256 columns, <= 1024 chunks) and
 * capped so that the partials of r and P, chunks x G x ceil(Mt / 64) x 64 (D + 1) floats, stay below 64 MiB (one chunk is always
 * allowed).  Workspace: those partials, chunks x G x ceil(Mt / 64) x D floats for the theta sums, G Mt^2 floats for S, and padding;
 * it does not grow with N.  VARGP_EINVAL before any launch as for the forward (every pointer but w is required).
 */
size_t vargp_gram_moments_bwd_workspace_bytes(int G, int Mt, int N, int D);
int vargp_gram_moments_bwd_chunks(int G, int Mt, int N, int D);
int vargp_gram_moments_bwd(const float* theta, const float* Z, const float* X, const float* w, const float* y, const float* gPhi,
                           const float* gc, float* gZ, float* gtheta, int G, int Mt, int N, int D, int nu2, void* ws,
                           size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gaussian sites of a non-Gaussian likelihood over a data set, for G independent outputs over one data matrix X [N, D] and ONE
 * hyper vector theta [D + 1] -- what one natural-gradient (conjugate-computation) iteration on q(u) needs of the data
 * (vargp_amd/sites.py).  Not in the reference.  q(u) enters through alpha [G, Mt] and a symmetric Q [G, Mt, Mt] (only its
 * symmetric part matters).  With k_n = k_theta(Z_g, x_n), the kernel of vargp_gram_moments (nu2, the two distance forms):
 *   mu_n = alpha[g] . k_n,   var_n = max(gamma^2 - k_n^T Q[g] k_n, 0)
 *   (ell, dmu, dvar) = E_{f ~ N(mu_n, var_n)} log p(y[g, n] | f) and its derivatives for (mu, var), as the vargp_<kind>_nll_bwd
 *   entries evaluate them (fp32 for Bernoulli, fp64 for the others; the 20-node Gauss-Hermite rule where there is no closed form)
 *   lam2[g, n] = w[g, n] max(-2 dvar, 0),   lam1 = w[g, n] dmu + lam2[g, n] mu_n
 *   c[g] = sum_n lam1 k_n   [G, Mt]
 *   sums[g] = (sum_n w ell, sum_n lam2, the number of points with w != 0 whose -2 dvar < 0 was clamped to 0, sum_n w)   [G, 4]
 * kind: VARGP_SITE_*.  y with row stride ldy (>= N), or ldy = 0: one row shared by every output; Bernoulli reads targets in
 * {0, 1} (no class-index form here).  log_scale [G], df, lognorm: Student-t only, as vargp_studentt_nll_fwd takes them (ignored,
 * and log_scale may be NULL, for the other kinds).  w == NULL: every weight is 1.  A point of weight 0 is not evaluated: it adds
 * exactly nothing to c and sums and gets lam2 = 0, whatever its row of X and its target hold.
 * K(Z, X) is never stored: all Mt rows of 64 columns of it live in LDS, so Mt <= 256 (VARGP_EINVAL above: the caller composes the
 * same quantities from the per-op entries).  Q K runs on the f32 MFMA.  The points are cut into vargp_site_moments_chunks(G, Mt,
 * N, D) chunks -- a function of the shapes alone: at most 1024, at least 256 columns each, about 1024 workgroups -- each
 * accumulated in fp32 (sums: fp64); a second launch adds the chunks in ascending order in fp64 and rounds once.  No atomics: two
 * calls on the same input are bitwise equal.  Nothing is read behind row N of X.
 * Workspace: per-chunk partials only, chunks x G x (ceil(Mt / 64) 256 + 32) bytes and padding, 8-byte aligned; it does not grow
 * with N beyond the chunk count.  VARGP_EINVAL before any launch: a null pointer other than w (and log_scale unless Student-t),
 * a size < 1, Mt > 256, G > 65535, an unknown kind or nu2, ldy in (0, N), df <= 0 for Student-t, a short or misaligned
 * workspace.  The two queries return 0 for a size < 1.
 */
#define VARGP_SITE_BERNOULLI_PROBIT 0
#define VARGP_SITE_BERNOULLI_LOGIT 1
#define VARGP_SITE_POISSON 2
#define VARGP_SITE_STUDENTT 3
size_t vargp_site_moments_workspace_bytes(int G, int Mt, int N, int D);
int vargp_site_moments_chunks(int G, int Mt, int N, int D);
int vargp_site_moments(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, const float* y,
                       int64_t ldy, const float* w, int kind, const float* log_scale, float df, float lognorm, float* lam2,
                       float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes,
                       vargp_stream_t stream);

/* The backward of the first sum of vargp_site_moments, value[g] = sum_n w ell = sums[g, 0], for theta, Z, alpha and Q (and the
 * Student-t log_scale) in one fused pass over the data: the M-step of variational EM on the site bound (vargp_amd/sites.py:
 * site_bound, fit_sites_).  X, y and w get no gradient.  Inputs as vargp_site_moments takes them, and gout [G], the upstream seed
 * s_g of every output.  With Qs the symmetric part of Q[g], q_n = k_n^T Qs k_n, mu_n and var_n as above (evaluated by the same
 * device functions as the forward: bitwise its values for a symmetric Q), (ell, dmu, dvar) the likelihood's value and TRUE signed
 * derivatives (not lam2: dvar is not clamped at 0) and u_n = 1 if gamma^2 - q_n > 0, else 0 (the variance clamp passes no gradient):
 *   gm_n = s_g w_n dmu_n,   gv_n = s_g w_n dvar_n u_n                                        gv [G, N] is WRITTEN
 *   galpha[g] = sum_n gm_n k_n                                                                [G, Mt]
 *   gQ[g]     = -sum_n gv_n k_n k_n^T  (symmetric) is NOT written: it is -Phi of vargp_gram_moments with w = gv
 *   gK[:, n]  = gm_n alpha[g] - 2 gv_n Qs k_n,   V = gK o (-2 dk/dd2)  (as vargp_gram_moments_bwd defines it per kernel; 0 at a zero
 *               distance for nu = 1/2); neither is ever stored
 *   r = V 1, cn = V^T 1, P = V X, wl_d = exp(-2 theta_d)
 *   gZ[g, i]  = -wl o (r_i z_i - P_i)                                                          [G, Mt, D]
 *   gtheta[d] = wl_d sum_g [sum_i z_id (r_i z_id - 2 P_id) + sum_n cn_n x_nd^2]                 d < D
 *   gtheta[D] = sum_g sum_n [2 gm_n mu_n + gv_n (2 gamma^2 - 4 q_n)]   (log gamma; COMPLETE here, nothing is left to the caller)
 *   gls[g]    = s_g sum_n w_n d ell_n / d log_scale[g]   [G], Student-t only (what vargp_studentt_nll_bwd's gparam holds, sign
 *               turned; gls may be NULL and is not written for the other kinds)
 * A point of weight 0 is not evaluated and its column of K is masked: it adds exactly nothing to any output and gets gv = 0,
 * whatever its row of X and its target hold (NaN included).
 * A workgroup owns (g, a chunk of N, a group of at most 128 values of d; D <= 32: one group) and walks 64 columns at a time: all
 * Mt rows of the 64 columns of K and of the weight -2 dk/dd2 live in LDS (Mt <= 256: 2 x 64 KB at the limit, VARGP_EINVAL above
 * it); Qs K runs on the f32 MFMA with the accumulators of all Mt rows in registers, V overwrites the weight in place, and P += V X
 * runs on the same MFMA.  Every group of d recomputes V.  The points are cut into vargp_site_bound_bwd_chunks(G, Mt, N, D) chunks --
 * a function of the shapes alone: the forward's rule (at most 1024, at least 256 columns each, about 1024 workgroups over G x
 * groups), capped so that the partials of r, galpha and P, chunks x G x ceil(Mt / 64) x 64 (D + 2) floats, stay below 64 MiB (one
 * chunk is always allowed) -- each accumulated in fp32 (the per-point scalars of gtheta[D] and gls: fp64); a last launch adds the
 * chunks in ascending order in fp64, forms gZ and gtheta there and rounds once.  No atomics: two calls on the same input are
 * bitwise equal.  Nothing is read behind row N of X.
 * Workspace: per-chunk partials only (the above, chunks x G x (D floats + 16 bytes), and padding), 8-byte aligned; it does not grow
 * with N beyond the chunk count.  VARGP_EINVAL before any launch: a null pointer other than w (and log_scale / gls unless
 * Student-t), a size < 1, Mt > 256, G > 65535, an unknown kind or nu2, ldy in (0, N), df <= 0 for Student-t, a short or misaligned
 * workspace.  The two queries return 0 for a size < 1.
 */
size_t vargp_site_bound_bwd_workspace_bytes(int G, int Mt, int N, int D);
int vargp_site_bound_bwd_chunks(int G, int Mt, int N, int D);
int vargp_site_bound_bwd(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, const float* y,
                         int64_t ldy, const float* w, int kind, const float* log_scale, float df, float lognorm, const float* gout,
                         float* gZ, float* gtheta, float* galpha, float* gv, float* gls, int G, int Mt, int N, int D, int nu2,
                         void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The three data passes of one natural-gradient iteration on q(u) of a SOFTMAX model (vargp_amd/sites.py: fit_q_softmax_).  Not
 * in the reference.  q factorises over the classes, so there is one Gaussian site per (class, point); the classes of a point are
 * coupled only in how the site parameters are computed.  Every entry checks its arguments on the host before any launch
 * (VARGP_EINVAL, vargp_last_error), works on the caller's stream and uses no atomics: partials are added in ascending chunk order
 * in fp64 and two calls on the same input are bitwise equal.
 *
 * vargp_site_marginals: mu[g, n] = alpha[g] . k_n, var[g, n] = max(gamma^2 - k_n^T Q[g] k_n, 0), both [G, N], with the operands,
 * the kernel, the chunking and the limit Mt <= 256 of vargp_site_moments -- it IS that entry's kernel, stopped after the
 * marginals: no likelihood, no c, no partials, no workspace and no second launch.  K(Z, X) is never stored.  VARGP_EINVAL: a
 * null pointer, a size < 1, Mt > 256, G > 65535, an unknown nu2.
 *
 * vargp_softmax_sites: mu, var [C, N] (fp32; var >= 0), y [N] int64 class indices, w [N] or NULL = 1, F draws per point.  With
 * f = mu + sqrt(var) eps and p = softmax(f) (per draw: logits shifted by their maximum, one exp per class):
 *   ell_n = mu[y_n, n] - mean_f logsumexp(f),   Ep_c = mean_f p_c,   Ev_c = mean_f p_c (1 - p_c)
 *   lam2[c, n] = w_n Ev_c  (>= 0: nothing is clamped),   lam1[c, n] = w_n ([y_n = c] - Ep_c) + lam2[c, n] mu[c, n]     [C, N]
 *   sums = (sum_n w_n ell_n, sum_cn lam2, the number of points with w != 0, sum_n w_n)                              [4]
 * eps [F, C, N], or NULL: the draws are generated inside the kernel from `seed` -- Philox4x32-10 + Box-Muller as the ELBO
 * programs', noise stream 2, step 0; the draws of (point n, sample f) are the groups (n F + f) ceil(C / 4) + j, element l of group
 * j belonging to class 4 j + l -- and the [F, C, N] tensor need not exist.  vargp_softmax_site_noise writes exactly those draws
 * to eps [F, C, N]; the two ways are bitwise equal.  A point of weight 0 is never evaluated: lam1 = lam2 = 0 and it adds exactly
 * nothing, whatever its mu, var and y hold.  A label outside [0, C) makes sums[0] NaN.  2 <= C <= 128: lanes run over points, the
 * class accumulators live in registers up to C = 16 and in LDS above (VARGP_EINVAL beyond 128).  The points are cut into at most
 * 1024 chunks by N alone.  Workspace: 32 bytes per chunk and padding, 8-byte aligned.  VARGP_EINVAL: a null pointer other than
 * w and eps, N or F < 1, F > 65535, C outside [2, 128], a short or misaligned workspace.
 *
 * vargp_gram_moments_v: vargp_gram_moments with a weight vector of its own for c: Phi[g] = sum_n w[g, n] k_n k_n^T as there, but
 * c[g] = sum_n v[g, n] k_n and sums[g] = (sum_n w, sum_n v).  The same kernel, chunking and workspace
 * (vargp_gram_moments_workspace_bytes); with v = w o y (rounded to fp32) Phi and c are bitwise vargp_gram_moments'.  The softmax
 * sites need it because lam1 / lam2 is not representable: lam2 underflows to 0 exactly at the confidently misclassified points,
 * where lam1 ~ 1 matters most.  VARGP_EINVAL as vargp_gram_moments.
 */
int vargp_site_marginals(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, float* mu,
                         float* var, int G, int Mt, int N, int D, int nu2, vargp_stream_t stream);
size_t vargp_softmax_sites_workspace_bytes(int C, int N);
int vargp_softmax_sites(const float* mu, const float* var, const int64_t* y, const float* w, const float* eps, uint64_t seed,
                        float* lam1, float* lam2, float* sums, int C, int N, int F, void* ws, size_t ws_bytes,
                        vargp_stream_t stream);
int vargp_softmax_site_noise(uint64_t seed, float* eps, int F, int C, int N, vargp_stream_t stream);
int vargp_gram_moments_v(const float* theta, const float* Z, const float* X, const float* w, const float* v, float* Phi, float* c,
                         float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The leave-one-out cavity of the Gaussian sites (vargp_amd/loo.py: VARGP.loo).  Not in the reference.  vargp_site_moments'
 * kernel with one more operand, V [G, Mv, Mt] (1 <= Mv <= Mt; for a whitened posterior V = H_t^T T[t, :], so that
 *   s[g, n] = |V[g] k_n|^2
 * is the variance that the new block of q(v) gives the site's direction T k_n).  Per 64 columns of K resident in LDS: alpha . k_n
 * and k_n^T Q k_n as there; then, in the registers the accumulators of Q K had, V K on the f32 MFMA, a 64-row panel of V at a
 * time, reduced to its column norms.  K(Z, X) and V K are never stored.
 * kind < 0, the marginals form: writes mu, var, s [G, N] and nothing else; y, w, the Student-t arguments, the other outputs and
 * the workspace are ignored and may be NULL.  One launch.
 * kind = VARGP_SITE_*, the site form: the likelihood's (dmu, dvar) at (mu_n, var_n) in the same launch, with the operands and the
 * conventions of vargp_site_moments, and with r = 1 - lam2 s, in fp64 from the fp32 moments and rounded once:
 *   lam2 = w max(-2 dvar, 0),   lam1 = w dmu + lam2 mu
 *   mu_c = (mu - s lam1) / r  (evaluated as mu - s w dmu / r),   var_c = var + lam2 s^2 / r
 * all [G, N], beside mu, var and s.  A point with r <= 0 or a non-finite mu_c or var_c is UNSTABLE: mu_c = var_c = NaN, and
 * n_unstable[g] (int64 [G]) counts them -- per-chunk partials in the workspace, added in ascending chunk order by a second launch.
 * A point of weight 0 is not evaluated: lam1 = lam2 = 0 and (mu_c, var_c) are written as exactly (mu, var).
 * The chunking is vargp_site_moments' (vargp_site_cavity_chunks); no atomics: two calls on the same input are bitwise equal.
 * Workspace (site form): chunks x G x 8 bytes and padding, 8-byte aligned.  VARGP_EINVAL before any launch as
 * vargp_site_moments, and for Mv < 1 or Mv > Mt.
 */
size_t vargp_site_cavity_workspace_bytes(int G, int Mt, int N, int D);
int vargp_site_cavity_chunks(int G, int Mt, int N, int D);
int vargp_site_cavity(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, const float* V,
                      const float* y, int64_t ldy, const float* w, int kind, const float* log_scale, float df, float lognorm,
                      float* mu, float* var, float* s, float* mu_c, float* var_c, float* lam1, float* lam2, long long* n_unstable,
                      int G, int Mt, int Mv, int N, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The backward of the softmax site bound (vargp_amd/sites.py: softmax_site_bound, fit_softmax_sites_; ops.softmax_site_bound_diff).
 * Not in the reference.  The value is vargp_softmax_sites' sums[0] at the marginals of vargp_site_marginals; its gradient is these
 * two entries and one vargp_gram_moments call.  Both check their arguments on the host before any launch (VARGP_EINVAL,
 * vargp_last_error), work on the caller's stream and use no atomics: two calls on the same input are bitwise equal.
 *
 * vargp_softmax_site_grads: the EXACT derivatives of the F-sample estimate sum_n w_n [mu[y_n, n] - mean_f logsumexp(f)] for the
 * marginals, seeded by s = gout[0] (a DEVICE pointer: the caller needs no host sync), with f, p, eps as vargp_softmax_sites has them:
 *   gmu[c, n]  = s w_n ([y_n = c] - mean_f p_c)                                                                       [C, N]
 *   gvar[c, n] = -s w_n / (2 sqrt(var[c, n])) mean_f (p_c eps_c)   where var[c, n] > 0, else exactly 0                [C, N]
 * the pathwise derivative for var, NOT the Price estimate -1/2 E p (1 - p) behind lam2: only this one is the derivative of the
 * sampled value (its slope is unbounded as var -> 0+; at var = 0 the convention is 0).  Layout, limits (2 <= C <= 128, F <= 65535),
 * the noise stream, the draw indexing and the chunking are vargp_softmax_sites'; every p comes from the same device functions;
 * eps NULL and the tensor vargp_softmax_site_noise writes give bitwise equal results.  Two accumulators per class (sum p_c, sum
 * p_c eps_c), in registers up to C = 16 and in LDS above (with the draw's logits and noise: 4 C x 64 floats).  Nothing is reduced
 * over the points: no workspace and no second launch.  A point of weight 0 is never evaluated and writes exact zeros, whatever
 * its mu, var and y hold.  VARGP_EINVAL: a null pointer other than w and eps, N or F < 1, F > 65535, C outside [2, 128].
 *
 * vargp_site_transport_bwd: vargp_site_bound_bwd with GIVEN per-point seeds gm, gv [G, N] (d value / d mu_n, d value / d var_n,
 * weights and upstream seed included) in place of a likelihood: no targets, no weights, no parameter, no gls.  With u_n =
 * [gamma^2 - q_n > 0] recomputed here, gv_out = gv o u [G, N] (gQ[g] = -Phi of vargp_gram_moments with w = gv_out), and gZ, gtheta
 * (complete, D + 1 entries) and galpha are that entry's formulas with gm_n = gm[g, n], gv_n = gv_out[g, n].  It IS that entry's
 * kernel with a policy that loads the two derivatives of a point from memory, and everything else is inherited: Mt <= 256 with the
 * K block and the weight block in LDS; Qs K and V X on the f32 MFMA; groups of at most 128 values of d; the chunk rule
 * (vargp_site_transport_bwd_chunks is vargp_site_bound_bwd_chunks) and a workspace of per-chunk partials that does not grow with N
 * beyond the chunk count; fp32 within a chunk, fp64 across chunks in ascending order by the reduce launch; no atomics, bitwise
 * reproducible; nothing is read behind row N of X.  A point whose gm and gv are both 0 is masked like a point of weight 0: it
 * adds exactly nothing, whatever its row of X holds (NaN included).  VARGP_EINVAL: a null pointer, a size < 1, Mt > 256,
 * G > 65535, an unknown nu2, a short or misaligned workspace.  The two queries return 0 for a size < 1.
 */
int vargp_softmax_site_grads(const float* mu, const float* var, const int64_t* y, const float* w, const float* eps, uint64_t seed,
                             const float* gout, float* gmu, float* gvar, int C, int N, int F, vargp_stream_t stream);
size_t vargp_site_transport_bwd_workspace_bytes(int G, int Mt, int N, int D);
int vargp_site_transport_bwd_chunks(int G, int Mt, int N, int D);
int vargp_site_transport_bwd(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, const float* gm,
                             const float* gv, float* gZ, float* gtheta, float* galpha, float* gv_out, int G, int Mt, int N, int D,
                             int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * KL(N(mu_q, Lq Lq^T) || N(mu_p, Lp Lp^T)) from its triangular ingredients (reference:
 * torch.distributions kl_divergence(MVN, MVN) as called from var_gp/vargp.py:182-190):
 *   kl = logdet_p - logdet_q + 0.5 * (|G|_F^2 + |d|^2 - M),  G = Lp^-1 Lq [nb, M, M],
 *   d = Lp^-1 (mu_q - mu_p) [nb, M];  logdet_* = sum log diag.
 * Forward reduces G and d; backward is gG = gkl * G, gd = gkl * d.
 */
int vargp_mvn_kl_fwd(const float* G, const float* d, const float* logdet_p, const float* logdet_q, float* kl,
                     int nbatch, int M, vargp_stream_t stream);
int vargp_mvn_kl_bwd(const float* G, const float* d, const float* gkl, float* gG, float* gd, int nbatch, int M,
                     vargp_stream_t stream);
/* logdet[b] = sum_i log L[b,i,i]; backward gL[b,i,i] = g[b] / L[b,i,i] (zeros elsewhere) */
int vargp_logdet_tril_fwd(const float* L, float* logdet, int nbatch, int n, vargp_stream_t stream);
int vargp_logdet_tril_bwd(const float* L, const float* g, float* gL, int nbatch, int n, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Monte-Carlo softmax likelihood (reference: MulticlassSoftmax, var_gp/likelihoods.py:13-63).
 *   mu, var [S, C, B]; eps [S, F, C, B]; y int64 [B].
 *   nll   = sum_b mean_{s,f} -log_softmax_c(mu + sqrt(var) eps)[y_b]           (likelihoods.py:33-47)
 *   probs[B, C] = mean_{s,f} softmax_c(...)                                       (likelihoods.py:49-63)
 * nll is accumulated with atomics into *nll, which the call zeroes first.
 */
int vargp_softmax_nll_fwd(const float* mu, const float* var, const float* eps, const int64_t* y, float* nll,
                          int S, int F, int C, int B, vargp_stream_t stream);
int vargp_softmax_nll_bwd(const float* mu, const float* var, const float* eps, const int64_t* y,
                          const float* gnll, float* gmu, float* gvar, int S, int F, int C, int B,
                          vargp_stream_t stream);
int vargp_softmax_predict(const float* mu, const float* var, const float* eps, float* probs, int S, int F,
                          int C, int B, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Independent multi-output Gaussian likelihood (reference: GaussianLikelihood, var_gp/likelihoods.py:66-110), closed form.
 *   mu, var [S, C, B]; obs_log_var [C]; y [C, B] with class stride ldy = B, or one target row [B] shared by every output
 *   (ldy = 0: the reference's y.unsqueeze(0).unsqueeze(-1) broadcast).  With v = var + exp(obs_log_var[c]), r = y - mu:
 *   nll = sum_b mean_{s,c} [ 1/2 log(2 pi v) + 1/2 r^2 / v ]                         (likelihoods.py:92-107)
 * fwd WRITES *nll (no accumulation).  bwd, seed = d total / d nll (device, 1 float), n = S C:
 *   gmu = -seed r / (v n),  gvar = seed (1/v - r^2/v^2) / (2 n)   [S, C, B]
 *   g_obs_log_var[c] = exp(obs_log_var[c]) sum_{s,b} gvar[s, c, b]                   [C]
 * and, with nll != NULL, also writes the (unseeded) value, so a training step needs one launch.  Deterministic: no float
 * atomics, every sum in a fixed order (same inputs -> bitwise identical outputs).
 */
int vargp_gauss_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var, float* nll,
                        int S, int C, int B, vargp_stream_t stream);
int vargp_gauss_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var,
                        const float* seed, float* gmu, float* gvar, float* g_obs_log_var, float* nll, int S, int C, int B,
                        vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Independent-output Bernoulli likelihood: binary, multi-label and one-vs-rest classification.  Not in the reference.
 *   p(t | f) = Lambda(s f), s = 2 t - 1; link 0: Lambda = Phi (probit), link 1: Lambda = logistic (logit).
 *   mu, var [S, C, B].  Exactly one of `t` and `labels` is non-NULL:
 *     t       float targets in {0, 1}, [C, B] with row stride ldt, or one row [B] shared by every output (ldt = 0);
 *     labels  int64 [B] class indices read as one-vs-rest, t[c, b] = (labels[b] == c); a label outside [0, C) matches no output
 *             (every output of that point is a negative) -- label values are not checked.
 *   With the 20-node Gauss-Hermite rule (x_k, w_k = numpy.polynomial.hermite.hermgauss(20), w^_k = w_k / sqrt(pi)), which is the
 *   definition of the expected log-likelihood and not an approximation left open:
 *     ell[s,c,b] = sum_k w^_k log Lambda(s_cb (mu + sqrt(2 var) x_k)),     nll = - sum_b sum_c mean_s ell   (SUM over outputs)
 * fwd WRITES *nll.  bwd, seed = d total / d nll (device, 1 float): gmu, gvar [S, C, B] = seed * the exact derivatives of that
 * sum; with nll != NULL it also writes the (unseeded) value, bit-equal to fwd's, so a training step needs one call.
 * predict: probs[B, C] = mean_s P(t = 1) -- probit: Phi(mu / sqrt(1 + var)); logit: the same rule on the logistic function.  The
 * rows are NOT normalised over the outputs.
 * ws: vargp_bernoulli_workspace_bytes(S, C, B) bytes of device scratch, used inside the call only (per-workgroup partial
 * values; may be NULL in bwd when nll is NULL).  Deterministic: no float atomics, every sum in a fixed order.
 */
size_t vargp_bernoulli_workspace_bytes(int S, int C, int B);
int vargp_bernoulli_nll_fwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels, int link,
                            float* nll, int S, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_bernoulli_nll_bwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels, int link,
                            const float* seed, float* gmu, float* gvar, float* nll, int S, int C, int B, float* ws,
                            size_t ws_bytes, vargp_stream_t stream);
int vargp_bernoulli_predict(const float* mu, const float* var, int link, float* probs, int S, int C, int B,
                            vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Poisson likelihood with a log link (counts), independent outputs, closed form.  Not in the reference.
 *   mu, var [S, C, B]; y non-negative floats (not checked), [C, B] with row stride ldy, or one row [B] shared by every output
 *   (ldy = 0).  With m = mu + var / 2:
 *     ell[s,c,b] = y mu - exp(m) - lgamma(y + 1),     nll = - sum_b sum_c mean_s ell   (SUM over outputs, as the Bernoulli
 *     likelihood: the ELBO of C independent outputs -- C times the Gaussian likelihood's mean-over-outputs convention)
 * fwd WRITES *nll.  bwd, seed = d total / d nll (device, 1 float):
 *     gmu = -seed (y - exp(m)) / S,   gvar = seed exp(m) / (2 S)     [S, C, B]
 * and, with nll != NULL, also writes the (unseeded) value, bit-equal to fwd's, so a training step needs one call.
 * exp(m) overflows fp32 above m ~ 88.7; value and gradients are then inf, as the formula says (nothing is clamped).
 * predict: rate[S, C, B] = E exp(f) = exp(m).
 * ws: vargp_poisson_workspace_bytes(S, C, B) bytes of 8-byte aligned device scratch, used inside the call only (per-workgroup
 * partial values, kept as doubles; may be NULL in bwd when nll is NULL).  Deterministic: no float atomics, every sum in a fixed
 * order.  Inputs and outputs are fp32; the element arithmetic and the sums run in fp64, so every output is rounded once.
 */
size_t vargp_poisson_workspace_bytes(int S, int C, int B);
int vargp_poisson_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, float* nll, int S, int C, int B,
                          float* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_poisson_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* seed, float* gmu,
                          float* gvar, float* nll, int S, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_poisson_predict(const float* mu, const float* var, float* rate, int S, int C, int B, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Student-t likelihood (robust regression), independent outputs.  Not in the reference.
 *   Fixed degrees of freedom df = nu > 0 (host float), learned log_scale [C], sigma_c = exp(log_scale[c]).  mu, var, y, ldy as
 *   above.  lognorm = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi) / 2, computed by the CALLER in double (the two lgamma cancel
 *   in fp32 at large nu) and passed as one float.  With the 20-node Gauss-Hermite rule of the Bernoulli section (x_k, w^_k),
 *   which is the definition of the expected log-likelihood and not an approximation left open, and
 *   r_k = y - (mu + sqrt(2 var) x_k):
 *     ell[s,c,b] = K_c - (nu + 1) / 2 sum_k w^_k log1p(r_k^2 / (nu sigma_c^2)),     K_c = lognorm - log_scale[c]
 *     nll = - sum_b sum_c mean_s ell   (SUM over outputs: C times the Gaussian likelihood's convention)
 * fwd WRITES *nll.  bwd, seed = d total / d nll (device, 1 float): gmu, gvar [S, C, B] and g_log_scale [C] = seed * the exact
 * derivatives of that sum (g_log_scale[c] = -seed / S sum_{s,b} d ell / d log_scale[c], in a fixed order); at var = 0 the
 * rule's variance gradient is exactly 0.  With nll != NULL bwd also writes the (unseeded) value, bit-equal to fwd's.
 * The predictive location is mu itself: there is no predict entry.
 * ws: vargp_studentt_workspace_bytes(S, C, B) bytes of 8-byte aligned device scratch, used inside the call only (per-workgroup
 * partial values and log_scale gradients, kept as doubles; always needed).  Deterministic: no float atomics, every sum in a fixed
 * order.  Inputs and outputs are fp32; the element arithmetic and the sums run in fp64, so every output is rounded once.
 */
size_t vargp_studentt_workspace_bytes(int S, int C, int B);
int vargp_studentt_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale, float df,
                           float lognorm, float* nll, int S, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_studentt_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale, float df,
                           float lognorm, const float* seed, float* gmu, float* gvar, float* g_log_scale, float* nll, int S,
                           int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Held-out log predictive density (LPD) of every likelihood above: log E_q[p(y | f)], the mixture over the hyper-samples of the
 * marginal likelihood of the targets (vargp_amd/csrc/lpd.hip).  Not in the reference.  (The nll entries give E_q[log p].)
 *   mu, var [S, C, B]: the predictive moments of f under hyper-sample s.  Targets and ldy / ldt / labels: exactly the conventions
 *   of the matching *_nll_fwd entry.  With the 20-node Gauss-Hermite rule of the Bernoulli section (x_k, w^_k), which here too is
 *   the definition and not an approximation left open, and f_k = mu + sqrt(2 var) x_k, the log marginal likelihood per (s, c, b):
 *     gauss             lp = log N(y; mu, var + exp(obs_log_var[c]))                                          (closed form)
 *     poisson           lp = logsumexp_k( log w^_k + y f_k - exp(f_k) - lgamma(y + 1) )
 *     studentt          lp = logsumexp_k( log w^_k + K_c - (nu + 1) / 2 log1p((y - f_k)^2 / (nu sigma_c^2)) ),  K_c, lognorm, df
 *                       as in the Student-t section
 *     bernoulli probit  lp = log Phi(s_cb mu / sqrt(1 + var)), s = 2 t - 1, evaluated as log(erfc(-z / sqrt2) / 2) in fp64: finite
 *                       for z >= -37; below, erfc underflows and lp = -inf (log 0), which drops out of the mixture without a NaN
 *     bernoulli logit   lp = logsumexp_k( log w^_k + log sigma(s_cb f_k) )
 *   The hyper-sample is shared by all outputs of a point, so the density of its whole target vector is the mixture of products:
 *     lpd[b]       = logsumexp_s( sum_c lp[s,c,b] ) - log S         [B]      (required)
 *     lpd_out[c,b] = logsumexp_s( lp[s,c,b] )       - log S         [C, B]   (per-output marginals; may be NULL)
 *   softmax, eps [S, F, C, B], y int64 [B] (labels unchecked, as vargp_softmax_nll_fwd; a label outside [0, C) gives a
 *   meaningless value for that point and reads nothing out of bounds):
 *     lpd[b] = logsumexp_{s,f}( log_softmax_c(mu + sqrt(var) eps)[y_b] ) - log(S F);  no per-output marginals.
 * Every logsumexp subtracts its running maximum; a term of -inf produces no NaN, and a point whose every term is -inf gets -inf.
 * No workspace.  Deterministic: no float atomics, every sum in a fixed order (same inputs -> bitwise identical outputs).  Inputs
 * and outputs are fp32; the element arithmetic and every sum run in fp64, so each output is rounded once.  No gradients.
 * Argument errors (NULL required pointer, non-positive size, bad link, both or neither of t and labels, ldy / ldt neither 0 nor
 * >= B, df <= 0) return VARGP_EINVAL before any launch.
 */
int vargp_softmax_lpd(const float* mu, const float* var, const float* eps, const int64_t* y, float* lpd, int S, int F, int C,
                      int B, vargp_stream_t stream);
int vargp_gauss_lpd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var, float* lpd,
                    float* lpd_out, int S, int C, int B, vargp_stream_t stream);
int vargp_bernoulli_lpd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels, int link,
                        float* lpd, float* lpd_out, int S, int C, int B, vargp_stream_t stream);
int vargp_poisson_lpd(const float* mu, const float* var, const float* y, int64_t ldy, float* lpd, float* lpd_out, int S, int C,
                      int B, vargp_stream_t stream);
int vargp_studentt_lpd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale, float df,
                       float lognorm, float* lpd, float* lpd_out, int S, int C, int B, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Predictive entropy of the classification likelihoods, split into noise and lack of knowledge (vargp_amd/csrc/uncertainty.hip).
 * The reference has no counterpart.  mu, var [S, C, B]: the predictive moments of f under hyper-sample s.  All values in nats.
 *     total    = H[ E p(y | theta, f) ]     the entropy of the predictive distribution
 *     expected = E H[ p(y | theta, f) ]     the mean entropy of the samples' own distributions: noise (aleatoric)
 *     mi       = max(total - expected, 0)   the mutual information of the label and (theta, f): lack of knowledge (epistemic)
 *   total >= expected holds exactly (Jensen: both sides use the same samples / the same rule); the clamp removes rounding only.
 *   softmax, eps [S, F, C, B]; the S F samples are p_sf = softmax_c(mu_s + sqrt(var_s) eps_sf):
 *     probs[b,c]  = mean_sf p_sf[c,b]                            [B, C]  (the definition of vargp_softmax_predict; may be NULL)
 *     total[b]    = - sum_c probs[b,c] log probs[b,c]            [B]     (0 log 0 = 0;  0 <= total <= log C)
 *     expected[b] = mean_sf ( - sum_c p_sf[c,b] log p_sf[c,b] )  [B]     evaluated as Z - sum_c p_c f_c with Z the max-shifted
 *                                                                        logsumexp_c f_c: log(0) is never evaluated
 *     mi[b]                                                      [B]
 *   Any C.  Nothing of size S F C B is written: ws holds S F B + B doubles, vargp_softmax_uncertainty_workspace_bytes(S, F, C, B)
 *   bytes of 8-byte aligned device scratch used inside the call only.
 *   bernoulli, link as in the Bernoulli section; the outputs are independent, so everything is per output (c, b).  With the
 *   20-node Gauss-Hermite rule of that section (x_k, w^_k), which here too is the definition -- for the probit link as well, where
 *   vargp_bernoulli_predict uses the closed form: probs differs from it by the rule's quadrature error -- f_k = mu + sqrt(2 var) x_k
 *   and h(p) = - p log p - (1 - p) log(1 - p):
 *     p_out[c,b]        = mean_s sum_k w^_k Lambda(f_k)          written to probs [B, C] (may be NULL)
 *     total_out[c,b]    = h(p_out)                               [C, B]  (may be NULL)   the 1 - p_out in h is accumulated as
 *                                                                        mean_s sum_k w^_k Lambda(-f_k), with its own digits
 *     expected_out[c,b] = mean_s sum_k w^_k h(Lambda(f_k))       [C, B]  (may be NULL)   from log Lambda(f_k) and log Lambda(-f_k)
 *                                                                        in fp64: finite and correct at |f| = 30 and beyond
 *     mi_out[c,b]       = max(total_out - expected_out, 0)       [C, B]  (may be NULL)
 *     total, expected, mi [B] = the sums over c of the three (required): the one-vs-rest score, an upper bound on the entropy
 *     of the joint label vector.  No workspace.
 * Deterministic: no float atomics, every sum in a fixed order (same inputs -> bitwise identical outputs).  Inputs and outputs are
 * fp32; the element arithmetic, every sum and the subtraction in mi run in fp64, so each output is rounded once.  No gradients.
 * Argument errors (NULL required pointer, non-positive size, bad link, workspace missing, misaligned or too small) return
 * VARGP_EINVAL before any launch.
 */
size_t vargp_softmax_uncertainty_workspace_bytes(int S, int F, int C, int B);
int vargp_softmax_uncertainty(const float* mu, const float* var, const float* eps, float* probs, float* total, float* expected,
                              float* mi, int S, int F, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream);
int vargp_bernoulli_uncertainty(const float* mu, const float* var, int link, float* probs, float* total, float* expected,
                                float* mi, float* total_out, float* expected_out, float* mi_out, int S, int C, int B,
                                vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Yogi optimiser step, fused over one flat parameter buffer (reference call site:
 * experiments/vargp.py:23,37 -> torch_optimizer.Yogi; algorithm from Zaheer et al. 2018).
 * bias1/bias2 = 1 - beta^t; if `step` (device pointer to the step count t as a float) is not NULL
 * the corrections are computed on the device from it instead, which keeps a captured graph valid.
 */
int vargp_yogi_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float bias1, float bias2, const float* step, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The first-task ELBO as one native program (vargp_amd/csrc/elbo_t0.hip).
 * Replaces, for a model without previous tasks, the whole of VARGP.loss (var_gp/vargp.py:156-194:
 * RBFKernel.sample_hypers / kl_hypers kernels.py:62-77, RBFKernel.compute kernels.py:24-56, cholesky and
 * linear_marginal_diag gp_utils.py:5-11,150-191, the MVN KL vargp.py:182-190, MulticlassSoftmax.loss
 * likelihoods.py:13-45) and its autograd backward (loss.backward(), experiments/vargp.py:35).
 *
 * Shapes: log_mean, log_logvar, prior_* (D+1); eps_theta (S, D+1); z (C, M, D); u_mean (C, M); u_tril_vec
 * (C, M(M+1)/2); x (B, D); y (B) int64; eps_f (S, F, C, B).  map_est != 0: theta = log_mean, S must be 1, kl_hypers = 0
 * (log_logvar / prior_* / eps_theta may be NULL).  eps_theta = eps_f = NULL: native noise, see rng_* below.
 * fwd writes scalars[0..2] = (kl_hypers, kl_u, nll) and info[0 .. S*C + C) (Cholesky status of K_uu[s,c] + eps I, then of
 * S_u[c] + eps I; 0 = ok, k = leading minor k not positive, results NaN-filled).
 * bwd needs the workspace exactly as fwd left it; seeds (device, 3 floats) = d total / d (kl_hypers, kl_u, nll).  It
 * OVERWRITES the five gradient buffers (shapes of the parameters).  Neither call allocates or synchronises.
 */
typedef struct vargp_elbo_t0_desc {
  int32_t S, C, M, D, B, F;
  int32_t map_est;
  float jitter;
  const float *log_mean, *log_logvar, *prior_log_mean, *prior_log_logvar;
  const float *z, *u_mean, *u_tril_vec;
  const float* x;
  const int64_t* y;
  const float *eps_theta, *eps_f;
  float* scalars;
  int32_t* info;
  void* ws;
  size_t ws_bytes;
  float* bump; /* optional: fwd adds 1.0f to *bump (a caller's device-side step counter rides along for free) */
  /* Native noise: with eps_f == NULL (and eps_theta == NULL) fwd draws both noise tensors itself from a counter-based
   * generator (Philox4x32-10 + Box-Muller) keyed by rng_seed; *rng_counter (device) is the step number, read by fwd's
   * first kernel and incremented by a later one.  Element (s, ...) is a function of the GLOBAL sample index
   * rng_sample_offset + s, so sample-parallel ranks (offset = rank * S, same seed and counter) see slices of one global
   * draw.  The drawn tensors stay in the workspace (bwd reads them there). */
  uint64_t rng_seed;
  uint32_t* rng_counter;
  int32_t rng_sample_offset;
  /* 1: bwd leaves the gradients of log_mean / log_logvar to vargp_yogi_step_multi_hyper (see vargp_hyper_grad_desc): it does
   * not touch g_log_mean / g_log_logvar (they may be NULL) and launches one kernel less */
  int32_t defer_hyper;
  /* 1 (only when a vargp_elbo_t0_bwd on this workspace follows before scalars[2] is read): for the shapes of the LDS-resident
   * backward with C <= 16 and F <= 16 the forward does NOT launch the Monte-Carlo softmax likelihood; the backward's tile kernel
   * evaluates it (value and gradient) and adds nll into scalars[2], which is therefore valid only after bwd.  Ignored (the
   * forward evaluates the likelihood as usual) for every other shape, and for a caller-supplied eps_f that does not sit on a
   * 16-byte boundary (the tile kernel reads it as float4). */
  int32_t defer_softmax;
  /* 1: the Monte-Carlo likelihood is the CALLER's -- a rank of a class-sharded step holds only some of the classes the
   * softmax couples (likelihoods.py:26-29).  fwd stops at the predictive moments and the KL (scalars[2] stays 0); y and eps_f
   * are not read (may be NULL), eps_theta must be given unless map_est.  Between fwd and bwd the caller stores
   * d total / d mu and d total / d var -- ALREADY multiplied by their seed -- into the workspace's gmu, gvar (S, C, B)
   * (vargp_elbo_t0_lik_buffers); bwd takes them as they are and ignores seeds[2].  defer_softmax is ignored. */
  int32_t ext_lik;
  /* Optional early hand-over of the Cholesky status (both NULL: none).  Right behind the launch that writes info -- the second of
   * the forward's four -- fwd enqueues a copy of info[0 .. S*C + C) to info_host (host memory, pinned for the copy to be
   * asynchronous) and records info_event (a hipEvent_t of the caller's) on the stream.  A caller that has to raise on a failed
   * factorisation before it returns (the reference raises inside torch.cholesky, gp_utils.py:5-11) waits for that event instead
   * of the whole forward: the rest of the forward runs while the host carries on.  fwd itself still does not synchronise. */
  int32_t* info_host;
  void* info_event;
} vargp_elbo_t0_desc;
/* Streams: the work is issued to `stream` in order.  With many hyper-samples (S C + C per-matrix chains > a third of the CUs) fwd and
 * bwd fork a library-owned side stream for the pivot / adjoint chains and join it before they return (events; graph dependencies
 * under hipGraph capture): to the caller the call is still one unit of work on `stream`.  VARGP_T0_SIDE=0 disables it. */
size_t vargp_elbo_t0_workspace_bytes(int S, int C, int M, int D, int B, int F);
int vargp_elbo_t0_fwd(const vargp_elbo_t0_desc* d, vargp_stream_t stream);
/* Where the program keeps the predictive moments mu, var (S, C, B) of its last fwd and the likelihood gradients gmu, gvar
 * (S, C, B) its bwd reads (pointers into d->ws; any of the four outputs may be NULL). */
int vargp_elbo_t0_lik_buffers(const vargp_elbo_t0_desc* d, float** mu, float** var, float** gmu, float** gvar);
/* Which launch sequence fwd and bwd take for this descriptor on a device of `cus` compute units (cus <= 0: the current
 * device's): every member of the program's plan (T0Plan, csrc/elbo_t0.hip), evaluated by the same code the two calls use, as
 * text in out -- one `name=value` line per member, a flag as true / false, a count as a decimal integer, NUL-terminated
 * (VARGP_EINVAL if out_bytes is too small; 1024 is plenty).  Read-only host arithmetic: with cus > 0 the device is not
 * touched, so it runs on a machine without one.  It reads the dimensions, map_est / defer_softmax / ext_lik, whether eps_f is
 * NULL (native noise) and the ALIGNMENT of z, x, eps_f and ws as given -- the pointers need not be valid (ws may be NULL) -- and
 * the VARGP_T0_* tuning switches as fwd and bwd see them (read once per process). */
int vargp_elbo_t0_plan(const vargp_elbo_t0_desc* d, int cus, char* out, size_t out_bytes);
/* ONE vargp_elbo_t0_bwd per vargp_elbo_t0_fwd: for the shapes of the LDS-resident backward (M <= 104, M % 4 == 0, B % 4 == 0,
 * D % 4 == 0, S <= 64) the forward clears the accumulators the backward adds into (and the tile counters of the backward's
 * persistent product workgroups) -- there is no clearing launch in bwd.
 * Enforced by the library (host-side state per workspace, checked when the call is issued): a second bwd on one fwd, or a bwd
 * whose z / x alignment differs from its forward's, returns VARGP_EINVAL with a message instead of accumulating into stale sums. */
int vargp_elbo_t0_bwd(const vargp_elbo_t0_desc* d, const float* seeds, float* g_log_mean, float* g_log_logvar, float* g_z,
                      float* g_u_mean, float* g_u_tril_vec, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The ELBO of a model WITH previous tasks as one native program (vargp_amd/csrc/elbo_tn.hip); nblk = 1 is a first-task
 * model of any M.  Replaces VARGP.compute_q / compute_pf_diag / forward / loss for ep_var_mean = True
 * (var_gp/vargp.py:35-194: the linear_joint chain gp_utils.py:101-147 over the earlier tasks, linear_marginal_diag
 * gp_utils.py:150-191, the conditional prior gp_cond gp_utils.py:68-98 + MVN KL vargp.py:146-190, RBFKernel kernels.py:24-77,
 * MulticlassSoftmax.loss likelihoods.py:13-45) and its autograd backward.  The chain is evaluated in its block form: ONE
 * kernel matrix over all Mt = nblk * M inducing points, ONE factorisation L = chol(K + eps I) with T = L^-1 (every
 * factor of the chain is a leading block of L), block-diagonal small products with T_ii, three Mt x Mt x B GEMMs
 * (tests/block_algorithm.py pins the identities against the chain in fp64).
 *
 * Caller-maintained packed operands (the program writes only the CURRENT task's part, on every fwd):
 *   z_all  (C, Mt, D):        rows [i*M, (i+1)*M) of class c = inducing points of task i; the last M rows are scratch
 *   rk_all (C, nblk, M, NR):  NR = 4 + M rounded up to 4;  row j of block i = [ u_mean_i[j] | 0 0 0 | Lu_i[j, :] | 0.. ],
 *                             Lu_i = vec2tril(u_tril_vec_i) (gp_utils.py:22-49); the last block is scratch
 * Other shapes as vargp_elbo_t0_desc.  y == NULL: predictive moments only (no likelihood / KL; eps_theta must be given
 * unless map_est) -- VARGP.forward / predict.  vargp_elbo_tn_moments returns where fwd left mu, var (S, C, B).
 * info[0 .. S*C): Cholesky status of K(z_<=t) + eps I per (s, c).
 */
typedef struct vargp_elbo_tn_desc {
  int32_t S, C, M, D, B, F, nblk;
  int32_t map_est;
  float jitter;
  const float *log_mean, *log_logvar, *prior_log_mean, *prior_log_logvar;
  const float *z, *u_mean, *u_tril_vec; /* current task */
  float* z_all;
  float* rk_all;
  const float* x;
  const int64_t* y;
  const float *eps_theta, *eps_f;
  float* scalars;
  int32_t* info;
  void* ws;
  size_t ws_bytes;
  float* bump;
  uint64_t rng_seed;
  uint32_t* rng_counter;
  int32_t rng_sample_offset;
  int32_t forward_only; /* 1: workspace sized by vargp_elbo_tn_workspace_bytes_fwd; moments only (y == NULL), no bwd / end */
  int32_t defer_hyper;  /* as vargp_elbo_t0_desc.defer_hyper (vargp_elbo_tn_bwd only) */
  int32_t ext_lik;      /* as vargp_elbo_t0_desc.ext_lik (vargp_elbo_tn_fwd / _bwd; buffers: vargp_elbo_tn_lik_buffers); y must still be non-NULL
                         * for fwd to evaluate the KL (it is not dereferenced) */
  /* ep_var_mean = False (reference var_gp/vargp.py:137-152, VARGP(..., ep_var_mean=False)): the variational mean of the
   * current task is NOT offset by the conditional prior's mean, so the KL keeps that mean, evaluated at n_v samples
   * u_<t ~ q(u_<t | theta): eps_u (n_v, S, C, (nblk - 1) M) standard normal, 1 <= n_v <= 16.  no_var_mean = 1 selects it
   * (nblk > 1, vargp_elbo_tn_fwd / _bwd only; ignored by the tiled calls); 0: ep_var_mean = True, eps_u is not read. */
  const float* eps_u;
  int32_t n_v;
  int32_t no_var_mean;
  /* as vargp_elbo_t0_desc.info_host / info_event (vargp_elbo_tn_fwd only): info[0 .. S*C) is copied out and the event recorded
   * right behind the blocked factorisation, before the products that consume it */
  int32_t* info_host;
  void* info_event;
  /* The stationary kernel that builds K(z_<=t) and K_uf: 0 = RBF (a zero-initialised descriptor is the program described
   * above), 1 | 3 | 5 = Matern with nu = 1/2, 3/2, 5/2 on the same scaled distance (same hyper-parameters).  The reference has
   * no Matern kernel: this replaces kernels.MaternKernel.compute of this package on the composed per-op route
   * (vargp_matern_gram_fwd / _bwd), with the same definition entry by entry (d2 clamped at 0, exactly gamma^2 on the diagonal
   * of K(z, z), the nu = 1/2 derivative defined as 0 where d2 <= 0).  Every entry below that takes the descriptor returns
   * VARGP_EINVAL for any other value.  The workspace sizes do not depend on it. */
  int32_t kernel_nu2;
} vargp_elbo_tn_desc;
/* sizeof(vargp_elbo_tn_desc) as the library was compiled (bindings check their mirror of the struct against it) */
size_t vargp_elbo_tn_desc_bytes(void);
size_t vargp_elbo_tn_workspace_bytes(int S, int C, int M, int D, int B, int F, int nblk);
/* Workspace of a program that only ever evaluates predictive moments (VARGP.forward / predict, var_gp/vargp.py:115-131,
 * 196-198: no likelihood, no KL, no backward): none of the gradient buffers.  Set d->forward_only = 1. */
size_t vargp_elbo_tn_workspace_bytes_fwd(int S, int C, int M, int D, int B, int F, int nblk);
int vargp_elbo_tn_fwd(const vargp_elbo_tn_desc* d, vargp_stream_t stream);
int vargp_elbo_tn_bwd(const vargp_elbo_tn_desc* d, const float* seeds, float* g_log_mean, float* g_log_logvar, float* g_z,
                      float* g_u_mean, float* g_u_tril_vec, vargp_stream_t stream);
int vargp_elbo_tn_moments(const vargp_elbo_tn_desc* d, float** mu, float** var);
int vargp_elbo_tn_lik_buffers(const vargp_elbo_tn_desc* d, float** mu, float** var, float** gmu, float** gvar);
/* The same ELBO over a data set swept in minibatch tiles (BASELINE config 5: N = 1e6, M = 2048, K_uf tiled in HBM): loss
 * AND gradient, with everything that does not depend on the data (kernel matrix of the inducing points, factorisation,
 * small products, KL) computed once.  Workspace / descriptor as for fwd with d->B = the widest tile; d->y must be non-NULL
 * (any label pointer), d->x is not read.
 *   begin: theta, K(z_<=t), L, T, the small products, kl_hypers and kl_u into scalars[0..1], scalars[2] = 0, accumulators = 0
 *   tile : x (Bt, D), y (Bt), Bt <= d->B, eps_f (S, F, C, Bt) or NULL (native noise, one generator step per tile):
 *          scalars[2] += the tile's nll; the tile's share of every gradient is accumulated.
 *          y == NULL (seeds, eps_f ignored): the predictive moments mu, var (S, C, Bt) of the tile only, left where
 *          vargp_elbo_tn_moments says (row stride Bt) -- the predictive sweep VARGP.predict(x, tile=) of a model with or
 *          without previous tasks (var_gp/vargp.py:196-198 called per batch by var_gp/train_utils.py:21-35), with the
 *          x-independent part (begin) done once; the only tile mode of a forward_only program
 *   end  : Cholesky / kernel-matrix backward of the accumulated gradients; OVERWRITES the five gradient buffers with the
 *          gradient of seeds . (kl_hypers, kl_u, sum of the tiles' nll)
 * seeds (device, 3 floats) must be the same pointer contents for every tile and for end. */
int vargp_elbo_tn_begin(const vargp_elbo_tn_desc* d, vargp_stream_t stream);
int vargp_elbo_tn_tile(const vargp_elbo_tn_desc* d, const float* seeds, const float* x, const int64_t* y, const float* eps_f,
                       int Bt, vargp_stream_t stream);
int vargp_elbo_tn_end(const vargp_elbo_tn_desc* d, const float* seeds, float* g_log_mean, float* g_log_logvar, float* g_z,
                      float* g_u_mean, float* g_u_tril_vec, vargp_stream_t stream);

/* The last step of either program's backward -- theta-gradient -> variational hyper-parameters (RBFKernel.sample_hypers /
 * kl_hypers, var_gp/kernels.py:62-77: theta = mean + eps exp(logvar / 2), plus the gamma^2 of the predictive variance and the
 * gradient of kl_hypers scaled by its seed) -- as data: what the deferred form needs to finish it inside the optimiser's
 * launch.  Filled by vargp_elbo_t0_hyper_desc / vargp_elbo_tn_hyper_desc after a bwd with defer_hyper = 1 (pointers into
 * the program's workspace: valid until its next fwd). */
typedef struct vargp_hyper_grad_desc {
  const float *log_mean, *log_logvar, *prior_log_mean, *prior_log_logvar;
  const float *eps_theta, *gtheta, *g2, *gkd, *seeds;
  int32_t S, C, D1, map_est;
} vargp_hyper_grad_desc;
int vargp_elbo_t0_hyper_desc(const vargp_elbo_t0_desc* d, const float* seeds, vargp_hyper_grad_desc* out);
int vargp_elbo_tn_hyper_desc(const vargp_elbo_tn_desc* d, const float* seeds, vargp_hyper_grad_desc* out);
/* vargp_yogi_step_multi with the gradients of tensors idx_mean (log_mean) and idx_logvar (log_logvar; -1 under map_est)
 * computed on the fly from h (and stored to g[idx_*] as well): the step of experiments/vargp.py:35-37 with one launch less. */
int vargp_yogi_step_multi_hyper(int ntensors, float* const* p, float* const* g, float* const* m, float* const* v,
                                const int64_t* n, float lr, float beta1, float beta2, float eps, const float* step,
                                int step_mode, const vargp_hyper_grad_desc* h, int idx_mean, int idx_logvar,
                                vargp_stream_t stream);

/* Minibatch i of an epoch, gathered on the device: x[r, :] = data[perm[i B + r], :], y[r] = targets[perm[i B + r]], r < B, with
 * i = (int)(*step_now - *step_base) read from DEVICE memory -- step_now is a step counter some kernel of the step advances (the
 * `bump` of the ELBO programs' descriptors), step_base its value at the start of the epoch.  Replaces the two index_select
 * launches per step of the training loop (reference: DataLoader(train_set, batch_size, shuffle=True), experiments/vargp.py:26)
 * by a launch that can sit INSIDE a captured graph of K steps: the minibatch index advances on the device, the host launches
 * graphs.  perm: n int64 indices (one permutation per epoch); rows past n clamp to the last index. */
int vargp_gather_minibatch(const float* data, const int64_t* targets, const int64_t* perm, const float* step_now,
                           const float* step_base, int64_t n, int B, int D, float* x, int64_t* y, vargp_stream_t stream);

/* Same update for up to 8 tensors in one launch.  `step` (device float) = the step count t.
 * step_mode 0: use t as is.  1: use t + 1 (the caller advances the stored count elsewhere, e.g. through the `bump`
 * pointer of vargp_elbo_t0_desc, so that the optimiser needs no "t += 1" launch of its own). */
int vargp_yogi_step_multi(int ntensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                          const int64_t* n, float lr, float beta1, float beta2, float eps, const float* step,
                          int step_mode, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Variational kernel hyper-parameters (reference: RBFKernel.sample_hypers / kl_hypers,
 * var_gp/kernels.py:62-77).  D1 = D + 1.
 *   sample: theta[S, D1] = mean + eps * exp(logvar / 2)           (Normal.rsample)
 *   kl:     sum_d KL(N(mean_d, e^logvar_d) || N(prior_mean_d, e^prior_logvar_d))
 */
int vargp_hyper_sample_fwd(const float* mean, const float* logvar, const float* eps, float* theta, int S, int D1,
                           vargp_stream_t stream);
int vargp_hyper_sample_bwd(const float* logvar, const float* eps, const float* gtheta, float* gmean,
                           float* glogvar, int S, int D1, vargp_stream_t stream);
int vargp_hyper_kl_fwd(const float* mean, const float* logvar, const float* prior_mean, const float* prior_logvar,
                       float* kl, int D1, vargp_stream_t stream);
int vargp_hyper_kl_bwd(const float* mean, const float* logvar, const float* prior_mean, const float* prior_logvar,
                       const float* gkl, float* gmean, float* glogvar, int D1, vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Deep-kernel feature map (reference: DeepRBFKernel.phi, var_gp/kernels.py:80-96 = Linear(D,256) - ReLU - Linear(256,256)
 * - ReLU - Linear(256,64) in front of the RBF kernel).  The three matrix products are vargp_bgemm; these two fuse the
 * bias and the activation around them:  y[r,c] = act(x[r,c] + bias[c]),  act = ReLU if relu else identity;
 * backward: gx = gy * (y > 0) (or gy), gbias[c] = sum_r gx[r,c]  (gbias is zeroed by the call).
 */
int vargp_bias_act_fwd(const float* x, const float* bias, float* y, int64_t rows, int cols, int relu, vargp_stream_t stream);
int vargp_bias_act_bwd(const float* y, const float* gy, float* gx, float* gbias, int64_t rows, int cols, int relu,
                       vargp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (no reference counterpart): when enabled, the heavy launches are bracketed by
 * hipEvents on their own stream, tagged "rbf_kuf" / "rbf_kuu" (distance GEMM incl. the split-K combine pass),
 * "rbf_kuf_gemm", "rbf_kuu_gemm", "rbf_kuf_bwd_gemm", "rbf_kuu_bwd_gemm", "chol_inv_small", "bgemm".
 * vargp_prof_read sums and clears one tag.
 */
int vargp_prof_enable(int on);
int vargp_prof_read(const char* tag, double* total_ms, int64_t* launches);
/* Launch replay, for timing one kernel of a step that otherwise runs inside a captured graph (hipEvents cannot
 * bracket a graph node, and an event pair around a single launch also times the dispatch gap):
 * vargp_prof_remember(1) makes the tagged launches ("rbf_kuf_gemm", "rbf_kuu_gemm", "rbf_kuu_bwd_gemm" = the pair
 * launch of the two W.Y products, "chol_rbf_gemm" = factorisations + K_uf GEMM, "bgemm", ...) keep a copy of their
 * arguments; vargp_prof_replay re-launches the most recent one with that tag `iters` times back to back between ONE
 * pair of hipEvents on `stream` and returns the average time per launch in microseconds.  The buffers of the
 * remembered launch must still be alive.  Synchronises. */
int vargp_prof_remember(int on);
/* Tuning aid: force the tile shape of subsequent vargp_bgemm / internal GEMM launches (0 = automatic choice,
 * 1 = 128x128x16, 2 = 128x64x32, 3 = 64x64x64).  Results do not depend on it beyond summation order. */
int vargp_tune_gemm_tile(int tile);
int vargp_prof_replay(const char* tag, int iters, double* avg_us, vargp_stream_t stream);
/* Time line of the first-task step as the GPU sees it -- also inside a replayed hipGraph, where hipEvents cannot bracket a
 * node: while switched on, every kernel of the step stamps the device's constant 100 MHz wall clock at its first
 * workgroup's start and (atomic max) at every workgroup's end into a small device table.
 *   mode 1: clear the table and switch the stamps on;  mode 2: switch them off;
 *   mode 0: copy the table to out[12][2] = (start, end) ticks of 10 ns per slot, 0 = the slot's kernel did not run;
 *   mode 3: out[12][2] = (shader-clock ticks (s_memtime), wall-clock ticks of 10 ns) that went by between the start and the end
 *           of WORKGROUP 0 of each slot's last launch: 100 MHz x the ratio = the clock the chip held under that kernel.
 * Slots: 0 t0_pro_kuu, 1 chol_rbf_gemm (9: end of its last factorisation), 2 gemm_kernel (any plain product: the last one
 * launched), 3 t0_fwd_fused, 4 t0_bwd_mid, 5 t0_bwdmat_gemm (8: end of its last matrix chain), 6 t0_puu_final,
 * 7 yogi_multi; 10 / 11: end of the Gram / row-norm role of t0_pro_kuu.  Synchronous (hipMemcpy to / from device symbols): call between steps, not inside a capture. */
int vargp_prof_spans(int mode, unsigned long long* out);

#ifdef __cplusplus
}
#endif
#endif /* VARGP_HIP_H */
