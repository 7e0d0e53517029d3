// Kernel matrices built on the scaled squared distance -- RBF / ARD (reference: RBFKernel.compute, var_gp/kernels.py:24-56)
// and Matern nu = 1/2, 3/2, 5/2 -- and their backward, on one frame.  The inner products run on the f32 MFMA through
// gemm.hip; this file has the pre-pass (1/sigma^2, gamma^2, weighted squared row norms, the pre-scaled shared y), the direct
// form for D <= kRbfDirectD, the split-K combine pass, the backward pre-pass (W and its row / column sums) and the backward
// finalisation (gX, gY, gtheta from W.Y).  What a kernel family adds is its epilogue k(d2) (common.h: EpiRbf, EpiMatern<NU2>)
// and its weight -2 dk/dd2 (gram_w_kernel<NU2>, NU2 == 0: RBF).
//
//   d2_ij  = sum_d w_d (x_id - y_jd)^2 = na_i + nb_j - 2 sum_d w_d x_id y_jd,   w = exp(-2 theta_d)
//   K_ij   = g2 k(d2_ij),  g2 = exp(2 theta_D);   RBF: k = exp(-d2 / 2);   Matern: matern_k of common.h, d2 clamped at 0
//   W_ij   = gK_ij * (-2 g2 dk/dd2)               RBF: -2 dk/dd2 is K itself, so W = gK o K;   Matern: matern_w
//   with r = rowsum W, c = colsum W, P = W Y, Q = W^T X:
//   gX_i   = -sum_s w_s o (r_i x_i - P_i)          gY_j = -sum_s w_s o (c_j y_j - Q_j)
//   gth_sd = w_sd [ sum_i x_id (r_i x_id - 2 P_id) + sum_j c_j y_jd^2 ]      gth_sD = 2 sum gK o K
// The Matern W needs r = sqrt(d2), which K does not give back, so its backward RECOMPUTES the distance product (epilogue
// EpiDist2: the clamped d2, 0 on the diagonal of a self product) instead of carrying d2 over from the forward call:
// workspaces stay call-local, as everywhere in this library (the Python layer pools one scratch buffer per stream).
#include "common.h"

namespace vargp {

struct GramWs {
  float *w, *g2, *na, *nb, *part, *ys, *Wm, *r, *c, *P, *Q;
  int64_t Dp;
  size_t bytes;
};

// recompute_d2 (Matern): the backward runs the distance product first, so the forward's buffers are the leading part of
// the backward's, and the direct form (D <= kRbfDirectD) reserves no split-K partials and no scaled y.  The RBF backward
// has no distance product; its forward reserves part / ys at every D (the byte counts are part of the C ABI).
static GramWs carve(void* ws, int S, int C, int M, int N, int D, bool backward, bool recompute_d2) {
  GramWs o{};
  o.Dp = round_up(D, 4);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.w = take((int64_t)S * o.Dp);
  o.g2 = take(S);
  if (!backward || recompute_d2) {
    const bool lean = recompute_d2 && D <= kRbfDirectD;
    o.na = take((int64_t)S * C * M);
    o.nb = take((int64_t)S * C * N);
    o.part = take(lean ? 0 : (int64_t)2 * S * C * M * N);   // split-K partial products (at most 2 splits)
    o.ys = take(lean ? 0 : (int64_t)S * N * D);             // y o w of a shared y (one copy per hyper-sample)
  }
  if (backward) {
    o.Wm = take((int64_t)S * C * M * N);
    o.r = take((int64_t)S * C * M);
    o.c = take((int64_t)S * C * N);
    o.P = take((int64_t)S * C * M * D);
    o.Q = take((int64_t)S * C * N * D);
  }
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

// what the two families call their launches: ProfScope / launch tags (read by bench.py and profiles/) and check_launch names
struct GramTags { const char *kuu, *kuf, *kuu_gemm, *kuf_gemm, *kuu_bwd_gemm, *kuf_bwd_gemm, *direct, *fwd, *bwd; };
static const GramTags kRbfTags = {"rbf_kuu", "rbf_kuf", "rbf_kuu_gemm", "rbf_kuf_gemm", "rbf_kuu_bwd_gemm", "rbf_kuf_bwd_gemm",
                                  "rbf_gram_fwd(direct)", "rbf_gram_fwd", "rbf_gram_bwd"};
static const GramTags kMaternTags = {"matern_kuu", "matern_kuf", "matern_kuu_gemm", "matern_kuf_gemm", "matern_kuu_bwd_gemm",
                                     "matern_kuf_bwd_gemm", "matern_gram(direct)", "matern_gram(gemm)", "matern_gram_bwd"};

// DistEpi code -> its epilogue type, once for this file: f(EPI{})
template <class F>
static int with_epi(int epi, F&& f) {
  switch (epi) {
    case kEpiRbf: return f(EpiRbf{});
    case kEpiMatern12: return f(EpiMatern<1>{});
    case kEpiMatern32: return f(EpiMatern<3>{});
    case kEpiMatern52: return f(EpiMatern<5>{});
    case kEpiDist2: return f(EpiDist2{});
  }
  VARGP_REQUIRE(false, "distance product: epilogue %d", epi);
}

__global__ void gram_prep_kernel(const float* __restrict__ theta, float* __restrict__ w, float* __restrict__ g2, int D,
                                 int64_t Dp) {
  const int s = blockIdx.x;
  const float* th = theta + (int64_t)s * (D + 1);
  for (int d = threadIdx.x; d < Dp; d += blockDim.x) w[s * Dp + d] = d < D ? expf(-2.f * th[d]) : 0.f;
  if (threadIdx.x == 0) g2[s] = expf(2.f * th[D]);
}

// Small input dimension (D <= kRbfDirectD, e.g. the 2-D toy problem): form the squared distance directly as
// sum_d w_d (x_d - y_d)^2 -- no cancellation, no GEMM; exactly 0 for coincident points, so the diagonal of a self product
// needs no special case.  One thread per kernel-matrix entry; ldk: row stride of K.
template <class EPI>
__global__ __launch_bounds__(256) void dist_direct_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                          const float* __restrict__ w, const float* __restrict__ g2,
                                                          float* __restrict__ K, int64_t ldk, int C, int M, int N, int D,
                                                          int64_t Dp, int y_shared, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int n = e % N, m = (e / N) % M, c = (e / ((int64_t)N * M)) % C;
  const int s = e / ((int64_t)N * M * C);
  const float* xr = X + ((int64_t)c * M + m) * D;
  const float* yr = Y ? (y_shared ? Y + (int64_t)n * D : Y + ((int64_t)c * N + n) * D) : X + ((int64_t)c * M + n) * D;
  const float* ws = w + s * Dp;
  float d2 = 0.f;
  for (int d = 0; d < D; ++d) { const float t = xr[d] - yr[d]; d2 = fmaf(ws[d] * t, t, d2); }
  K[(((int64_t)s * C + c) * M + m) * ldk + n] = EPI::off(g2[s], d2);
}

// split-K: the epilogue over the summed partial inner products, d2 = na + nb - 2 (ab_0 + ab_1 ...); same arithmetic as the
// fused GEMM epilogue.  One thread per entry of the flattened [nb0][rows][N] result.
template <class EPI>
__global__ __launch_bounds__(256) void dist_combine_kernel(const float* __restrict__ part, int nsplit, int64_t sSplit,
                                                           const float* __restrict__ na, const float* __restrict__ nbv,
                                                           const float* __restrict__ g2, float* __restrict__ K,
                                                           int64_t rows_per_s, int N, int64_t nb_stride_s,
                                                           int64_t nb_stride_c, int Mb, int same_xy, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int col = e % N;
  const int64_t row = e / N;                 // s * rows_per_s + (c * Mb + m)
  const int64_t s = row / rows_per_s, rc = row % rows_per_s;
  const int64_t c = rc / Mb;
  const int m = rc % Mb;
  float ab = 0.f;
  for (int k = 0; k < nsplit; ++k) ab += part[k * sSplit + e];
  const float d2 = na[row] + nbv[s * nb_stride_s + c * nb_stride_c + col] - 2.f * ab;
  K[e] = (same_xy && m == col) ? EPI::diag(g2[s]) : EPI::off(g2[s], d2);
}

// prep + both norm passes in one launch: nrm_x[s][row] = sum_d w_sd x[row][d]^2 (likewise y), w_sd = exp(-2 theta_sd)
// evaluated on the fly; the blocks with blockIdx.x == 0 also store w (zero-padded to Dp) and g2 = exp(2 theta_sD) for the
// GEMM that follows.  One wave per row; grid (ceil((xrows + yrows) / 4), S).
// ys / xs (nullable): the scaled copies y o w, [S][yrows][D], and x o w, [S][xrows][D] -- with a pre-scaled operand the
// distance GEMM needs no per-k scaling (GemmParams.kscale = NULL).
__global__ __launch_bounds__(256) void rbf_prep_norm_kernel(const float* __restrict__ theta, const float* __restrict__ x,
                                                            const float* __restrict__ y, float* __restrict__ w,
                                                            float* __restrict__ g2, float* __restrict__ na,
                                                            float* __restrict__ nb, int64_t xrows, int64_t yrows, int D,
                                                            int64_t Dp, float* __restrict__ ys, float* __restrict__ xs) {
  const int s = blockIdx.y, lane = threadIdx.x & 63;
  const float* th = theta + (int64_t)s * (D + 1);
  if (blockIdx.x == 0) {
    for (int d = threadIdx.x; d < Dp; d += 256) w[s * Dp + d] = d < D ? expf(-2.f * th[d]) : 0.f;
    if (threadIdx.x == 0) g2[s] = expf(2.f * th[D]);
  }
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= xrows + yrows) return;
  const bool isx = row < xrows;
  const float* xr = isx ? x + row * D : y + (row - xrows) * D;
  float* yo = isx ? (xs ? xs + ((int64_t)s * xrows + row) * D : nullptr)
                  : (ys ? ys + ((int64_t)s * yrows + (row - xrows)) * D : nullptr);
  // sixteen 64-wide chunks per pass, ALL their loads first (clamped index), then the arithmetic and the stores: D = 784 is one
  // pass -- one memory round trip for the row instead of D / 256 with a store's acknowledgement in front of every next load
  // (vmcnt retires in order)
  float acc0 = 0.f, acc1 = 0.f;
  for (int d0 = 0; d0 < D; d0 += 1024) {
    float xv[16], tv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int d = min(d0 + 64 * q + lane, D - 1);
      xv[q] = xr[d]; tv[q] = th[d];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int d = d0 + 64 * q + lane;
      const float wv = expf(-2.f * tv[q]);
      const float v = d < D ? xv[q] : 0.f;
      if (q & 1) acc1 = fmaf(v * v, wv, acc1); else acc0 = fmaf(v * v, wv, acc0);
      if (yo && d < D) yo[d] = v * wv;
    }
  }
  const float acc = wave_sum(acc0 + acc1);
  if (lane == 0) {
    if (isx) na[(int64_t)s * xrows + row] = acc; else nb[(int64_t)s * yrows + (row - xrows)] = acc;
  }
}

// W = gK o (-2 g2 dk/dd2) with its row sums r, column sums c and 2 sum gK o K (= dlog gamma) into gtheta[s, D], in one pass.
// NU2 == 0 (RBF): W = gK o K, whose sum is the gamma total too -- d2m and g2 are not read.  Matern: W from the recomputed
// d2; d2m and W may be the same buffer (a thread reads the entry it then writes).
// grid (ceil(N/256), ceil(Mb/WROWS), nb): a thread owns one column of a strip of WROWS rows; r and c are accumulated with
// float atomics (pre-zeroed by the caller), the total with one atomic per block.
constexpr int WROWS = 8;
template <int NU2>
__global__ __launch_bounds__(256) void gram_w_kernel(const float* __restrict__ K, const float* __restrict__ gK,
                                                     const float* d2m, const float* __restrict__ g2, float* W,
                                                     float* __restrict__ r, float* __restrict__ c,
                                                     float* __restrict__ gtheta, int Mb, int N, int Cb, int D) {
  __shared__ float red[4];
  const int col = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int row0 = blockIdx.y * WROWS;
  const int64_t b = blockIdx.z;
  const bool cok = col < N;
  const int64_t base = b * Mb * N;
  float g = 0.f;
  if constexpr (NU2 != 0) g = g2[b / Cb];
  float csum = 0.f, ksum = 0.f;
  const int rend = min(WROWS, Mb - row0);
  for (int rr = 0; rr < rend; ++rr) {
    const int64_t off = base + (int64_t)(row0 + rr) * N + col;
    float v = 0.f;
    if (cok) {
      if constexpr (NU2 == 0) {
        v = K[off] * gK[off];
        W[off] = v;
      } else {
        const float gk = gK[off];
        v = gk * matern_w<NU2>(g, d2m[off]);
        W[off] = v;
        ksum = fmaf(gk, K[off], ksum);
      }
    }
    csum += v;
    const float rs = wave_sum(v);
    if (lane == 0 && rs != 0.f) atomicAdd(&r[b * Mb + row0 + rr], rs);
  }
  if (cok) atomicAdd(&c[b * N + col], csum);
  const float tot = block_sum<256>(NU2 == 0 ? csum : ksum, red);
  if (threadIdx.x == 0) atomicAdd(&gtheta[(b / Cb) * (D + 1) + D], 2.f * tot);
}

// Square case (Y = X) in one pass: Ws = W + W^T without its diagonal, r = its row sums (= row + column sums of W), and
// 2 sum gK o K (diagonal included) into gtheta[s, D].  kSelfRows consecutive rows of one matrix per block, a wave takes
// every 4th.  RBF (NU2 == 0): Ws_ij = K_ij gK_ij + K_ji gK_ji, whose sum with the diagonal's is the gamma total.  Matern:
// d2 is symmetric, so Ws_ij = (gK_ij + gK_ji) w(d2_ij); d2m and Ws may be the same buffer.
constexpr int kSelfRows = 16;
template <int NU2>
__global__ __launch_bounds__(256) void gram_w_self_kernel(const float* __restrict__ K, const float* __restrict__ gK,
                                                          const float* d2m, const float* __restrict__ g2, float* Ws,
                                                          float* __restrict__ r, float* __restrict__ gtheta, int M, int Cb,
                                                          int D, int nchunk) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x / nchunk;
  const int i0 = ((int)blockIdx.x % nchunk) * kSelfRows, i1 = min(M, i0 + kSelfRows);
  const float* Kb = K + b * M * M;
  const float* gKb = gK + b * M * M;
  const float* db = d2m + b * M * M;
  float g = 0.f;
  if constexpr (NU2 != 0) g = g2[b / Cb];
  float tot = 0.f, dsum = 0.f, ksum = 0.f;
  for (int i = i0 + (threadIdx.x >> 6); i < i1; i += 4) {
    float acc = 0.f;
    for (int j = lane; j < M; j += 64) {
      // The diagonal: K_ii = gamma^2 does not depend on x_i or the lengthscales (the reference's autograd cancels it
      // exactly: -2 g + g + g on the entry (i, i) of its Gram, kernels.py:44-54), so it must not reach P = Ws x and r, whose
      // difference would otherwise leave rounding noise of order eps W_ii x_i where the reference has an exact zero (with
      // underflowing off-diagonals -- MNIST pixels at the initial lengthscale -- the whole gradient).  It only counts for gamma.
      const bool dg = i == j;
      if constexpr (NU2 == 0) {
        const float v = Kb[(int64_t)i * M + j] * gKb[(int64_t)i * M + j] + Kb[(int64_t)j * M + i] * gKb[(int64_t)j * M + i];
        Ws[b * M * M + (int64_t)i * M + j] = dg ? 0.f : v;
        acc += dg ? 0.f : v;
        dsum += dg ? v : 0.f;
      } else {
        const float gij = gKb[(int64_t)i * M + j];
        const float gs = gij + gKb[(int64_t)j * M + i];
        const float v = dg ? 0.f : gs * matern_w<NU2>(g, db[(int64_t)i * M + j]);
        Ws[b * M * M + (int64_t)i * M + j] = v;
        acc += v;
        ksum = fmaf(gij, Kb[(int64_t)i * M + j], ksum);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) r[b * M + i] = acc;
    if constexpr (NU2 == 0) tot += acc;
  }
  if constexpr (NU2 == 0) {
    tot += wave_sum(dsum);
    const float t = block_sum<256>(lane == 0 ? tot : 0.f, red);   // every lane of a wave holds the wave's total
    if (threadIdx.x == 0) atomicAdd(&gtheta[(b / Cb) * (D + 1) + D], t);
  } else {
    const float t = block_sum<256>(ksum, red);
    if (threadIdx.x == 0) atomicAdd(&gtheta[(b / Cb) * (D + 1) + D], 2.f * t);
  }
}

// Finalise one side.  rows = points of this side (flattened over classes), S samples.
//   g[row][d]  (+)= -sum_s w_sd (R_s,row x_row,d - P_s,row,d)            (if g != null)
//   gtheta[s][d] += w_sd sum_row x (R x - kappa P)                         (P may be null -> 0)
// block = 64 d-columns x 4 row lanes, RPB rows per block.
constexpr int RPB = 32;
__global__ __launch_bounds__(256) void rbf_final_kernel(const float* __restrict__ x, const float* __restrict__ R,
                                                        const float* __restrict__ P, const float* __restrict__ theta,
                                                        float* __restrict__ g, float* __restrict__ gtheta,
                                                        int64_t rows, int D, int64_t Dp, int S, float kappa,
                                                        int accumulate) {
  __shared__ float red[4][64];
  const int dx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + dx;
  const int64_t row0 = (int64_t)blockIdx.y * RPB;
  const bool dok = d < D;
  float xa[RPB / 4], ga[RPB / 4];
#pragma unroll
  for (int j = 0; j < RPB / 4; ++j) {
    const int64_t row = row0 + ry + 4 * j;
    xa[j] = (dok && row < rows) ? x[row * D + d] : 0.f;
    ga[j] = 0.f;
  }
  for (int s = 0; s < S; ++s) {
    const float wv = dok ? expf(-2.f * theta[(int64_t)s * (D + 1) + d]) : 0.f;   // 1/sigma_d^2
    float th = 0.f;
#pragma unroll
    for (int j = 0; j < RPB / 4; ++j) {
      const int64_t row = row0 + ry + 4 * j;
      if (row < rows) {
        const float rr = R[(int64_t)s * rows + row];
        const float pv = (P && dok) ? P[((int64_t)s * rows + row) * D + d] : 0.f;
        const float rx = rr * xa[j];
        ga[j] -= wv * (rx - pv);
        th += xa[j] * (rx - kappa * pv);
      }
    }
    __syncthreads();
    red[ry][dx] = th;
    __syncthreads();
    if (ry == 0 && dok) {
      const float t = red[0][dx] + red[1][dx] + red[2][dx] + red[3][dx];
      atomicAdd(&gtheta[(int64_t)s * (D + 1) + d], wv * t);
    }
  }
  if (g && dok) {
#pragma unroll
    for (int j = 0; j < RPB / 4; ++j) {
      const int64_t row = row0 + ry + 4 * j;
      if (row < rows) {
        if (accumulate) g[row * D + d] += ga[j]; else g[row * D + d] = ga[j];
      }
    }
  }
}

int rbf_prep_norm_launch(const float* theta, const float* x, int64_t xrows, const float* y, int64_t yrows, float* w,
                         float* g2, float* na, float* nb, int S, int D, int64_t Dp, hipStream_t st, float* ys, float* xs) {
  hipLaunchKernelGGL(rbf_prep_norm_kernel, dim3(cdiv(xrows + yrows, 4), S), dim3(256), 0, st, theta, x, y, w, g2, na, nb,
                     xrows, yrows, D, Dp, ys, xs);
  return check_launch("rbf_prep_norm");
}

int rbf_final_launch(const float* x, const float* R, const float* P, const float* theta, float* g, float* gtheta, int64_t rows,
                     int D, int64_t Dp, int S, float kappa, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(rbf_final_kernel, dim3(cdiv(D, 64), cdiv(rows, RPB)), dim3(256), 0, st, x, R, P, theta, g, gtheta, rows, D,
                     Dp, S, kappa, accumulate);
  return check_launch("rbf_final");
}

template <class EPI>
static void direct_launch(const float* X, const float* Y, const float* w, const float* g2, float* K, int64_t ldk, int S, int C,
                          int M, int N, int D, int64_t Dp, int y_shared, hipStream_t st) {
  const int64_t total = (int64_t)S * C * M * N;
  hipLaunchKernelGGL(dist_direct_kernel<EPI>, dim3(cdiv(total, 256)), dim3(256), 0, st, X, Y, w, g2, K, ldk, C, M, N, D, Dp,
                     y_shared, total);
}

// the direct form for a caller that has run the pre-pass itself (the ELBO programs): K [S, C, M, ldk] with the epilogue
// `epi` (a DistEpi other than kEpiPlain)
int dist_direct_launch(const float* X, const float* Y, const float* w, const float* g2, float* K, int64_t ldk, int S, int C,
                       int M, int N, int D, int64_t Dp, int y_shared, int epi, hipStream_t st) {
  const int rc = with_epi(epi, [&](auto e) {
    direct_launch<decltype(e)>(X, Y, w, g2, K, ldk, S, C, M, N, D, Dp, y_shared, st);
    return (int)VARGP_OK;
  });
  if (rc) return rc;
  return check_launch(epi == kEpiRbf ? kRbfTags.direct : kMaternTags.direct);
}

// The distance product of one call with the epilogue EPI (code `epi`) into out[S, C, M, N]: pre-pass, then the direct
// kernel, the fused GEMM, or split-K partials + combine pass.
template <class EPI>
static int gram_dist(const float* theta, const float* X, const float* Y, float* out, int S, int C, int M, int N, int D,
                     int y_shared, const GramWs& o, int epi, const GramTags& tg, hipStream_t st) {
  const bool self = (Y == nullptr);
  if (D <= kRbfDirectD) {
    hipLaunchKernelGGL(gram_prep_kernel, dim3(S), dim3(256), 0, st, theta, o.w, o.g2, D, o.Dp);
    direct_launch<EPI>(X, Y, o.w, o.g2, out, N, S, C, M, N, D, o.Dp, y_shared, st);
    return check_launch(tg.direct);
  }
  const int64_t xrows = (int64_t)C * M, yrows = y_shared ? N : (int64_t)C * N;
  // shared y (the minibatch): pre-scaled once per hyper-sample by the norm pass, so that the GEMM's main loop carries no
  // scale loads / multiplies
  const bool prescale = y_shared && !self;
  int rc = rbf_prep_norm_launch(theta, X, xrows, Y, self ? (int64_t)0 : yrows, o.w, o.g2, o.na, o.nb, S, D, o.Dp, st,
                                prescale ? o.ys : (float*)nullptr, (float*)nullptr);
  if (rc) return rc;
  // shared Y: the classes' inducing points are just more rows of one [C*M, D] x [D, N] product
  const int Cb = y_shared ? 1 : C, Mb = y_shared ? C * M : M;
  GemmParams p{};
  p.A = X; p.B = self ? X : Y; p.C = out; p.D = nullptr;
  p.M = Mb; p.N = N; p.K = D; p.lda = D; p.ldb = D; p.ldc = N; p.ldd = 0;
  p.nb1 = Cb; p.nb2 = 1;
  p.sA[0] = 0; p.sA[1] = (int64_t)Mb * D;
  p.sB[0] = 0; p.sB[1] = y_shared ? 0 : (int64_t)N * D;
  p.sC[0] = (int64_t)Cb * Mb * N; p.sC[1] = (int64_t)Mb * N;
  p.alpha = 1.f; p.beta = 0.f;
  p.kscale = o.w; p.ks_ld = o.Dp; p.g2 = o.g2;
  p.na = o.na; p.sNa[0] = xrows; p.sNa[1] = Mb;
  p.nbv = self ? o.na : o.nb; p.sNb[0] = self ? xrows : yrows; p.sNb[1] = (self || !y_shared) ? N : 0;
  p.same_xy = self ? 1 : 0;
  if (prescale) { p.B = o.ys; p.sB[0] = (int64_t)N * D; p.kscale = nullptr; }
  const int nsplit = rbf_splitk(Mb, N, D, S * Cb);
  {
    ProfScope whole(self ? tg.kuu : tg.kuf, st);    // distance GEMM (+ combine pass if K was split)
    const int64_t total = (int64_t)S * Cb * Mb * N;
    if (nsplit > 1) { p.splitk = nsplit; p.sSplit = total; p.C = o.part; }
    // (epi == kEpiRbf: launch_gemm(..., rbf = true, ...) is exactly this call)
    rc = launch_gemm_epi(p, 0, 1, S * Cb, epi, st, self ? tg.kuu_gemm : tg.kuf_gemm);
    if (rc) return rc;
    if (nsplit > 1)
      hipLaunchKernelGGL(dist_combine_kernel<EPI>, dim3(cdiv(total, 256)), dim3(256), 0, st, o.part, nsplit, p.sSplit, o.na,
                         self ? o.na : o.nb, o.g2, out, (int64_t)Cb * Mb, N, self ? xrows : yrows,
                         (self || !y_shared) ? (int64_t)N : 0, Mb, self ? 1 : 0, total);
  }
  return check_launch(tg.fwd);
}

// The backward of one call: (Matern: d2 into Wm,) W over it with r, c and the gamma total, then P = W . Y, finalise X,
// Q = W^T . X, finalise Y.
template <int NU2>
static int gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK, float* gX, float* gY,
                    float* gtheta, int S, int C, int M, int N, int D, int y_shared, int accumulate, const GramWs& o,
                    const GramTags& tg, hipStream_t st) {
  const bool self = (Y == nullptr);
  const int Cb = y_shared ? 1 : C, Mb = y_shared ? C * M : M;
  const int64_t xrows = (int64_t)C * M, yrows = y_shared ? N : (int64_t)C * N;
  const int nb = S * Cb;
  int rc;
  if constexpr (NU2 != 0) {   // d2 into Wm, then W over it in place (each thread reads the entry it writes)
    rc = gram_dist<EpiDist2>(theta, X, Y, o.Wm, S, C, M, N, D, y_shared, o, kEpiDist2, tg, st);
    if (rc) return rc;
  }
  if (!accumulate) zero_async(gtheta, sizeof(float) * (size_t)S * (D + 1), st);
  if (self) {
    const int nchunk = cdiv(M, kSelfRows);
    hipLaunchKernelGGL(gram_w_self_kernel<NU2>, dim3(nb * nchunk), dim3(256), 0, st, K, gK, o.Wm, o.g2, o.Wm, o.r, gtheta, M,
                       Cb, D, nchunk);
  } else {
    zero_async(o.r, sizeof(float) * (size_t)(o.P - o.r), st);   // r and c are adjacent
    hipLaunchKernelGGL(gram_w_kernel<NU2>, dim3(cdiv(N, 256), cdiv(Mb, WROWS), nb), dim3(256), 0, st, K, gK, o.Wm, o.g2, o.Wm,
                       o.r, o.c, gtheta, Mb, N, Cb, D);
  }
  // P = W . Y   ([Mb, N] x [N, D]) per (s, class-batch)
  GemmParams p{};
  p.A = o.Wm; p.B = self ? X : Y; p.C = o.P;
  p.M = Mb; p.N = D; p.K = N; p.lda = N; p.ldb = D; p.ldc = D;
  p.nb1 = Cb; p.nb2 = 1;
  p.sA[0] = (int64_t)Cb * Mb * N; p.sA[1] = (int64_t)Mb * N;
  p.sB[0] = 0; p.sB[1] = y_shared ? 0 : (int64_t)N * D;
  p.sC[0] = (int64_t)Cb * Mb * D; p.sC[1] = (int64_t)Mb * D;
  p.alpha = 1.f;
  rc = launch_gemm(p, 0, 0, nb, false, st, self ? tg.kuu_bwd_gemm : tg.kuf_bwd_gemm);
  if (rc) return rc;
  rc = rbf_final_launch(X, o.r, o.P, theta, gX, gtheta, xrows, D, o.Dp, S, self ? 1.f : 2.f, accumulate, st);
  if (rc) return rc;
  if (!self) {
    const float* Qp = nullptr;
    if (gY) {  // Q = W^T . X  ([N, Mb] x [Mb, D])
      GemmParams q{};
      q.A = o.Wm; q.B = X; q.C = o.Q;
      q.M = N; q.N = D; q.K = Mb; q.lda = N; q.ldb = D; q.ldc = D;
      q.nb1 = Cb; q.nb2 = 1;
      q.sA[0] = (int64_t)Cb * Mb * N; q.sA[1] = (int64_t)Mb * N;
      q.sB[0] = 0; q.sB[1] = (int64_t)Mb * D;
      q.sC[0] = (int64_t)Cb * N * D; q.sC[1] = (int64_t)N * D;
      q.alpha = 1.f;
      rc = launch_gemm(q, 1, 0, nb, false, st);
      if (rc) return rc;
      Qp = o.Q;
    }
    rc = rbf_final_launch(Y, o.c, Qp, theta, gY, gtheta, yrows, D, o.Dp, S, 0.f, accumulate, st);
    if (rc) return rc;
  }
  return check_launch(tg.bwd);
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_rbf_workspace_bytes(int S, int C, int M, int N, int D, int backward) {
  return carve(nullptr, S, C, M, N, D, backward != 0, false).bytes + 256;
}

extern "C" size_t vargp_matern_workspace_bytes(int S, int C, int M, int N, int D, int backward) {
  return carve(nullptr, S, C, M, N, D, backward != 0, true).bytes + 256;
}

extern "C" int vargp_rbf_gram_fwd(const float* theta, const float* X, const float* Y, float* K, int S, int C, int M,
                                  int N, int D, int y_shared, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && ws, "rbf_gram_fwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && M > 0 && D > 0, "rbf_gram_fwd: bad dims");
  if (!Y) { N = M; y_shared = 0; }
  VARGP_REQUIRE(N > 0, "rbf_gram_fwd: bad N");
  VARGP_REQUIRE(ws_bytes >= vargp_rbf_workspace_bytes(S, C, M, N, D, 0), "rbf_gram_fwd: workspace too small");
  const GramWs o = carve(ws, S, C, M, N, D, false, false);
  return gram_dist<EpiRbf>(theta, X, Y, K, S, C, M, N, D, y_shared, o, kEpiRbf, kRbfTags, as_stream(stream));
}

extern "C" int vargp_rbf_gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK,
                                  float* gX, float* gY, float* gtheta, int S, int C, int M, int N, int D,
                                  int y_shared, int accumulate, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && gK && gtheta && ws, "rbf_gram_bwd: null pointer");
  if (!Y) { N = M; y_shared = 0; gY = nullptr; }
  VARGP_REQUIRE(ws_bytes >= vargp_rbf_workspace_bytes(S, C, M, N, D, 1), "rbf_gram_bwd: workspace too small");
  const GramWs o = carve(ws, S, C, M, N, D, true, false);
  return gram_bwd<0>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, kRbfTags, as_stream(stream));
}

extern "C" int vargp_matern_gram_fwd(const float* theta, const float* X, const float* Y, float* K, int S, int C, int M, int N,
                                     int D, int y_shared, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && ws, "matern_gram_fwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && M > 0 && D > 0, "matern_gram_fwd: bad dims");
  VARGP_REQUIRE(nu2 == 1 || nu2 == 3 || nu2 == 5, "matern_gram_fwd: nu2 = %d (1, 3 or 5)", nu2);
  if (!Y) { N = M; y_shared = 0; }
  VARGP_REQUIRE(N > 0, "matern_gram_fwd: bad N");
  VARGP_REQUIRE(ws_bytes >= vargp_matern_workspace_bytes(S, C, M, N, D, 0), "matern_gram_fwd: workspace too small");
  const GramWs o = carve(ws, S, C, M, N, D, false, true);
  const int epi = nu2 == 1 ? kEpiMatern12 : nu2 == 3 ? kEpiMatern32 : kEpiMatern52;
  return with_epi(epi, [&](auto e) {
    return gram_dist<decltype(e)>(theta, X, Y, K, S, C, M, N, D, y_shared, o, epi, kMaternTags, as_stream(stream));
  });
}

extern "C" int vargp_matern_gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK,
                                     float* gX, float* gY, float* gtheta, int S, int C, int M, int N, int D, int y_shared,
                                     int nu2, int accumulate, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && gK && gtheta && ws, "matern_gram_bwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && M > 0 && D > 0, "matern_gram_bwd: bad dims");
  VARGP_REQUIRE(nu2 == 1 || nu2 == 3 || nu2 == 5, "matern_gram_bwd: nu2 = %d (1, 3 or 5)", nu2);
  if (!Y) { N = M; y_shared = 0; gY = nullptr; }
  VARGP_REQUIRE(N > 0, "matern_gram_bwd: bad N");
  VARGP_REQUIRE(ws_bytes >= vargp_matern_workspace_bytes(S, C, M, N, D, 1), "matern_gram_bwd: workspace too small");
  const GramWs o = carve(ws, S, C, M, N, D, true, true);
  hipStream_t st = as_stream(stream);
  if (nu2 == 1) return gram_bwd<1>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, kMaternTags, st);
  if (nu2 == 3) return gram_bwd<3>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, kMaternTags, st);
  return gram_bwd<5>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, kMaternTags, st);
}
