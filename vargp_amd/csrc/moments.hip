// Weighted moments of the cross-kernel over a whole data set, for G independent outputs over ONE data matrix X [N][D] and ONE
// hyper vector -- what the closed-form optimal q(u) of a Gaussian likelihood needs of the data (collapsed.py; nothing of this is
// in the reference).  With k_n = k_theta(Z_g, x_n), an Mt-vector:
//   Phi_g = sum_n w_gn k_n k_n^T,   c_g = sum_n w_gn y_gn k_n,   sums_g = (sum_n w_gn, sum_n w_gn y_gn^2).
// K(Z, X) never reaches global memory.  A workgroup owns one (output g, lower-triangle 64 x 64 tile (ti, tj) of Phi, chunk of N).
// It walks its chunk 64 columns at a time: the two 64-row panels of K behind the tile (one on the diagonal) are built in LDS as
// [column][row], then 32 v_mfma_f32_32x32x2_f32 per wave add w K_i K_j^T over the 64 columns to the tile's accumulators (four
// waves as 2 x 2, fragment maps as in gemm.hip), which stay in registers for the whole chunk.  The tiles of column tj = 0 also
// form their panel's share of c, and tile (0, 0) the two sums.
//   D <= kRbfDirectD: the scaled distance directly, d2 = sum_d w_d (z_d - x_d)^2 in ascending d (the arithmetic of gram.hip's
//   direct form); the Z panels are staged once per workgroup, the 64 points of X once per step.
//   D  > kRbfDirectD: d2 = |a|^2 + |b|^2 - 2 a.b with a = z / lengthscale, b = x / lengthscale: slabs of 32 values of d of both are
//   staged in LDS, a.b on the same MFMA, the squared norms from the staged slabs themselves -- no pre-pass and no buffer over N.
// Columns behind the end of the chunk are MASKED: their K entries and weights are written as zeros whatever X holds there (the
// loads themselves are guarded).  A zero weight multiplies a finite K entry: it adds exactly nothing.
// No atomics.  A second launch adds the chunks' partial tiles in ascending chunk order in fp64, rounds once to fp32 and writes
// entry (i, j), j <= i, to both triangles: Phi is bitwise symmetric and two calls on the same input are bitwise equal.
// The chunking depends on the shapes alone (mom_plan): at most kMoMaxChunks chunks of at least kMoMinChunk columns, as many as
// give the launch about kMoTargetWg workgroups.
// vargp_gram_moments_v is the same kernel with VW = true: c = sum_n v_n k_n with a weight vector v of its own in place of w y
// (a.y holds v), sums = (sum w, sum v).  The softmax sites need it: lam1 / lam2 is not representable where lam2 underflows.
#include "dataset_pass.h"      // the tiling constants, the chunking rule and the other pieces shared with sites.hip

namespace vargp {

typedef float mo_f32x16 __attribute__((ext_vector_type(16)));

struct MomPlan {
  int nt, ntri;              // tiles per side, lower-triangle tiles
  Chunks ch;                 // ch.nch chunks of ch.len columns
  float *pphi, *pc, *ps;     // partials [G][nch][ntri][64 * 64], [G][nch][nt * 64], [G][nch][2]
  size_t bytes;
};

static MomPlan mom_plan(void* ws, int G, int Mt, int N) {
  MomPlan o{};
  o.nt = cdiv(Mt, kMoT);
  o.ntri = o.nt * (o.nt + 1) / 2;
  o.ch = chunk_rule(N, (int64_t)G * o.ntri);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.pphi = take((int64_t)G * o.ch.nch * o.ntri * kMoT * kMoT);
  o.pc = take((int64_t)G * o.ch.nch * o.nt * kMoT);
  o.ps = take((int64_t)G * o.ch.nch * 2);
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

struct MomArgs {
  const float *theta, *Z, *X, *w, *y;
  float *Phi, *c, *sums;
  MomPlan p;
  int G, Mt, N, D;
};

// lower-triangle tile (ti, tj), tj <= ti, from its linear index
__device__ __forceinline__ void mo_tile(int t, int& ti, int& tj) {
  ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  tj = t - ti * (ti + 1) / 2;
}

// grid (ntri * nch, G): blockIdx.x = chunk * ntri + tile
template <class EPI, bool DIRECT, bool VW>
__global__ __launch_bounds__(256) void moments_kernel(const MomArgs a) {
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  __shared__ float Ks[2][T * LD];                                // the K panels of the tile's rows and columns: [n][m]
  __shared__ float stage[DIRECT ? 3 * T * kMoDl : 3 * BK * LD];  // DIRECT: Z_i, Z_j, X rows; else the slabs of a_i, a_j, b: [k][r]
  __shared__ float wl[kRbfDirectD];                              // DIRECT: exp(-2 theta_d)
  __shared__ float wn[T], wyn[T];                                // w_n and w_n y_n of the step's columns (0 behind the end)
  __shared__ float nrm[3][T];                                    // !DIRECT: |a_i|^2, |a_j|^2, |b|^2
  __shared__ float cred[4 * T];

  const int Mt = a.Mt, D = a.D, ntri = a.p.ntri;
  const int chunk = blockIdx.x / ntri, t = blockIdx.x - chunk * ntri;
  int ti, tj;
  mo_tile(t, ti, tj);
  const bool two = ti != tj;
  const int i0 = ti * T, j0 = tj * T;
  const int64_t g = blockIdx.y;
  const int64_t cbeg = (int64_t)chunk * a.p.ch.len;
  const int64_t cend = cbeg + a.p.ch.len < a.N ? cbeg + a.p.ch.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const float g2 = expf(2.f * a.theta[D]);
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const float* __restrict__ yg = a.y + g * (int64_t)a.N;
  const int Dl = D | 1;

  mo_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float cacc = 0.f, sw = 0.f, syy = 0.f;

  if constexpr (DIRECT) {
    for (int e = tid; e < T * D; e += 256) {
      const int r = e / D, d = e - r * D;
      stage[r * Dl + d] = i0 + r < Mt ? Zg[(int64_t)(i0 + r) * D + d] : 0.f;
      stage[T * kMoDl + r * Dl + d] = j0 + r < Mt ? Zg[(int64_t)(j0 + r) * D + d] : 0.f;
    }
    if (tid < D) wl[tid] = expf(-2.f * a.theta[tid]);
  }

  for (int64_t n0 = cbeg; n0 < cend; n0 += T) {
    if (tid < T) {
      const int64_t n = n0 + tid;
      float wv = 0.f, yv = 0.f;
      if (n < cend) { wv = wg ? wg[n] : 1.f; yv = yg[n]; }
      wn[tid] = wv;
      if constexpr (VW) {
        wyn[tid] = yv;
        sw += wv;
        syy += yv;
      } else {
        wyn[tid] = wv * yv;
        sw += wv;
        syy = fmaf(wv * yv, yv, syy);
      }
    }
    if constexpr (DIRECT) {
      float* Xs = stage + 2 * T * kMoDl;
      for (int e = tid; e < T * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[r * Dl + d] = n0 + r < cend ? X[(n0 + r) * D + d] : 0.f;
      }
      __syncthreads();
      // lanes = rows of the panel, the wave's 16 columns in registers; the point of X is a broadcast read
      for (int p = 0; p < (two ? 2 : 1); ++p) {
        const float* zr = stage + p * T * kMoDl + lane * Dl;
        const float* xr = Xs + 16 * wave * Dl;
        float d2[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) d2[q] = 0.f;
        for (int d = 0; d < D; ++d) {
          const float zv = zr[d], wv = wl[d];
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float v = zv - xr[q * Dl + d]; d2[q] = fmaf(wv * v, v, d2[q]); }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q)
          Ks[p][(16 * wave + q) * LD + lane] = n0 + 16 * wave + q < cend ? EPI::off(g2, d2[q]) : 0.f;
      }
    } else {
      float* Ai = stage;
      float* Aj = stage + BK * LD;
      float* Bs = stage + 2 * BK * LD;
      mo_f32x16 di, dj;
#pragma unroll
      for (int r = 0; r < 16; ++r) di[r] = dj[r] = 0.f;
      float nr = 0.f;
      const int k = tid & 31;
      for (int k0 = 0; k0 < D; k0 += BK) {
        const bool kok = k0 + k < D;
        const float sq = kok ? expf(-a.theta[k0 + k]) : 0.f;           // 1 / lengthscale
#pragma unroll
        for (int r = tid >> 5; r < T; r += 8) {
          Ai[k * LD + r] = (kok && i0 + r < Mt) ? sq * Zg[(int64_t)(i0 + r) * D + k0 + k] : 0.f;
          if (two) Aj[k * LD + r] = (kok && j0 + r < Mt) ? sq * Zg[(int64_t)(j0 + r) * D + k0 + k] : 0.f;
          Bs[k * LD + r] = (kok && n0 + r < cend) ? sq * X[(n0 + r) * D + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
          const float bf = Bs[(kk + h) * LD + wc + l31];
          di = __builtin_amdgcn_mfma_f32_32x32x2f32(Ai[(kk + h) * LD + wr + l31], bf, di, 0, 0, 0);
          if (two) dj = __builtin_amdgcn_mfma_f32_32x32x2f32(Aj[(kk + h) * LD + wr + l31], bf, dj, 0, 0, 0);
        }
        if (wave < 3 && (wave != 1 || two)) {
          const float* src = stage + wave * BK * LD + lane;
#pragma unroll
          for (int kk = 0; kk < BK; ++kk) { const float v = src[kk * LD]; nr = fmaf(v, v, nr); }
        }
        __syncthreads();
      }
      if (wave < 3) nrm[wave][lane] = nr;
      __syncthreads();
      // the wave's 32 x 32 block of each panel: rows wr.. of Z against the columns wc.. of X
      const int col = wc + l31;
      const bool cok = n0 + col < cend;
      const float nb = nrm[2][col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
        Ks[0][col * LD + row] = cok ? EPI::off(g2, nrm[0][row] + nb - 2.f * di[r]) : 0.f;
        if (two) Ks[1][col * LD + row] = cok ? EPI::off(g2, nrm[1][row] + nb - 2.f * dj[r]) : 0.f;
      }
    }
    __syncthreads();

    // the symmetric rank update of the step: acc += (K_i o w) K_j^T over the 64 columns
    const float* Ki = Ks[0];
    const float* Kj = Ks[two ? 1 : 0];
#pragma unroll
    for (int kk = 0; kk < T; kk += 2) {
      const int n = kk + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ki[n * LD + wr + l31] * wn[n], Kj[n * LD + wc + l31], acc, 0, 0, 0);
    }
    if (tj == 0) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s = fmaf(Ki[(16 * wave + q) * LD + lane], wyn[16 * wave + q], s);
      cacc += s;
    }
    __syncthreads();
  }

  const int64_t part = g * a.p.ch.nch + chunk;
  float* out = a.p.pphi + (part * ntri + t) * (T * T);
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(wr + (r & 3) + 8 * (r >> 2) + 4 * h) * T + wc + l31] = acc[r];
  if (tj == 0) {
    cred[wave * T + lane] = cacc;
    __syncthreads();
    if (tid < T) a.p.pc[part * a.p.nt * T + i0 + tid] = wave4_sum(cred, tid);
  }
  if (t == 0 && wave == 0) {
    sw = wave_sum(sw);
    syy = wave_sum(syy);
    if (lane == 0) { a.p.ps[part * 2] = sw; a.p.ps[part * 2 + 1] = syy; }
  }
}

// The chunks' partials in ascending chunk order, in fp64.  grid (ntri * 16 + cdiv(Mt, 256) + 1, G): 256 entries of a tile | 256
// entries of c | the two sums
__global__ __launch_bounds__(256) void moments_reduce_kernel(const MomArgs a) {
  constexpr int T = kMoT;
  const int Mt = a.Mt, ntri = a.p.ntri, nch = a.p.ch.nch;
  const int64_t g = blockIdx.y;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b < ntri * 16) {
    const int t = b >> 4, e = (b & 15) * 256 + tid;
    int ti, tj;
    mo_tile(t, ti, tj);
    const int i = ti * T + e / T, j = tj * T + e % T;
    if (i >= Mt || j > i) return;
    const float* p = a.p.pphi + ((g * nch) * ntri + t) * (int64_t)(T * T) + e;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * ntri * (T * T)];
    float* Phi = a.Phi + g * (int64_t)Mt * Mt;
    Phi[(int64_t)i * Mt + j] = (float)s;
    Phi[(int64_t)j * Mt + i] = (float)s;
  } else if (b < ntri * 16 + (Mt + 255) / 256) {
    const int i = (b - ntri * 16) * 256 + tid;
    if (i >= Mt) return;
    const float* p = a.p.pc + (g * nch) * (int64_t)(a.p.nt * T) + i;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * a.p.nt * T];
    a.c[g * Mt + i] = (float)s;
  } else if (tid < 2) {
    const float* p = a.p.ps + (g * nch) * 2 + tid;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[2 * q];
    a.sums[g * 2 + tid] = (float)s;
  }
}

template <class EPI, bool VW>
static void moments_launch(const MomArgs& a, hipStream_t st) {
  const dim3 grid(a.p.ntri * a.p.ch.nch, a.G), blk(256);
  if (a.D <= kRbfDirectD) hipLaunchKernelGGL((moments_kernel<EPI, true, VW>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((moments_kernel<EPI, false, VW>), grid, blk, 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The backward of the pass, for theta and Z (X, w and y get no gradient).  Given gPhi [G][Mt][Mt] (ANY matrix, not symmetric) and
// gc [G][Mt], in the notation of gram.hip's header:
//   S = gPhi + gPhi^T,  gK = (S K + gc y^T) diag(w),  V = gK o (-2 dk/dd2)   (Mt x N, neither ever reaches global memory)
//   r = V 1,  cn = V^T 1,  P = V X,  q_d = sum_n cn_n x_nd^2
//   gZ_i = -wl o (r_i z_i - P_i),   gtheta_d = wl_d [sum_i z_id (r_i z_id - 2 P_id) + q_d]  (d < D; entry D is the caller's).
// A pre-launch writes S to the workspace.  A workgroup owns (output g, 64-row panel i of Z, chunk of N, group of 64 NP values of
// d) and walks its chunk 64 columns at a time.  Per step, for EVERY panel j: K_j is built in LDS as the forward builds it (the
// panel j == i also leaves its weight -2 dk/dd2), the tile S_ij is staged as [k][row], and 32 v_mfma_f32_32x32x2_f32 per wave add
// S_ij K_j to the 64 x 64 accumulators of gK_i (four waves as 2 x 2).  Then V_i = (gK_i o w + gc_i (w y)^T) o weight overwrites the
// weight in LDS; r_i and the panel's share of cn come from it by plain sums, and P_i += V_i X on the same MFMA, the step's 64 rows
// of X staged 64 values of d at a time (the four waves as 2 row halves x 2 halves of the 64 values; NP accumulator tiles per wave
// stay in registers for the whole chunk).  q's share rides on the staged X.  D > 64 NP: the grid is split over groups of d and
// every group recomputes V (group 0 alone writes r).
// The forward's contract holds: columns behind the end of the chunk are masked (guarded loads, K and weight written as zeros); a
// zero weight multiplies finite numbers; no atomics; a last launch adds the chunks' partials of r, P and q in ascending chunk
// order in fp64, forms gZ and gtheta there and rounds once.  The chunking (mom_bwd_plan) depends on the shapes alone: as the
// forward's, and capped so that the partials of P stay below kMoBwdBudget bytes.
constexpr int kMoBwdNPMax = 7;                  // accumulator tiles of P per wave: 64 * 7 = 448 values of d per group
constexpr size_t kMoBwdBudget = 64u << 20;      // bytes of the per-chunk partials of r and P, at most (one chunk always fits)

struct MomBwdPlan {
  int nt, np, ngrp;          // panels, P tiles per wave, groups of d
  Chunks ch;                 // ch.nch chunks of ch.len columns
  float *S, *pr, *pp, *pq;   // S [G][Mt][Mt]; partials r [G][nch][nt][64], P [G][nch][nt][64][D], q [G][nch][nt][D]
  size_t bytes;
};

static MomBwdPlan mom_bwd_plan(void* ws, int G, int Mt, int N, int D) {
  MomBwdPlan o{};
  o.nt = cdiv(Mt, kMoT);
  o.np = D <= 64 ? 1 : (D <= 128 ? 2 : kMoBwdNPMax);
  o.ngrp = cdiv(D, 64 * o.np);
  const int64_t per = (int64_t)G * o.nt * kMoT * (D + 1) * (int64_t)sizeof(float);
  o.ch = chunk_rule(N, (int64_t)G * o.nt * o.ngrp, (int64_t)kMoBwdBudget / per);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.S = take((int64_t)G * Mt * Mt);
  o.pr = take((int64_t)G * o.ch.nch * o.nt * kMoT);
  o.pp = take((int64_t)G * o.ch.nch * o.nt * kMoT * D);
  o.pq = take((int64_t)G * o.ch.nch * o.nt * D);
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

struct MomBwdArgs {
  const float *theta, *Z, *X, *w, *y, *gPhi, *gc;
  float *gZ, *gtheta;
  MomBwdPlan p;
  int G, Mt, N, D;
};

// S = gPhi + gPhi^T.  grid (cdiv(Mt * Mt, 256), G)
__global__ __launch_bounds__(256) void moments_bwd_sym_kernel(const MomBwdArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, mm = (int64_t)a.Mt * a.Mt;
  if (e >= mm) return;
  const int i = (int)(e / a.Mt), j = (int)(e - (int64_t)i * a.Mt);
  const float* gp = a.gPhi + blockIdx.y * mm;
  a.p.S[blockIdx.y * mm + e] = gp[e] + gp[(int64_t)j * a.Mt + i];
}

// grid ((nch * nt + panel) * ngrp + group, G)
template <class EPI, bool DIRECT, int NP>
__global__ __launch_bounds__(256) void moments_bwd_kernel(const MomBwdArgs a) {
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  __shared__ float Ks[T * LD];                                   // K_j of the step: [n][m]
  __shared__ float Vs[T * LD];                                   // the weight of panel i, then V_i: [n][m]
  __shared__ float Ss[T * LD];                                   // S_ij: [k = row of panel j][row of panel i]; then X of the step: [n][d]
  __shared__ float stage[DIRECT ? 2 * T * kMoDl : 2 * BK * LD];  // DIRECT: Z_j, X rows; else the slabs of a_j, b: [k][r]
  __shared__ float wl[kRbfDirectD];
  __shared__ float wn[T], wyn[T], gci[T], cn[T];
  __shared__ float nrm[2][T];                                    // !DIRECT: |a_j|^2, |b|^2
  __shared__ float cred[4 * T];

  const int Mt = a.Mt, D = a.D, nt = a.p.nt, ngrp = a.p.ngrp;
  const int grp = blockIdx.x % ngrp, pc = blockIdx.x / ngrp;
  const int chunk = pc / nt, ti = pc - chunk * nt;
  const int i0 = ti * T, dg0 = grp * 64 * NP;
  const int64_t g = blockIdx.y;
  const int64_t cbeg = (int64_t)chunk * a.p.ch.len;
  const int64_t cend = cbeg + a.p.ch.len < a.N ? cbeg + a.p.ch.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const float g2 = expf(2.f * a.theta[D]);
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ Sg = a.p.S + g * (int64_t)Mt * Mt;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const float* __restrict__ yg = a.y + g * (int64_t)a.N;
  const int Dl = D | 1;

  mo_f32x16 pacc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) pacc[p][r] = 0.f;
  float qacc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) qacc[p] = 0.f;
  float racc = 0.f;

  if (tid < T) gci[tid] = i0 + tid < Mt ? a.gc[g * Mt + i0 + tid] : 0.f;
  if constexpr (DIRECT) {
    if (tid < D) wl[tid] = expf(-2.f * a.theta[tid]);
  }

  for (int64_t n0 = cbeg; n0 < cend; n0 += T) {
    if (tid < T) {
      const int64_t n = n0 + tid;
      float wv = 0.f, yv = 0.f;
      if (n < cend) { wv = wg ? wg[n] : 1.f; yv = yg[n]; }
      wn[tid] = wv;
      wyn[tid] = wv * yv;
    }
    if constexpr (DIRECT) {
      float* Xs = stage + T * kMoDl;
      for (int e = tid; e < T * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[r * Dl + d] = n0 + r < cend ? X[(n0 + r) * D + d] : 0.f;
      }
    }
    mo_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int tj = 0; tj < nt; ++tj) {
      const int j0 = tj * T;
      const bool own = tj == ti;
      // S_ij as [k][row]: rows and columns behind Mt are zeros, so the padding rows of either panel add nothing
      for (int e = tid; e < T * T; e += 256) {
        const int r = e >> 6, k = e & 63;
        Ss[k * LD + r] = (i0 + r < Mt && j0 + k < Mt) ? Sg[(int64_t)(i0 + r) * Mt + j0 + k] : 0.f;
      }
      if constexpr (DIRECT) {
        const float* Xs = stage + T * kMoDl;
        for (int e = tid; e < T * D; e += 256) {
          const int r = e / D, d = e - r * D;
          stage[r * Dl + d] = j0 + r < Mt ? Zg[(int64_t)(j0 + r) * D + d] : 0.f;
        }
        __syncthreads();
        const float* zr = stage + lane * Dl;
        const float* xr = Xs + 16 * wave * Dl;
        float d2[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) d2[q] = 0.f;
        for (int d = 0; d < D; ++d) {
          const float zv = zr[d], wv = wl[d];
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float v = zv - xr[q * Dl + d]; d2[q] = fmaf(wv * v, v, d2[q]); }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const bool ok = n0 + 16 * wave + q < cend;
          Ks[(16 * wave + q) * LD + lane] = ok ? EPI::off(g2, d2[q]) : 0.f;
          if (own) Vs[(16 * wave + q) * LD + lane] = ok ? EpiDk<EPI>::w(g2, d2[q]) : 0.f;
        }
      } else {
        float* Aj = stage;
        float* Bs = stage + BK * LD;
        mo_f32x16 dj;
#pragma unroll
        for (int r = 0; r < 16; ++r) dj[r] = 0.f;
        float nr = 0.f;
        const int k = tid & 31;
        for (int k0 = 0; k0 < D; k0 += BK) {
          const bool kok = k0 + k < D;
          const float sq = kok ? expf(-a.theta[k0 + k]) : 0.f;           // 1 / lengthscale
#pragma unroll
          for (int r = tid >> 5; r < T; r += 8) {
            Aj[k * LD + r] = (kok && j0 + r < Mt) ? sq * Zg[(int64_t)(j0 + r) * D + k0 + k] : 0.f;
            Bs[k * LD + r] = (kok && n0 + r < cend) ? sq * X[(n0 + r) * D + k0 + k] : 0.f;
          }
          __syncthreads();
#pragma unroll
          for (int kk = 0; kk < BK; kk += 2)
            dj = __builtin_amdgcn_mfma_f32_32x32x2f32(Aj[(kk + h) * LD + wr + l31], Bs[(kk + h) * LD + wc + l31], dj, 0, 0, 0);
          if (wave < 2) {
            const float* src = stage + wave * BK * LD + lane;
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) { const float v = src[kk * LD]; nr = fmaf(v, v, nr); }
          }
          __syncthreads();
        }
        if (wave < 2) nrm[wave][lane] = nr;
        __syncthreads();
        const int col = wc + l31;
        const bool cok = n0 + col < cend;
        const float nb = nrm[1][col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float d2 = nrm[0][row] + nb - 2.f * dj[r];
          Ks[col * LD + row] = cok ? EPI::off(g2, d2) : 0.f;
          if (own) Vs[col * LD + row] = cok ? EpiDk<EPI>::w(g2, d2) : 0.f;
        }
      }
      __syncthreads();
      // gK_i += S_ij K_j: A = S_ij [row][k], B = K_j [k][n]
      acc = sk_tile(acc, Ss, Ks, LD, wr + l31, wc + l31, h);
      __syncthreads();
    }

    // V_i = (gK_i o w + gc_i (w y)^T) o weight, in place; a masked column has weight 0 and w 0
    {
      const int col = wc + l31;
      const float wv = wn[col], wy = wyn[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
        Vs[col * LD + row] = fmaf(acc[r], wv, gci[row] * wy) * Vs[col * LD + row];
      }
    }
    __syncthreads();
    {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += Vs[(16 * wave + q) * LD + lane];
      racc += s;
      // cn of the step: four threads per column, 16 rows each
      const int n = tid >> 2, qd = tid & 3;
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += Vs[n * LD + 16 * qd + q];
      cred[qd * T + n] = t;
    }
    __syncthreads();
    if (tid < T) cn[tid] = wave4_sum(cred, tid);

    // P_i += V_i X, 64 values of d at a time; waves as (row half, half of the 64 values)
    const int pr = (wave & 1) * 32, pd = (wave >> 1) * 32;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c0 = dg0 + p * 64;
      if (c0 < D) {
        for (int e = tid; e < T * T; e += 256) {
          const int n = e >> 6, c = e & 63;
          Ss[n * LD + c] = (n0 + n < cend && c0 + c < D) ? X[(n0 + n) * D + c0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < T; kk += 2)
          pacc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(kk + h) * LD + pr + l31], Ss[(kk + h) * LD + pd + l31], pacc[p], 0, 0, 0);
        {
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float xv = Ss[(16 * wave + q) * LD + lane]; s = fmaf(cn[16 * wave + q] * xv, xv, s); }
          qacc[p] += s;
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }

  const int64_t part = (g * a.p.ch.nch + chunk) * nt + ti;
  {
    const int pr = (wave & 1) * 32, pd = (wave >> 1) * 32;
    float* out = a.p.pp + part * T * D;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d = dg0 + p * 64 + pd + l31;
      if (d < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(pr + (r & 3) + 8 * (r >> 2) + 4 * h) * D + d] = pacc[p][r];
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    __syncthreads();
    cred[wave * T + lane] = qacc[p];
    __syncthreads();
    const int d = dg0 + p * 64 + tid;
    if (tid < T && d < D) a.p.pq[part * D + d] = wave4_sum(cred, tid);
  }
  if (grp == 0) {
    __syncthreads();
    cred[wave * T + lane] = racc;
    __syncthreads();
    if (tid < T) a.p.pr[part * T + tid] = wave4_sum(cred, tid);
  }
}

// The chunks' partials in ascending chunk order in fp64, then gZ and gtheta.  grid (cdiv(G * Mt * D, 256) + D): 256 entries of gZ
// | one value of d of gtheta (every thread a strided share of the (g, row) pairs and of the partials of q, then a fixed tree)
__global__ __launch_bounds__(256) void moments_bwd_reduce_kernel(const MomBwdArgs a) {
  constexpr int T = kMoT;
  __shared__ double red[256];
  const int Mt = a.Mt, D = a.D, nt = a.p.nt, nch = a.p.ch.nch, tid = threadIdx.x;
  const int64_t total = (int64_t)a.G * Mt * D;
  const int nz = (int)((total + 255) / 256);
  const BwdPartials b{a.p.pr, a.p.pp, a.p.pq, nch, nt * T, nt};
  if ((int)blockIdx.x < nz) {
    const int64_t e = (int64_t)blockIdx.x * 256 + tid;
    if (e < total) gz_entry(b, a.theta, a.Z, a.gZ, e, Mt, D);
    return;
  }
  gtheta_d_block(b, a.theta, a.Z, a.gtheta, red, blockIdx.x - nz, a.G, Mt, D);
}

template <class EPI>
static void moments_bwd_launch(const MomBwdArgs& a, hipStream_t st) {
  const dim3 grid(a.p.ch.nch * a.p.nt * a.p.ngrp, a.G), blk(256);
  if (a.D <= kRbfDirectD) hipLaunchKernelGGL((moments_bwd_kernel<EPI, true, 1>), grid, blk, 0, st, a);
  else if (a.p.np == 1) hipLaunchKernelGGL((moments_bwd_kernel<EPI, false, 1>), grid, blk, 0, st, a);
  else if (a.p.np == 2) hipLaunchKernelGGL((moments_bwd_kernel<EPI, false, 2>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((moments_bwd_kernel<EPI, false, kMoBwdNPMax>), grid, blk, 0, st, a);
}

}  // namespace vargp

using namespace vargp;

extern "C" int vargp_gram_moments_bwd_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_bwd_plan(nullptr, G, Mt, N, D).ch.nch;
}

extern "C" size_t vargp_gram_moments_bwd_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_bwd_plan(nullptr, G, Mt, N, D).bytes + 256;
}

extern "C" int vargp_gram_moments_bwd(const float* theta, const float* Z, const float* X, const float* w, const float* y,
                                      const float* gPhi, const float* gc, float* gZ, float* gtheta, int G, int Mt, int N, int D,
                                      int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && Z && X && y && gPhi && gc && gZ && gtheta && ws, "gram_moments_bwd: null pointer");
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "gram_moments_bwd: bad dims");
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "gram_moments_bwd: nu2 = %d (0: RBF; 1, 3, 5: Matern)", nu2);
  VARGP_REQUIRE(G <= 65535, "gram_moments_bwd: G = %d (at most 65535)", G);
  VARGP_REQUIRE(ws_bytes >= vargp_gram_moments_bwd_workspace_bytes(G, Mt, N, D), "gram_moments_bwd: workspace too small");
  MomBwdArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.w = w; a.y = y; a.gPhi = gPhi; a.gc = gc; a.gZ = gZ; a.gtheta = gtheta;
  a.p = mom_bwd_plan(ws, G, Mt, N, D);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  VARGP_REQUIRE((int64_t)a.p.ch.nch * a.p.nt * a.p.ngrp < (1ll << 31) && (int64_t)G * Mt * D / 256 + D < (1ll << 31) - 1,
                "gram_moments_bwd: Mt = %d, D = %d need too many workgroups", Mt, D);
  hipStream_t st = as_stream(stream);
  ProfScope whole("gram_moments_bwd", st);
  hipLaunchKernelGGL(moments_bwd_sym_kernel, dim3(cdiv((int64_t)Mt * Mt, 256), G), dim3(256), 0, st, a);
  with_epi(nu2, [&](auto epi) { moments_bwd_launch<decltype(epi)>(a, st); });
  hipLaunchKernelGGL(moments_bwd_reduce_kernel, dim3(cdiv((int64_t)G * Mt * D, 256) + D), dim3(256), 0, st, a);
  return check_launch("gram_moments_bwd");
}

extern "C" int vargp_gram_moments_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_plan(nullptr, G, Mt, N).ch.nch;
}

extern "C" size_t vargp_gram_moments_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_plan(nullptr, G, Mt, N).bytes + 256;
}

// both forward entries: y is the targets (VW = false) or the weight vector v of c (VW = true)
template <bool VW>
static int moments_entry(const char* name, const float* theta, const float* Z, const float* X, const float* w, const float* y,
                         float* Phi, float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes,
                         vargp_stream_t stream) {
  VARGP_REQUIRE(theta && Z && X && y && Phi && c && sums && ws, "%s: null pointer", name);
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "%s: bad dims", name);
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "%s: nu2 = %d (0: RBF; 1, 3, 5: Matern)", name, nu2);
  VARGP_REQUIRE(G <= 65535, "%s: G = %d (at most 65535)", name, G);
  VARGP_REQUIRE(ws_bytes >= vargp_gram_moments_workspace_bytes(G, Mt, N, D), "%s: workspace too small", name);
  MomArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.w = w; a.y = y; a.Phi = Phi; a.c = c; a.sums = sums;
  a.p = mom_plan(ws, G, Mt, N);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  VARGP_REQUIRE((int64_t)a.p.ntri * a.p.ch.nch < (1ll << 31), "%s: Mt = %d needs too many tiles", name, Mt);
  hipStream_t st = as_stream(stream);
  ProfScope whole(name, st);
  with_epi(nu2, [&](auto epi) { moments_launch<decltype(epi), VW>(a, st); });
  hipLaunchKernelGGL(moments_reduce_kernel, dim3(a.p.ntri * 16 + cdiv(Mt, 256) + 1, G), dim3(256), 0, st, a);
  return check_launch(name);
}

extern "C" int vargp_gram_moments(const float* theta, const float* Z, const float* X, const float* w, const float* y, float* Phi,
                                  float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes,
                                  vargp_stream_t stream) {
  return moments_entry<false>("gram_moments", theta, Z, X, w, y, Phi, c, sums, G, Mt, N, D, nu2, ws, ws_bytes, stream);
}

extern "C" int vargp_gram_moments_v(const float* theta, const float* Z, const float* X, const float* w, const float* v, float* Phi,
                                    float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes,
                                    vargp_stream_t stream) {
  return moments_entry<true>("gram_moments_v", theta, Z, X, w, v, Phi, c, sums, G, Mt, N, D, nu2, ws, ws_bytes, stream);
}
