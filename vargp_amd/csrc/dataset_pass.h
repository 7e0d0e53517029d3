// What the fused passes over a whole data set share: moments.hip (weighted moments of the cross-kernel and their backward) and
// sites.hip (Gaussian sites of a non-Gaussian likelihood and the backward of their bound).  Every such pass is 256 threads (four
// waves) walking a chunk of N 64 columns at a time, with 64-row panels of K(Z, X) in LDS as [column][row]; a last launch adds the
// chunks' partials in ascending chunk order in fp64.  Here, ONCE: the tiling constants; chunk_rule, the rule that cuts N into
// chunks from the shapes alone; with_epi, the dispatch on the kernel family; EpiDk, the weight -2 dk/dd2 of an epilogue;
// wave4_sum, the order in which the four waves' shares are added; sk_tile, a staged 64 x 64 tile times a panel of K on the MFMA
// (the accumulator goes through it BY VALUE: by reference it cost up to 44 VGPRs and a wave of occupancy); and the fp64 tail
// that forms gZ and gtheta_d in the two backward reductions.  The K-panel builders and the V X step stay written out in each
// kernel: DESIGN.md, "What the data-set passes share", says why.
#pragma once
#include "common.h"

namespace vargp {

constexpr int kMoT = 64;               // tile side of Phi = rows of a panel = columns of X per step
constexpr int kSiMaxMt = 4 * kMoT;     // sites.hip holds the K block of ALL Mt rows x kMoT columns in LDS: Mt above this has no fused pass
constexpr int kMoLD = kMoT + 1;
constexpr int kMoBK = 32;              // values of d per slab (D > kRbfDirectD)
constexpr int kMoDl = kRbfDirectD | 1; // row stride of the staged points (direct form)
constexpr int kMoTargetWg = 1024;
constexpr int kMoMinChunk = 256;
constexpr int kMoMaxChunks = 1024;

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The chunking of all four passes: at most kMoMaxChunks chunks of at least kMoMinChunk columns (a multiple of kMoT each), as many
// as give a launch of wg_per_chunk workgroups per chunk about kMoTargetWg workgroups, and at most `fit` of them (a workspace
// budget; one chunk always fits).
struct Chunks {
  int64_t len;               // columns per chunk
  int nch;
};
static inline Chunks chunk_rule(int N, int64_t wg_per_chunk, int64_t fit = kMoMaxChunks) {
  int64_t want = cdiv(kMoTargetWg, wg_per_chunk);
  const int64_t most = cdiv(N, kMoMinChunk);
  want = want < most ? want : most;
  want = want < fit ? want : fit;
  want = want < 1 ? 1 : (want > kMoMaxChunks ? kMoMaxChunks : want);
  Chunks o{};
  o.len = round_up(cdiv(N, want), kMoT);
  o.nch = cdiv(N, o.len);
  return o;
}

// f(EPI{}) for the epilogue that a (checked) nu2 names
template <class F>
static auto with_epi(int nu2, F f) {
  switch (nu2) {
    case 0: return f(EpiRbf{});
    case 1: return f(EpiMatern<1>{});
    case 3: return f(EpiMatern<3>{});
    default: return f(EpiMatern<5>{});
  }
}

// ---- device -------------------------------------------------------------------------------------------------------------------------
// -2 dk/dd2 of an epilogue: the RBF's is K itself, the Matern's matern_w
template <class EPI> struct EpiDk;
template <> struct EpiDk<EpiRbf> {
  static __device__ __forceinline__ float w(float g2, float d2) { return EpiRbf::off(g2, d2); }
};
template <int NU2> struct EpiDk<EpiMatern<NU2>> {
  static __device__ __forceinline__ float w(float g2, float d2) { return matern_w<NU2>(g2, d2); }
};

// the four waves' shares of 64 values, cred [4][64], added in the one order every pass uses
__device__ __forceinline__ float wave4_sum(const float* cred, int i) {
  return (cred[i] + cred[kMoT + i]) + (cred[2 * kMoT + i] + cred[3 * kMoT + i]);
}

typedef float dp_f32x16 __attribute__((ext_vector_type(16)));

// acc + S K_j, 32 MFMA per wave (the four waves as 2 x 2 blocks of 32 x 32): a 64 x 64 tile staged as Ss [k][row] (stride
// kMoLD) times the 64 rows of K at Kj [column * ldk + k]; row and col are the lane's of the wave's block, h = lane >> 5
__device__ __forceinline__ dp_f32x16 sk_tile(dp_f32x16 acc, const float* Ss, const float* Kj, int ldk, int row, int col, int h) {
#pragma unroll
  for (int kk = 0; kk < kMoT; kk += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ss[(kk + h) * kMoLD + row], Kj[col * ldk + kk + h], acc, 0, 0, 0);
  return acc;
}

// ---- the fp64 tail of a backward: gZ and gtheta_d from the chunks' partials ---------------------------------------------------------
// pr [G][nch][MtP], pp [G][nch][MtP][D], pq [G][nch][nq][D], MtP = 64 nt; the chunks are added in ascending order
struct BwdPartials {
  const float *pr, *pp, *pq;
  int nch, MtP, nq;
};
__device__ __forceinline__ void bwd_r_p(const BwdPartials& b, int64_t g, int m, int d, int D, double& r, double& P) {
  const int64_t at = g * b.nch * b.MtP + m;
  r = 0.0; P = 0.0;
  for (int q = 0; q < b.nch; ++q) {
    r += (double)b.pr[at + (int64_t)q * b.MtP];
    P += (double)b.pp[(at + (int64_t)q * b.MtP) * D + d];
  }
}
// a fixed tree over the 256 threads' values (red: 256 doubles of LDS); the sum in every thread
__device__ __forceinline__ double block_tree_sum(double* red, double s) {
  const int tid = threadIdx.x;
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}
// gZ[e] = -wl_d (r_i z_id - P_id), e over [G][Mt][D]
__device__ __forceinline__ void gz_entry(const BwdPartials& b, const float* theta, const float* Z, float* gZ, int64_t e, int Mt,
                                         int D) {
  const int d = (int)(e % D);
  const int64_t gm = e / D;
  double r, P;
  bwd_r_p(b, gm / Mt, (int)(gm % Mt), d, D, r, P);
  gZ[e] = (float)(-exp(-2.0 * (double)theta[d]) * (r * (double)Z[e] - P));
}
// gtheta_d = wl_d [sum_(g, i) z_id (r_i z_id - 2 P_id) + sum q_d] by one workgroup: every thread a strided share of the (g, row)
// pairs and of the partials of q, then the tree
__device__ __forceinline__ void gtheta_d_block(const BwdPartials& b, const float* theta, const float* Z, float* gtheta, double* red,
                                               int d, int G, int Mt, int D) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t gm = tid; gm < (int64_t)G * Mt; gm += 256) {
    double r, P;
    bwd_r_p(b, gm / Mt, (int)(gm % Mt), d, D, r, P);
    const double z = (double)Z[gm * D + d];
    s += z * (r * z - 2.0 * P);
  }
  for (int64_t e = tid; e < (int64_t)G * b.nch * b.nq; e += 256) s += (double)b.pq[e * D + d];
  s = block_tree_sum(red, s);
  if (tid == 0) gtheta[d] = (float)(exp(-2.0 * (double)theta[d]) * s);
}

}  // namespace vargp
