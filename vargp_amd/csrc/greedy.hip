// Greedy conditional-variance selection of inducing points: a pivoted Cholesky of K(X_cand, X_cand) (Burt et al., JMLR 2020) for
// G independent candidate sets over ONE data matrix X [N][D] and ONE hyper vector -- nothing of this is in the reference.  Per set,
// M times: pick the unselected candidate with the largest residual variance d, form its Cholesky column over all candidates,
//   c_i = k(x_i, x_p) - sum_j LT[j][i] LT[j][p],   LT[r][i] = c_i / sqrt(d_p),   d_i = max(d_i - LT[r][i]^2, 0),
// and mark it.  The factorisation may start from k0 rows the caller supplies (the previous tasks' inducing points, init.py).
//
// One launch per step, M + 1 launches per call, nothing returns to the host between them, and no workgroup ever waits for
// another inside a launch: the set-wide argmax is split over the kernel boundary.  A workgroup owns a tile of kGrTile candidates
// of one set.  At its END it writes its tile's best (key, position, d) to a table; at its START the workgroup of the next
// step reduces that table -- cdiv(Nc, kGrTile) entries, every workgroup of the set redundantly -- and so knows the pivot.  The
// table is double-buffered by step parity: step k reads half k & 1 while it writes half (k + 1) & 1.  The pivot's d comes from
// the table, never from d[] itself, which the tile that owns the pivot rewrites during the same launch.
//   key_i = -1 for a selected candidate, else d_i if d_i > eps, else 0;   larger key wins, the lower position on a tie.
// A pivot with d_p <= eps means the set is exhausted: the row is written as zeros and d is left alone.
//
// Layout: LT [G][k0 + M][Nc] is k-major, so the downdate reads LT[j][i] coalesced along i (lanes = candidates, the four waves
// take j mod 4 and their partial sums are added in a fixed order) and the new row is one contiguous store.  The kernel column
// k(x_i, x_p): one wave per candidate row, lanes along d (16 bytes per lane when D % 4 == 0 and X is 16-byte aligned), four
// rows in flight per wave, the distance formed directly as sum_d w_d (x_id - x_pd)^2, w_d = exp(-2 theta_d) -- the arithmetic
// of gram.hip's direct form at every D, so coincident points get exactly gamma^2.  The pivot's row, w and LT[:, p] are staged
// in LDS once per workgroup (up to kGrCapD values of d and kGrCapR rows; beyond that they are read through the caches).
// Deterministic: no atomics, every sum in an order fixed by the shapes alone.  Every load is guarded: any Nc, D, M >= 1.
#include <limits.h>
#include "common.h"

namespace vargp {

constexpr int kGrTile = 64;          // candidates per workgroup: the lanes of one wave in the downdate
constexpr int kGrCapD = 4096;        // values of d of the pivot row and of w held in LDS
constexpr int kGrCapR = 2048;        // entries of LT[:, p] held in LDS

struct GreedyWs {
  float *w, *tkey, *td;       // w [Dp]; table [2][G][ntiles]: key and d of each tile's best ...
  int32_t *tpos, *mask;       // ... and its position; mask [G][Nc]: 1 = selected
  int ntiles;
  size_t bytes;
};

static GreedyWs greedy_carve(void* ws, int G, int Nc, int D) {
  GreedyWs o{};
  o.ntiles = cdiv(Nc, kGrTile);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  const int64_t nt = (int64_t)2 * G * o.ntiles;
  o.w = take(round_up(D, 4));
  o.tkey = take(nt);
  o.td = take(nt);
  o.tpos = reinterpret_cast<int32_t*>(take(nt));
  o.mask = reinterpret_cast<int32_t*>(take((int64_t)G * Nc));
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

struct GreedyArgs {
  const float *theta, *X;
  const int32_t* cand;
  float *LT, *d;
  int32_t* pick;
  float* pivot;
  GreedyWs ws;
  int G, Nc, N, D, k0, M;
  float eps;
};

// (key, pos, d) <- the better of it and (ok, op, od): the larger key, the lower position on a tie
__device__ __forceinline__ void gr_take(float& key, int& pos, float& d, float ok, int op, float od) {
  if (ok > key || (ok == key && op < pos)) { key = ok; pos = op; d = od; }
}
__device__ __forceinline__ void gr_wave_best(float& key, int& pos, float& d) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ok = __shfl_xor(key, off, 64), od = __shfl_xor(d, off, 64);
    const int op = __shfl_xor(pos, off, 64);
    gr_take(key, pos, d, ok, op, od);
  }
}
// the row of X behind position i of set g; row numbers outside [0, N) are clamped into it (no load leaves X)
__device__ __forceinline__ int64_t gr_row(const GreedyArgs& a, int64_t g, int i) {
  const int r = a.cand ? a.cand[g * a.Nc + i] : i;
  return r < 0 ? 0 : (r >= a.N ? a.N - 1 : r);
}
// the key of candidate i after this step and the tile's entry of the next step's table (wave 0: lanes = the tile's candidates)
__device__ __forceinline__ void gr_publish(const GreedyArgs& a, int64_t g, int i, bool selected, float dv, int half) {
  float key = -2.f, bd = 0.f;
  int pos = INT_MAX;
  if (i < a.Nc) {
    key = selected ? -1.f : (dv > a.eps ? dv : 0.f);
    pos = i;
    bd = dv;
  }
  gr_wave_best(key, pos, bd);
  if ((threadIdx.x & 63) == 0) {
    const int64_t e = ((int64_t)half * a.G + g) * a.ws.ntiles + blockIdx.x;
    a.ws.tkey[e] = key;
    a.ws.tpos[e] = pos;
    a.ws.td[e] = bd;
  }
}

// Launch 0: w = exp(-2 theta) for the steps, the mask cleared, d = gamma^2 when the factorisation starts empty, and the
// table of step 0.  grid (ntiles, G)
__global__ __launch_bounds__(256) void greedy_init_kernel(const GreedyArgs a) {
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.y;
  if (blockIdx.x == 0 && g == 0)
    for (int d = tid; d < ((a.D + 3) & ~3); d += 256) a.ws.w[d] = d < a.D ? expf(-2.f * a.theta[d]) : 0.f;
  if (tid >= kGrTile) return;
  const int i = blockIdx.x * kGrTile + tid;
  float dv = 0.f;
  if (i < a.Nc) {
    a.ws.mask[g * a.Nc + i] = 0;
    if (a.k0 == 0) a.d[g * a.Nc + i] = dv = expf(2.f * a.theta[a.D]);
    else dv = a.d[g * a.Nc + i];
  }
  gr_publish(a, g, i, false, dv, 0);
}

// d2 of four candidate rows against the pivot row: lanes along d, the lane's share only (the caller sums over the wave)
template <bool VEC>
__device__ __forceinline__ void gr_dist4(const float* const (&row)[4], const float* xp, const float* w, int D, int lane, float (&acc)[4]) {
  if constexpr (VEC) {
    const float4* xp4 = reinterpret_cast<const float4*>(xp);
    const float4* w4 = reinterpret_cast<const float4*>(w);
    for (int q = lane; q < D / 4; q += 64) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = row[u] ? reinterpret_cast<const float4*>(row[u])[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 p = xp4[q], ww = w4[q];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = v[u].x - p.x; acc[u] = fmaf(ww.x * t, t, acc[u]);
        t = v[u].y - p.y; acc[u] = fmaf(ww.y * t, t, acc[u]);
        t = v[u].z - p.z; acc[u] = fmaf(ww.z * t, t, acc[u]);
        t = v[u].w - p.w; acc[u] = fmaf(ww.w * t, t, acc[u]);
      }
    }
  } else {
    for (int q = lane; q < D; q += 64) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = row[u] ? row[u][q] : 0.f;
      const float p = xp[q], ww = w[q];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const float t = v[u] - p; acc[u] = fmaf(ww * t, t, acc[u]); }
    }
  }
}

// Step k: grid (ntiles, G), dynamic LDS = (2 Dl + Rl) floats, Dl = min(round_up(D, 4), kGrCapD), Rl = min(k0 + M, kGrCapR)
template <class EPI, bool VEC>
__global__ __launch_bounds__(256) void greedy_step_kernel(const GreedyArgs a, const int k) {
  extern __shared__ float4 gr_smem4[];
  __shared__ float part[4][kGrTile];
  __shared__ float kcol[kGrTile];
  __shared__ float rkey[4], rd[4];
  __shared__ int rpos[4];

  const int Nc = a.Nc, D = a.D, R = a.k0 + a.M, r = a.k0 + k;
  const int ntiles = a.ws.ntiles;
  const int64_t g = blockIdx.y;
  const int i0 = blockIdx.x * kGrTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the pivot: the best entry of the table the previous launch left
  float key = -2.f, dp = 0.f;
  int p = INT_MAX;
  {
    const int64_t e0 = ((int64_t)(k & 1) * a.G + g) * ntiles;
    for (int t = tid; t < ntiles; t += 256) gr_take(key, p, dp, a.ws.tkey[e0 + t], a.ws.tpos[e0 + t], a.ws.td[e0 + t]);
    gr_wave_best(key, p, dp);
    if (lane == 0) { rkey[wave] = key; rpos[wave] = p; rd[wave] = dp; }
    __syncthreads();
    key = rkey[0]; p = rpos[0]; dp = rd[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) gr_take(key, p, dp, rkey[q], rpos[q], rd[q]);
    p = p < 0 ? 0 : (p >= Nc ? Nc - 1 : p);          // (M <= Nc: an unselected candidate exists; the clamp guards the loads)
  }
  const bool go = dp > a.eps;
  float* LTg = a.LT + g * (int64_t)R * Nc;
  float* dg = a.d + g * Nc;

  if (go) {
    const int Dl = (D + 3) & ~3;
    const bool d_lds = Dl <= kGrCapD, r_lds = R <= kGrCapR;
    float* sm = reinterpret_cast<float*>(gr_smem4);
    float* xp_s = sm;
    float* w_s = sm + (d_lds ? Dl : 0);
    float* col_s = sm + (d_lds ? 2 * Dl : 0);
    const float* xp_g = a.X + gr_row(a, g, p) * D;
    if (d_lds)
      for (int q = tid; q < Dl; q += 256) { xp_s[q] = q < D ? xp_g[q] : 0.f; w_s[q] = a.ws.w[q]; }
    if (r_lds)
      for (int j = tid; j < r; j += 256) col_s[j] = LTg[(int64_t)j * Nc + p];
    __syncthreads();

    // the kernel column of the tile: wave `wave` takes the rows 16 wave .. 16 wave + 15, four at a time
    const float g2 = expf(2.f * a.theta[D]);
#pragma unroll 1
    for (int q = 0; q < 16; q += 4) {
      const float* row[4];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 16 * wave + q + u;
        row[u] = i < Nc ? a.X + gr_row(a, g, i) * D : nullptr;
      }
      if (d_lds) gr_dist4<VEC>(row, xp_s, w_s, D, lane, acc);
      else gr_dist4<VEC>(row, xp_g, a.ws.w, D, lane, acc);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float d2 = wave_sum(acc[u]);
        if (lane == 0) kcol[16 * wave + q + u] = EPI::off(g2, d2);
      }
    }

    // the downdate: lanes = candidates, wave `wave` takes the rows j = wave, wave + 4, ...
    {
      const int i = i0 + lane;
      float s = 0.f;
      if (i < Nc) {
        const float* lt = LTg + i;
        if (r_lds) {
#pragma unroll 4
          for (int j = wave; j < r; j += 4) s = fmaf(lt[(int64_t)j * Nc], col_s[j], s);
        } else {
#pragma unroll 4
          for (int j = wave; j < r; j += 4) s = fmaf(lt[(int64_t)j * Nc], LTg[(int64_t)j * Nc + p], s);
        }
      }
      part[wave][lane] = s;
    }
    __syncthreads();
  }

  if (wave == 0) {
    const int i = i0 + lane;
    float dv = 0.f;
    bool selected = false;
    if (i < Nc) {
      dv = dg[i];
      float l = 0.f;
      if (go) {
        const float c = kcol[lane] - ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
        l = c / sqrtf(dp);
        dv = fmaxf(dv - l * l, 0.f);
        dg[i] = dv;
      }
      LTg[(int64_t)r * Nc + i] = l;
      selected = a.ws.mask[g * Nc + i] != 0;
      if (i == p) { selected = true; a.ws.mask[g * Nc + i] = 1; }
    }
    gr_publish(a, g, i, selected, dv, (k + 1) & 1);
    if (blockIdx.x == 0 && lane == 0) {
      a.pick[g * a.M + k] = p;
      a.pivot[g * a.M + k] = dp;
    }
  }
}

template <class EPI>
static void greedy_launch_steps(const GreedyArgs& a, bool vec, size_t lds, hipStream_t st) {
  const dim3 grid(a.ws.ntiles, a.G), blk(256);
  for (int k = 0; k < a.M; ++k) {
    if (vec) hipLaunchKernelGGL((greedy_step_kernel<EPI, true>), grid, blk, lds, st, a, k);
    else hipLaunchKernelGGL((greedy_step_kernel<EPI, false>), grid, blk, lds, st, a, k);
  }
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_greedy_workspace_bytes(int G, int Nc, int D, int Mtot) {
  if (G <= 0 || Nc <= 0 || D <= 0 || Mtot <= 0) return 0;
  return greedy_carve(nullptr, G, Nc, D).bytes + 256;
}

extern "C" int vargp_greedy_select(const float* theta, const float* X, const int32_t* cand, float* LT, float* d, int32_t* pick,
                                   float* pivot, int G, int Nc, int N, int D, int k0, int M, int nu2, float eps, void* ws,
                                   size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && LT && d && pick && pivot && ws, "greedy_select: null pointer");
  VARGP_REQUIRE(G > 0 && Nc > 0 && N > 0 && D > 0 && M > 0, "greedy_select: bad dims");
  VARGP_REQUIRE(k0 >= 0, "greedy_select: k0 = %d", k0);
  VARGP_REQUIRE(M <= Nc, "greedy_select: M = %d points from Nc = %d candidates", M, Nc);
  VARGP_REQUIRE(cand || Nc <= N, "greedy_select: without a candidate list Nc = %d rows of N = %d", Nc, N);
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "greedy_select: nu2 = %d (0: RBF; 1, 3, 5: Matern)", nu2);
  VARGP_REQUIRE(G <= 65535, "greedy_select: G = %d (at most 65535)", G);
  VARGP_REQUIRE((int64_t)k0 + M < (1ll << 31), "greedy_select: k0 + M = %lld rows (below 2^31)", (long long)k0 + M);
  VARGP_REQUIRE(ws_bytes >= vargp_greedy_workspace_bytes(G, Nc, D, k0 + M), "greedy_select: workspace too small");
  GreedyArgs a{};
  a.theta = theta; a.X = X; a.cand = cand; a.LT = LT; a.d = d; a.pick = pick; a.pivot = pivot;
  a.ws = greedy_carve(ws, G, Nc, D);
  a.G = G; a.Nc = Nc; a.N = N; a.D = D; a.k0 = k0; a.M = M; a.eps = eps;
  hipStream_t st = as_stream(stream);
  ProfScope whole("greedy_select", st);
  hipLaunchKernelGGL(greedy_init_kernel, dim3(a.ws.ntiles, G), dim3(256), 0, st, a);
  const int Dl = (int)round_up(D, 4), R = k0 + M;
  const size_t lds = sizeof(float) * ((Dl <= kGrCapD ? 2 * Dl : 0) + (R <= kGrCapR ? R : 0));
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  switch (nu2) {
    case 0: greedy_launch_steps<EpiRbf>(a, vec, lds, st); break;
    case 1: greedy_launch_steps<EpiMatern<1>>(a, vec, lds, st); break;
    case 3: greedy_launch_steps<EpiMatern<3>>(a, vec, lds, st); break;
    default: greedy_launch_steps<EpiMatern<5>>(a, vec, lds, st); break;
  }
  return check_launch("greedy_select");
}
