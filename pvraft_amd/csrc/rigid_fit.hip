// K20: robust rigid fit of a flow field (absent in the reference): weighted
// Kabsch inside a Cauchy IRLS loop, the whole loop in ONE launch.  (K22, the
// same fit once per labelled segment, follows at the end of the file.)
//
//   w0_i = prior_i (1 without a prior; 0 for a non-finite coordinate, a
//          non-finite weight or a weight <= 0)
//   for k = 0 .. iters:
//     (R, t) = argmin sum_i w_i |R src_i + t - dst_i|^2,  det R = +1
//     r_i    = |R src_i + t - dst_i|
//     if k < iters:  w_i = w0_i / (1 + (r_i / thresh)^2)
//   out: R (B,3,3), t (B,3), r (B,N) of the LAST fit (+INF where a coordinate
//        is non-finite), ok (B)
//
// Geometry: one workgroup of 1024 lanes (16 waves) per batch element, grid
// (B).  Nothing crosses workgroups: no grid barrier, no spin wait, no
// atomics.  Up to RF_REG_POINTS = 4096 points stay in registers for all
// rounds, PPL = 1/2/4 statically indexed slots per lane (point i sits in
// slot i / 1024 of lane i % 1024); larger clouds run the same code with
// PPL = 0, which re-reads the points from global memory in every pass
// (196 KB at 8192 points, 3.1 MB at 131072: L2 resident).  Eight slots per
// lane were tried: next to the fp64 accumulators and their temporaries they
// do not fit the 128 VGPRs that 16 waves per workgroup leave (the compiler
// went to scratch), so 8192 points stream.
//
// Centring / conditioning: a first in-block pass takes the UNWEIGHTED mean c
// of the usable src points (fp64 sums, rounded to fp32).  Every point is
// then held as p = src - c and d = dst - src (fp32; d is exact whenever the
// flow is smaller than the coordinate) -- src is accumulated against dst -
// src, never against dst.  The sixteen sums of a round,
//   sum w, sum w p (3), sum w d (3), sum w p (p + d)^T (9),
// are accumulated in fp64 -- per lane, then a wave butterfly, then a
// fixed-order fold of the 16 wave sums through LDS -- in two passes of eight
// sums (eight fp64 accumulators per lane instead of sixteen; the weight is
// recomputed in the second pass).  Products of fp32 operands are exact in
// fp64, so the weighted-centroid correction
// H = sum w p q^T - (sum w p)(sum w q)^T / sum w loses nothing that matters.
// The fold order is fixed: results are bit-reproducible run to run.
// Residuals use the small-rotation form e = (R - I) p + t' - d with
// t' = dbar - (R - I) pbar (pivot frame), so the rounding of a coordinate is
// scaled by |R - I|; the reported t = t' - (R - I) c.
//
// Solver: lane 0 runs a one-sided (Hestenes) cyclic Jacobi SVD of the 3x3 H
// in fp32 (H itself comes from the fp64 sums), statically indexed, at most
// RF_SWEEPS sweeps.  With H V = U S the two leading pairs give u1, u2, v1,
// v2; u3 = u1 x u2 and v3 = v1 x v2 make R = V U^T proper by construction
// (this IS the det sign fix: the flip lands on the smallest singular value).
// Rank 2 (planar) never touches the third column; rank 1 (collinear)
// completes u2 with a unit vector orthogonal to u1; rank 0 returns I.  The
// same code instantiated in fp64 needed > 128 VGPRs with the points resident.
//
// ok = false when fewer than 3 points have positive weight or any sum is
// non-finite: then R = I and t = weighted mean of d under w0 (0 when there
// is no usable point).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs per
// lane: PPL=1 88, PPL=2 96, PPL=4 116, streaming 118; no AGPRs; scratch 0
// bytes for every instantiation; LDS 1248 bytes.
#include <hip/hip_runtime.h>
#include "common.h"

#define RF_THREADS 1024
#define RF_WAVES (RF_THREADS / WAVE)
#define RF_MAX_PPL 4
#define RF_REG_POINTS (RF_THREADS * RF_MAX_PPL)
#define RF_NSUM 16
#define RF_HALF 8  // sums per accumulation pass (two passes per round)
#define RF_SWEEPS 12

int rigid_fit_reg_points() { return RF_REG_POINTS; }

DEV_INLINE double rf_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// wave-uniform LDS value -> scalar register
DEV_INLINE float rf_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

struct RfShared {
  double part[RF_WAVES][RF_HALF];  // per-wave partial sums
  double tot[RF_NSUM];             // block totals
  double tfall[3];                 // fallback translation (round 0 mean of d)
  float E[9];                      // R - I
  float tp[3];                     // t' (pivot frame)
  float c[3];                      // pivot
  int n_use;
  int ok;
};

// Block-wide fixed-order sum of RF_HALF per-lane fp64 values: wave
// butterfly, then lane j < RF_HALF folds quantity j over the 16 waves in
// ascending order into sh.tot[base + j], valid for every lane after the
// closing barrier.
DEV_INLINE void rf_block_sum(double (&acc)[RF_HALF], RfShared &sh, int base) {
#pragma unroll
  for (int j = 0; j < RF_HALF; ++j) acc[j] = rf_wave_sum(acc[j]);
  if (lane_id() == 0) {
#pragma unroll
    for (int j = 0; j < RF_HALF; ++j) sh.part[wave_id()][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x < RF_HALF) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < RF_WAVES; ++w) s += sh.part[w][threadIdx.x];
    sh.tot[base + threadIdx.x] = s;
  }
  __syncthreads();
}

template <typename T> struct RfEps;
template <> struct RfEps<double> {
  static constexpr double orth = 1e-32, tiny = 1e-280;
};
template <> struct RfEps<float> {
  static constexpr float orth = 1e-14f, tiny = 1e-30f;
};

template <typename T>
DEV_INLINE void rf_rotate(T (&B)[3][3], T (&V)[3][3], const int i,
                          const int j, bool &moved) {
  T al = T(0.0), be = T(0.0), ga = T(0.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    al += B[k][i] * B[k][i];
    be += B[k][j] * B[k][j];
    ga += B[k][i] * B[k][j];
  }
  if (ga * ga <= RfEps<T>::orth * al * be) return;  // orthogonal to working precision
  moved = true;
  const T zeta = (be - al) / (T(2.0) * ga);
  const T tt = copysign(T(1.0), zeta) / (fabs(zeta) + sqrt(T(1.0) + zeta * zeta));
  const T cs = T(1.0) / sqrt(T(1.0) + tt * tt);
  const T sn = cs * tt;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T bi = B[k][i], bj = B[k][j];
    B[k][i] = cs * bi - sn * bj;
    B[k][j] = sn * bi + cs * bj;
    const T vi = V[k][i], vj = V[k][j];
    V[k][i] = cs * vi - sn * vj;
    V[k][j] = sn * vi + cs * vj;
  }
}

template <typename T>
DEV_INLINE void rf_swap_cols(T (&B)[3][3], T (&V)[3][3],
                             T (&n)[3], const int i, const int j) {
  if (n[i] >= n[j]) return;
  const T tn = n[i];
  n[i] = n[j];
  n[j] = tn;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T tb = B[k][i];
    B[k][i] = B[k][j];
    B[k][j] = tb;
    const T tv = V[k][i];
    V[k][i] = V[k][j];
    V[k][j] = tv;
  }
}

// E = R - I for the proper rotation maximising tr(R H), H = sum w p q^T.
template <typename T>
DEV_INLINE void rf_rotation(const T (&H)[3][3], T (&E)[3][3]) {
  T B[3][3], V[3][3];
  T hmax = T(0.0);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) hmax = fmax(hmax, fabs(H[a][b]));
  const T ih = hmax > T(0.0) ? T(1.0) / hmax : T(0.0);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      E[a][b] = T(0.0);
      V[a][b] = a == b ? T(1.0) : T(0.0);
      B[a][b] = H[a][b] * ih;
    }
  if (!(hmax > T(0.0))) return;  // rank 0: every rotation attains the minimum

  for (int sweep = 0; sweep < RF_SWEEPS; ++sweep) {
    bool moved = false;
    rf_rotate(B, V, 0, 1, moved);
    rf_rotate(B, V, 0, 2, moved);
    rf_rotate(B, V, 1, 2, moved);
    if (!moved) break;
  }
  T n[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    n[j] = B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j];
  rf_swap_cols(B, V, n, 0, 1);
  rf_swap_cols(B, V, n, 0, 2);
  rf_swap_cols(B, V, n, 1, 2);

  const T i1 = T(1.0) / sqrt(n[0]);  // n[0] > 0 since hmax > 0
  const T u1[3] = {B[0][0] * i1, B[1][0] * i1, B[2][0] * i1};
  const T pr = B[0][1] * u1[0] + B[1][1] * u1[1] + B[2][1] * u1[2];
  T u2[3] = {B[0][1] - pr * u1[0], B[1][1] - pr * u1[1],
                  B[2][1] - pr * u1[2]};
  T n2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
  if (!(n2 > RfEps<T>::tiny)) {
    // rank 1: u2 = u1 x (the axis u1 leans on least), never zero
    const T ax = fabs(u1[0]), ay = fabs(u1[1]), az = fabs(u1[2]);
    if (ax <= ay && ax <= az) {
      u2[0] = T(0.0), u2[1] = u1[2], u2[2] = -u1[1];
    } else if (ay <= az) {
      u2[0] = -u1[2], u2[1] = T(0.0), u2[2] = u1[0];
    } else {
      u2[0] = u1[1], u2[1] = -u1[0], u2[2] = T(0.0);
    }
    n2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
  }
  const T i2 = T(1.0) / sqrt(n2);
  u2[0] *= i2, u2[1] *= i2, u2[2] *= i2;
  const T u3[3] = {u1[1] * u2[2] - u1[2] * u2[1],
                        u1[2] * u2[0] - u1[0] * u2[2],
                        u1[0] * u2[1] - u1[1] * u2[0]};
  const T v3[3] = {V[1][0] * V[2][1] - V[2][0] * V[1][1],
                        V[2][0] * V[0][1] - V[0][0] * V[2][1],
                        V[0][0] * V[1][1] - V[1][0] * V[0][1]};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      E[a][b] = V[a][0] * u1[b] + V[a][1] * u2[b] + v3[a] * u3[b] -
                (a == b ? T(1.0) : T(0.0));
}

// One point as the rounds see it: w0 > 0 usable, 0 = finite but unweighted,
// -1 = a non-finite coordinate (p = d = 0 then).
struct RfPoint {
  float px, py, pz, dx, dy, dz, w0;
};

DEV_INLINE RfPoint rf_load(const float *__restrict__ src,
                           const float *__restrict__ dst,
                           const float *__restrict__ prior, long i) {
  RfPoint P;
  const float sx = src[i * 3 + 0], sy = src[i * 3 + 1], sz = src[i * 3 + 2];
  const float qx = dst[i * 3 + 0], qy = dst[i * 3 + 1], qz = dst[i * 3 + 2];
  const float w = prior ? prior[i] : 1.f;
  const bool fin = isfinite(sx) && isfinite(sy) && isfinite(sz) &&
                   isfinite(qx) && isfinite(qy) && isfinite(qz);
  P.px = fin ? sx : 0.f;
  P.py = fin ? sy : 0.f;
  P.pz = fin ? sz : 0.f;
  P.dx = fin ? qx - sx : 0.f;
  P.dy = fin ? qy - sy : 0.f;
  P.dz = fin ? qz - sz : 0.f;
  // a difference of finite coordinates can still overflow
  const bool dfin = isfinite(P.dx) && isfinite(P.dy) && isfinite(P.dz);
  if (!dfin) P.px = P.py = P.pz = P.dx = P.dy = P.dz = 0.f;
  P.w0 = !(fin && dfin) ? -1.f : (isfinite(w) && w > 0.f ? w : 0.f);
  return P;
}

template <int PPL>
__global__ __launch_bounds__(RF_THREADS) void rigid_fit_kernel(
    const float *__restrict__ src,    // (B, N, 3)
    const float *__restrict__ dst,    // (B, N, 3)
    const float *__restrict__ prior,  // (B, N) or null
    float *__restrict__ R_out,        // (B, 3, 3)
    float *__restrict__ t_out,        // (B, 3)
    float *__restrict__ res_out,      // (B, N)
    unsigned char *__restrict__ ok_out,  // (B)
    int N, float inv_th2, int iters) {
  __shared__ RfShared sh;
  constexpr int NS = PPL > 0 ? PPL : 1;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  src += (long)b * N * 3;
  dst += (long)b * N * 3;
  if (prior) prior += (long)b * N;
  res_out += (long)b * N;

  RfPoint P[NS];
  if constexpr (PPL > 0) {
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int i = s * RF_THREADS + tid;
      if (i < N) {
        P[s] = rf_load(src, dst, prior, i);
      } else {
        P[s].px = P[s].py = P[s].pz = P[s].dx = P[s].dy = P[s].dz = 0.f;
        P[s].w0 = 0.f;
      }
    }
  }

  double acc[RF_HALF];

  // ---- pass 0: pivot = unweighted mean of the usable src points ----------
#pragma unroll
  for (int j = 0; j < RF_HALF; ++j) acc[j] = 0.0;
  {
    auto visit = [&](const RfPoint &Q) __attribute__((always_inline)) {
      const bool use = Q.w0 > 0.f;
      acc[0] += use ? 1.0 : 0.0;
      acc[1] += use ? (double)Q.px : 0.0;
      acc[2] += use ? (double)Q.py : 0.0;
      acc[3] += use ? (double)Q.pz : 0.0;
    };
    if constexpr (PPL > 0) {
#pragma unroll
      for (int s = 0; s < PPL; ++s) visit(P[s]);
    } else {
#pragma unroll 4
      for (int i = tid; i < N; i += RF_THREADS)
        visit(rf_load(src, dst, prior, i));
    }
  }
  rf_block_sum(acc, sh, 0);
  if (tid == 0) {
    const double n = sh.tot[0];
    float c[3] = {0.f, 0.f, 0.f};
    if (n > 0.0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = (float)(sh.tot[1 + a] / n);
        c[a] = isfinite(v) ? v : 0.f;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sh.c[a] = c[a];
      sh.tp[a] = 0.f;
      sh.tfall[a] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) sh.E[a] = 0.f;
    sh.n_use = (int)n;
    sh.ok = 1;
  }
  __syncthreads();
  const float cx = rf_uniform(sh.c[0]), cy = rf_uniform(sh.c[1]),
              cz = rf_uniform(sh.c[2]);
  if constexpr (PPL > 0) {
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      // unusable slots keep p = 0
      if (P[s].w0 >= 0.f && s * RF_THREADS + tid < N) {
        P[s].px -= cx;
        P[s].py -= cy;
        P[s].pz -= cz;
      }
    }
  }

  // ---- IRLS rounds -------------------------------------------------------
  float E[9], tp[3];
#pragma unroll
  for (int a = 0; a < 9; ++a) E[a] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) tp[a] = 0.f;

  // squared residual of a (pivot-frame) point under the current fit
  auto resid2 = [&](const RfPoint &Q) __attribute__((always_inline)) {
    const float ex = fmaf(E[0], Q.px, fmaf(E[1], Q.py, fmaf(E[2], Q.pz, tp[0] - Q.dx)));
    const float ey = fmaf(E[3], Q.px, fmaf(E[4], Q.py, fmaf(E[5], Q.pz, tp[1] - Q.dy)));
    const float ez = fmaf(E[6], Q.px, fmaf(E[7], Q.py, fmaf(E[8], Q.pz, tp[2] - Q.dz)));
    return fmaf(ex, ex, fmaf(ey, ey, ez * ez));
  };
  auto centred = [&](RfPoint Q) __attribute__((always_inline)) {
    if (Q.w0 >= 0.f) {
      Q.px -= cx;
      Q.py -= cy;
      Q.pz -= cz;
    }
    return Q;
  };

  bool ok = true;
  for (int k = 0; k <= iters; ++k) {
    // The sixteen sums are taken in two passes of eight (tot[0..7], then
    // tot[8..15]): sixteen fp64 accumulators next to eight resident points
    // and their fp64 temporaries do not fit 128 VGPRs.  The weight is
    // recomputed in the second pass (twelve fp32 FMAs).
    for (int half = 0; half < 2; ++half) {
      if constexpr (PPL > 0) {
        // The resident points are loop-invariant; without this the compiler
        // hoists their fp64 conversions and products out of the round loop
        // (18+ VGPRs per point, i.e. scratch).  An empty asm that "modifies"
        // each value pins that work inside the pass.
#pragma unroll
        for (int s = 0; s < PPL; ++s)
          asm volatile("" : "+v"(P[s].px), "+v"(P[s].py), "+v"(P[s].pz),
                            "+v"(P[s].dx), "+v"(P[s].dy), "+v"(P[s].dz),
                            "+v"(P[s].w0));
      }
#pragma unroll
      for (int j = 0; j < RF_HALF; ++j) acc[j] = 0.0;
      auto visit = [&](const RfPoint &Q) __attribute__((always_inline)) {
        float w = fmaxf(Q.w0, 0.f);
        if (k > 0) {
          w = w / fmaf(resid2(Q), inv_th2, 1.f);
          if (!(w > 0.f)) w = 0.f;  // overflowed residual: the point drops out
        }
        const double wd = w;
        const double px = Q.px, py = Q.py, pz = Q.pz;
        const double dx = Q.dx, dy = Q.dy, dz = Q.dz;
        if (half == 0) {
          const double wx = wd * px;
          acc[0] += wd;
          acc[1] += wx;
          acc[2] = fma(wd, py, acc[2]);
          acc[3] = fma(wd, pz, acc[3]);
          acc[4] = fma(wd, dx, acc[4]);
          acc[5] = fma(wd, dy, acc[5]);
          acc[6] = fma(wd, dz, acc[6]);
          acc[7] = fma(wx, px + dx, acc[7]);
        } else {
          const double wx = wd * px, wy = wd * py, wz = wd * pz;
          const double qx = px + dx, qy = py + dy, qz = pz + dz;
          acc[0] = fma(wx, qy, acc[0]);
          acc[1] = fma(wx, qz, acc[1]);
          acc[2] = fma(wy, qx, acc[2]);
          acc[3] = fma(wy, qy, acc[3]);
          acc[4] = fma(wy, qz, acc[4]);
          acc[5] = fma(wz, qx, acc[5]);
          acc[6] = fma(wz, qy, acc[6]);
          acc[7] = fma(wz, qz, acc[7]);
        }
      };
      if constexpr (PPL > 0) {
#pragma unroll
        for (int s = 0; s < PPL; ++s) visit(P[s]);
      } else {
#pragma unroll 4
        for (int i = tid; i < N; i += RF_THREADS)
          visit(centred(rf_load(src, dst, prior, i)));
      }
      rf_block_sum(acc, sh, half * RF_HALF);
    }

    if (tid == 0) {
      bool fin = true;
#pragma unroll
      for (int j = 0; j < RF_NSUM; ++j) fin = fin && isfinite(sh.tot[j]);
      const double sw = sh.tot[0];
      bool good = fin && sw > 0.0 && sh.n_use >= 3;
      double Ed[3][3], tpd[3];
      if (fin && sw > 0.0) {
        const double iw = 1.0 / sw;
        const double pm[3] = {sh.tot[1] * iw, sh.tot[2] * iw, sh.tot[3] * iw};
        const double dm[3] = {sh.tot[4] * iw, sh.tot[5] * iw, sh.tot[6] * iw};
        if (k == 0) {
#pragma unroll
          for (int a = 0; a < 3; ++a) sh.tfall[a] = dm[a];
        }
        if (good) {
          double H[3][3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2)
              H[a][c2] = sh.tot[7 + 3 * a + c2] - sw * pm[a] * (pm[c2] + dm[c2]);
          float Hs[3][3], Es[3][3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) Hs[a][c2] = (float)H[a][c2];
          rf_rotation<float>(Hs, Es);
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) Ed[a][c2] = (double)Es[a][c2];
#pragma unroll
          for (int a = 0; a < 3; ++a)
            tpd[a] = dm[a] - (Ed[a][0] * pm[0] + Ed[a][1] * pm[1] +
                              Ed[a][2] * pm[2]);
#pragma unroll
          for (int a = 0; a < 3; ++a)
            good = good && isfinite(tpd[a]) && isfinite(Ed[a][0]) &&
                   isfinite(Ed[a][1]) && isfinite(Ed[a][2]);
        }
      }
      if (!good) {
        // R = I, t = mean of d under the prior weights (0 if none)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          tpd[a] = sh.tfall[a];
#pragma unroll
          for (int c2 = 0; c2 < 3; ++c2) Ed[a][c2] = 0.0;
        }
        sh.ok = 0;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sh.tp[a] = (float)tpd[a];
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) sh.E[3 * a + c2] = (float)Ed[a][c2];
      }
      if (k == iters || !good) {
        const double cd[3] = {(double)cx, (double)cy, (double)cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          t_out[b * 3 + a] = (float)(tpd[a] - (Ed[a][0] * cd[0] + Ed[a][1] * cd[1] +
                                               Ed[a][2] * cd[2]));
#pragma unroll
          for (int c2 = 0; c2 < 3; ++c2)
            R_out[b * 9 + 3 * a + c2] = (float)(Ed[a][c2] + (a == c2 ? 1.0 : 0.0));
        }
        ok_out[b] = good ? 1 : 0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 9; ++a) E[a] = rf_uniform(sh.E[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) tp[a] = rf_uniform(sh.tp[a]);
    ok = sh.ok != 0;
    if (!ok) break;  // block-uniform
  }

  // ---- residuals of the last fit -----------------------------------------
  if constexpr (PPL > 0) {
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int i = s * RF_THREADS + tid;
      if (i < N) res_out[i] = P[s].w0 < 0.f ? INFINITY : sqrtf(resid2(P[s]));
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < N; i += RF_THREADS) {
      const RfPoint Q = centred(rf_load(src, dst, prior, i));
      res_out[i] = Q.w0 < 0.f ? INFINITY : sqrtf(resid2(Q));
    }
  }
}

void launch_rigid_fit(const float *src, const float *dst, const float *prior,
                      float *R, float *t, float *res, unsigned char *ok, int B,
                      int N, float thresh, int iters, hipStream_t stream) {
  const float inv_th2 = 1.f / (thresh * thresh);
  dim3 grid(B), block(RF_THREADS);
#define RF_LAUNCH(PPL)                                                       \
  hipLaunchKernelGGL(rigid_fit_kernel<PPL>, grid, block, 0, stream, src, dst, \
                     prior, R, t, res, ok, N, inv_th2, iters)
  if (N <= 1 * RF_THREADS) RF_LAUNCH(1);
  else if (N <= 2 * RF_THREADS) RF_LAUNCH(2);
  else if (N <= RF_REG_POINTS) RF_LAUNCH(4);
  else RF_LAUNCH(0);
#undef RF_LAUNCH
}

// ---------------------------------------------------------------------------
// K22: segmented robust rigid fit -- the loop above once per labelled segment
// (object) of a cloud, all segments in ONE launch.
//
//   labels (B,N) int32: -1 or a segment 0 .. M-1 (anything else counts as -1)
//   out: R (B,M,3,3), t (B,M,3), ok (B,M); r (B,N) with respect to the point's
//        own segment, +INF for label -1 or a non-finite coordinate
//
// Geometry: grid (M, B), one workgroup of 256 lanes (4 waves) per segment.
// Objects have 50 to 1000 points: 256 lanes give such a segment one to four
// points per lane and round, the block fold crosses four waves instead of
// sixteen, and M * B = 32 .. 64 workgroups spread over as many CUs -- 1024
// lanes would idle three quarters of them on a typical object and buy
// nothing, the segments already run in parallel.
//
// The workgroup scans its batch element's labels ONCE and compacts its members
// in ascending index order (wave ballot + prefix over the four waves), so the
// fold order is fixed and the result bit-reproducible.  Up to SF_CAP = 1024
// members are kept in LDS (pivot-centred p, d, w0 and the point index, 32 KB),
// and every round costs in proportion to the segment, not to N.  A larger
// segment streams instead: every pass walks the labels again and re-reads its
// members from global memory (L2), like PPL = 0 above.  Workgroup m = 0 also
// writes the +INF residual of the points that belong to no segment, so every
// residual is written exactly once and nothing is pre-filled.
//
// The math is the one above, unchanged: rf_load, the pivot-centred fp64 sums in
// two passes of eight, rf_rotation<float> on lane 0, the small-rotation
// residual; no atomics, no host sync.  The accumulation and the lane-0 solve
// are written out a second time here on purpose: moving them into inline
// helpers shared with rigid_fit_kernel was tried and changed that kernel's
// register allocation and instruction stream (88 -> 78 VGPRs at PPL = 1), and
// K20 is to stay the code it was.  A change to one copy belongs in the other.
//
// Resources (same tool): 118 VGPRs, no AGPRs, scratch 0 bytes, LDS 33264 bytes.
#define SF_THREADS 256
#define SF_WAVES (SF_THREADS / WAVE)
#define SF_CAP 1024

int segmented_fit_capacity() { return SF_CAP; }

struct SfShared {
  double part[SF_WAVES][RF_HALF];
  double tot[RF_NSUM];
  double tfall[3];
  float E[9];
  float tp[3];
  float c[3];
  int n_use;
  int ok;
  int wcnt[SF_WAVES];
};

// rf_block_sum for four waves
DEV_INLINE void sf_block_sum(double (&acc)[RF_HALF], SfShared &sh, int base) {
#pragma unroll
  for (int j = 0; j < RF_HALF; ++j) acc[j] = rf_wave_sum(acc[j]);
  if (lane_id() == 0) {
#pragma unroll
    for (int j = 0; j < RF_HALF; ++j) sh.part[wave_id()][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x < RF_HALF) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SF_WAVES; ++w) s += sh.part[w][threadIdx.x];
    sh.tot[base + threadIdx.x] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(SF_THREADS) void segmented_rigid_fit_kernel(
    const float *__restrict__ src,    // (B, N, 3)
    const float *__restrict__ dst,    // (B, N, 3)
    const float *__restrict__ prior,  // (B, N) or null
    const int *__restrict__ labels,   // (B, N)
    float *__restrict__ R_out,        // (B, M, 3, 3)
    float *__restrict__ t_out,        // (B, M, 3)
    float *__restrict__ res_out,      // (B, N)
    unsigned char *__restrict__ ok_out,  // (B, M)
    int N, int M, float inv_th2, int iters) {
  __shared__ SfShared sh;
  __shared__ float mpx[SF_CAP], mpy[SF_CAP], mpz[SF_CAP];
  __shared__ float mdx[SF_CAP], mdy[SF_CAP], mdz[SF_CAP], mw0[SF_CAP];
  __shared__ int midx[SF_CAP];
  const int m = blockIdx.x;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int seg = b * M + m;
  src += (long)b * N * 3;
  dst += (long)b * N * 3;
  if (prior) prior += (long)b * N;
  labels += (long)b * N;
  res_out += (long)b * N;

  // ---- one scan of the labels: ordered compaction of the members ----------
  int n_mem = 0;  // block-uniform
  for (int base = 0; base < N; base += SF_THREADS) {
    const int i = base + tid;
    const int lab = i < N ? labels[i] : m + 1;
    const bool mem = i < N && lab == m;
    if (m == 0 && i < N && (lab < 0 || lab >= M)) res_out[i] = INFINITY;
    const unsigned long long bal = __ballot(mem);
    if (lane_id() == 0) sh.wcnt[wave_id()] = __popcll(bal);
    __syncthreads();
    int off = n_mem, tot = 0;
#pragma unroll
    for (int w = 0; w < SF_WAVES; ++w) {
      const int c = sh.wcnt[w];
      off += w < wave_id() ? c : 0;
      tot += c;
    }
    const int pos = off + __popcll(bal & ((1ull << lane_id()) - 1ull));
    if (mem && pos < SF_CAP) {
      const RfPoint Q = rf_load(src, dst, prior, i);
      mpx[pos] = Q.px, mpy[pos] = Q.py, mpz[pos] = Q.pz;
      mdx[pos] = Q.dx, mdy[pos] = Q.dy, mdz[pos] = Q.dz;
      mw0[pos] = Q.w0;
      midx[pos] = i;
    }
    n_mem += tot;
    __syncthreads();
  }
  const bool resident = n_mem <= SF_CAP;  // block-uniform

  auto member = [&](int j) __attribute__((always_inline)) {
    RfPoint Q;
    Q.px = mpx[j], Q.py = mpy[j], Q.pz = mpz[j];
    Q.dx = mdx[j], Q.dy = mdy[j], Q.dz = mdz[j];
    Q.w0 = mw0[j];
    return Q;
  };

  double acc[RF_HALF];

  // ---- pass 0: pivot = unweighted mean of the usable src points ----------
#pragma unroll
  for (int j = 0; j < RF_HALF; ++j) acc[j] = 0.0;
  {
    auto visit = [&](const RfPoint &Q) __attribute__((always_inline)) {
      const bool use = Q.w0 > 0.f;
      acc[0] += use ? 1.0 : 0.0;
      acc[1] += use ? (double)Q.px : 0.0;
      acc[2] += use ? (double)Q.py : 0.0;
      acc[3] += use ? (double)Q.pz : 0.0;
    };
    if (resident) {
      for (int j = tid; j < n_mem; j += SF_THREADS) visit(member(j));
    } else {
      for (int i = tid; i < N; i += SF_THREADS)
        if (labels[i] == m) visit(rf_load(src, dst, prior, i));
    }
  }
  sf_block_sum(acc, sh, 0);
  if (tid == 0) {
    const double n = sh.tot[0];
    float c[3] = {0.f, 0.f, 0.f};
    if (n > 0.0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = (float)(sh.tot[1 + a] / n);
        c[a] = isfinite(v) ? v : 0.f;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sh.c[a] = c[a];
      sh.tp[a] = 0.f;
      sh.tfall[a] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) sh.E[a] = 0.f;
    sh.n_use = (int)n;
    sh.ok = 1;
  }
  __syncthreads();
  const float cx = rf_uniform(sh.c[0]), cy = rf_uniform(sh.c[1]),
              cz = rf_uniform(sh.c[2]);
  if (resident) {
    for (int j = tid; j < n_mem; j += SF_THREADS) {
      if (mw0[j] >= 0.f) {  // unusable members keep p = 0
        mpx[j] -= cx;
        mpy[j] -= cy;
        mpz[j] -= cz;
      }
    }
  }
  // each lane re-reads only the slots it wrote: no barrier needed here

  // ---- IRLS rounds -------------------------------------------------------
  float E[9], tp[3];
#pragma unroll
  for (int a = 0; a < 9; ++a) E[a] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) tp[a] = 0.f;

  auto resid2 = [&](const RfPoint &Q) __attribute__((always_inline)) {
    const float ex = fmaf(E[0], Q.px, fmaf(E[1], Q.py, fmaf(E[2], Q.pz, tp[0] - Q.dx)));
    const float ey = fmaf(E[3], Q.px, fmaf(E[4], Q.py, fmaf(E[5], Q.pz, tp[1] - Q.dy)));
    const float ez = fmaf(E[6], Q.px, fmaf(E[7], Q.py, fmaf(E[8], Q.pz, tp[2] - Q.dz)));
    return fmaf(ex, ex, fmaf(ey, ey, ez * ez));
  };
  auto centred = [&](RfPoint Q) __attribute__((always_inline)) {
    if (Q.w0 >= 0.f) {
      Q.px -= cx;
      Q.py -= cy;
      Q.pz -= cz;
    }
    return Q;
  };

  bool ok = true;
  for (int k = 0; k <= iters; ++k) {
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int j = 0; j < RF_HALF; ++j) acc[j] = 0.0;
      auto visit = [&](const RfPoint &Q) __attribute__((always_inline)) {
        float w = fmaxf(Q.w0, 0.f);
        if (k > 0) {
          w = w / fmaf(resid2(Q), inv_th2, 1.f);
          if (!(w > 0.f)) w = 0.f;  // overflowed residual: the point drops out
        }
        const double wd = w;
        const double px = Q.px, py = Q.py, pz = Q.pz;
        const double dx = Q.dx, dy = Q.dy, dz = Q.dz;
        if (half == 0) {
          const double wx = wd * px;
          acc[0] += wd;
          acc[1] += wx;
          acc[2] = fma(wd, py, acc[2]);
          acc[3] = fma(wd, pz, acc[3]);
          acc[4] = fma(wd, dx, acc[4]);
          acc[5] = fma(wd, dy, acc[5]);
          acc[6] = fma(wd, dz, acc[6]);
          acc[7] = fma(wx, px + dx, acc[7]);
        } else {
          const double wx = wd * px, wy = wd * py, wz = wd * pz;
          const double qx = px + dx, qy = py + dy, qz = pz + dz;
          acc[0] = fma(wx, qy, acc[0]);
          acc[1] = fma(wx, qz, acc[1]);
          acc[2] = fma(wy, qx, acc[2]);
          acc[3] = fma(wy, qy, acc[3]);
          acc[4] = fma(wy, qz, acc[4]);
          acc[5] = fma(wz, qx, acc[5]);
          acc[6] = fma(wz, qy, acc[6]);
          acc[7] = fma(wz, qz, acc[7]);
        }
      };
      if (resident) {
        for (int j = tid; j < n_mem; j += SF_THREADS) visit(member(j));
      } else {
        for (int i = tid; i < N; i += SF_THREADS)
          if (labels[i] == m) visit(centred(rf_load(src, dst, prior, i)));
      }
      sf_block_sum(acc, sh, half * RF_HALF);
    }

    if (tid == 0) {
      bool fin = true;
#pragma unroll
      for (int j = 0; j < RF_NSUM; ++j) fin = fin && isfinite(sh.tot[j]);
      const double sw = sh.tot[0];
      bool good = fin && sw > 0.0 && sh.n_use >= 3;
      double Ed[3][3], tpd[3];
      if (fin && sw > 0.0) {
        const double iw = 1.0 / sw;
        const double pm[3] = {sh.tot[1] * iw, sh.tot[2] * iw, sh.tot[3] * iw};
        const double dm[3] = {sh.tot[4] * iw, sh.tot[5] * iw, sh.tot[6] * iw};
        if (k == 0) {
#pragma unroll
          for (int a = 0; a < 3; ++a) sh.tfall[a] = dm[a];
        }
        if (good) {
          double H[3][3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2)
              H[a][c2] = sh.tot[7 + 3 * a + c2] - sw * pm[a] * (pm[c2] + dm[c2]);
          float Hs[3][3], Es[3][3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) Hs[a][c2] = (float)H[a][c2];
          rf_rotation<float>(Hs, Es);
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) Ed[a][c2] = (double)Es[a][c2];
#pragma unroll
          for (int a = 0; a < 3; ++a)
            tpd[a] = dm[a] - (Ed[a][0] * pm[0] + Ed[a][1] * pm[1] +
                              Ed[a][2] * pm[2]);
#pragma unroll
          for (int a = 0; a < 3; ++a)
            good = good && isfinite(tpd[a]) && isfinite(Ed[a][0]) &&
                   isfinite(Ed[a][1]) && isfinite(Ed[a][2]);
        }
      }
      if (!good) {
        // R = I, t = mean of d under the prior weights (0 if none)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          tpd[a] = sh.tfall[a];
#pragma unroll
          for (int c2 = 0; c2 < 3; ++c2) Ed[a][c2] = 0.0;
        }
        sh.ok = 0;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sh.tp[a] = (float)tpd[a];
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) sh.E[3 * a + c2] = (float)Ed[a][c2];
      }
      if (k == iters || !good) {
        const double cd[3] = {(double)cx, (double)cy, (double)cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          t_out[seg * 3 + a] = (float)(tpd[a] - (Ed[a][0] * cd[0] + Ed[a][1] * cd[1] +
                                                 Ed[a][2] * cd[2]));
#pragma unroll
          for (int c2 = 0; c2 < 3; ++c2)
            R_out[seg * 9 + 3 * a + c2] = (float)(Ed[a][c2] + (a == c2 ? 1.0 : 0.0));
        }
        ok_out[seg] = good ? 1 : 0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 9; ++a) E[a] = rf_uniform(sh.E[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) tp[a] = rf_uniform(sh.tp[a]);
    ok = sh.ok != 0;
    if (!ok) break;  // block-uniform
  }

  // ---- residuals of the last fit, members only ---------------------------
  if (resident) {
    for (int j = tid; j < n_mem; j += SF_THREADS) {
      const RfPoint Q = member(j);
      res_out[midx[j]] = Q.w0 < 0.f ? INFINITY : sqrtf(resid2(Q));
    }
  } else {
    for (int i = tid; i < N; i += SF_THREADS) {
      if (labels[i] != m) continue;
      const RfPoint Q = centred(rf_load(src, dst, prior, i));
      res_out[i] = Q.w0 < 0.f ? INFINITY : sqrtf(resid2(Q));
    }
  }
}

void launch_segmented_rigid_fit(const float *src, const float *dst,
                                const float *prior, const int *labels, float *R,
                                float *t, float *res, unsigned char *ok, int B,
                                int N, int M, float thresh, int iters,
                                hipStream_t stream) {
  const float inv_th2 = 1.f / (thresh * thresh);
  hipLaunchKernelGGL(segmented_rigid_fit_kernel, dim3(M, B), dim3(SF_THREADS), 0,
                     stream, src, dst, prior, labels, R, t, res, ok, N, M, inv_th2,
                     iters);
}
