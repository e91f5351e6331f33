// K8: fused kNN-correlation branch head: Conv2d(4->C) -> GroupNorm ->
// PReLU -> max over k, in one kernel pipeline.
//
// Reference semantics (model/corr.py:75-98 kNN branch; knn_conv defined
// at corr.py:23-29): raw per-candidate features [corr; rel-xyz]
// (B, 4, K, N) run through a 1x1 conv to C=64 channels, GroupNorm(8),
// PReLU, then max-pool over the K candidates.  Run as a GEMM the conv materialises a (B, C, K, N)
// activation (~33 M elements at the flagship shape) that GroupNorm and
// the pool each re-read -- ~1.5 ms/step of traffic + launches for a
// 4-wide contraction.
//
// Here the conv is evaluated INLINE: the edge vector has only 4
// components, so v[c, j, n] = W[c, :4] @ raw[:, j, n] + cb[c] is 4 FMAs
// from wave-uniform (SGPR) weights.  The reduce pass streams raw once,
// tracks per-(n, c) extremes of v over j (act(GN(v)) is piecewise
// monotone in v -- same argument as edge_gnmp) plus the GroupNorm
// sums, and the shared egnmp pick/finalize kernels produce the pooled
// output; the (B, C, K, N) tensor never exists, forward or backward.
//
// Channels are processed in CH=16 chunks (blockIdx.y): full-C state
// would need ~300 VGPRs/thread, so each chunk re-streams raw (4 MB; L2-
// resident after the first chunk) and owns 2 of the 8 groups.  All
// reductions are deterministic via per-block scratch partials folded by
// egnmp_sum_partials (no global atomics).
//
// Backward (three launches, no CSR -- the domain has no cross-point
// coupling): v is never recomputed.  The GroupNorm backward element is
// affine in v and v is affine in raw, so the dense part of d_raw is one
// 4x4 affine map per batch element and dW / dcb follow from the 14 raw
// moments; only the pooled argmax positions add a per-channel term.  See
// the derivation above the backward kernels.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include "common.h"

#define KG_THREADS 256
// channels per forward chunk (blockIdx.y): 4 (more blocks, the reduce is
// latency-bound at 1 wave/SIMD otherwise); the backward has no chunks

// shared folding / finalize / pick infrastructure (edge_gnmp.hip,
// group_norm.hip)
void launch_gn_finalize_scratch(const float *, long, float *, float *, long,
                                int, float, hipStream_t);
__global__ void egnmp_sum_partials_kernel(const float *__restrict__,
                                          float *__restrict__, long, int);
void launch_gnmp_pick(const float *, const float *, const unsigned char *,
                      const unsigned char *, const float *, const float *,
                      const float *, const float *, void *, unsigned char *,
                      float *, int, long, int, int, int, float,
                      const float *, bool, bool, hipStream_t);

// ---------------------------------------------------------------- forward

template <int KG_CH>
__global__ __launch_bounds__(KG_THREADS) void kg_fwd_reduce_kernel(
    const float *__restrict__ raw,  // (B, 4, K, N)
    const float *__restrict__ W,    // (C, 4)
    const float *__restrict__ cb,   // (C) conv bias
    float *__restrict__ scratch,    // (B*G*2, gridX*chunks*B)
    float *__restrict__ vmax, float *__restrict__ vmin,  // (B, N, C) fp32
    unsigned char *__restrict__ amax, unsigned char *__restrict__ amin,
    long N, int K, int C, int G) {
  const int b = blockIdx.z;
  const int B = gridDim.z;
  const int chunk = blockIdx.y;
  const int c0 = chunk * KG_CH;
  const int Cg = C / G;
  const int g0 = c0 / Cg;                       // first group touched
  const int NG = (c0 + KG_CH - 1) / Cg - g0 + 1;  // groups touched (<=8)
  const int n_out = B * G * 2;

  // weights are wave-uniform: the compiler keeps these in SGPRs
  float wr[KG_CH][4], br[KG_CH];
#pragma unroll
  for (int c = 0; c < KG_CH; ++c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) wr[c][e] = W[(c0 + c) * 4 + e];
    br[c] = cb[c0 + c];
  }

  // (waves, NG<=8, 2): this block's group sums, kept per wave and folded
  // in wave order so the result does not depend on wave scheduling
  constexpr int NW = KG_THREADS / WAVE;
  __shared__ float bins[NW * 16];
  if (threadIdx.x < (unsigned)(NW * 16)) bins[threadIdx.x] = 0.f;
  float *wbins = bins + wave_id() * 16;
  __syncthreads();

  const float *rawb = raw + (long)b * 4 * K * N;
  float s[8] = {}, ss[8] = {};  // per local group (launcher checks NG<=8)

  for (long n = (long)blockIdx.x * KG_THREADS + threadIdx.x; n < N;
       n += (long)gridDim.x * KG_THREADS) {
    float vmx[KG_CH], vmn[KG_CH], vs[KG_CH];
    int jmx[KG_CH], jmn[KG_CH];
#pragma unroll
    for (int c = 0; c < KG_CH; ++c) {
      vmx[c] = -INFINITY;
      vmn[c] = INFINITY;
      vs[c] = 0.f;
      jmx[c] = 0;
      jmn[c] = 0;
    }
    for (int j = 0; j < K; ++j) {
      const float r0 = rawb[((long)0 * K + j) * N + n];
      const float r1 = rawb[((long)1 * K + j) * N + n];
      const float r2 = rawb[((long)2 * K + j) * N + n];
      const float r3 = rawb[((long)3 * K + j) * N + n];
#pragma unroll
      for (int c = 0; c < KG_CH; ++c) {
        const float v = wr[c][0] * r0 + wr[c][1] * r1 + wr[c][2] * r2 +
                        wr[c][3] * r3 + br[c];
        vs[c] += v;
        ss[(c0 + c) / Cg - g0] += v * v;
        if (v > vmx[c]) {
          vmx[c] = v;
          jmx[c] = j;
        }
        if (v < vmn[c]) {
          vmn[c] = v;
          jmn[c] = j;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < KG_CH; ++c) s[(c0 + c) / Cg - g0] += vs[c];
    const long pi = ((long)b * N + n) * C + c0;
#pragma unroll
    for (int c4 = 0; c4 < KG_CH / 4; ++c4) {
      *(float4 *)(vmax + pi + c4 * 4) =
          make_float4(vmx[c4 * 4], vmx[c4 * 4 + 1], vmx[c4 * 4 + 2],
                      vmx[c4 * 4 + 3]);
      *(float4 *)(vmin + pi + c4 * 4) =
          make_float4(vmn[c4 * 4], vmn[c4 * 4 + 1], vmn[c4 * 4 + 2],
                      vmn[c4 * 4 + 3]);
      uchar4 ax, an;
      ax.x = (unsigned char)jmx[c4 * 4];
      ax.y = (unsigned char)jmx[c4 * 4 + 1];
      ax.z = (unsigned char)jmx[c4 * 4 + 2];
      ax.w = (unsigned char)jmx[c4 * 4 + 3];
      an.x = (unsigned char)jmn[c4 * 4];
      an.y = (unsigned char)jmn[c4 * 4 + 1];
      an.z = (unsigned char)jmn[c4 * 4 + 2];
      an.w = (unsigned char)jmn[c4 * 4 + 3];
      *(uchar4 *)(amax + pi + c4 * 4) = ax;
      *(uchar4 *)(amin + pi + c4 * 4) = an;
    }
  }
#pragma unroll
  for (int g = 0; g < 8; ++g)
    if (g < NG) {
      atomicAdd(&wbins[g * 2 + 0], s[g]);
      atomicAdd(&wbins[g * 2 + 1], ss[g]);
    }
  __syncthreads();
  // scratch layout: (B*G*2 rows, gridX*chunks*B cols); rows not covered
  // by this chunk get zero so the fold stays correct
  const long cols = (long)gridDim.x * gridDim.y * B;
  const long col = ((long)blockIdx.x * gridDim.y + chunk) * B + b;
  for (unsigned i = threadIdx.x; i < (unsigned)n_out; i += KG_THREADS) {
    const int row_b = i / (G * 2);
    const int row_g = (i % (G * 2)) / 2;
    const int half = i & 1;
    float v = 0.f;
    if (row_b == b && row_g >= g0 && row_g < g0 + NG) {
      const int k = (row_g - g0) * 2 + half;
      v = bins[k];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += bins[w * 16 + k];
    }
    scratch[(long)i * cols + col] = v;
  }
}

// ---------------------------------------------------------------- backward
//
// The GroupNorm backward element is affine in the conv output and the
// conv output is affine in the 4-vector raw[:, j, n], so the dense part of
// the gradient is a 4x4 affine map per batch element; only the pooled
// argmax positions carry a per-channel term.  With, per (b, c) of group g,
//   r = rstd[b,g], m = mean[b,g], s1/s2 = the two GN backward sums,
//   L = (C/G)*K*N, gsel[c,n] = gated, gamma-scaled pooled gradient,
//   p = r*(s1 + s2*r*(cb[c] - m))/L,   q = r*r*s2/L,
//   a[e] = sum_c p*W[c,e],   M[e,f] = sum_c q*W[c,e]*W[c,f],
//   S[e] = sum_{j,n} raw[e], RR[e,f] = sum_{j,n} raw[e]*raw[f]:
//   d_raw[e,j,n] = -(a[e] + sum_f M[e,f]*raw[f,j,n])
//                  + sum_{c: am[c,n]=j} W[c,e]*r*gsel[c,n]
//   dW[c,e] = sum_b (r*sum_n gsel*raw[e,am,n] - p*S[e]
//                    - q*sum_f W[c,f]*RR[f,e])
//   dcb[c]  = sum_b (r*sum_n gsel - p*K*N - q*sum_f W[c,f]*S[f])
// Three launches: reduce (pooled-domain sums, gathers, raw moments; fp32
// per-block partials), coefficients (fp64 fold + closed forms), apply
// (d_raw written once).

#define KG_NT 64            // points per reduce block / apply wave
#define KG_JC 8             // candidates per apply block
#define KG_NCOEF 20         // a[4] + M[4][4] per batch element
#define KG_COEF_THREADS 512
#define KG_CC 8             // channels per coefficient block
#define KG_TS 4             // tile ranges folded side by side
#define KG_CMAX 128         // launcher: C <= KG_CMAX, C / G >= 4
#define KG_NR 9             // partial rows per channel
#define KG_NVMAX (2 * (KG_CMAX / 4) + 30 + KG_NR * KG_CC)

// per-block partial row: [s1,s2 per g | (dbeta,dgamma) per c | dslope |
// P0 per c | P per (c,e) | S[4] | RR[10] | dslope low word | low words of
// S, RR | A per c | Bv per c].  The moments and dslope are fp64 sums kept
// as a high and a low fp32 word.  A / Bv: sums of gv and gv*(v - mean)
// over the negative-branch elements, for the dslope correction below.
__host__ __device__ inline int kg_npart(int C, int G) {
  return 2 * G + 9 * C + 30;
}

DEV_INLINE double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// pass 1.  One block = one tile of KG_NT points of one batch element.
// CM: dy is channel-major (B, C, N) and is staged through the LDS tile;
// otherwise (B, N, C), read directly.  Either way each (n, c) element is
// consumed by the same thread in the same order, so the two layouts give
// bit-equal results.  The tile is then reused to hand r*gsel and the
// argmax to the apply pass channel-major (coalesced for one point/lane).
// No atomics: per-thread sums go through LDS slots and are folded in
// thread order, so the block partial does not depend on scheduling.
template <typename T, bool CM>
__global__ __launch_bounds__(KG_THREADS) void kg_bwd_reduce_kernel(
    const T *__restrict__ dy,
    const float *__restrict__ raw,           // (B, 4, K, N)
    const float *__restrict__ W, const float *__restrict__ cb,
    const unsigned char *__restrict__ am,    // (B, N, C) pooled argmax
    const float *__restrict__ vsel,          // (B, N, C)
    const float *__restrict__ mean, const float *__restrict__ rstd,
    const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ part,                // (B, tiles, n_part)
    float *__restrict__ gsT,                 // (B, C, N) r * gsel
    unsigned char *__restrict__ amT,         // (B, C, N)
    long N, int K, int C, int G, const float *__restrict__ slope_ptr) {
  const int b = blockIdx.z;
  const long n0 = (long)blockIdx.x * KG_NT;
  const float slope = *slope_ptr;
  const int Cg = C / G;
  const int tpc = C / 4;
  const int ppb = KG_THREADS / tpc;
  const int p_l = (int)threadIdx.x / tpc;
  const int c4 = (int)threadIdx.x % tpc;
  const int n_part = kg_npart(C, G);
  const int o_c = 2 * G, o_sl = o_c + 2 * C, o_p0 = o_sl + 1,
            o_p = o_p0 + C, o_mo = o_p + 4 * C, o_sl_lo = o_mo + 14,
            o_mo_lo = o_mo + 15, o_a = o_mo + 29, o_bv = o_a + C;
  constexpr int NW = KG_THREADS / WAVE;
  constexpr int TP = KG_NT + 1;  // padded tile pitch
  constexpr int NV = 11;         // per-channel sums of one thread

  extern __shared__ float kg_smem[];
  float *tile = kg_smem;                       // (C, TP)
  float *res = tile + C * TP;                  // (n_part) block partial
  float *chs = res + n_part;                   // (2, C) per-channel s1/s2
  unsigned char *amS = (unsigned char *)(chs + 2 * C);  // (C, NT)
  __shared__ float st[NV * KG_THREADS];        // per-thread sums, one quad
  __shared__ double wmo[NW * 14];              // per-wave raw moments
  __shared__ double wsl[NW];                   // per-wave dslope
  if (CM) {
    for (unsigned i = threadIdx.x; i < (unsigned)(C * KG_NT);
         i += KG_THREADS) {
      const int c = i / KG_NT, nl = i % KG_NT;
      if (n0 + nl < N)
        tile[c * TP + nl] = (float)dy[((long)b * C + c) * N + n0 + nl];
    }
    __syncthreads();
  }

  // raw moments: lane = point, waves stride over j; the butterfly sums
  // are order-fixed.  fp64: the closed forms subtract them from each
  // other, and the group statistics re-derived from them in the
  // coefficient pass have to be better than the saved fp32 ones.
  {
    const int nl = threadIdx.x % KG_NT;
    const long n = n0 + nl;
    double S[4] = {}, RR[10] = {};
    if (n < N) {
      const float *rp = raw + (long)b * 4 * K * N + n;
      for (int j = threadIdx.x / KG_NT; j < K; j += KG_THREADS / KG_NT) {
        double x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (double)rp[((long)e * K + j) * N];
        int k = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          S[e] += x[e];
#pragma unroll
          for (int f = e; f < 4; ++f) RR[k++] += x[e] * x[f];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) S[e] = wave_sum_f64(S[e]);
#pragma unroll
    for (int k = 0; k < 10; ++k) RR[k] = wave_sum_f64(RR[k]);
    if (lane_id() == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) wmo[wave_id() * 14 + e] = S[e];
#pragma unroll
      for (int k = 0; k < 10; ++k) wmo[wave_id() * 14 + 4 + k] = RR[k];
    }
  }

  // pooled domain: thread = (point, channel quad); v[e] = {sum_dx,
  // sum_dxx, dbeta, dgamma, P0, P[4], A, Bv} of channel c4*4+e.  dslope
  // sums terms that cancel, so its element and its sum are formed in fp64.
  float v[4][NV] = {};
  double d_sl = 0.;
  if (p_l < ppb) {
    float m[4], r[4], ga[4], be[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c4 * 4 + e;
      m[e] = mean[b * G + c / Cg];
      r[e] = rstd[b * G + c / Cg];
      ga[e] = gamma[c];
      be[e] = beta[c];
    }
    const float *rawb = raw + (long)b * 4 * K * N;
    for (int nl = p_l; nl < KG_NT && n0 + nl < N; nl += ppb) {
      const long n = n0 + nl;
      const long pi = ((long)b * N + n) * C + c4 * 4;
      const float4 sv = *(const float4 *)(vsel + pi);
      const uchar4 aq = *(const uchar4 *)(am + pi);
      const float svv[4] = {sv.x, sv.y, sv.z, sv.w};
      const int ks[4] = {aq.x, aq.y, aq.z, aq.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c4 * 4 + e;
        const float xhat = (svv[e] - m[e]) * r[e];
        float gv = CM ? tile[c * TP + nl] : (float)dy[pi + e];
        const float pre = xhat * ga[e] + be[e];
        const float *rp = rawb + (long)ks[e] * N + n;
        float rv[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) rv[f] = rp[(long)f * K * N];
        if (pre <= 0.f) {
          // the minority branch after a max-pool: a few terms near
          // pre = 0, where the fp32 rounding of the saved v dominates the
          // sum, so v is re-formed in fp64 from the gathered raw
          double vd = (double)cb[c];
#pragma unroll
          for (int f = 0; f < 4; ++f)
            vd += (double)W[c * 4 + f] * (double)rv[f];
          const double vc = vd - (double)m[e];
          d_sl += (double)gv *
                  (vc * (double)r[e] * (double)ga[e] + (double)be[e]);
          v[e][9] += gv;
          v[e][10] += gv * (float)vc;
        }
        gv = pre > 0.f ? gv : gv * slope;
        const float dxhat = gv * ga[e];
        v[e][0] += dxhat;
        v[e][1] += dxhat * xhat;
        v[e][2] += gv;
        v[e][3] += gv * xhat;
        v[e][4] += dxhat;
#pragma unroll
        for (int f = 0; f < 4; ++f) v[e][5 + f] += dxhat * rv[f];
        tile[c * TP + nl] = dxhat * r[e];
        amS[c * KG_NT + nl] = (unsigned char)ks[e];
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d_sl += __shfl_xor(d_sl, off, WAVE);
  if (lane_id() == 0) wsl[wave_id()] = d_sl;
  // fold the per-thread sums over the points of the tile, one channel of
  // the quad per round, in thread order
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) st[k * KG_THREADS + threadIdx.x] = v[e][k];
    __syncthreads();
    for (int o = threadIdx.x; o < NV * tpc; o += KG_THREADS) {
      const int k = o / tpc, cq = o % tpc;
      double acc = 0.;
      for (int p = 0; p < ppb; ++p)
        acc += (double)st[k * KG_THREADS + p * tpc + cq];
      const int c = cq * 4 + e;
      const float a = (float)acc;
      if (k < 2) chs[k * C + c] = a;
      else if (k < 4) res[o_c + 2 * c + (k - 2)] = a;
      else if (k == 4) res[o_p0 + c] = a;
      else if (k < 9) res[o_p + c * 4 + (k - 5)] = a;
      else if (k == 9) res[o_a + c] = a;
      else res[o_bv + c] = a;
    }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)(2 * G)) {
    const int g = threadIdx.x >> 1, h = threadIdx.x & 1;
    double acc = 0.;
    for (int c = g * Cg; c < (g + 1) * Cg; ++c) acc += (double)chs[h * C + c];
    res[threadIdx.x] = (float)acc;
  } else if (threadIdx.x >= WAVE && threadIdx.x < WAVE + 14) {
    const int k = threadIdx.x - WAVE;
    double acc = wmo[k];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += wmo[w * 14 + k];
    const float hi = (float)acc;
    res[o_mo + k] = hi;
    res[o_mo_lo + k] = (float)(acc - (double)hi);
  } else if (threadIdx.x == 2 * WAVE) {
    double acc = wsl[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += wsl[w];
    const float hi = (float)acc;
    res[o_sl] = hi;
    res[o_sl_lo] = (float)(acc - (double)hi);
  }
  __syncthreads();
  float *prow = part + ((long)b * gridDim.x + blockIdx.x) * n_part;
  for (unsigned i = threadIdx.x; i < (unsigned)n_part; i += KG_THREADS)
    prow[i] = res[i];
  for (unsigned i = threadIdx.x; i < (unsigned)(C * KG_NT); i += KG_THREADS) {
    const int c = i / KG_NT, nl = i % KG_NT;
    if (n0 + nl < N) {
      const long o = ((long)b * C + c) * N + n0 + nl;
      gsT[o] = tile[c * TP + nl];
      amT[o] = amS[c * KG_NT + nl];
    }
  }
}

// pass 2: fold the block partials in fixed order in fp64 and evaluate the
// closed forms.  Block (s, b) owns KG_CC channels of batch element b: it
// folds their rows plus the group sums and the moments, and writes that
// batch element's share of dW / dcb / dgamma / dbeta to pgrad (B, 7, C)
// fp64 (+ one dslope share per block behind it); the apply pass sums the
// shares.  Block (0, b) also writes coef (B, 20) = a[4] | M[4][4] in fp32.
__global__ __launch_bounds__(KG_COEF_THREADS) void kg_bwd_coef_kernel(
    const float *__restrict__ part, const float *__restrict__ W,
    const float *__restrict__ cb, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gamma,
    float eps, float *__restrict__ coef, double *__restrict__ pgrad,
    int tiles, long N, int K, int C, int G) {
  const int b = blockIdx.y, B = gridDim.y;
  const int c0 = blockIdx.x * KG_CC;
  const int n_part = kg_npart(C, G);
  const int o_c = 2 * G, o_sl = o_c + 2 * C, o_p0 = o_sl + 1,
            o_p = o_p0 + C, o_mo = o_p + 4 * C, o_mo_lo = o_mo + 15,
            o_a = o_mo + 29, o_bv = o_a + C;
  const int Cg = C / G;
  const int tid = threadIdx.x;
  // local rows: [s1,s2 per g | S[4] RR[10] dslope-low | dslope-high |
  // low words of S, RR | (dbeta, dgamma, P0, P[4], A, Bv) per owned
  // channel]
  const int l_mo = 2 * G, l_molo = l_mo + 16, l_ch = l_mo + 30;
  const int nv = l_ch + KG_NR * KG_CC;
  __shared__ double f4[KG_TS * KG_NVMAX], fold[KG_NVMAX], pq[2 * KG_CMAX],
      slc[KG_CC];

  const int th = (tiles + KG_TS - 1) / KG_TS;
  for (int s = tid; s < nv * KG_TS; s += KG_COEF_THREADS) {
    const int h = s / nv, lv = s % nv;
    int row;
    if (lv < l_mo) {
      row = lv;
    } else if (lv < l_mo + 15) {
      row = o_mo + (lv - l_mo);
    } else if (lv == l_mo + 15) {
      row = o_sl;
    } else if (lv < l_ch) {
      row = o_mo_lo + (lv - l_molo);
    } else {
      const int t = lv - l_ch, c = c0 + t / KG_NR, k = t % KG_NR;
      row = k < 2    ? o_c + 2 * c + k
            : k == 2 ? o_p0 + c
            : k < 7  ? o_p + 4 * c + k - 3
            : k == 7 ? o_a + c
                     : o_bv + c;
    }
    const int t0 = h * th, t1 = min(tiles, t0 + th);
    const float *src = part + (long)b * tiles * n_part + row;
    double acc = 0.;
#pragma unroll 16
    for (int t = t0; t < t1; ++t) acc += (double)src[(long)t * n_part];
    f4[h * KG_NVMAX + lv] = acc;
  }
  __syncthreads();
  for (int lv = tid; lv < nv; lv += KG_COEF_THREADS) {
    double a = f4[lv];
#pragma unroll
    for (int h = 1; h < KG_TS; ++h) a += f4[h * KG_NVMAX + lv];
    fold[lv] = a;
  }
  __syncthreads();
  if (tid < 14) fold[l_mo + tid] += fold[l_molo + tid];  // high + low word
  __syncthreads();

  const double L = (double)Cg * (double)K * (double)N;
  const double KN = (double)K * (double)N;
  if (tid < KG_CC) {
    const int c = c0 + tid;
    const int g = c / Cg;
    const double r = (double)rstd[b * G + g], m = (double)mean[b * G + g];
    const double s1 = fold[2 * g], s2 = fold[2 * g + 1];
    const double p = r * (s1 + s2 * r * ((double)cb[c] - m)) / L;
    const double q = r * r * s2 / L;
    const double *S = fold + l_mo;
    const double *RR = S + 4;  // upper triangle, row-major
    const double *ch = fold + l_ch + tid * KG_NR;
    double w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (double)W[c * 4 + e];
    double wS = 0.;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double wrr = 0.;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int lo = e < f ? e : f, hi = e < f ? f : e;
        wrr += w[f] * RR[lo * 4 - lo * (lo - 1) / 2 + (hi - lo)];
      }
      pgrad[((long)b * 7 + e) * C + c] = r * ch[3 + e] - p * S[e] - q * wrr;
      wS += w[e] * S[e];
    }
    pgrad[((long)b * 7 + 4) * C + c] = r * ch[2] - p * KN - q * wS;
    pgrad[((long)b * 7 + 5) * C + c] = ch[1];
    pgrad[((long)b * 7 + 6) * C + c] = ch[0];
    // dslope: the reduce pass formed its terms with the saved fp32 mean /
    // rstd, whose last-bit errors are the whole error of a sum of a few
    // terms near pre = 0.  Group statistics in fp64 from the fp64 moments:
    //   mean = avg_c (W_c.S/KN + cb_c)
    //   E[v^2] = avg_c (W_c RR W_c^T/KN + 2 cb_c W_c.S/KN + cb_c^2)
    // and, exactly, pre(md, rd) = pre(m, r)
    //   + gamma*((v - m)*(rd - r) - rd*(md - m)), summed as A / Bv.
    double gm = 0., ge2 = 0.;
    for (int cc = g * Cg; cc < (g + 1) * Cg; ++cc) {
      double u[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = (double)W[cc * 4 + e];
      double uS = 0., uRu = 0.;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uS += u[e] * S[e];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const int lo = e < f ? e : f, hi = e < f ? f : e;
          uRu += u[e] * u[f] * RR[lo * 4 - lo * (lo - 1) / 2 + (hi - lo)];
        }
      }
      const double bc = (double)cb[cc];
      gm += uS / KN + bc;
      ge2 += uRu / KN + 2. * bc * uS / KN + bc * bc;
    }
    const double md = gm / (double)Cg;
    const double var = ge2 / (double)Cg - md * md;
    const double rd = 1. / sqrt((var > 0. ? var : 0.) + (double)eps);
    slc[tid] = (double)gamma[c] * ((rd - r) * ch[8] - rd * (md - m) * ch[7]);
  }
  __syncthreads();
  if (tid == 0) {
    // this block's dslope share; block 0 adds the in-pass sum
    double acc = blockIdx.x == 0 ? fold[l_mo + 15] + fold[l_mo + 14] : 0.;
#pragma unroll
    for (int i = 0; i < KG_CC; ++i) acc += slc[i];
    pgrad[(long)B * 7 * C + (long)b * gridDim.x + blockIdx.x] = acc;
  }
  if (blockIdx.x != 0) return;
  for (int c = tid; c < C; c += KG_COEF_THREADS) {
    const int g = c / Cg;
    const double r = (double)rstd[b * G + g], m = (double)mean[b * G + g];
    const double s1 = fold[2 * g], s2 = fold[2 * g + 1];
    pq[c] = r * (s1 + s2 * r * ((double)cb[c] - m)) / L;
    pq[KG_CMAX + c] = r * r * s2 / L;
  }
  __syncthreads();
  // 20 outputs x 16 lanes: strided partial sums, then a butterfly inside
  // each 16-lane group (order-fixed)
  if (tid < KG_NCOEF * 16) {
    const int o = tid / 16, l = tid % 16;
    double acc = 0.;
    if (o < 4) {
      for (int c = l; c < C; c += 16) acc += pq[c] * (double)W[c * 4 + o];
    } else {
      const int e = (o - 4) / 4, f = (o - 4) % 4;
      for (int c = l; c < C; c += 16)
        acc += pq[KG_CMAX + c] * (double)W[c * 4 + e] * (double)W[c * 4 + f];
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
    if (l == 0) coef[b * KG_NCOEF + o] = (float)acc;
  }
}

// pass 3: one point per lane, KG_JC candidates per block, d_raw written
// once.  The sparse term is a channel loop with statically unrolled slot
// compares (a dynamically indexed accumulator array would go to scratch);
// channels are added in index order, so the result is order-fixed.  a, M
// and W are wave-uniform (SGPR operands).
__global__ __launch_bounds__(KG_NT) void kg_bwd_apply_kernel(
    const float *__restrict__ raw, const float *__restrict__ W,
    const float *__restrict__ coef, const float *__restrict__ gsT,
    const unsigned char *__restrict__ amT, float *__restrict__ draw,
    const double *__restrict__ pgrad, float *__restrict__ dW,
    float *__restrict__ dcb, float *__restrict__ dgamma,
    float *__restrict__ dbeta, float *__restrict__ dslope, int accumulate,
    long N, int K, int C) {
  const int b = blockIdx.z;
  const int j_lo = blockIdx.y * KG_JC;
  const long n = (long)blockIdx.x * KG_NT + threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && b == 0) {
    // parameter gradients: sum the per-b shares in order; written, or
    // added into the parameters' fp32 grad buffers (one writer per
    // element, so no atomics)
    const int B = gridDim.z;
    for (int i = threadIdx.x; i < 7 * C + 1; i += KG_NT) {
      const int k = i / C, c = i % C;
      double acc = 0.;
      if (k < 7) {
        for (int bb = 0; bb < B; ++bb)
          acc += pgrad[((long)bb * 7 + k) * C + c];
      } else {  // dslope: one share per coefficient block
        for (int s = 0; s < B * (C / KG_CC); ++s)
          acc += pgrad[(long)B * 7 * C + s];
      }
      float *dst = k < 4    ? dW + c * 4 + k
                   : k == 4 ? dcb + c
                   : k == 5 ? dgamma + c
                   : k == 6 ? dbeta + c
                            : dslope;
      *dst = accumulate ? *dst + (float)acc : (float)acc;
    }
  }
  if (n >= N) return;
  float a[4], M[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = coef[b * KG_NCOEF + e];
#pragma unroll
    for (int f = 0; f < 4; ++f) M[e][f] = coef[b * KG_NCOEF + 4 + e * 4 + f];
  }
  const float *rawb = raw + (long)b * 4 * K * N + n;
  float d[KG_JC][4];
#pragma unroll
  for (int jj = 0; jj < KG_JC; ++jj) {
    const int j = j_lo + jj;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < K) {
#pragma unroll
      for (int f = 0; f < 4; ++f) x[f] = rawb[((long)f * K + j) * N];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      d[jj][e] = -(a[e] + M[e][0] * x[0] + M[e][1] * x[1] + M[e][2] * x[2] +
                   M[e][3] * x[3]);
  }
  const float *gp = gsT + (long)b * C * N + n;
  const unsigned char *ap = amT + (long)b * C * N + n;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const int jr = (int)ap[(long)c * N] - j_lo;
    const float g = gp[(long)c * N];
    float t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = W[c * 4 + e] * g;
#pragma unroll
    for (int jj = 0; jj < KG_JC; ++jj) {
      const float hit = jr == jj ? 1.f : 0.f;  // exact: adds t or 0
#pragma unroll
      for (int e = 0; e < 4; ++e) d[jj][e] = fmaf(hit, t[e], d[jj][e]);
    }
  }
  float *dp = draw + (long)b * 4 * K * N + n;
#pragma unroll
  for (int jj = 0; jj < KG_JC; ++jj) {
    const int j = j_lo + jj;
    if (j < K) {
#pragma unroll
      for (int e = 0; e < 4; ++e) dp[((long)e * K + j) * N] = d[jj][e];
    }
  }
}

// --------------------------------------------------------------- launchers

void launch_kg_fwd(const float *raw, const float *W, const float *cb,
                   float *scratch, float *ws, float *mean, float *rstd,
                   const float *gamma, const float *beta, float *vmax,
                   float *vmin, unsigned char *amax, unsigned char *amin,
                   void *y, unsigned char *am, float *vsel,
                   int B, long N, int K, int C, int G, float eps,
                   const float *slope_ptr, bool bf16, int nblk,
                   bool channel_major, hipStream_t stream) {
  const int chunks = C / 4;
  const dim3 grid(nblk, chunks, B);
  hipLaunchKernelGGL(kg_fwd_reduce_kernel<4>, grid, dim3(KG_THREADS), 0,
                     stream, raw, W, cb, scratch, vmax, vmin, amax, amin, N,
                     K, C, G);
  (void)ws;
  launch_gn_finalize_scratch(scratch, (long)nblk * chunks * B, mean, rstd,
                             (long)(C / G) * K * N, B * G, eps, stream);
  launch_gnmp_pick(vmax, vmin, amax, amin, mean, rstd, gamma, beta, y, am,
                   vsel, B, N, C, G, 2, 0.f, slope_ptr, bf16, channel_major,
                   stream);
}

int kg_bwd_tiles(long N) { return (int)((N + KG_NT - 1) / KG_NT); }
long kg_bwd_part_len(int B, long N, int C, int G) {
  return (long)B * kg_bwd_tiles(N) * kg_npart(C, G);
}
// fp64 per-b shares of the parameter gradients, in floats
long kg_bwd_pgrad_len(int B, int C) {
  return 2 * ((long)B * 7 * C + (long)B * (C / KG_CC));
}

// dy: (B, C, N) when dy_channel_major else (B, N, C).  accumulate: the
// five parameter gradients are ADDED into dW..dslope (the parameters' own
// fp32 grad buffers) instead of written.
void launch_kg_bwd(const void *dy, bool dy_channel_major, const float *raw,
                   const float *W, const float *cb, const unsigned char *am,
                   const float *vsel, const float *mean, const float *rstd,
                   const float *gamma, const float *beta, float *part,
                   float *coef, double *pgrad, float *gsT,
                   unsigned char *amT, float *draw, float *dW, float *dcb,
                   float *dgamma, float *dbeta,
                   float *dslope, bool accumulate, int B, long N, int K,
                   int C, int G, float eps, const float *slope_ptr, bool bf16,
                   hipStream_t stream) {
  const int tiles = kg_bwd_tiles(N);
  const int n_part = kg_npart(C, G);
  {
    const dim3 rgrid(tiles, 1, B);
    const size_t lds =
        ((size_t)C * (KG_NT + 1) + (size_t)n_part + 2 * C) * sizeof(float) +
        (size_t)C * KG_NT;
#define KG_RED(T, CM)                                                       \
  hipLaunchKernelGGL((kg_bwd_reduce_kernel<T, CM>), rgrid,                  \
                     dim3(KG_THREADS), lds, stream, (const T *)dy, raw, W,  \
                     cb, am, vsel, mean, rstd, gamma, beta, part, gsT, amT, \
                     N, K, C, G, slope_ptr)
    if (bf16) {
      if (dy_channel_major) KG_RED(__hip_bfloat16, true);
      else KG_RED(__hip_bfloat16, false);
    } else {
      if (dy_channel_major) KG_RED(float, true);
      else KG_RED(float, false);
    }
#undef KG_RED
  }
  hipLaunchKernelGGL(kg_bwd_coef_kernel, dim3(C / KG_CC, B),
                     dim3(KG_COEF_THREADS), 0, stream, part, W, cb, mean,
                     rstd, gamma, eps, coef, pgrad, tiles, N, K, C, G);
  {
    const dim3 agrid(tiles, (K + KG_JC - 1) / KG_JC, B);
    hipLaunchKernelGGL(kg_bwd_apply_kernel, agrid, dim3(KG_NT), 0, stream,
                       raw, W, coef, gsT, amT, draw, pgrad, dW, dcb, dgamma,
                       dbeta, dslope, accumulate ? 1 : 0, N, K, C);
  }
}
