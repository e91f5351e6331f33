// K23: robust ground-plane fit (absent in the reference): seeded RANSAC
// hypotheses, exact integer scores, Tukey-biweight refinement, per-point
// heights.  Four launches, kernel boundaries are the only global
// synchronisation, no host sync, every loop capped, bit-reproducible.
//
//   A  plane_hyp_kernel     one lane per (b, h): three seeded draws (first
//                           eligible of 8 tries per slot), the plane through
//                           them, the validity tests.  Writes idx, a record
//                           (n, t2, p0, n.up) and count = 0 (valid) / -1.
//   B  plane_score_kernel   H x N point-to-plane tests.  One HYPOTHESIS per
//                           lane (record in registers, private int counter);
//                           a tile of PL_TILE points is staged in LDS as
//                           three coordinate planes and read by broadcast
//                           (all lanes read the same address), ineligible
//                           points as x = NaN so every comparison fails.
//                           grid (point tiles, ceil(H / PL_BLOCK), B), one
//                           integer atomicAdd per lane at the end: exact and
//                           order-independent.  Invalid hypotheses skip it.
//   C  plane_refine_kernel  one workgroup of 512 lanes (8 waves) per batch
//                           element: argmax over H (ties to the smallest h),
//                           then up to 16 rounds of reweighted least squares.
//                           The points stream from global memory (L2) in
//                           every round; eleven fp64 sums (W, sum w q, sum w
//                           q q^T, #w>0) of pivot-centred points q = p - p0
//                           go through a wave butterfly and a fixed-order
//                           LDS fold of the 8 wave sums; lane 0 runs a cyclic
//                           Jacobi of the 3x3 covariance in fp64 (statically
//                           indexed, at most PL_SWEEPS sweeps).  A rejected
//                           round ends the loop: the plane did not move, so
//                           the next round would be rejected again.
//   D  plane_height_kernel  elementwise over (B, N): fp64 pivot-centred
//                           height rounded to fp32, and both labels.
//
// Stage A/B arithmetic is fp32 with every operation rounded on its own
// (fp contract off for this file), so the counts are the same integers as in
// the torch reference and the numpy oracle.
//
// Layout of B: hypothesis-per-lane was chosen because it is the layout
// knn_interp.hip and chamfer.hip already use (LDS broadcast tile, private
// counter, no cross-lane traffic in the loop) and needs one atomic per lane;
// the mirror layout (points in registers, hypotheses wave-uniform, ballot +
// popcount) was NOT built or measured.  PL_TILE = 256 gives 32 workgroups at
// N = 8192 and 512 at N = 131072 for H <= 256 (256 CUs): the small case is
// launch-latency bound either way, the large one fills the chip twice.
//
// C runs on one CU per batch element.  With 1024 lanes the eleven fp64
// accumulators next to the fp64 Jacobi did not fit the 128 VGPRs that 16 waves
// per workgroup leave (36 bytes of scratch), so it runs 512 lanes.  Measured
// on MI355X at H = 256, 3 rounds (scripts/ground_bench.py): A + B take 0.029
// ms at every N from 8192 to 131072, the whole call 0.052 / 0.094 / 0.271 ms
// at N = 8192 / 32768 / 131072, i.e. C + D dominate at the large size (0.24
// ms).  Splitting a round over several workgroups would need a launch per
// round (partials folded by the next kernel); it was not done: the call is
// 2 % of one 8192-point Predictor call at N = 131072.  Loading 4 or 8 points
// per lane ahead of their use was tried and measured slower (0.296 against
// 0.270 ms at N = 131072, alternating runs): about 45 fp64 operations per
// point and round keep one CU busy, the L2 latency is not what it waits for.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), no AGPRs
// and scratch 0 bytes for all four:
//   plane_hyp_kernel     28 VGPRs, LDS 0 bytes
//   plane_score_kernel   43 VGPRs, LDS 3072 bytes
//   plane_refine_kernel  151 VGPRs, LDS 904 bytes
//   plane_height_kernel  8 VGPRs, LDS 0 bytes
#include <hip/hip_runtime.h>
#include "common.h"

#pragma clang fp contract(off)

#define PL_BLOCK 256   // hypotheses (lanes) per workgroup of A and B
#define PL_TILE 256    // points per LDS tile of B
#define PL_TRIES 8
#define PL_RF_THREADS 512
#define PL_RF_WAVES (PL_RF_THREADS / WAVE)
#define PL_NSUM 11
#define PL_SWEEPS 12
#define PL_REC 8       // floats per hypothesis record
#define PL_P64 8       // doubles per final plane: n(3), dp, p0(3), ok
#define PL_GAP 1e-9    // eigenvalue separation, relative to the largest

int plane_score_tile() { return PL_TILE; }
int plane_score_block() { return PL_BLOCK; }
int plane_refine_block() { return PL_RF_THREADS; }

DEV_INLINE unsigned pl_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

DEV_INLINE bool pl_eligible(const float *__restrict__ xyz,
                            const unsigned char *__restrict__ mask, long i) {
  if (mask && !mask[i]) return false;
  return isfinite(xyz[i * 3 + 0]) && isfinite(xyz[i * 3 + 1]) &&
         isfinite(xyz[i * 3 + 2]);
}

// ---- A ---------------------------------------------------------------------
__global__ __launch_bounds__(PL_BLOCK) void plane_hyp_kernel(
    const float *__restrict__ xyz,           // (B, N, 3)
    const unsigned char *__restrict__ mask,  // (B, N) or null
    int *__restrict__ idx_out,               // (B, H, 3)
    float *__restrict__ rec,                 // (B, H, PL_REC)
    int *__restrict__ count,                 // (B, H)
    int N, int H, unsigned seed, float upx, float upy, float upz, float cos2,
    float thresh2) {
  const int h = blockIdx.x * PL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (h >= H) return;
  xyz += (long)b * N * 3;
  if (mask) mask += (long)b * N;
  const unsigned key = pl_mix(seed ^ pl_mix((unsigned)b * 0x9E3779B1u + 1u));

  int id[3];
  bool valid = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int pick = -1;
#pragma unroll
    for (int t = 0; t < PL_TRIES; ++t) {
      const unsigned c =
          pl_mix(key ^ (((unsigned)h * 3u + (unsigned)j) * 8u + (unsigned)t)) %
          (unsigned)N;
      if (pick < 0 && pl_eligible(xyz, mask, (long)c)) pick = (int)c;
    }
    id[j] = pick;
    valid = valid && pick >= 0;
  }
  valid = valid && id[0] != id[1] && id[0] != id[2] && id[1] != id[2];

  float nx = 0.f, ny = 0.f, nz = 0.f, t2 = -1.f, nu = 0.f;
  float p0x = 0.f, p0y = 0.f, p0z = 0.f;
  if (valid) {
    p0x = xyz[(long)id[0] * 3 + 0];
    p0y = xyz[(long)id[0] * 3 + 1];
    p0z = xyz[(long)id[0] * 3 + 2];
    const float ux = xyz[(long)id[1] * 3 + 0] - p0x;
    const float uy = xyz[(long)id[1] * 3 + 1] - p0y;
    const float uz = xyz[(long)id[1] * 3 + 2] - p0z;
    const float vx = xyz[(long)id[2] * 3 + 0] - p0x;
    const float vy = xyz[(long)id[2] * 3 + 1] - p0y;
    const float vz = xyz[(long)id[2] * 3 + 2] - p0z;
    nx = (uy * vz) - (uz * vy);
    ny = (uz * vx) - (ux * vz);
    nz = (ux * vy) - (uy * vx);
    const float nn = (nx * nx + ny * ny) + nz * nz;
    nu = (nx * upx + ny * upy) + nz * upz;
    valid = isfinite(nn) && nn > 0.f && nu * nu >= cos2 * nn;
    t2 = thresh2 * nn;
  }
  const long o = (long)b * H + h;
  float *r = rec + o * PL_REC;
  if (!valid) {
    id[0] = id[1] = id[2] = -1;
    t2 = -1.f;  // no e * e is <= -1: the score loop counts nothing
  }
  idx_out[o * 3 + 0] = id[0];
  idx_out[o * 3 + 1] = id[1];
  idx_out[o * 3 + 2] = id[2];
  r[0] = nx, r[1] = ny, r[2] = nz, r[3] = t2;
  r[4] = p0x, r[5] = p0y, r[6] = p0z, r[7] = nu;
  count[o] = valid ? 0 : -1;
}

// ---- B ---------------------------------------------------------------------
__global__ __launch_bounds__(PL_BLOCK) void plane_score_kernel(
    const float *__restrict__ xyz, const unsigned char *__restrict__ mask,
    const float *__restrict__ rec, int *__restrict__ count, int N, int H) {
  __shared__ float sx[PL_TILE], sy[PL_TILE], sz[PL_TILE];
  const int b = blockIdx.z;
  const int h = blockIdx.y * PL_BLOCK + threadIdx.x;
  xyz += (long)b * N * 3;
  if (mask) mask += (long)b * N;

  // PL_TILE == PL_BLOCK: every lane stages one point
  {
    const long i = (long)blockIdx.x * PL_TILE + threadIdx.x;
    float x = NAN, y = 0.f, z = 0.f;
    if (i < N && pl_eligible(xyz, mask, i)) {
      x = xyz[i * 3 + 0];
      y = xyz[i * 3 + 1];
      z = xyz[i * 3 + 2];
    }
    sx[threadIdx.x] = x;
    sy[threadIdx.x] = y;
    sz[threadIdx.x] = z;
  }
  __syncthreads();

  float nx = 0.f, ny = 0.f, nz = 0.f, t2 = -1.f, px = 0.f, py = 0.f, pz = 0.f;
  if (h < H) {
    const float *r = rec + ((long)b * H + h) * PL_REC;
    nx = r[0], ny = r[1], nz = r[2], t2 = r[3];
    px = r[4], py = r[5], pz = r[6];
  }
  int cnt = 0;
#pragma unroll 8
  for (int i = 0; i < PL_TILE; ++i) {
    const float e = ((sx[i] - px) * nx + (sy[i] - py) * ny) + (sz[i] - pz) * nz;
    cnt += (e * e <= t2) ? 1 : 0;
  }
  if (h < H && t2 >= 0.f && cnt > 0) atomicAdd(&count[(long)b * H + h], cnt);
}

// ---- C ---------------------------------------------------------------------
struct PlShared {
  double part[PL_RF_WAVES][PL_NSUM];
  double tot[PL_NSUM];
  double plane[4];  // n (3), dp  (pivot frame)
  long long wkey[PL_RF_WAVES];
  long long best;
  int go;
};

DEV_INLINE double pl_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

DEV_INLINE long long pl_wave_max(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(v, off, WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// one two-sided Jacobi rotation of the symmetric A on the (P, Q) plane
template <int P, int Q>
DEV_INLINE void pl_jacobi_rot(double (&A)[3][3], double (&V)[3][3], bool &moved) {
  const double apq = A[P][Q];
  const double app = A[P][P], aqq = A[Q][Q];
  if (apq * apq <= 1e-32 * fabs(app * aqq) || apq == 0.0) return;
  moved = true;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double s = c * t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

__global__ __launch_bounds__(PL_RF_THREADS) void plane_refine_kernel(
    const float *__restrict__ xyz, const unsigned char *__restrict__ mask,
    const float *__restrict__ rec, const int *__restrict__ count,
    float *__restrict__ normal_out,       // (B, 3)
    float *__restrict__ offset_out,       // (B)
    int *__restrict__ count_out,          // (B)
    int *__restrict__ best_out,           // (B)
    int *__restrict__ rounds_out,         // (B)
    unsigned char *__restrict__ ok_out,   // (B)
    double *__restrict__ plane64,         // (B, PL_P64)
    int N, int H, int iters, double thresh, float upx, float upy, float upz,
    float cos2) {
  __shared__ PlShared sh;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  xyz += (long)b * N * 3;
  if (mask) mask += (long)b * N;
  rec += (long)b * H * PL_REC;
  count += (long)b * H;

  // ---- argmax over H: largest count, ties to the smallest h ---------------
  long long key = -1;
  for (int h = tid; h < H; h += PL_RF_THREADS) {  // H <= 4096: <= 8 trips
    const int c = count[h];
    if (c >= 0) {
      const long long k = ((long long)c << 32) | (long long)(0x7fffffff - h);
      key = k > key ? k : key;
    }
  }
  key = pl_wave_max(key);
  if (lane_id() == 0) sh.wkey[wave_id()] = key;
  __syncthreads();
  if (tid == 0) {
    long long m = -1;
#pragma unroll
    for (int w = 0; w < PL_RF_WAVES; ++w) m = sh.wkey[w] > m ? sh.wkey[w] : m;
    sh.best = m;
  }
  __syncthreads();
  const long long bk = sh.best;
  if (bk < 0) {  // block-uniform: no valid hypothesis
    if (tid == 0) {
      normal_out[b * 3 + 0] = upx;
      normal_out[b * 3 + 1] = upy;
      normal_out[b * 3 + 2] = upz;
      offset_out[b] = 0.f;
      count_out[b] = 0;
      best_out[b] = -1;
      rounds_out[b] = 0;
      ok_out[b] = 0;
      double *p = plane64 + (long)b * PL_P64;
#pragma unroll
      for (int a = 0; a < PL_P64; ++a) p[a] = 0.0;
    }
    return;
  }
  const int best = 0x7fffffff - (int)(bk & 0xffffffffll);
  const int best_count = (int)(bk >> 32);
  const float *r = rec + (long)best * PL_REC;
  const double p0x = r[4], p0y = r[5], p0z = r[6];
  const double ux = upx, uy = upy, uz = upz;
  double nx, ny, nz, dp = 0.0;
  {
    const double ax = r[0], ay = r[1], az = r[2];
    const double s = (r[7] < 0.f ? -1.0 : 1.0) / sqrt(ax * ax + ay * ay + az * az);
    nx = ax * s, ny = ay * s, nz = az * s;
  }
  const double inv_th = 1.0 / thresh;
  int rounds = 0;

  for (int k = 0; k < iters; ++k) {  // iters <= 16
    double acc[PL_NSUM];
#pragma unroll
    for (int j = 0; j < PL_NSUM; ++j) acc[j] = 0.0;
#pragma unroll 2
    for (int i = tid; i < N; i += PL_RF_THREADS) {
      const float fx = xyz[(long)i * 3 + 0], fy = xyz[(long)i * 3 + 1],
                  fz = xyz[(long)i * 3 + 2];
      const bool el = (!mask || mask[i]) && isfinite(fx) && isfinite(fy) && isfinite(fz);
      const double qx = (double)fx - p0x, qy = (double)fy - p0y, qz = (double)fz - p0z;
      const double hh = (nx * qx + ny * qy + nz * qz) + dp;
      double w = 0.0;
      if (el && fabs(hh) < thresh) {
        const double u = hh * inv_th;
        const double v = 1.0 - u * u;
        w = v * v;
      }
      if (w > 0.0) {
        const double wx = w * qx, wy = w * qy, wz = w * qz;
        acc[0] += w;
        acc[1] += wx;
        acc[2] += wy;
        acc[3] += wz;
        acc[4] = fma(wx, qx, acc[4]);
        acc[5] = fma(wx, qy, acc[5]);
        acc[6] = fma(wx, qz, acc[6]);
        acc[7] = fma(wy, qy, acc[7]);
        acc[8] = fma(wy, qz, acc[8]);
        acc[9] = fma(wz, qz, acc[9]);
        acc[10] += 1.0;
      }
    }
#pragma unroll
    for (int j = 0; j < PL_NSUM; ++j) acc[j] = pl_wave_sum(acc[j]);
    if (lane_id() == 0) {
#pragma unroll
      for (int j = 0; j < PL_NSUM; ++j) sh.part[wave_id()][j] = acc[j];
    }
    __syncthreads();
    if (tid < PL_NSUM) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < PL_RF_WAVES; ++w) s += sh.part[w][tid];
      sh.tot[tid] = s;
    }
    __syncthreads();

    if (tid == 0) {
      bool good = false;
      double mx = 0.0, my = 0.0, mz = 0.0, ndp = 0.0;
      const double W = sh.tot[0];
      if (sh.tot[10] >= 3.0 && W > 0.0) {
        const double iw = 1.0 / W;
        const double cx = sh.tot[1] * iw, cy = sh.tot[2] * iw, cz = sh.tot[3] * iw;
        double A[3][3], V[3][3];
        A[0][0] = sh.tot[4] - W * cx * cx;
        A[0][1] = A[1][0] = sh.tot[5] - W * cx * cy;
        A[0][2] = A[2][0] = sh.tot[6] - W * cx * cz;
        A[1][1] = sh.tot[7] - W * cy * cy;
        A[1][2] = A[2][1] = sh.tot[8] - W * cy * cz;
        A[2][2] = sh.tot[9] - W * cz * cz;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) V[a][c] = a == c ? 1.0 : 0.0;
        for (int sweep = 0; sweep < PL_SWEEPS; ++sweep) {
          bool moved = false;
          pl_jacobi_rot<0, 1>(A, V, moved);
          pl_jacobi_rot<0, 2>(A, V, moved);
          pl_jacobi_rot<1, 2>(A, V, moved);
          if (!moved) break;
        }
        const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
        // smallest eigenvalue (ties to the lowest column), statically selected
        const bool s0 = l0 <= l1 && l0 <= l2;
        const bool s1 = !s0 && l1 <= l2;
        const double lmin = s0 ? l0 : (s1 ? l1 : l2);
        const double lmax = fmax(l0, fmax(l1, l2));
        const double la = s0 ? l1 : l0, lb = s0 ? l2 : (s1 ? l2 : l1);
        const double lmid = fmin(la, lb);
        mx = s0 ? V[0][0] : (s1 ? V[0][1] : V[0][2]);
        my = s0 ? V[1][0] : (s1 ? V[1][1] : V[1][2]);
        mz = s0 ? V[2][0] : (s1 ? V[2][1] : V[2][2]);
        const double nrm = sqrt(mx * mx + my * my + mz * mz);
        const bool sep = (lmid - lmin) > PL_GAP * lmax;
        if (sep && nrm > 0.0 && isfinite(nrm)) {
          double d = mx * ux + my * uy + mz * uz;
          const double s = (d < 0.0 ? -1.0 : 1.0) / nrm;
          mx *= s, my *= s, mz *= s;
          d = mx * ux + my * uy + mz * uz;
          ndp = -(mx * cx + my * cy + mz * cz);
          good = d * d >= (double)cos2 && isfinite(ndp);
        }
      }
      if (good) {
        sh.plane[0] = mx, sh.plane[1] = my, sh.plane[2] = mz, sh.plane[3] = ndp;
      }
      sh.go = good ? 1 : 0;
    }
    __syncthreads();
    const bool go = sh.go != 0;
    if (go) {
      nx = sh.plane[0], ny = sh.plane[1], nz = sh.plane[2], dp = sh.plane[3];
      ++rounds;
    }
    __syncthreads();  // sh.plane / sh.part are rewritten in the next round
    if (!go) break;   // block-uniform: the same plane would be rejected again
  }

  if (tid == 0) {
    normal_out[b * 3 + 0] = (float)nx;
    normal_out[b * 3 + 1] = (float)ny;
    normal_out[b * 3 + 2] = (float)nz;
    offset_out[b] = (float)(dp - (nx * p0x + ny * p0y + nz * p0z));
    count_out[b] = best_count;
    best_out[b] = best;
    rounds_out[b] = rounds;
    ok_out[b] = 1;
    double *p = plane64 + (long)b * PL_P64;
    p[0] = nx, p[1] = ny, p[2] = nz, p[3] = dp;
    p[4] = p0x, p[5] = p0y, p[6] = p0z, p[7] = 1.0;
  }
}

// ---- D ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void plane_height_kernel(
    const float *__restrict__ xyz, const double *__restrict__ plane64,
    float *__restrict__ height, unsigned char *__restrict__ ground,
    unsigned char *__restrict__ inlier, int N, float thresh) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double *p = plane64 + (long)b * PL_P64;
  const long o = (long)b * N + i;
  const float fx = xyz[o * 3 + 0], fy = xyz[o * 3 + 1], fz = xyz[o * 3 + 2];
  float hf = INFINITY;
  if (p[7] != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(fz)) {
    const double hh = (p[0] * ((double)fx - p[4]) + p[1] * ((double)fy - p[5]) +
                       p[2] * ((double)fz - p[6])) + p[3];
    const float v = (float)hh;
    hf = isfinite(v) ? v : INFINITY;
  }
  height[o] = hf;
  ground[o] = hf <= thresh ? 1 : 0;
  inlier[o] = fabsf(hf) <= thresh ? 1 : 0;
}

void launch_plane_hypotheses(const float *xyz, const unsigned char *mask,
                             int *idx, float *rec, int *count, int B, int N,
                             int H, unsigned seed, float upx, float upy,
                             float upz, float cos2, float thresh2,
                             hipStream_t stream) {
  hipLaunchKernelGGL(plane_hyp_kernel, dim3((H + PL_BLOCK - 1) / PL_BLOCK, B),
                     dim3(PL_BLOCK), 0, stream, xyz, mask, idx, rec, count, N, H,
                     seed, upx, upy, upz, cos2, thresh2);
  hipLaunchKernelGGL(plane_score_kernel,
                     dim3((N + PL_TILE - 1) / PL_TILE,
                          (H + PL_BLOCK - 1) / PL_BLOCK, B),
                     dim3(PL_BLOCK), 0, stream, xyz, mask, rec, count, N, H);
}

void launch_plane_refine(const float *xyz, const unsigned char *mask,
                         const float *rec, const int *count, float *normal,
                         float *offset, float *height, unsigned char *ground,
                         unsigned char *inlier, int *count_out, int *best,
                         int *rounds, unsigned char *ok, double *plane64, int B,
                         int N, int H, int iters, double thresh, float upx,
                         float upy, float upz, float cos2, hipStream_t stream) {
  hipLaunchKernelGGL(plane_refine_kernel, dim3(B), dim3(PL_RF_THREADS), 0,
                     stream, xyz, mask, rec, count, normal, offset, count_out,
                     best, rounds, ok, plane64, N, H, iters, thresh, upx, upy,
                     upz, cos2);
  hipLaunchKernelGGL(plane_height_kernel, dim3((N + 255) / 256, B), dim3(256), 0,
                     stream, xyz, plane64, height, ground, inlier, N,
                     (float)thresh);
}
