// K24: noise filter (absent in the reference): per point the number of
// neighbours within a radius and the mean distance to the k nearest ones, on a
// hashed cell grid with edge = radius, then cloud statistics and the flags.
//
//   q = floor(fp32(x * inv)) per coordinate, inv = fp32(1) / fp32(radius) from
//   the host.  Eligible: masked, finite, -2^20 <= q < 2^20 on all three axes
//   (the level-0 rules of voxel_sample.hip), cell c = int(q).
//   j is a neighbour of i: j != i, both eligible, max|c_i - c_j| <= 1 and
//   d2 = (dx*dx + dy*dy) + dz*dz <= r2, every operation an fp32 operation
//   rounded on its own (fp contract off for this file), r2 from the host.
//   count_i = neighbours; mean_dist_i = (sqrt of the k smallest d2, correctly
//   rounded, summed ascending in fp32) / fp32(k), +INF if count_i < k or k = 0.
//   mean / std (population, two passes) / threshold = mean + ratio * std in
//   fp64 over the finite mean_dist; keep = eligible, count >= min_neighbors and
//   not (k >= 1 and (count < k or fp64(mean_dist) > threshold)).
//   out: keep (B,N) bool, count (B,N) int32 (-1 ineligible), mean_dist (B,N),
//   stats (B,3) fp64, ok (B) bool.
//
// 9 launches.  Kernel boundaries and __syncthreads() inside one workgroup are
// the only synchronisation; no lane or workgroup ever waits for another one's
// progress.  All atomics are integer (compare-and-swap, add).  The order in
// which they land decides only the order of the points inside a cell of the
// sorted array; count is an integer and the k smallest d2 a multiset, so no
// output depends on it.
//
//  1. nf_init_kernel     table keys = empty word, cell counters = 0, status = 0:
//                        every workspace word that is read later is written
//                        here or by a later kernel before its use.
//  2. nf_count_kernel    one lane per point: eligibility, the 63-bit cell key
//                        (three 21-bit fields biased by 2^20); the point finds
//                        or claims the slot of its key in a table of T >= 2 N
//                        slots (a power of two) per cloud, ONE compare-and-swap
//                        per probe step, capped at T steps (status[b] at the
//                        cap), adds 1 to the cell counter and remembers the
//                        slot.  Ineligible points get count = -1, mean_dist =
//                        +INF here.
//  3. nf_scan_kernel     exclusive scan of the counters inside every run of
//                        NF_THREADS slots, the run totals to bsum.
//  4. nf_offset_kernel   one wave per cloud: exclusive scan of bsum in steps
//                        of NF_SCAN, the eligible total.  No look-back.
//  5. nf_scatter_kernel  one integer add per point on its cell's cursor (the
//                        scanned counter: afterwards it holds the cell's END),
//                        then (x, y, z, index) into the cell-sorted array.
//  6. nf_query_kernel    one lane per sorted position, so a wave mostly shares
//                        its 27 table lookups (plain loads: the table is final)
//                        and streams the same members as 16-byte loads.  The k
//                        smallest d2 sit in KCAP registers (instantiations 0,
//                        8, 16, padded with +INF, statically indexed insertion:
//                        no scratch).  All points in one cell cost O(N^2)
//                        member tests; that terminates and is accepted.
//  7. nf_stat_kernel     pass 1: per-workgroup fp64 sum and number of the
//                        finite mean_dist, in index order with a fixed tree.
//  8. nf_stat_kernel     pass 2: every workgroup folds the pass-1 partials
//                        itself (fixed order, the same bits in every workgroup)
//                        to the mean, then its partial of (m - mean)^2.
//  9. nf_flag_kernel     every workgroup folds both partial rows to mean, std
//                        and threshold; keep; workgroup 0 writes stats and ok.
//                        With status set: keep = 0, count = -1, mean_dist =
//                        +INF, stats = 0.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs /
// LDS bytes / scratch bytes: init 12 / 0 / 0, count 12 / 0 / 0, scan 10 / 16 / 0,
// offset 14 / 0 / 0, scatter 10 / 0 / 0, query<0> 19 / 0 / 0, query<8> 27 / 0 / 0,
// query<16> 35 / 0 / 0, stat 16 / 2048 / 0, flag 16 / 2048 / 0; no AGPRs, 8 waves
// per SIMD everywhere.
#include <hip/hip_runtime.h>
#include "common.h"

#pragma clang fp contract(off)

#define NF_THREADS 256
#define NF_WAVES (NF_THREADS / WAVE)
#define NF_SCAN 64  // lanes of the run-total scan: one wave
#define NF_RANGE (1 << 20)
#define NF_EMPTY (~0ull)  // no key has bit 63 set

typedef unsigned long long nf_u64;

int noise_filter_block() { return NF_THREADS; }
int noise_filter_scan() { return NF_SCAN; }

// slot hash: the 64-bit finaliser voxel_sample.hip uses (lattice inputs give
// arithmetic-progression keys)
DEV_INLINE unsigned nf_slot_hash(nf_u64 k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

DEV_INLINE nf_u64 nf_key(int cx, int cy, int cz) {
  return ((nf_u64)(cx + NF_RANGE) << 42) | ((nf_u64)(cy + NF_RANGE) << 21) | (nf_u64)(cz + NF_RANGE);
}

// Cell of a point; false if the point is not eligible (the mask aside).
DEV_INLINE bool nf_cell(float x, float y, float z, float inv, int &cx, int &cy, int &cz) {
  const float qx = floorf(x * inv), qy = floorf(y * inv), qz = floorf(z * inv);
  const float lo = -(float)NF_RANGE, hi = (float)NF_RANGE;
  const bool el = isfinite(x) && isfinite(y) && isfinite(z) && qx >= lo && qx < hi && qy >= lo &&
                  qy < hi && qz >= lo && qz < hi;
  cx = el ? (int)qx : 0;
  cy = el ? (int)qy : 0;
  cz = el ? (int)qz : 0;
  return el;
}

// Finds or claims the slot of `key`; -1 at the cap.
DEV_INLINE int nf_insert(nf_u64 *keys, int T, nf_u64 key) {
  unsigned s = nf_slot_hash(key) & (unsigned)(T - 1);
  for (int step = 0; step < T; ++step) {
    nf_u64 seen = NF_EMPTY;
    const bool claimed = __hip_atomic_compare_exchange_strong(
        keys + s, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (claimed || seen == key) return (int)s;
    s = (s + 1u) & (unsigned)(T - 1);
  }
  return -1;
}

// Slot of `key` in the finished table, -1 if the cell is empty, -2 at the cap.
DEV_INLINE int nf_find(const nf_u64 *__restrict__ keys, int T, nf_u64 key) {
  unsigned s = nf_slot_hash(key) & (unsigned)(T - 1);
  for (int step = 0; step < T; ++step) {
    const nf_u64 seen = keys[s];
    if (seen == key) return (int)s;
    if (seen == NF_EMPTY) return -1;
    s = (s + 1u) & (unsigned)(T - 1);
  }
  return -2;
}

__global__ __launch_bounds__(NF_THREADS) void nf_init_kernel(
    nf_u64 *__restrict__ keys, int *__restrict__ cnt, long slots, int *__restrict__ status, int B) {
  const long t = (long)blockIdx.x * NF_THREADS + threadIdx.x;
  const long stride = (long)gridDim.x * NF_THREADS;
  for (long j = t; j < slots; j += stride) {
    keys[j] = NF_EMPTY;
    cnt[j] = 0;
  }
  for (long j = t; j < B; j += stride) status[j] = 0;
}

__global__ __launch_bounds__(NF_THREADS) void nf_count_kernel(
    const float *__restrict__ xyz,           // (B, N, 3)
    const unsigned char *__restrict__ mask,  // (B, N) or null
    nf_u64 *keys, int *cnt,                  // (B, T) each
    int *__restrict__ slot,                  // (B, N)
    int *__restrict__ count, float *__restrict__ md, int *status, int N, int T, float inv) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * NF_THREADS + threadIdx.x;
  if (i >= N) return;
  const long g = (long)b * N + i;
  int cx, cy, cz;
  const bool el = nf_cell(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], inv, cx, cy, cz) &&
                  (mask == nullptr || mask[g] != 0);
  int s = -1;
  if (el) {
    s = nf_insert(keys + (long)b * T, T, nf_key(cx, cy, cz));
    if (s < 0)
      __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      atomicAdd(cnt + (long)b * T + s, 1);
  }
  slot[g] = s;
  if (s < 0) {  // the query kernel writes every other point
    count[g] = -1;
    md[g] = INFINITY;
  }
}

// Exclusive prefix of v over the workgroup's NF_THREADS lanes.
DEV_INLINE int nf_block_excl(int v, int *wsum) {
  int x = v;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int y = __shfl_up(x, off, WAVE);
    if (lane_id() >= off) x += y;
  }
  if (lane_id() == WAVE - 1) wsum[wave_id()] = x;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < NF_WAVES; ++w) base += w < wave_id() ? wsum[w] : 0;
  return base + x - v;
}

__global__ __launch_bounds__(NF_THREADS) void nf_scan_kernel(
    const int *__restrict__ cnt, int *__restrict__ cur, int *__restrict__ bsum, int T) {
  __shared__ int wsum[NF_WAVES];
  const int b = blockIdx.y;
  const int s = blockIdx.x * NF_THREADS + threadIdx.x;
  const int v = s < T ? cnt[(long)b * T + s] : 0;
  const int ex = nf_block_excl(v, wsum);
  if (s < T) cur[(long)b * T + s] = ex;
  if (threadIdx.x == NF_THREADS - 1) bsum[(long)b * gridDim.x + blockIdx.x] = ex + v;
}

__global__ __launch_bounds__(NF_SCAN) void nf_offset_kernel(
    int *__restrict__ bsum, int *__restrict__ elig, int nrun) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  bsum += (long)b * nrun;
  int run = 0;
  for (int base = 0; base < nrun; base += NF_SCAN) {
    const int j = base + lane;
    const int v = j < nrun ? bsum[j] : 0;
    int x = v;
#pragma unroll
    for (int off = 1; off < NF_SCAN; off <<= 1) {
      const int y = __shfl_up(x, off, WAVE);
      if (lane >= off) x += y;
    }
    if (j < nrun) bsum[j] = run + x - v;
    run += __shfl(x, NF_SCAN - 1, WAVE);
  }
  if (lane == 0) elig[b] = run;
}

__global__ __launch_bounds__(NF_THREADS) void nf_scatter_kernel(
    const float *__restrict__ xyz, const int *__restrict__ slot, int *cur,
    const int *__restrict__ bsum, float4 *__restrict__ sorted, int N, int T, int nrun) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * NF_THREADS + threadIdx.x;
  if (i >= N) return;
  const long g = (long)b * N + i;
  const int s = slot[g];
  if (s < 0) return;
  const int pos = bsum[(long)b * nrun + s / NF_THREADS] + atomicAdd(cur + (long)b * T + s, 1);
  if (pos < N)  // holds by construction: the counters sum to at most N
    sorted[(long)b * N + pos] =
        make_float4(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], __int_as_float(i));
}

template <int KCAP>
__global__ __launch_bounds__(NF_THREADS) void nf_query_kernel(
    const float4 *__restrict__ sorted, const nf_u64 *__restrict__ keys,
    const int *__restrict__ cnt, const int *__restrict__ cur, const int *__restrict__ bsum,
    const int *__restrict__ elig, int *__restrict__ count, float *__restrict__ md, int *status,
    int N, int T, int nrun, float inv, float r2, int k) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * NF_THREADS + threadIdx.x;
  if (p >= elig[b]) return;
  sorted += (long)b * N;
  keys += (long)b * T;
  cnt += (long)b * T;
  cur += (long)b * T;
  bsum += (long)b * nrun;
  const float4 me = sorted[p];
  int cx, cy, cz;
  nf_cell(me.x, me.y, me.z, inv, cx, cy, cz);
  float best[KCAP > 0 ? KCAP : 1];
#pragma unroll
  for (int s = 0; s < KCAP; ++s) best[s] = INFINITY;
  int n = 0;
  bool capped = false;
  for (int c = 0; c < 27; ++c) {
    const int nx = cx + c / 9 - 1, ny = cy + (c / 3) % 3 - 1, nz = cz + c % 3 - 1;
    if (nx < -NF_RANGE || nx >= NF_RANGE || ny < -NF_RANGE || ny >= NF_RANGE || nz < -NF_RANGE ||
        nz >= NF_RANGE)
      continue;  // no eligible point has such a cell
    const int s = nf_find(keys, T, nf_key(nx, ny, nz));
    if (s < 0) {
      capped = capped || s == -2;
      continue;
    }
    int end = bsum[s / NF_THREADS] + cur[s];
    if (end > N) end = N;
    int j = end - cnt[s];
    if (j < 0) j = 0;
    for (; j < end; ++j) {
      const float4 o = sorted[j];
      const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (j != p && d2 <= r2) {
        ++n;
        if (KCAP > 0 && d2 < best[KCAP > 0 ? KCAP - 1 : 0]) {
#pragma unroll
          for (int t = KCAP - 1; t >= 1; --t) {
            const float lo = best[t - 1];
            best[t] = d2 < lo ? lo : (d2 < best[t] ? d2 : best[t]);
          }
          best[0] = d2 < best[0] ? d2 : best[0];
        }
      }
    }
  }
  if (capped) __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // sqrtf and / are the correctly rounded sequences (v_sqrt_f32 plus the fma
  // correction, v_div_scale / fmas / fixup) without fast-math flags.  HIP's
  // __fsqrt_rn is NOT: unless OCML_BASIC_ROUNDED_OPERATIONS is defined it is
  // the bare v_sqrt_f32, and mean_dist came out one ulp off the oracle's on
  // an MI355X with it.
  float m = INFINITY;
  if (KCAP > 0 && k >= 1 && n >= k) {
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < KCAP; ++t)
      if (t < k) sum = sum + sqrtf(best[t]);
    m = sum / (float)k;
  }
  const long g = (long)b * N + __float_as_int(me.w);
  count[g] = n;
  md[g] = m;
}

// Sum over the workgroup in a fixed tree; every lane returns the total.
DEV_INLINE double nf_block_sum(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int off = NF_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double t = red[0];
  __syncthreads();  // red may be reused
  return t;
}

// Fold of one row of per-workgroup partials, the same bits in every
// workgroup that calls it: lane t sums elements t, t + NF_THREADS, ... in
// order, then the fixed tree.
DEV_INLINE double nf_fold(const double *__restrict__ part, int nblk, double *red) {
  double v = 0.0;
  for (int j = threadIdx.x; j < nblk; j += NF_THREADS) v += part[j];
  return nf_block_sum(v, red);
}

// part: (B, 3, nblk) doubles: sum of the finite mean_dist, their number, sum of
// the squared deviations.  pass 0 fills rows 0 and 1, pass 1 row 2.
__global__ __launch_bounds__(NF_THREADS) void nf_stat_kernel(
    const float *__restrict__ md, double *__restrict__ part, int N, int pass) {
  __shared__ double red[NF_THREADS];
  const int b = blockIdx.y;
  const int i = blockIdx.x * NF_THREADS + threadIdx.x;
  const int nblk = gridDim.x;
  part += (long)b * 3 * nblk;
  const float m = i < N ? md[(long)b * N + i] : INFINITY;
  const bool fin = isfinite(m);
  if (pass == 0) {
    const double s = nf_block_sum(fin ? (double)m : 0.0, red);
    const double c = nf_block_sum(fin ? 1.0 : 0.0, red);
    if (threadIdx.x == 0) {
      part[blockIdx.x] = s;
      part[nblk + blockIdx.x] = c;
    }
  } else {
    const double s = nf_fold(part, nblk, red);
    const double c = nf_fold(part + nblk, nblk, red);
    const double mean = c > 0.0 ? s / c : 0.0;
    const double d = fin ? (double)m - mean : 0.0;
    const double q = nf_block_sum(d * d, red);
    if (threadIdx.x == 0) part[2 * nblk + blockIdx.x] = q;
  }
}

__global__ __launch_bounds__(NF_THREADS) void nf_flag_kernel(
    const double *__restrict__ part, const int *__restrict__ status, int *__restrict__ count,
    float *__restrict__ md, unsigned char *__restrict__ keep, double *__restrict__ stats,
    unsigned char *__restrict__ ok, int N, int k, int min_nb, double ratio) {
  __shared__ double red[NF_THREADS];
  const int b = blockIdx.y;
  const int i = blockIdx.x * NF_THREADS + threadIdx.x;
  const int nblk = gridDim.x;
  part += (long)b * 3 * nblk;
  const bool failed = status[b] != 0;  // final: every probe ran in an earlier launch
  const double s = nf_fold(part, nblk, red);
  const double c = nf_fold(part + nblk, nblk, red);
  const double q = nf_fold(part + 2 * nblk, nblk, red);
  const bool some = c > 0.0 && k >= 1 && !failed;
  const double mean = some ? s / c : 0.0;
  const double sd = some ? sqrt(q / c) : 0.0;
  const double thr = some ? mean + ratio * sd : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[b * 3 + 0] = mean;
    stats[b * 3 + 1] = sd;
    stats[b * 3 + 2] = thr;
    ok[b] = failed ? 0 : 1;
  }
  if (i >= N) return;
  const long g = (long)b * N + i;
  if (failed) {
    count[g] = -1;
    md[g] = INFINITY;
    keep[g] = 0;
    return;
  }
  const int n = count[g];
  const bool far = k >= 1 && (n < k || (double)md[g] > thr);
  keep[g] = (n >= 0 && n >= min_nb && !far) ? 1 : 0;
}

// keys: B * T words; cells: 2 * B * T ints (counters, cursors); slot: B * N
// ints; sorted: B * N float4; bsum: B * nrun ints, nrun = ceil(T / block);
// meta: 2 * B ints (status, eligible); part: 3 * B * nblk doubles, nblk =
// ceil(N / block).  T is a power of two >= 2 N.
void launch_noise_filter(const float *xyz, const unsigned char *mask, unsigned long long *keys,
                         int *cells, int *slot, float *sorted, int *bsum, int *meta, double *part,
                         unsigned char *keep, int *count, float *md, double *stats,
                         unsigned char *ok, int B, int N, int T, float inv, float r2, int k,
                         int min_nb, double ratio, hipStream_t stream) {
  const long BT = (long)B * T;
  int *cnt = cells, *cur = cells + BT;
  int *status = meta, *elig = meta + B;
  float4 *srt = reinterpret_cast<float4 *>(sorted);
  const int nblk = (N + NF_THREADS - 1) / NF_THREADS;
  const int nrun = (T + NF_THREADS - 1) / NF_THREADS;
  const dim3 block(NF_THREADS), pts(nblk, B), runs(nrun, B);
  long init_blocks = (BT + NF_THREADS - 1) / NF_THREADS;
  if (init_blocks > 8192) init_blocks = 8192;
  hipLaunchKernelGGL(nf_init_kernel, dim3((unsigned)init_blocks), block, 0, stream, keys, cnt, BT,
                     status, B);
  hipLaunchKernelGGL(nf_count_kernel, pts, block, 0, stream, xyz, mask, keys, cnt, slot, count, md,
                     status, N, T, inv);
  hipLaunchKernelGGL(nf_scan_kernel, runs, block, 0, stream, cnt, cur, bsum, T);
  hipLaunchKernelGGL(nf_offset_kernel, dim3(B), dim3(NF_SCAN), 0, stream, bsum, elig, nrun);
  hipLaunchKernelGGL(nf_scatter_kernel, pts, block, 0, stream, xyz, slot, cur, bsum, srt, N, T,
                     nrun);
  if (k == 0)
    hipLaunchKernelGGL(nf_query_kernel<0>, pts, block, 0, stream, srt, keys, cnt, cur, bsum, elig,
                       count, md, status, N, T, nrun, inv, r2, k);
  else if (k <= 8)
    hipLaunchKernelGGL(nf_query_kernel<8>, pts, block, 0, stream, srt, keys, cnt, cur, bsum, elig,
                       count, md, status, N, T, nrun, inv, r2, k);
  else
    hipLaunchKernelGGL(nf_query_kernel<16>, pts, block, 0, stream, srt, keys, cnt, cur, bsum, elig,
                       count, md, status, N, T, nrun, inv, r2, k);
  hipLaunchKernelGGL(nf_stat_kernel, pts, block, 0, stream, md, part, N, 0);
  hipLaunchKernelGGL(nf_stat_kernel, pts, block, 0, stream, md, part, N, 1);
  hipLaunchKernelGGL(nf_flag_kernel, pts, block, 0, stream, part, status, count, md, keep, stats,
                     ok, N, k, min_nb, ratio);
}
